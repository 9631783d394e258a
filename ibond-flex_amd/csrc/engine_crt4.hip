// Split-pair CRT encryption for 2049..4096-bit key holders (kernels_crt4.hpp): instantiations, geometry, launches.
#include "engine_crt4.hpp"

namespace fpai {

template <typename K>
static int occupancy(K kernel) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, LANE_BLOCK, 0) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

int crt4_geometry(int cus, long long chunk, Crt4Geom* g) {
  const long long lb = (chunk + LANE_BLOCK - 1) / LANE_BLOCK, pb = (chunk + D4_PAIRS - 1) / D4_PAIRS;
  auto clamp = [](long long v, long long cap) { return (int)std::max<long long>(1, std::min<long long>(v, cap)); };
  g->gx_a = clamp(lb, (long long)occupancy(k_crt4_a<D4_S>) * cus / 2);
  g->gx_b = clamp(pb, (long long)occupancy(k_crt4_b<D4_S>) * cus / 2);
  g->scratch_bytes = (size_t)2 * std::max(g->gx_a, g->gx_b) * LANE_BLOCK * lane_scratch_words<D4_S>() * 4;
  return 0;
}

hipError_t crt4_launch_a(const Crt4Params& p, const Crt4Geom& g, hipStream_t st) {
  const long long lb = (p.n + LANE_BLOCK - 1) / LANE_BLOCK;
  hipLaunchKernelGGL(k_crt4_pre<D4_S>, dim3((int)std::min<long long>(g.gx_a, lb), 2), dim3(LANE_BLOCK), 0, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_crt4_a<D4_S>, dim3((int)std::min<long long>(g.gx_a, lb), 2), dim3(LANE_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t crt4_launch_b(const Crt4Params& p, const Crt4Geom& g, hipStream_t st) {
  const long long pb = (p.n + D4_PAIRS - 1) / D4_PAIRS;
  hipLaunchKernelGGL(k_crt4_b<D4_S>, dim3((int)std::min<long long>(g.gx_b, pb), 2), dim3(LANE_BLOCK), 0, st, p);
  return hipGetLastError();
}

}  // namespace fpai
