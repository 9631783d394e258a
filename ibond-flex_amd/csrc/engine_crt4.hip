// Split-pair CRT encryption for 2049..4096-bit key holders (kernels_crt4.hpp) at 74 limbs and, for the 3072-bit band,
// at 56: instantiations, geometry, launches.
#include "engine_crt4.hpp"

namespace fpai {

template <typename K>
static int occupancy(K kernel) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, LANE_BLOCK, 0) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

template <int S>
static void geometry(int cus, long long chunk, Crt4Geom* g) {
  const long long lb = (chunk + LANE_BLOCK - 1) / LANE_BLOCK, pb = (chunk + D4_PAIRS - 1) / D4_PAIRS;
  auto clamp = [](long long v, long long cap) { return (int)std::max<long long>(1, std::min<long long>(v, cap)); };
  g->gx_a = clamp(lb, (long long)occupancy(k_crt4_a<S>) * cus / 2);
  g->gx_b = clamp(pb, (long long)occupancy(k_crt4_b<S>) * cus / 2);
  g->scratch_bytes = (size_t)2 * std::max(g->gx_a, g->gx_b) * LANE_BLOCK * lane_scratch_words<S>() * 4;
}

int crt4_geometry(int S, int cus, long long chunk, Crt4Geom* g) {
  if (S == D4_S) geometry<D4_S>(cus, chunk, g);
  else if (S == D4_S3) geometry<D4_S3>(cus, chunk, g);
  else return -1;
  return 0;
}

template <int S>
static hipError_t launch_a(const Crt4Params& p, const Crt4Geom& g, hipStream_t st) {
  const long long lb = (p.n + LANE_BLOCK - 1) / LANE_BLOCK;
  hipLaunchKernelGGL(k_crt4_pre<S>, dim3((int)std::min<long long>(g.gx_a, lb), 2), dim3(LANE_BLOCK), 0, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_crt4_a<S>, dim3((int)std::min<long long>(g.gx_a, lb), 2), dim3(LANE_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t crt4_launch_a(int S, const Crt4Params& p, const Crt4Geom& g, hipStream_t st) {
  if (S == D4_S) return launch_a<D4_S>(p, g, st);
  if (S == D4_S3) return launch_a<D4_S3>(p, g, st);
  return hipErrorInvalidValue;
}

template <int S>
static hipError_t launch_b(const Crt4Params& p, const Crt4Geom& g, hipStream_t st) {
  const long long pb = (p.n + D4_PAIRS - 1) / D4_PAIRS;
  hipLaunchKernelGGL(k_crt4_b<S>, dim3((int)std::min<long long>(g.gx_b, pb), 2), dim3(LANE_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t crt4_launch_b(int S, const Crt4Params& p, const Crt4Geom& g, hipStream_t st) {
  if (S == D4_S) return launch_b<D4_S>(p, g, st);
  if (S == D4_S3) return launch_b<D4_S3>(p, g, st);
  return hipErrorInvalidValue;
}

}  // namespace fpai
