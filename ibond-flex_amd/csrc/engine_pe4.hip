// Pair-group public-key encryption for n of 2049..4096 bits (kernels_pe4.hpp): instantiations, geometry, launches.
#include "engine_pe4.hpp"

#include <algorithm>

namespace fpai {

static size_t pre_lds() { return (size_t)PE4_GPB * 2 * PE4_S * 4; }
static size_t pow_lds() { return ((size_t)PE4_GPB * 2 * PE4_S + PE4_S) * 4; }
static size_t fin_lds() { return (size_t)PE4_GPB * PE4_FSLOT * 4; }

template <typename K>
static int occupancy(K kernel, size_t lds) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, BLOCK, lds) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

int pe4_geometry(int cus, long long chunk, Pe4Geom* g) {
  const long long gb = (chunk + PE4_GPB - 1) / PE4_GPB;
  auto clamp = [](long long v, long long cap) { return (int)std::max<long long>(1, std::min<long long>(v, cap)); };
  g->gx_pre = clamp(gb, (long long)occupancy(k_pe4_pre<PE4_TPI, PE4_LL>, pre_lds()) * cus);
  g->gx_pow = clamp(gb, (long long)occupancy(k_pe4_pow<PE4_TPI, PE4_LL>, pow_lds()) * cus);
  g->gx_fin = clamp(gb, (long long)occupancy(k_pe4_fin<PE4_TPI, PE4_LL>, fin_lds()) * cus);
  g->scratch_bytes = (size_t)g->gx_pow * BLOCK * PE4_SCRATCH_WORDS * 4;
  return 0;
}

hipError_t pe4_launch(const Pe4Params& p, const Pe4Geom& g, hipStream_t st, hipEvent_t* ev) {
  const long long gb = (p.n + PE4_GPB - 1) / PE4_GPB;
  if (ev && ev[0]) (void)hipEventRecord(ev[0], st);
  hipLaunchKernelGGL((k_pe4_pre<PE4_TPI, PE4_LL>), dim3((int)std::min<long long>(g.gx_pre, gb)), dim3(BLOCK), pre_lds(), st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (ev && ev[1]) (void)hipEventRecord(ev[1], st);
  hipLaunchKernelGGL((k_pe4_pow<PE4_TPI, PE4_LL>), dim3((int)std::min<long long>(g.gx_pow, gb)), dim3(BLOCK), pow_lds(), st, p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && ev[2]) (void)hipEventRecord(ev[2], st);
  hipLaunchKernelGGL((k_pe4_fin<PE4_TPI, PE4_LL>), dim3((int)std::min<long long>(g.gx_fin, gb)), dim3(BLOCK), fin_lds(), st, p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && ev[3]) (void)hipEventRecord(ev[3], st);
  return hipSuccess;
}

}  // namespace fpai
