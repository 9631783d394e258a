// 1024-bit public-key fixed-base kernels (kernels_pfb1.hpp): instantiations and launches.
#include "engine_pfb1.hpp"

namespace fpai {

int pfb1_occupancy(int* occ) {
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pfb1<PFB1_S>, LANE_BLOCK, 0) != hipSuccess || *occ < 1) *occ = 1;
  return 0;
}

hipError_t pfb1_build(const Pfb1Const* d_c, int nbases, int K, int W, uint4* table, hipStream_t st) {
  constexpr int B = PFB1_SETUP_BLOCK;
  hipLaunchKernelGGL(k_pfb1_chain<PFB1_S>, dim3((nbases + B - 1) / B), dim3(B), 0, st, d_c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int LO = W / 2, HI = W - LO;
  const int nent = (1 << LO) + (1 << HI);
  hipLaunchKernelGGL(k_pfb1_lohi<PFB1_S>, dim3((nent + B - 1) / B, K), dim3(B), 0, st, d_c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_pfb1_fill<PFB1_S>, dim3((1 << W) / B, K), dim3(B), 0, st, d_c, table);
  return hipGetLastError();
}

hipError_t pfb1_launch(const Pfb1Params& p, int gx, hipStream_t st) {
  hipLaunchKernelGGL(k_pfb1<PFB1_S>, dim3(gx), dim3(LANE_BLOCK), 0, st, p);
  return hipGetLastError();
}

}  // namespace fpai
