// 2049..4096-bit public-key fixed-base kernels (kernels_pfb4.hpp): instantiations and launches.
#include "engine_pfb4.hpp"

#include <atomic>

namespace fpai {

// k_pfb4's two row buffers per group are above the 64 KiB a launch gets unasked: asked for once per device
static hipError_t pfb4_ask_lds() {
  static std::atomic<unsigned long long> asked{0};   // a bit per device
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (asked.load(std::memory_order_acquire) >> dev & 1ull) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pfb4<PE4_TPI, PE4_LL>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)PFB4_LDS);
  if (e == hipSuccess) asked.fetch_or(1ull << dev, std::memory_order_release);
  return e;
}

int pfb4_occupancy(int* occ) {
  if (pfb4_ask_lds() != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pfb4<PE4_TPI, PE4_LL>, BLOCK, PFB4_LDS) != hipSuccess || *occ < 1)
    *occ = 1;
  return 0;
}

hipError_t pfb4_build(const Pfb4Const* d_c, int nbases, int K, int W, uint32_t* table, hipStream_t st) {
  constexpr int B = PFB4_SETUP_BLOCK, G = B / PE4_TPI;   // groups per block
  hipLaunchKernelGGL((k_pfb4_chain<PE4_TPI, PE4_LL>), dim3((nbases + G - 1) / G), dim3(B), 0, st, d_c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int LO = W / 2, HI = W - LO;
  const int nent = (1 << LO) + (1 << HI);
  hipLaunchKernelGGL((k_pfb4_lohi<PE4_TPI, PE4_LL>), dim3((nent + G - 1) / G, K), dim3(B), 0, st, d_c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL((k_pfb4_fill<PE4_TPI, PE4_LL>), dim3(((1 << W) + G - 1) / G, K), dim3(B), 0, st, d_c, table);
  return hipGetLastError();
}

hipError_t pfb4_launch(const Pfb4Params& p, int gx, hipStream_t st) {
  const hipError_t e = pfb4_ask_lds();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_pfb4<PE4_TPI, PE4_LL>), dim3(gx), dim3(BLOCK), PFB4_LDS, st, p);
  return hipGetLastError();
}

}  // namespace fpai
