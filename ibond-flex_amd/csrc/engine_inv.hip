// Modular inversion kernels (kernels_inv.hpp): instantiations and launches.
#include "engine_inv.hpp"

namespace fpai {

// clears a status word on the stream (a kernel, not a memset, so that a captured graph can hold it)
__global__ void k_modinv_clear(uint32_t* word) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *word = 0u;
}

hipError_t modinv_launch(const ModinvParams& p, int count, hipStream_t st) {
  if (p.W < 1 || p.W > MODINV_MAX_WORDS || count < 1) return hipErrorInvalidValue;
  if (p.any_noinv) hipLaunchKernelGGL(k_modinv_clear, dim3(1), dim3(64), 0, st, p.any_noinv);
  switch ((p.W + 63) / 64) {
    case 1: hipLaunchKernelGGL(k_modinv<1>, dim3(count), dim3(64), 0, st, p); break;
    case 2: hipLaunchKernelGGL(k_modinv<2>, dim3(count), dim3(64), 0, st, p); break;
    case 3: hipLaunchKernelGGL(k_modinv<3>, dim3(count), dim3(64), 0, st, p); break;
    default: hipLaunchKernelGGL(k_modinv<4>, dim3(count), dim3(64), 0, st, p); break;
  }
  return hipGetLastError();
}

hipError_t modinv_clear(uint32_t* word, hipStream_t st) {
  hipLaunchKernelGGL(k_modinv_clear, dim3(1), dim3(64), 0, st, word);
  return hipGetLastError();
}

hipError_t modinv_attributes(int W, int* vgprs, int* blocks_per_cu) {
  const void* fn;
  switch ((W + 63) / 64) {
    case 1: fn = (const void*)k_modinv<1>; break;
    case 2: fn = (const void*)k_modinv<2>; break;
    case 3: fn = (const void*)k_modinv<3>; break;
    default: fn = (const void*)k_modinv<4>; break;
  }
  hipFuncAttributes at{};
  hipError_t e = hipFuncGetAttributes(&at, fn);
  if (e != hipSuccess) return e;
  *vgprs = at.numRegs;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fn, 64, 0);
}

}  // namespace fpai
