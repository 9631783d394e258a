// Re-randomisation kernel (kernels_obf.hpp): instantiations and launches.
#include "engine_obf.hpp"

namespace fpai {

int obf_occupancy(int tpi, int* occ) {
  hipError_t e;
  if (tpi == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_obf_mul<2>, BLOCK, obf_lds_bytes());
  else if (tpi == 4) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_obf_mul<4>, BLOCK, obf_lds_bytes());
  else if (tpi == 8) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_obf_mul<8>, BLOCK, obf_lds_bytes());
  else return -1;
  if (e != hipSuccess || *occ < 1) *occ = 1;
  return 0;
}

hipError_t obf_launch(int tpi, const ObfMulParams& p, int grid, hipStream_t st) {
  const size_t lds = obf_lds_bytes();
  if (tpi == 2) hipLaunchKernelGGL(k_obf_mul<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_obf_mul<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_obf_mul<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
