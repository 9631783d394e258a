// Wide-integer kernels (kernels_big.hpp): instantiations and launches.
#include "engine_big.hpp"

#include <algorithm>

namespace fpai {

int mul_big_occupancy(int tpi, int xw, int* occ) {
  hipError_t e;
  const size_t lds = mul_big_lds_bytes(tpi, xw);
  if (tpi == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_mul_big<2>, BLOCK, lds);
  else if (tpi == 4) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_mul_big<4>, BLOCK, lds);
  else if (tpi == 8) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_mul_big<8>, BLOCK, lds);
  else return -1;
  if (e != hipSuccess || *occ < 1) *occ = 1;
  return 0;
}

hipError_t mul_big_launch(int tpi, const MulBigParams& p, int grid, hipStream_t st) {
  const size_t lds = mul_big_lds_bytes(tpi, p.k.xw);
  if (tpi == 2) hipLaunchKernelGGL(k_mul_big<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_mul_big<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_mul_big<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t big_c0_launch(int tpi, const BigC0Params& p, int cus, hipStream_t st) {
  const size_t lds = big_c0_lds_bytes(tpi);
  const long long gpb = BLOCK / tpi;
  const int grid = (int)std::max<long long>(1, std::min<long long>((p.n + gpb - 1) / gpb, 8ll * cus));
  if (tpi == 2) hipLaunchKernelGGL(k_big_c0<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_big_c0<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_big_c0<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
