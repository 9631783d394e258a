// Obfuscator-pool kernels (kernels_pool.hpp): instantiations and launches.
#include "engine_pool.hpp"

namespace fpai {

template <int TPI>
static hipError_t pool_occ(int which, int* occ) {
  if (which == 0) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pool_enc<TPI>, BLOCK, pool_lds_bytes());
  if (which == 1) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pool_join<TPI>, BLOCK, pool_lds_bytes());
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pool_split<TPI>, BLOCK, pool_lds_bytes());
}

int pool_occupancy(int tpi, int which, int* occ) {
  hipError_t e;
  if (tpi == 2) e = pool_occ<2>(which, occ);
  else if (tpi == 4) e = pool_occ<4>(which, occ);
  else if (tpi == 8) e = pool_occ<8>(which, occ);
  else return -1;
  if (e != hipSuccess || *occ < 1) *occ = 1;
  return 0;
}

hipError_t pool_enc_launch(int tpi, const PoolEncParams& p, int grid, hipStream_t st) {
  const size_t lds = pool_lds_bytes();
  if (tpi == 2) hipLaunchKernelGGL(k_pool_enc<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_pool_enc<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_pool_enc<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t pool_join_launch(int tpi, const PoolEncParams& p, int grid, hipStream_t st) {
  const size_t lds = pool_lds_bytes();
  if (tpi == 2) hipLaunchKernelGGL(k_pool_join<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_pool_join<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_pool_join<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t pool_split_launch(int tpi, const PoolSplitParams& p, int grid, hipStream_t st) {
  const size_t lds = pool_lds_bytes();
  if (tpi == 2) hipLaunchKernelGGL(k_pool_split<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_pool_split<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_pool_split<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
