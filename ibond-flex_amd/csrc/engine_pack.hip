// Packed-plaintext kernels (kernels_pack.hpp): instantiations and launches.
#include "engine_pack.hpp"

namespace fpai {

int pack_occupancy(int tpi, int* occ) {
  hipError_t e;
  if (tpi == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pack_mul<2>, BLOCK, pack_lds_bytes(2));
  else if (tpi == 4) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pack_mul<4>, BLOCK, pack_lds_bytes(4));
  else if (tpi == 8) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pack_mul<8>, BLOCK, pack_lds_bytes(8));
  else return -1;
  if (e != hipSuccess || *occ < 1) *occ = 1;
  return 0;
}

hipError_t pack_launch(int tpi, const PackMulParams& p, int grid, hipStream_t st) {
  const size_t lds = pack_lds_bytes(tpi);
  if (tpi == 2) hipLaunchKernelGGL(k_pack_mul<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_pack_mul<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_pack_mul<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

int fold_occupancy(int tpi, int* occ) {
  hipError_t e;
  if (tpi == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pack_fold<2>, BLOCK, fold_lds_bytes());
  else if (tpi == 4) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pack_fold<4>, BLOCK, fold_lds_bytes());
  else if (tpi == 8) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k_pack_fold<8>, BLOCK, fold_lds_bytes());
  else return -1;
  if (e != hipSuccess || *occ < 1) *occ = 1;
  return 0;
}

hipError_t fold_launch(int tpi, const PackFoldParams& p, int grid, hipStream_t st) {
  const size_t lds = fold_lds_bytes();
  if (tpi == 2) hipLaunchKernelGGL(k_pack_fold<2>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_pack_fold<4>, dim3(grid), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_pack_fold<8>, dim3(grid), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t unpack_launch(const UnpackParams& p, int grid, hipStream_t st) {
  hipLaunchKernelGGL(k_unpack<0>, dim3(grid), dim3(UNPACK_BLOCK), unpack_lds_bytes(p.pt_words), st, p);
  return hipGetLastError();
}

}  // namespace fpai
