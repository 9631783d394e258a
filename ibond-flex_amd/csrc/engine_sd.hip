// Segmented weighted-sum kernels (kernels_sd.hpp): instantiations, geometry and launches.
#include "engine_sd.hpp"

#include <algorithm>

namespace fpai {

namespace {

template <typename F>
int blocks_per_cu(F kernel, size_t lds) {
  int occ = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, BLOCK, lds) != hipSuccess || occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  return occ;
}

int grid_for(long long units, int tpi, int occ, int cus) {
  const long long gpb = BLOCK / tpi;
  return (int)std::max<long long>(1, std::min<long long>((units + gpb - 1) / gpb, (long long)occ * cus));
}

int flat_grid(long long n, int cus) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8ll * cus)); }

}  // namespace

hipError_t sd_sign_launch(const SdSignParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_sd_sign<0>, dim3(flat_grid(p.nnz, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t sd_gather_launch(const SdGatherParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_sd_gather<0>, dim3(flat_grid(p.n * p.ct_words, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t sd_acc_launch(int tpi, const SdAccParams& p, int cus, hipStream_t st) {
  const size_t lds = sd_acc_lds_bytes(tpi);
  const long long units = p.q1 - p.q0;
  if (tpi == 2) hipLaunchKernelGGL(k_sd_acc<2>, dim3(grid_for(units, 2, blocks_per_cu(k_sd_acc<2>, lds), cus)), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_sd_acc<4>, dim3(grid_for(units, 4, blocks_per_cu(k_sd_acc<4>, lds), cus)), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_sd_acc<8>, dim3(grid_for(units, 8, blocks_per_cu(k_sd_acc<8>, lds), cus)), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
