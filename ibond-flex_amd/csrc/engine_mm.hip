// Fused matrix-product kernels (kernels_mm.hpp): instantiations, geometry and launches.
#include "engine_mm.hpp"

#include <algorithm>

namespace fpai {

namespace {

constexpr size_t tab_lds_bytes() { return (size_t)BLOCK * L * 4; }

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

}  // namespace

hipError_t mm_sign_launch(const MmSignParams& p, int cus, hipStream_t st) {
  const long long n = p.K * p.d;
  const int grid = (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8ll * cus));
  hipLaunchKernelGGL(k_mm_sign<0>, dim3(grid), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t mm_tab_launch(int tpi, const MmTabParams& p, int cus, hipStream_t st) {
  const size_t lds = tab_lds_bytes();
  const long long units = p.mb * p.kb * (p.has_neg ? 2 : 1);
  if (tpi == 2) hipLaunchKernelGGL(k_mm_tab<2>, dim3(grid_for(units, 2, blocks_per_cu(k_mm_tab<2>, lds), cus)), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_mm_tab<4>, dim3(grid_for(units, 4, blocks_per_cu(k_mm_tab<4>, lds), cus)), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_mm_tab<8>, dim3(grid_for(units, 8, blocks_per_cu(k_mm_tab<8>, lds), cus)), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t mm_acc_launch(int tpi, const MmAccParams& p, int cus, hipStream_t st) {
  const size_t lds = mm_acc_lds_bytes(tpi);
  const long long units = (p.kb + MM_KC - 1) / MM_KC * p.mb * p.d;
  if (tpi == 2) hipLaunchKernelGGL(k_mm_acc<2>, dim3(grid_for(units, 2, blocks_per_cu(k_mm_acc<2>, lds), cus)), dim3(BLOCK), lds, st, p);
  else if (tpi == 4) hipLaunchKernelGGL(k_mm_acc<4>, dim3(grid_for(units, 4, blocks_per_cu(k_mm_acc<4>, lds), cus)), dim3(BLOCK), lds, st, p);
  else if (tpi == 8) hipLaunchKernelGGL(k_mm_acc<8>, dim3(grid_for(units, 8, blocks_per_cu(k_mm_acc<8>, lds), cus)), dim3(BLOCK), lds, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
