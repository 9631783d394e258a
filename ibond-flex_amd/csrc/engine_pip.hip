// Bucket-method kernels (kernels_pip.hpp): instantiations, geometry and launches.
#include "engine_pip.hpp"

#include <algorithm>

namespace fpai {

namespace {

constexpr size_t slot_lds_bytes() { return (size_t)BLOCK * L * 4; }   // one S-limb slot per lane group

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

// one launch of a lane-group kernel template at the context's group size
#define PIP_LAUNCH(KERNEL, units)                                                                                      \
  do {                                                                                                                 \
    const size_t lds = slot_lds_bytes();                                                                               \
    if (tpi == 2) hipLaunchKernelGGL(KERNEL<2>, dim3(grid_for(units, 2, blocks_per_cu(KERNEL<2>, lds), cus)), dim3(BLOCK), lds, st, p); \
    else if (tpi == 4) hipLaunchKernelGGL(KERNEL<4>, dim3(grid_for(units, 4, blocks_per_cu(KERNEL<4>, lds), cus)), dim3(BLOCK), lds, st, p); \
    else if (tpi == 8) hipLaunchKernelGGL(KERNEL<8>, dim3(grid_for(units, 8, blocks_per_cu(KERNEL<8>, lds), cus)), dim3(BLOCK), lds, st, p); \
    else return hipErrorInvalidValue;                                                                                  \
    return hipGetLastError();                                                                                          \
  } while (0)

}  // namespace

hipError_t pip_scan_launch(const PipScanParams& p, int cus, hipStream_t st) {
  const int grid = (int)std::max<long long>(1, std::min<long long>(p.Np, 8ll * cus));
  hipLaunchKernelGGL(k_pip_scan<0>, dim3(grid), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t pip_plan_launch(const PipPlanParams& p, int cus, hipStream_t st) {
  const size_t lds = pip_plan_lds_bytes(p.w, p.nwin);
  if (lds > ((size_t)64 << 10)) {   // above the 64 KiB a launch gets unasked: the CU's 160 KiB, one block per CU
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pip_plan<0>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long long per_cu = std::max<long long>(1, ((long long)160 << 10) / (long long)lds);
  const int grid = (int)std::max<long long>(1, std::min<long long>(p.nob, std::min<long long>(per_cu, 8) * cus));
  hipLaunchKernelGGL(k_pip_plan<0>, dim3(grid), dim3(256), lds, st, p);
  return hipGetLastError();
}

hipError_t pip_acc_launch(int tpi, const PipAccParams& p, long long max_units, int cus, hipStream_t st) {
  PIP_LAUNCH(k_pip_acc, max_units);
}

hipError_t pip_red_launch(int tpi, const PipRedParams& p, int cus, hipStream_t st) {
  PIP_LAUNCH(k_pip_red, p.nob * 2 * p.nwin);
}

hipError_t pip_horner_launch(int tpi, const PipHornerParams& p, int cus, hipStream_t st) {
  PIP_LAUNCH(k_pip_horner, p.nob * 2);
}

}  // namespace fpai
