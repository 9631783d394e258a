// Broadcast-multiply kernels (kernels_mulb.hpp): instantiations, geometry and launches.
#include "engine_mulb.hpp"

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

int grid_for(long long units, long long per_block, int occ, int cus) {
  return (int)std::max<long long>(1, std::min<long long>((units + per_block - 1) / per_block, (long long)occ * cus));
}

template <int TPI>
void tab_launch(MulbTabParams p, int cus, hipStream_t st) {
  const size_t lds = (size_t)BLOCK * L * 4;
  const int occ = blocks_per_cu(k_mulb_tab<TPI>, lds);
  for (p.phase = 0; p.phase < 2; ++p.phase) {
    const long long units = p.phase ? p.nb * MULB_WIN : p.nb;
    hipLaunchKernelGGL(k_mulb_tab<TPI>, dim3(grid_for(units, BLOCK / TPI, occ, cus)), dim3(BLOCK), lds, st, p);
  }
}

template <int TPI>
void acc_launch(const MulbAccParams& p, int cus, hipStream_t st) {
  const size_t lds = mulb_acc_lds_bytes(TPI);
  const long long units = p.nb * ((p.F + 64 / TPI - 1) / (64 / TPI));   // one wave each
  hipLaunchKernelGGL(k_mulb_acc<TPI>, dim3(grid_for(units, BLOCK / 64, blocks_per_cu(k_mulb_acc<TPI>, lds), cus)),
                     dim3(BLOCK), lds, st, p);
}

}  // namespace

hipError_t mulb_plan_launch(const MulbPlanParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_mulb_plan<0>, dim3(grid_for(p.N, 4, 8, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t mulb_tab_launch(int tpi, MulbTabParams p, int cus, hipStream_t st) {
  if (tpi == 2) tab_launch<2>(p, cus, st);
  else if (tpi == 4) tab_launch<4>(p, cus, st);
  else if (tpi == 8) tab_launch<8>(p, cus, st);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t mulb_acc_launch(int tpi, const MulbAccParams& p, int cus, hipStream_t st) {
  if (tpi == 2) acc_launch<2>(p, cus, st);
  else if (tpi == 4) acc_launch<4>(p, cus, st);
  else if (tpi == 8) acc_launch<8>(p, cus, st);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
