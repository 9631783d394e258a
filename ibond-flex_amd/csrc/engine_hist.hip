// Histogram kernels (kernels_hist.hpp): instantiations, geometry and launches.
#include "engine_hist.hpp"

#include <algorithm>

namespace fpai {

namespace {

template <typename F>
int blocks_per_cu(F kernel, size_t lds) {
  int occ = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 256, lds) != hipSuccess || occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  return occ;
}

// x blocks for `units` tiles of one feature, so that x * y fills the resident blocks once
dim3 hist_grid(long long units, long long feats, int occ, int cus) {
  const long long y = std::min<long long>(feats, 65535);
  const long long resident = (long long)occ * cus;
  const long long x = std::max<long long>(1, std::min<long long>(units, (resident + y - 1) / y));
  return dim3((unsigned)x, (unsigned)y);
}

size_t hist_lds(HistParams& p) {
  const long long nb = (long long)p.nodes * p.B;
  p.lds = nb <= HIST_LDS_CELLS ? 1 : 0;
  return p.lds ? (size_t)nb * 4 : 0;
}

}  // namespace

hipError_t hist_count_launch(HistParams p, int cus, hipStream_t st) {
  if (p.f1 <= p.f0) return hipErrorInvalidValue;
  const size_t lds = hist_lds(p);
  const dim3 g = hist_grid((p.N + 255) / 256, p.f1 - p.f0, blocks_per_cu(k_hist_count<0>, lds), cus);
  hipLaunchKernelGGL(k_hist_count<0>, g, dim3(256), lds, st, p);
  return hipGetLastError();
}

hipError_t hist_scatter_launch(HistParams p, int cus, hipStream_t st) {
  if (p.f1 <= p.f0) return hipErrorInvalidValue;
  const size_t lds = hist_lds(p);
  const dim3 g = hist_grid((p.N + HIST_TILE - 1) / HIST_TILE, p.f1 - p.f0, blocks_per_cu(k_hist_scatter<0>, lds), cus);
  hipLaunchKernelGGL(k_hist_scatter<0>, g, dim3(256), lds, st, p);
  return hipGetLastError();
}

hipError_t hist_rows_launch(const HistRowsParams& p, int cus, hipStream_t st) {
  const long long n = p.nruns * HIST_RUN;
  const int g = (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8ll * cus));
  hipLaunchKernelGGL(k_hist_rows<0>, dim3(g), dim3(256), 0, st, p);
  return hipGetLastError();
}

template <int TPI>
static hipError_t hist_acc_launch_t(const HistAccParams& p, int cus, hipStream_t st) {
  constexpr int GPB = BLOCK / TPI;
  const size_t lds = (size_t)GPB * TPI * L * 4;
  int occ = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_hist_acc<TPI>, BLOCK, lds) != hipSuccess || occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  const int grid = (int)std::max<long long>(1, std::min<long long>((p.nruns + GPB - 1) / GPB, (long long)occ * cus));
  hipLaunchKernelGGL(k_hist_acc<TPI>, dim3(grid), dim3(BLOCK), lds, st, p);
  return hipGetLastError();
}

hipError_t hist_acc_launch(int tpi, const HistAccParams& p, int cus, hipStream_t st) {
  if (p.nruns <= 0) return hipSuccess;
  if (tpi == 2) return hist_acc_launch_t<2>(p, cus, st);
  if (tpi == 4) return hist_acc_launch_t<4>(p, cus, st);
  if (tpi == 8) return hist_acc_launch_t<8>(p, cus, st);
  return hipErrorInvalidValue;
}

}  // namespace fpai
