// Scan kernels (kernels_scan.hpp): instantiations, geometry and launches.
#include "engine_scan.hpp"

#include <algorithm>

namespace fpai {

namespace {

template <int TPI>
constexpr size_t scan_lds() {
  return (size_t)(BLOCK / TPI) * 2 * TPI * L * 4;   // the B slot and the parked accumulator of every group
}

template <int TPI>
int scan_occ() {
  int occ = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_scan<TPI>, BLOCK, scan_lds<TPI>()) != hipSuccess || occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  return occ;
}

template <int TPI>
hipError_t scan_launch_t(const ScanParams& p, int cus, hipStream_t st) {
  constexpr int GPB = BLOCK / TPI;
  const long long ninst = p.outer * p.tiles * p.inner;
  const int grid = (int)std::max<long long>(1, std::min<long long>((ninst + GPB - 1) / GPB, (long long)scan_occ<TPI>() * cus));
  hipLaunchKernelGGL(k_scan<TPI>, dim3(grid), dim3(BLOCK), scan_lds<TPI>(), st, p);
  return hipGetLastError();
}

}  // namespace

long long scan_slots(int tpi, int cus) {
  if (tpi == 2) return (long long)scan_occ<2>() * cus * (BLOCK / 2);
  if (tpi == 4) return (long long)scan_occ<4>() * cus * (BLOCK / 4);
  if (tpi == 8) return (long long)scan_occ<8>() * cus * (BLOCK / 8);
  return 0;
}

hipError_t scan_launch(int tpi, const ScanParams& p, int cus, hipStream_t st) {
  if (p.outer <= 0 || p.tiles <= 0 || p.inner <= 0) return hipSuccess;
  if (tpi == 2) return scan_launch_t<2>(p, cus, st);
  if (tpi == 4) return scan_launch_t<4>(p, cus, st);
  if (tpi == 8) return scan_launch_t<8>(p, cus, st);
  return hipErrorInvalidValue;
}

}  // namespace fpai
