// Device-list segmented weighted-sum kernels (kernels_sdi.hpp): instantiations, geometry and launches.
#include "engine_sdi.hpp"

#include <algorithm>
#include <atomic>

namespace fpai {

namespace {

template <typename F>
hipError_t rows_launch(F kernel, int tpi, const SdiRowsParams& p, int cus, hipStream_t st) {
  const size_t lds = sdi_lds_bytes(tpi);
  if (lds > ((size_t)64 << 10)) {   // above the 64 KiB a launch gets unasked (lane groups of 8): asked for once per device
    static std::atomic<unsigned long long> asked{0};   // a bit per device; only k_sdi_rows<8> gets here
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!(asked.load(std::memory_order_acquire) >> dev & 1ull)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      asked.fetch_or(1ull << dev, std::memory_order_release);
    }
  }
  const long long per_cu = std::max<long long>(1, ((long long)160 << 10) / (long long)lds);
  const int grid = (int)std::max<long long>(1, std::min<long long>(p.rows, per_cu * cus));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SDI_WAVE), lds, st, p);
  return hipGetLastError();
}

int flat_grid(long long n, int cus) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8ll * cus)); }

}  // namespace

hipError_t sdi_rows_launch(int tpi, const SdiRowsParams& p, int cus, hipStream_t st) {
  if (tpi == 2) return rows_launch(k_sdi_rows<2>, 2, p, cus, st);
  if (tpi == 4) return rows_launch(k_sdi_rows<4>, 4, p, cus, st);
  if (tpi == 8) return rows_launch(k_sdi_rows<8>, 8, p, cus, st);
  return hipErrorInvalidValue;
}

hipError_t sdi_fill_launch(const SdiFinParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_sdi_fill<0>, dim3(flat_grid(p.nseg * p.W, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t sdi_out_launch(const SdiFinParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_sdi_out<0>, dim3(flat_grid(std::max(p.nseg * p.W, p.total), cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace fpai
