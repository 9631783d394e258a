// Sparse histogram kernels (kernels_shist.hpp): instantiations, geometry and launches.
#include "engine_shist.hpp"

#include <algorithm>

namespace fpai {

namespace {

template <typename K>
int shist_grid(K kernel, const SHistParams& p, int cus) {
  int occ = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 256, 0) != hipSuccess || occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  const long long tiles = (p.nnz + p.N + SHIST_TILE - 1) / SHIST_TILE;
  return (int)std::max<long long>(1, std::min<long long>(tiles, (long long)occ * cus));
}

}  // namespace

hipError_t shist_indptr_launch(const long long* indptr, long long N, unsigned* err, int cus, hipStream_t st) {
  const int g = (int)std::max<long long>(1, std::min<long long>((N + 255) / 256, 8ll * cus));
  hipLaunchKernelGGL(k_shist_indptr<0>, dim3(g), dim3(256), 0, st, indptr, N, err);
  return hipGetLastError();
}

hipError_t shist_count_launch(const SHistParams& p, int cus, hipStream_t st) {
  if (p.f1 <= p.f0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_shist_pass<0>, dim3(shist_grid(k_shist_pass<0>, p, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t shist_scatter_launch(const SHistParams& p, int cus, hipStream_t st) {
  if (p.f1 <= p.f0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_shist_pass<1>, dim3(shist_grid(k_shist_pass<1>, p, cus)), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace fpai
