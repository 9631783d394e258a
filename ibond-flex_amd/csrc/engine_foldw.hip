// The fold on 16-lane rows (kernels_foldw.hpp): instantiations and launch.
#include "engine_foldw.hpp"

#include <algorithm>

#include "kernels_foldw.hpp"

namespace fpai {

hipError_t foldw_launch(int k, const PackFoldParams& p, hipStream_t st) {
  const long long blocks = (p.n + crtw::GPW - 1) / crtw::GPW;
  const int gx = (int)std::min<long long>(blocks, 1ll << 20);
  if (k == 74) hipLaunchKernelGGL((crtw::k_pack_fold_w<74>), dim3(gx), dim3(crtw::BLOCK_W), 0, st, p);
  else if (k == 148) hipLaunchKernelGGL((crtw::k_pack_fold_w<148>), dim3(gx), dim3(crtw::BLOCK_W), 0, st, p);
  else if (k == 296) hipLaunchKernelGGL((crtw::k_pack_fold_w<296>), dim3(gx), dim3(crtw::BLOCK_W), 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fpai
