// Host interface of the 16-lane-row fold translation unit (engine_foldw.hip, kernels_foldw.hpp).
#pragma once
#include "kernels_pack.hpp"

namespace fpai {

// true where a row kernel exists for n^2 of k limbs (74, 148, 296: the sizes of k_pe_w)
constexpr bool foldw_has(int k) { return k == 74 || k == 148 || k == 296; }
// k_pack_fold_w<k> over p.n outputs, four per block; hipErrorInvalidValue for other sizes
hipError_t foldw_launch(int k, const PackFoldParams& p, hipStream_t st);

}  // namespace fpai
