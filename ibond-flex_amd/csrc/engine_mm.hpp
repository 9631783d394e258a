// Host interface of the fused matrix-product translation unit (engine_mm.hip, kernels_mm.hpp).
#pragma once
#include "kernels_mm.hpp"

namespace fpai {

// bytes of one ciphertext's window table (16 rows of S limbs) at group size tpi
constexpr size_t mm_entry_bytes(int tpi) { return (size_t)16 * tpi * L * 4; }
// Grids: the kernels' grid-stride loops over `units` lane groups, at most their resident blocks on `cus` CUs.
// hipErrorInvalidValue: unsupported group size.
hipError_t mm_sign_launch(const MmSignParams& p, int cus, hipStream_t st);
hipError_t mm_tab_launch(int tpi, const MmTabParams& p, int cus, hipStream_t st);
hipError_t mm_acc_launch(int tpi, const MmAccParams& p, int cus, hipStream_t st);

}  // namespace fpai
