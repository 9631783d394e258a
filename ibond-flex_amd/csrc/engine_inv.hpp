// Host interface of the modular inversion translation unit (engine_inv.hip, kernels_inv.hpp).
#pragma once
#include "kernels_inv.hpp"

namespace fpai {

// k_modinv over `count` values, one wave each (p.W in 1 .. MODINV_MAX_WORDS, count >= 1); with p.any_noinv set, the
// word is cleared on the stream first
hipError_t modinv_launch(const ModinvParams& p, int count, hipStream_t st);
// *word = 0 on the stream (a kernel, so that it can be captured)
hipError_t modinv_clear(uint32_t* word, hipStream_t st);
// registers per lane and waves per SIMD of k_modinv at W words, as the runtime reports them
hipError_t modinv_attributes(int W, int* vgprs, int* blocks_per_cu);

}  // namespace fpai
