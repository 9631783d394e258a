// Host interface of the segmented weighted-sum translation unit (engine_sd.hip, kernels_sd.hpp).
#pragma once
#include "kernels_sd.hpp"

namespace fpai {

// Grids as in engine_mm.hpp. hipErrorInvalidValue: unsupported group size.
hipError_t sd_sign_launch(const SdSignParams& p, int cus, hipStream_t st);
hipError_t sd_gather_launch(const SdGatherParams& p, int cus, hipStream_t st);
hipError_t sd_acc_launch(int tpi, const SdAccParams& p, int cus, hipStream_t st);

}  // namespace fpai
