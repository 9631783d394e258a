// Host interface of the broadcast-multiply translation unit (engine_mulb.hip, kernels_mulb.hpp).
#pragma once
#include "kernels_mulb.hpp"

namespace fpai {

// bytes of one ciphertext's comb (16 windows of 16 rows of S limbs) at group size tpi
constexpr size_t mulb_entry_bytes(int tpi) { return mulb_entry_limbs(tpi) * 4; }
// Grids: the kernels' grid-stride loops, at most their resident blocks on `cus` CUs. mulb_tab_launch runs both phases.
// hipErrorInvalidValue: unsupported group size.
hipError_t mulb_plan_launch(const MulbPlanParams& p, int cus, hipStream_t st);
hipError_t mulb_tab_launch(int tpi, MulbTabParams p, int cus, hipStream_t st);
hipError_t mulb_acc_launch(int tpi, const MulbAccParams& p, int cus, hipStream_t st);

}  // namespace fpai
