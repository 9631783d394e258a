// Host interface of the pair-group public-key encryption unit for n of 2049..4096 bits (engine_pe4.hip, kernels_pe4.hpp).
#pragma once
#include "kernels_pe4.hpp"

namespace fpai {

struct Pe4Geom {
  int gx_pre = 0, gx_pow = 0, gx_fin = 0;   // blocks
  size_t scratch_bytes = 0;                  // k_pe4_pow's tiles: sized by its grid, not by the call
};
int pe4_geometry(int cus, long long chunk, Pe4Geom* g);
// k_pe4_pre, k_pe4_pow, k_pe4_fin on `st`; ev[0..3] nullable
hipError_t pe4_launch(const Pe4Params& p, const Pe4Geom& g, hipStream_t st, hipEvent_t* ev);

}  // namespace fpai
