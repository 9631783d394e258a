// Host interface of the split-pair CRT encryption unit for 2049..4096-bit key holders (engine_crt4.hip, kernels_crt4.hpp).
#pragma once
#include <algorithm>

#include "kernels_crt4.hpp"

namespace fpai {

struct Crt4Geom {
  int gx_a = 0, gx_b = 0;      // blocks per half: k_crt4_a (LANE_BLOCK elements each), k_crt4_b (D4_PAIRS each)
  size_t scratch_bytes = 0;    // per-lane tiles, sized by the larger grid
};
int crt4_geometry(int cus, long long chunk, Crt4Geom* g);
// k_crt4_a (p.y <- stage A), then k_crt4_b (p.u <- stage B), halves on blockIdx.y
hipError_t crt4_launch_a(const Crt4Params& p, const Crt4Geom& g, hipStream_t st);
hipError_t crt4_launch_b(const Crt4Params& p, const Crt4Geom& g, hipStream_t st);

}  // namespace fpai
