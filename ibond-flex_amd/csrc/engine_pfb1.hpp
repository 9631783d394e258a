// Host interface of the 1024-bit public-key fixed-base unit (engine_pfb1.hip, kernels_pfb1.hpp).
#pragma once
#include "kernels_pfb1.hpp"

namespace fpai {

// blocks per CU of k_pfb1 (64 KB of LDS per block, 256 VGPRs per lane: two)
int pfb1_occupancy(int* occ);
// per-key construction on `st`: k_pfb1_chain, k_pfb1_lohi, k_pfb1_fill
hipError_t pfb1_build(const Pfb1Const* d_c, int nbases, int K, int W, uint4* table, hipStream_t st);
// k_pfb1 on a grid of gx blocks
hipError_t pfb1_launch(const Pfb1Params& p, int gx, hipStream_t st);

}  // namespace fpai
