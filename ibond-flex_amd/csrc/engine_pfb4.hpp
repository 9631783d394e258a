// Host interface of the 2049..4096-bit public-key fixed-base unit (engine_pfb4.hip, kernels_pfb4.hpp).
#pragma once
#include "kernels_pfb4.hpp"

namespace fpai {

// blocks per CU of k_pfb4 (PFB4_LDS = 76.6 KB of LDS per block: two)
int pfb4_occupancy(int* occ);
// per-key construction on `st`: k_pfb4_chain, k_pfb4_lohi, k_pfb4_fill
hipError_t pfb4_build(const Pfb4Const* d_c, int nbases, int K, int W, uint32_t* table, hipStream_t st);
// k_pfb4 on a grid of gx blocks
hipError_t pfb4_launch(const Pfb4Params& p, int gx, hipStream_t st);

}  // namespace fpai
