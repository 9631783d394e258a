// Host interface of the re-randomisation translation unit (engine_obf.hip, kernels_obf.hpp).
#pragma once
#include "kernels_obf.hpp"

namespace fpai {

// dynamic LDS bytes of k_obf_mul (one S-limb slot per lane group)
constexpr size_t obf_lds_bytes() { return (size_t)BLOCK * L * 4; }
// blocks per CU of k_obf_mul<tpi> (-1: unsupported group size)
int obf_occupancy(int tpi, int* occ);
hipError_t obf_launch(int tpi, const ObfMulParams& p, int grid, hipStream_t st);

}  // namespace fpai
