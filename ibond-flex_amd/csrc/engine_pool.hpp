// Host interface of the obfuscator-pool translation unit (engine_pool.hip, kernels_pool.hpp).
#pragma once
#include "kernels_pool.hpp"

namespace fpai {

// dynamic LDS bytes of the three kernels: one S-limb slot per lane group
constexpr size_t pool_lds_bytes() { return (size_t)BLOCK * L * 4; }
// blocks per CU of k_pool_enc<tpi> (which: 0), k_pool_join<tpi> (1), k_pool_split<tpi> (2); -1: unsupported group size
int pool_occupancy(int tpi, int which, int* occ);
hipError_t pool_enc_launch(int tpi, const PoolEncParams& p, int grid, hipStream_t st);
hipError_t pool_join_launch(int tpi, const PoolEncParams& p, int grid, hipStream_t st);
hipError_t pool_split_launch(int tpi, const PoolSplitParams& p, int grid, hipStream_t st);

}  // namespace fpai
