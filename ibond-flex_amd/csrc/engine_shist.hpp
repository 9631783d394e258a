// Host interface of the sparse histogram translation unit (engine_shist.hip, kernels_shist.hpp).
#pragma once
#include "kernels_shist.hpp"

namespace fpai {

// grid: the rows up to 8 blocks per CU
hipError_t shist_indptr_launch(const long long* indptr, long long N, unsigned* err, int cus, hipStream_t st);
// Grids: the tiles of nnz + N units up to the resident blocks (occupancy query x CUs).
// hipErrorInvalidValue: an empty feature range.
hipError_t shist_count_launch(const SHistParams& p, int cus, hipStream_t st);
hipError_t shist_scatter_launch(const SHistParams& p, int cus, hipStream_t st);

}  // namespace fpai
