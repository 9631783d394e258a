// Host interface of the histogram translation unit (engine_hist.hip, kernels_hist.hpp).
#pragma once
#include "kernels_hist.hpp"

namespace fpai {

// Grids: x covers the samples up to the resident blocks (occupancy query x CUs), y the features of the launch.
// p.lds is set here from nodes * B. hipErrorInvalidValue: an empty feature range.
hipError_t hist_count_launch(HistParams p, int cus, hipStream_t st);
hipError_t hist_scatter_launch(HistParams p, int cus, hipStream_t st);
hipError_t hist_rows_launch(const HistRowsParams& p, int cus, hipStream_t st);
// one lane group per run, resident blocks by the occupancy query; hipErrorInvalidValue: unsupported group size
hipError_t hist_acc_launch(int tpi, const HistAccParams& p, int cus, hipStream_t st);

}  // namespace fpai
