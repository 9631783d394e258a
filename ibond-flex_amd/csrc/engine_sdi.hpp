// Host interface of the device-list segmented weighted-sum translation unit (engine_sdi.hip, kernels_sdi.hpp).
#pragma once
#include "kernels_sdi.hpp"

namespace fpai {

// One block of one wave per row, as many blocks per CU as the row tables leave room for in LDS (4 / 3 / 2 at lane groups
// of 2 / 4 / 8), striding over the rows. hipErrorInvalidValue: unsupported group size.
hipError_t sdi_rows_launch(int tpi, const SdiRowsParams& p, int cus, hipStream_t st);
hipError_t sdi_fill_launch(const SdiFinParams& p, int cus, hipStream_t st);
hipError_t sdi_out_launch(const SdiFinParams& p, int cus, hipStream_t st);

}  // namespace fpai
