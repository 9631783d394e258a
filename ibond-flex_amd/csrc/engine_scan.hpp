// Host interface of the scan translation unit (engine_scan.hip, kernels_scan.hpp).
#pragma once
#include "kernels_scan.hpp"

namespace fpai {

// Lane groups of k_scan<tpi> that the chip holds at once (occupancy query x CUs x groups per block); 0: unsupported
// group size.
long long scan_slots(int tpi, int cus);
// One lane group per (o, tile, i), resident blocks by the occupancy query. hipErrorInvalidValue: unsupported group size.
hipError_t scan_launch(int tpi, const ScanParams& p, int cus, hipStream_t st);

}  // namespace fpai
