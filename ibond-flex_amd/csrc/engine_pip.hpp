// Host interface of the bucket-method translation unit (engine_pip.hip, kernels_pip.hpp).
#pragma once
#include "kernels_pip.hpp"

namespace fpai {

// The window of a call, from K alone. Product-count model per output, with nwin = ceil(64 / w) windows (a 53-bit
// float64 or 63-bit int64 magnitude and a few digits of alignment):
//
//   products(w) = nwin K  (accumulation)  +  2 nwin 2^w  (running sums)  +  nwin w  (Horner squarings)
//
//   w = 4: 16 K + 576    w = 5: 13 K + 897    w = 6: 11 K + 1474    w = 7: 10 K + 2630    w = 8: 8 K + 4160
//
// The smallest K at which each w is the cheapest (w = 7 never is: 8 passes it at K = 765, before 7 passes 6 at 1156):
struct PipWindow {
  long long min_k;
  int w;
};
constexpr PipWindow PIP_WINDOWS[] = {{0, 4}, {108, 5}, {289, 6}, {896, 8}};

inline int pip_window(long long K) {
  int w = PIP_WMIN;
  for (const PipWindow& e : PIP_WINDOWS)
    if (K >= e.min_k) w = e.w;
  return w;
}
// member slots per output: a 64-bit magnitude at any shift has non-zero digits in at most this many windows per term
inline long long pip_member_slots(long long K, int w) { return K * ((64 + w - 2) / w + 1); }
// units per output: ceil(members / PIP_RUN) summed over the cells is at most members / PIP_RUN + non-empty cells
inline long long pip_unit_slots(long long K, int w, int nwin) {
  const long long ms = pip_member_slots(K, w), cells = (2ll * nwin) << w;
  return ms / PIP_RUN + (ms < cells ? ms : cells) + 1;
}

// Grids: one block per output (scan, plan); the lane-group kernels' grid-stride loops over `units` groups, at most their
// resident blocks on `cus` CUs. hipErrorInvalidValue: unsupported group size.
hipError_t pip_scan_launch(const PipScanParams& p, int cus, hipStream_t st);
hipError_t pip_plan_launch(const PipPlanParams& p, int cus, hipStream_t st);
hipError_t pip_acc_launch(int tpi, const PipAccParams& p, long long max_units, int cus, hipStream_t st);
hipError_t pip_red_launch(int tpi, const PipRedParams& p, int cus, hipStream_t st);
hipError_t pip_horner_launch(int tpi, const PipHornerParams& p, int cus, hipStream_t st);

}  // namespace fpai
