// Host interface of the wide-integer translation unit (engine_big.hip, kernels_big.hpp).
#pragma once
#include "kernels_big.hpp"

namespace fpai {

// dynamic LDS bytes: k_big_c0 keeps a zero-fenced copy of n next to the groups' slots, k_mul_big the groups' exponents
constexpr size_t big_c0_lds_bytes(int tpi) { return ((size_t)BLOCK * L + (size_t)tpi * L * 3 / 2) * 4; }
constexpr size_t mul_big_lds_bytes(int tpi, int xw) { return ((size_t)BLOCK * L + (size_t)(BLOCK / tpi) * xw) * 4; }

// The window of k_mul_big for exponents of up to `bits` bits: the one with the fewest Montgomery products,
//   (2^w - 2) table products + ceil(bits / w) window products + bits squarings,
// among w = 1 .. BIG_WIN_MAX (a lane's tiles take 160 B x 2^w of scratch; ties go to the smaller table).
inline int big_window(int bits) {
  int best = 1;
  long long cost = -1;
  for (int w = 1; w <= BIG_WIN_MAX; ++w) {
    const long long c = ((1ll << w) - 2) + (bits + w - 1) / w;
    if (cost < 0 || c < cost) {
      cost = c;
      best = w;
    }
  }
  return best;
}

// blocks per CU of k_mul_big<tpi> (-1: unsupported group size)
int mul_big_occupancy(int tpi, int xw, int* occ);
hipError_t mul_big_launch(int tpi, const MulBigParams& p, int grid, hipStream_t st);
hipError_t big_c0_launch(int tpi, const BigC0Params& p, int cus, hipStream_t st);

}  // namespace fpai
