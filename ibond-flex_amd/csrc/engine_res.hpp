// Host interface of the resident-buffer translation unit (engine_res.hip; the kernels: kernels_res.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fpai {

constexpr int RES_BLOCK = 256;
constexpr int32_t RES_EMPTY_EXP = INT32_MIN;   // the exponent of the identity (ciphertext 1): an empty segment's

struct TakeParams {
  const uint32_t* in;      // [N][W]
  const int32_t* in_exp;   // [N]
  const long long* index;  // [M], every entry -1 or in [0, N): checked on the host before the launch
  long long M;
  int W;
  uint32_t* out;           // [M][W]
  int32_t* out_exp;        // [M]
};

struct CheckBelowParams {
  const uint32_t* ct;         // [N][W]
  long long N;
  int W;
  const uint32_t* limit;      // [W] little-endian 32-bit words of n^2
  unsigned long long* first;  // set to ~0 before the launch; the smallest i with ct[i] >= limit
};

// grids are capped at 8 blocks per CU and stride over the work
hipError_t take_launch(const TakeParams& p, int cus, hipStream_t st);
hipError_t check_below_launch(const CheckBelowParams& p, int cus, hipStream_t st);

}  // namespace fpai
