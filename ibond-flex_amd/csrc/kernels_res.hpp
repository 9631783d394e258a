// Kernels of the device-resident ciphertext buffers: k_take (rows gathered by an index) and k_check_below (the
// wire-ingest range check). Both move or compare words only: no arithmetic on ciphertexts, plain C++, vector loads
// and stores.
#pragma once
#include "engine_res.hpp"

namespace fpai {

// out[j] = in[index[j]] (words and exponent); index[j] == -1 writes ciphertext 1 with exponent INT32_MIN. A work item
// is one VEC-word piece of an output row, consecutive lanes take consecutive pieces of a row (coalesced on both sides),
// and the grid strides over the pieces. VEC = 4 (16-byte loads and stores) needs W % 4 == 0 and 16-byte aligned bases:
// every row then starts on a 16-byte boundary; VEC = 1 serves every other width (W = 65 of a 1035-bit key).
template <int VEC>
__global__ void __launch_bounds__(RES_BLOCK) k_take(TakeParams p) {
  const long long per_row = p.W / VEC;
  const long long total = p.M * per_row;
  const long long step = (long long)gridDim.x * RES_BLOCK;
  for (long long t = (long long)blockIdx.x * RES_BLOCK + threadIdx.x; t < total; t += step) {
    const long long j = t / per_row;
    const int q = (int)(t - j * per_row);
    const long long src = p.index[j];
    if constexpr (VEC == 4) {
      uint4 v = make_uint4(q == 0 ? 1u : 0u, 0u, 0u, 0u);
      if (src >= 0) v = reinterpret_cast<const uint4*>(p.in + src * p.W)[q];
      reinterpret_cast<uint4*>(p.out + j * p.W)[q] = v;
    } else {
      uint32_t v = q == 0 ? 1u : 0u;
      if (src >= 0) v = p.in[src * p.W + q];
      p.out[j * p.W + q] = v;
    }
    if (q == 0) p.out_exp[j] = src >= 0 ? p.in_exp[src] : RES_EMPTY_EXP;
  }
}

// One lane per row, from the top limb down: the first limb that differs from the limit decides, so a row of a random
// residue costs one word. A row equal to the limit is not below it.
__global__ void __launch_bounds__(RES_BLOCK) k_check_below(CheckBelowParams p) {
  const long long step = (long long)gridDim.x * RES_BLOCK;
  for (long long i = (long long)blockIdx.x * RES_BLOCK + threadIdx.x; i < p.N; i += step) {
    const uint32_t* row = p.ct + i * p.W;
    bool bad = true;
    for (int w = p.W - 1; w >= 0; --w) {
      const uint32_t a = row[w], b = p.limit[w];
      if (a != b) {
        bad = a > b;
        break;
      }
    }
    if (bad) atomicMin(p.first, (unsigned long long)i);
  }
}

}  // namespace fpai
