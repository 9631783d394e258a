// Re-randomisation of ciphertext arrays (PaillierEncryptedNumber.apply_obfuscation, encrypted_number.py:58-63 ->
// obfuscator.py:23-37, over arrays): out_i = c_i s_i mod n^2 with s_i = r_i^n mod n^2 already computed by the
// encrypt chains (the encryption of the integer 0: c0 = 1, so E0 = r^n).
//
//   k_obf_mul<TPI>   one element per group of TPI lanes, like k_add and k_mul (bn_group.hpp). Both operands are read
//                    into registers before the result is written, so `out` may be either of them (the in-place call
//                    of pai_obfuscate_dev, and the out-of-place one whose r^n was written straight into `out`).
//                    Operands come in through the group's LDS slot (stage_words_to_limbs, as in k_add: rows 16-byte
//                    aligned where ct_words % 4 == 0) and s only when it becomes the multiplicand: 4 VGPRs spilled,
//                    against 319 with both operands unpacked by words_to_limbs ahead of the products.
//
// No exponents: the product keeps the exponent of c, so no alignment can go wrong and none of k_add's schedule sort
// (memset, plan, scan, scatter) is launched. Cost: two Montgomery products of S limbs, (c R^2 R^-1) s R^-1 = c s.
#pragma once
#include "kernels.hpp"

namespace fpai {

struct ObfMulParams {
  const uint32_t* c;      // [n][W] ciphertext words, each < n^2
  const uint32_t* s;      // [n][W] r^n mod n^2 words
  uint32_t* out;          // [n][W]; may alias c or s
  long long n;
  const uint32_t* N;      // n^2, limbs (S)
  const uint32_t* R2;     // R^2 mod n^2
  uint32_t mprime;
  int ct_words;
};

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_obf_mul(ObfMulParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    uint32_t a[L];
    stage_words_to_limbs<TPI>(slot, p.c + t * p.ct_words, p.ct_words, a, tig);
    // step 0: a <- c R^2 R^-1 = c R; step 1: a <- (c R) s R^-1 = c s (one montmul site, like run_program). s is read
    // only when it becomes the multiplicand, so it is never live across a product
#pragma unroll 1
    for (int step = 0; step < 2; ++step) {
      if (step == 0) {
        copy_g_to_lds<TPI>(slot, p.R2, tig);
      } else {
        uint32_t b[L];
        stage_words_to_limbs<TPI>(slot, p.s + t * p.ct_words, p.ct_words, b, tig);
        write_limbs_lds<TPI>(slot, b, tig);
      }
      montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
    }
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(slot, a, p.out + t * p.ct_words, p.ct_words, valid, tig);
  }
}

}  // namespace fpai
