// Modular inversion by a binary extended GCD that takes 31 steps at a time (kernels_inv.hpp k_modinv): the parts that
// touch no multi-word number, host and device, no HIP needed. tests/cpu/modinv_check.cpp drives them through a plain
// C++ outer loop; the kernel drives them with the numbers spread over a wavefront.
//
// The scheme is T. Pornin's "Optimized Binary GCD for Modular Inversion" (IACR ePrint 2020/972, Algorithm 2) with
// k = 32. State: a, b (x and m at the start, b always odd) and u, v (1 and 0) with a = x u, b = x v (mod m). One round:
//   1. n = max(len(a), len(b)). Two 64-bit words stand for a and b: their low 31 bits under their bits n-33 .. n-1
//      (the numbers themselves while n <= 64).                                             modinv_approx
//   2. 31 steps of the binary GCD on the two words alone: if a is odd { if a < b swap; a -= b }; a /= 2. The low 31
//      bits decide every parity exactly, the top 33 bits decide the comparisons almost always like the full numbers
//      would. The steps are recorded as a matrix: 2^31 a' = f0 a + g0 b, 2^31 b' = f1 a + g1 b.    modinv_steps31
//   3. The matrix is applied to the full numbers, exactly. A comparison that the approximation got wrong shows as a
//      negative a' or b': it is negated together with its matrix row.
//   4. The same rows are applied to (u, v) modulo m, the division by 2^31 done as one Montgomery step. modinv_row_k
// Rows: |f| + |g| <= 2^31 in each row, and f g <= 0 (the rows start as (1, 0), (0, 1), a step subtracts the row of the
// other sign pattern or swaps the two), so a row applied to (P, N) is +-(cp P - cn N) with two unsigned coefficients of
// at most 2^31: no signed multi-word arithmetic anywhere.                                          modinv_row_plan
//
// Round count. One step of the exact binary GCD lowers len(a) + len(b) by at least one while a != 0, from at most
// 2 len(m) to 1 (a = 0, b = gcd), so 2 len(m) - 1 steps always suffice; Pornin's section 3 shows the same total for the
// approximated steps (a round of k - 1 = 31 steps lowers len(a) + len(b) by at least 31 while a != 0; the proof needs
// b odd, x < m and the 33 + 31 bit split used here). Rounds past the end change nothing: with a = 0 the matrix is
// (1, 0; 0, 2^31) and the Montgomery step returns v itself. So the count is fixed by len(m) alone, with no exit that
// depends on x.                                                                                     modinv_rounds
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MODINV_HD __host__ __device__ __forceinline__
#else
#define MODINV_HD inline
#endif

namespace fpai {

constexpr int MODINV_K = 31;   // steps per round

// rounds for a modulus of mbits bits (mbits >= 1)
MODINV_HD int modinv_rounds(int mbits) { return (2 * mbits - 1 + MODINV_K - 1) / MODINV_K; }

// -m^-1 mod 2^31 for odd m (its low word suffices): Newton's iteration, 5 bits -> 10 -> 20 -> 40
MODINV_HD uint32_t modinv_neg_minv31(uint32_t m0) {
  uint32_t y = m0 * 3u ^ 2u;   // 5 correct bits
  y *= 2u - m0 * y;
  y *= 2u - m0 * y;
  y *= 2u - m0 * y;
  return (0u - y) & 0x7fffffffu;
}

// The word that stands for a number in a round. lo: its words 0 and 1; hi: its words jt and jt - 1, jt >= 1 the index of
// the top non-zero word of a | b; s = 32 - clz(that word of a | b), 1 .. 32.
MODINV_HD uint64_t modinv_approx(uint64_t lo, uint64_t hi, int jt, int s) {
  if (jt <= 1) return lo;                                   // n <= 64: exact
  return ((hi >> (s - 1)) << 31) | (lo & 0x7fffffffull);    // bits n-33 .. n-1 over bits 0 .. 30
}

struct ModinvMat {
  int64_t f0, g0, f1, g1;   // each in [-2^31, 2^31]
};

MODINV_HD ModinvMat modinv_steps31(uint64_t xa, uint64_t xb) {
  int64_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
#pragma unroll 1
  for (int i = 0; i < MODINV_K; ++i) {
    const bool odd = (xa & 1u) != 0;
    if (odd && xa < xb) {
      const uint64_t t = xa; xa = xb; xb = t;
      const int64_t tf = f0; f0 = f1; f1 = tf;
      const int64_t tg = g0; g0 = g1; g1 = tg;
    }
    if (odd) {
      xa -= xb;
      f0 -= f1;
      g0 -= g1;
    }
    xa >>= 1;
    f1 += f1;
    g1 += g1;
  }
  return ModinvMat{f0, g0, f1, g1};
}

// A row (f, g), f g <= 0, applied to a pair (A, B) is sgn (cp P - cn N): P is B when p_is_b, else A; N the other.
// flip: the caller found the result negative on (a, b) and negates the row.
struct ModinvRow {
  uint32_t cp, cn;   // <= 2^31 each, cp + cn <= 2^31
  bool p_is_b;
};
MODINV_HD ModinvRow modinv_row_plan(int64_t f, int64_t g, bool flip) {
  if (flip) { f = -f; g = -g; }
  if (g > 0 || f < 0) return ModinvRow{(uint32_t)g, (uint32_t)(-f), true};
  return ModinvRow{(uint32_t)f, (uint32_t)(-g), false};
}

// The Montgomery step of cp P - cn N (P, N in [0, m)): t0 is the low word of that difference. The multiple of m that
// clears its low 31 bits is k m, 0 <= k < 2^31; where k >= 2^31 - cp the step adds (k - 2^31) m instead, as
// sub = 2^31 - k <= cp times -m, so that the quotient lies in (-m, m) and one conditional + m ends the reduction.
struct ModinvK {
  uint32_t k;      // coefficient of m (neg = false) or of -m (neg = true)
  bool neg;
};
MODINV_HD ModinvK modinv_row_k(uint32_t t0, uint32_t cp, uint32_t ninv31) {
  const uint32_t k = (t0 * ninv31) & 0x7fffffffu;
  if ((uint64_t)k + cp >= 0x80000000ull) return ModinvK{0x80000000u - k, true};
  return ModinvK{k, false};
}

}  // namespace fpai
