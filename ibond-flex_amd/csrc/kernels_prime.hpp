// Key generation's prime search (gmpy_math.py:77-87 getprimeover -> gmpy2.next_prime; keypair.py:93-127): the
// strong-probable-prime test of _bigint.is_probable_prime, one (candidate, base) pair per DPP row of 16 lanes, on the
// row engine of kernels_crtw.hpp (its CIOS steps, normalize and sub). A key does not exist yet, so nothing comes from a
// context: every row has its own modulus and derives its own Montgomery constants.
//
//   k_mr_w<K>   work item w = (start index, offset, base a): n = x[start] + offset (odd, bit BITS - 1 set, below
//               2^BITS: the host's sieve guarantees it), m' = -n^-1 mod 2^28 by Newton on limb 0, R mod n (R = 2^(28 K))
//               from 2^(BITS - 1) < n by doublings with a conditional subtraction, a R mod n from R mod n by double
//               and add over a's bits, n - 1 = 2^s d in the row's LDS slot, y = a^d by a fixed 4-bit window (the
//               table a^0..a^15 in Montgomery form in 16 LDS slots of the row; every digit multiplies, digit 0 by
//               R mod n, so the loop is the same for every row of the wave), then the verdict: y == 1 or y == n - 1,
//               or n - 1 met within s - 1 squarings (the wave squares to its largest s, finished rows predicated
//               off). One uint8 per work item.
//
// K = 10, 19, 37, 74 limbs for 256-, 512-, 1024- and 2048-bit candidates. One wave per block, four rows.
#pragma once
#include "kernels_crtw.hpp"

namespace fpai {
namespace prime {

using crtw::BLOCK_W;
using crtw::GPW;
using crtw::TPI;

// The row's geometry, as crtw::Geom, but never fewer than two limbs per lane: the rotating CIOS step hands a carry to
// the lane's NEXT accumulator, so one limb per lane (K = 10 would give that) has nowhere to keep it.
template <int K>
struct Geom {
  static constexpr int LW = crtw::Geom<K>::LW < 2 ? 2 : crtw::Geom<K>::LW;
  static constexpr int W = TPI * LW;
};

// a <- a B R^-1 mod m (crtw::mont on this geometry): a < 2m, B < 2m -> result < 2m, R = 2^(28 K) > 4m
template <int K>
__device__ __forceinline__ void mont(uint32_t (&a)[Geom<K>::LW], const uint32_t* B, const uint32_t (&m)[Geom<K>::LW],
                                     uint32_t mprime, int lane, int tig) {
  constexpr int LW = Geom<K>::LW;
  uint64_t P[LW];
#pragma unroll
  for (int i = 0; i < LW; ++i) P[i] = 0ull;
  crtw::steps<K, LW>(P, a, B, m, mprime, std::make_integer_sequence<int, K>{});
  crtw::normalize<LW, K % LW>(P, a, lane, tig);
}

template <int K>
constexpr int bits_of() { return K == 10 ? 256 : K == 19 ? 512 : K == 37 ? 1024 : 2048; }

constexpr int WIN = 4;                  // exponent window (bits)
constexpr int NTAB = 1 << WIN;          // a^0 .. a^15
constexpr int NSLOT = NTAB + 2;         // the table, the squaring operand, n - 1

struct Params {
  const uint32_t* x;        // [nstarts][BITS / 32] little-endian words of the starts
  const uint32_t* work;     // [nwork][3]: start index, offset, base
  long long nwork;
  int nstarts;
  uint8_t* verdict;         // [nwork]: 1 = strong probable prime to the base
};

// row-uniform: a == b over the row's limbs
template <int LW>
__device__ __forceinline__ bool row_eq(const uint32_t (&a)[LW], const uint32_t (&b)[LW], int lane, int tig) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < LW; ++i) o |= a[i] ^ b[i];
  return ((ballot(o != 0u) >> (lane - tig)) & 0xFFFFull) == 0ull;
}

// t <- t - n when t >= n (t < 2n)
template <int LW>
__device__ __forceinline__ void cond_sub(uint32_t (&t)[LW], const uint32_t (&n)[LW], int lane, int tig) {
  uint32_t d[LW];
  if (!crtw::sub<LW>(t, n, d, lane, tig)) {
#pragma unroll
    for (int i = 0; i < LW; ++i) t[i] = d[i];
  }
}

// t <- 2 t mod n (t < n)
template <int LW>
__device__ __forceinline__ void dbl_mod(uint32_t (&t)[LW], const uint32_t (&n)[LW], int lane, int tig) {
  uint64_t P[LW];
#pragma unroll
  for (int i = 0; i < LW; ++i) P[i] = (uint64_t)t[i] << 1;
  crtw::normalize<LW, 0>(P, t, lane, tig);
  cond_sub<LW>(t, n, lane, tig);
}

// WIN bits of the exponent slot (28-bit limbs, SW words) from bit position pos; zero above the slot
template <int SW>
__device__ __forceinline__ uint32_t exp_digit(const uint32_t* E, int pos) {
  const int k = pos / LB, sh = pos - k * LB;
  const uint32_t lo = k < SW ? E[k] : 0u;
  const uint32_t hi = k + 1 < SW ? E[k + 1] : 0u;
  return (uint32_t)(((((uint64_t)hi << LB) | lo) >> sh) & (NTAB - 1));
}

template <int K>
__global__ __launch_bounds__(BLOCK_W) void k_mr_w(Params p) {
  constexpr int LW = Geom<K>::LW, SW = Geom<K>::W;
  constexpr int BITS = bits_of<K>(), XW = BITS / 32;
  static_assert(LB * K >= BITS + 2, "R > 4 n");
  static_assert(BITS % WIN == 0 && SW % 4 == 0, "window digits, 16-byte slots");
  __shared__ __attribute__((aligned(16))) uint32_t sm[GPW * NSLOT * SW];
  const int lane = threadIdx.x, tig = lane & (TPI - 1), g = lane / TPI;
  uint32_t* T = sm + g * NSLOT * SW;        // a^k R mod n at T + k SW
  uint32_t* SQ = T + NTAB * SW;
  uint32_t* E = SQ + SW;                    // n - 1
  for (long long base = (long long)blockIdx.x * GPW; base < p.nwork; base += (long long)gridDim.x * GPW) {
    const long long w = base + g;
    const bool valid = w < p.nwork;
    const long long ww = valid ? w : p.nwork - 1;
    uint32_t si = p.work[ww * 3];
    const uint32_t off = p.work[ww * 3 + 1], a = p.work[ww * 3 + 2];
    if (si >= (uint32_t)p.nstarts) si = 0u;
    // n = x[start] + offset: the carry ripples over the row through normalize's look-ahead
    uint32_t n[LW];
    {
      const uint32_t* xs = p.x + (size_t)si * XW;
      uint64_t P[LW];
#pragma unroll
      for (int j = 0; j < LW; ++j) {
        const int bit = (tig * LW + j) * LB, wi = bit >> 5, sh = bit & 31;
        const uint64_t lo = wi < XW ? (uint64_t)xs[wi] : 0ull;
        const uint64_t hi = wi + 1 < XW ? (uint64_t)xs[wi + 1] : 0ull;
        P[j] = (uint64_t)((uint32_t)(((hi << 32) | lo) >> sh) & LMASK);
      }
      if (tig == 0) P[0] += off;
      crtw::normalize<LW, 0>(P, n, lane, tig);
    }
    // m' = -n^-1 mod 2^28
    uint32_t mprime;
    {
      const uint32_t n0 = bcast0<TPI>(n[0]);
      uint32_t v = 1u;
#pragma unroll
      for (int i = 0; i < 6; ++i) v *= 2u - n0 * v;
      mprime = (0u - v) & LMASK;
    }
    // R mod n from 2^(BITS - 1) < n
    uint32_t oneR[LW];
#pragma unroll
    for (int j = 0; j < LW; ++j) {
      constexpr int tb = BITS - 1;
      oneR[j] = (tig * LW + j == tb / LB) ? 1u << (tb % LB) : 0u;
    }
    for (int i = 0; i < LB * K - (BITS - 1); ++i) dbl_mod<LW>(oneR, n, lane, tig);
    // a R mod n: double and add over a's bits, from the wave's highest set bit
    uint32_t aR[LW];
#pragma unroll
    for (int j = 0; j < LW; ++j) aR[j] = 0u;
    {
      int hb = 31;
      while (hb > 0 && ballot(((a >> hb) & 1u) != 0u) == 0ull) --hb;
      for (int b = hb; b >= 0; --b) {
        dbl_mod<LW>(aR, n, lane, tig);
        uint64_t P[LW];
        const uint32_t bit = (a >> b) & 1u;
#pragma unroll
        for (int j = 0; j < LW; ++j) P[j] = (uint64_t)aR[j] + (bit ? oneR[j] : 0u);
        crtw::normalize<LW, 0>(P, aR, lane, tig);
        cond_sub<LW>(aR, n, lane, tig);
      }
    }
    // n - 1 (n is odd) to the row's slot; s = its trailing zeros
    int s;
    {
      uint32_t e[LW];
#pragma unroll
      for (int j = 0; j < LW; ++j) e[j] = n[j];
      if (tig == 0) e[0] &= ~1u;
      crtw::put<LW, SW>(E, e, tig);
      int pos = 0x7FFFFFFF;
#pragma unroll
      for (int j = LW - 1; j >= 0; --j)
        if (e[j] != 0u) pos = (tig * LW + j) * LB + __builtin_ctz(e[j]);
      const uint32_t nz = (uint32_t)(ballot(pos != 0x7FFFFFFF) >> (lane - tig)) & 0xFFFFu;   // nonzero: bit BITS - 1 is set
      const int first = nz ? __builtin_ctz(nz) : 0;
      s = min(__shfl(pos, (lane - tig) + first), BITS);
    }
    // The table a^k R mod n (k = 0..15), then y = a^d with d = (n - 1) >> s < 2^BITS: BITS / 4 digits from the top,
    // four squarings and one product each. One loop, so that the kernel holds one copy of the unrolled product:
    // steps 0..NTAB - 3 are the table's products by a R, the rest are the digits below the top one.
    uint32_t acc[LW];
    crtw::put<LW, SW>(T, oneR, tig);
    crtw::put<LW, SW>(T + SW, aR, tig);
#pragma unroll
    for (int j = 0; j < LW; ++j) acc[j] = aR[j];
    constexpr int NTB = NTAB - 2, ND = BITS / WIN;
#pragma unroll 1
    for (int it = 0; it < NTB + ND - 1; ++it) {
      const bool tab = it < NTB;
      const int nsq = tab ? 0 : WIN;
#pragma unroll 1
      for (int q = 0; q <= nsq; ++q) {
        const uint32_t* B = SQ;
        if (q < nsq) crtw::put<LW, SW>(SQ, acc, tig);
        else B = tab ? T + SW : T + exp_digit<SW>(E, s + (ND - 2 - (it - NTB)) * WIN) * SW;
        mont<K>(acc, B, n, mprime, lane, tig);
      }
      if (tab) crtw::put<LW, SW>(T + (it + 2) * SW, acc, tig);
      if (it == NTB - 1) crtw::get<LW>(T + exp_digit<SW>(E, s + BITS - WIN) * SW, acc, tig);
    }
    // the verdict, on canonical values in Montgomery form: 1 is R mod n, n - 1 is n - R mod n
    uint32_t negR[LW], y[LW];
    (void)crtw::sub<LW>(n, oneR, negR, lane, tig);
#pragma unroll
    for (int j = 0; j < LW; ++j) y[j] = acc[j];
    cond_sub<LW>(y, n, lane, tig);
    const bool is1 = row_eq<LW>(y, oneR, lane, tig), ism1 = row_eq<LW>(y, negR, lane, tig);
    bool pass = is1 || ism1;
    for (int r = 1;; ++r) {
      const bool active = !pass && r < s;
      if (ballot(active) == 0ull) break;
      crtw::put<LW, SW>(SQ, acc, tig);
      mont<K>(acc, SQ, n, mprime, lane, tig);
#pragma unroll
      for (int j = 0; j < LW; ++j) y[j] = acc[j];
      cond_sub<LW>(y, n, lane, tig);
      const bool hit = row_eq<LW>(y, negR, lane, tig);
      pass = pass || (active && hit);
    }
    if (valid && tig == 0) p.verdict[w] = pass ? 1u : 0u;
  }
}

}  // namespace prime
}  // namespace fpai
