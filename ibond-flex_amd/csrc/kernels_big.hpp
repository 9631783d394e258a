// Wide-integer plain operands (PAI_BIG): Python ints beyond 64 bits as [N][xw] little-endian 32-bit magnitude words plus
// a sign byte, always at exponent 0 (FixedPointNumber.encode of an int, fixedpoint_number.py:56-57, 67-69).
//
//   k_big_c0<TPI>   c0 = 1 + n M mod n^2 with M = |v| 16^E (v >= 0) or n - |v| 16^E (v < 0), E = max(e_x, 0) for
//                   E(x) + v (k_plain's rule) and 0 for an encryption. One element per group of TPI lanes. The group
//                   cuts the shifted magnitude into LB-bit limbs in its LDS slot, compares it against max_int limb for
//                   limb (sub_limbs: the reference's exact |M| > max_int), and forms the HALF-WIDTH product n x M by
//                   columns: lane t owns columns [L t, L t + L) of the result, walks the limbs M_k of the magnitude
//                   (an LDS broadcast per k) and multiplies each into the L limbs n_(col - k), read from a zero-fenced
//                   copy of n that the block shares in LDS. The walk ends at the wave's longest magnitude, so a call
//                   of 128-bit values does 5 x L multiply-accumulates per lane where a full-width one does S/2 x L.
//                   Accumulators are lazy 64-bit sums (at most S/2 = 148 products < 2^56 each); one normalize.
//   k_mul_big<TPI>  c^|k| mod n^2 for a per-element exponent of up to nb bits: left-to-right fixed window `win`
//                   (1..6, chosen per call by the host from the call's exponent width, engine_big.hpp) over exponent
//                   words that the group stages ONCE in LDS; 2^win per-lane tiles x^0 .. x^(2^win - 1) in global
//                   scratch as in k_mul; the window count is the wave maximum and shorter exponents run leading zero
//                   digits (tile 0 = R). Negative scalars set neg[t] for the caller's batch inversion, like k_mul.
#pragma once
#include "kernels.hpp"

namespace fpai {

constexpr int BIG_WIN_MAX = 6;   // 64 tiles of TROW words per lane

struct BigOperand {
  const uint32_t* x;      // [*][xw] magnitudes, element i at x + i xs xw
  const uint8_t* neg;     // [*] (nullable: all non-negative), element i at neg[i xs]
  int xw;                 // words per magnitude, 1 .. ct_words / 2
  long long xs;           // 1: one operand per element, 0: one for all
};

struct BigC0Params {
  BigOperand v;
  const int32_t* exp;     // nullable: ciphertext exponents e_x (E = max(e_x, 0)); null: E = 0
  long long n;
  uint32_t* c0;           // [n][W] out
  int32_t* e0;            // [n] out: E
  int32_t* status;        // [n] out (nullable): ST_OK or ST_ENC_RANGE
  const uint32_t* N;      // n^2, limbs (S)
  const uint32_t* nl;     // n, limbs (S, zero padded)
  const uint32_t* maxint; // n // 3 - 1, limbs (S, zero padded)
  int ct_words;
  int nb;                 // bits of n
};

// bits [b, b + LB) of the magnitude (b may be negative: the bits below 0 are zero)
__device__ __forceinline__ uint32_t big_limb_at(const uint32_t* __restrict__ x, int xw, int b) {
  const int wi = b >> 5, sh = b & 31;   // arithmetic shift: floor for negative b
  const uint64_t lo = (wi >= 0 && wi < xw) ? (uint64_t)x[wi] : 0ull;
  const uint64_t hi = (wi + 1 >= 0 && wi + 1 < xw) ? (uint64_t)x[wi + 1] : 0ull;
  return (uint32_t)(((hi << 32) | lo) >> sh) & LMASK;
}

// bit length of the group's magnitude (each lane scans words tig, tig + TPI, ..), uniform over the group
template <int TPI>
__device__ __forceinline__ int big_bits(const uint32_t* __restrict__ x, int xw, int tig) {
  int bits = 0;
  for (int j = tig; j < xw; j += TPI) {
    const uint32_t w = x[j];
    if (w) bits = 32 * j + 32 - __clz(w);
  }
#pragma unroll
  for (int s = TPI / 2; s >= 1; s >>= 1) bits = max(bits, __shfl_xor(bits, s));
  return bits;
}

// dynamic LDS of k_big_c0: [GPB slots of S limbs][S / 2 zero limbs][n: S limbs]
template <int TPI>
__global__ __launch_bounds__(BLOCK) void k_big_c0(BigC0Params p) {
  constexpr int S = TPI * L;
  constexpr int H = S / 2;                 // limbs of a magnitude that can pass the range test (nb <= LB H)
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t* nz = smem + GPB * S;           // nz[H + j] = n_j, nz[0 .. H) = 0: column - k may run below 0
  for (int j = threadIdx.x; j < H + S; j += BLOCK) nz[j] = j < H ? 0u : p.nl[j - H];
  __syncthreads();
  uint32_t m[L], mx[L];
  load_limbs_g<TPI>(p.N, m, tig);
  load_limbs_g<TPI>(p.maxint, mx, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long ii = valid ? inst : p.n - 1;
    const uint32_t* xv = p.v.x + ii * p.v.xs * p.v.xw;
    const int E = p.exp ? max(p.exp[ii], 0) : 0;
    const int vbits = big_bits<TPI>(xv, p.v.xw, tig);
    // more than nb bits after the shift is past max_int already, and 4 E must not wrap (k_plain's test)
    bool range = vbits != 0 && (E > p.nb / 4 || vbits + 4 * E > p.nb);
    const int mbits = (vbits == 0 || range) ? 0 : vbits + 4 * E;
    // |M| = |v| 2^(4E) as LB-bit limbs in the slot (zero where the value ends, and for a value out of range)
    wave_lds_fence();
    for (int k = tig; k < S; k += TPI) slot[k] = (k * LB < mbits) ? big_limb_at(xv, p.v.xw, k * LB - 4 * E) : 0u;
    wave_lds_fence();
    uint32_t X[L], Dn[L];
#pragma unroll
    for (int i = 0; i < L; ++i) X[i] = slot[tig * L + i];
    if (sub_limbs<TPI>(mx, X, Dn, lane, tig)) range = true;     // max_int < |M|: the reference's exact test
    const bool neg = !range && mbits != 0 && p.v.neg != nullptr && p.v.neg[ii * p.v.xs] != 0;
    int nk = range ? 0 : (mbits + LB - 1) / LB;                  // limbs to walk: the wave's longest magnitude
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) nk = max(nk, __shfl_xor(nk, s));
    uint64_t P[L];
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = 0;
    const uint32_t* ncol = nz + H + tig * L;                     // ncol[i - k] = n_(column i - k)
    for (int k = 0; k < nk; ++k) {
      const uint32_t mk = range ? 0u : slot[k];
#pragma unroll
      for (int i = 0; i < L; ++i) P[i] += (uint64_t)ncol[i - k] * mk;
    }
    uint32_t a[L];
    normalize<TPI>(P, X, lane, tig);                             // n |M| < n^2 / 3
    (void)sub_limbs<TPI>(m, X, Dn, lane, tig);                   // n^2 - n |M|
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = (uint64_t)(neg ? Dn[i] : X[i]) + ((tig == 0 && i == 0) ? 1u : 0u);
    normalize<TPI>(P, a, lane, tig);
    emit_words<TPI>(slot, a, p.c0 + ii * p.ct_words, p.ct_words, valid, tig);
    if (valid && tig == 0) {
      p.e0[ii] = E;
      if (p.status) p.status[ii] = range ? ST_ENC_RANGE : ST_OK;
    }
  }
}

struct MulBigParams {
  const uint32_t* ct;     // ciphertext words [n][W]
  const int32_t* exp;     // ciphertext exponents [n]
  BigOperand k;           // the scalars
  int win;                // window bits, 1 .. BIG_WIN_MAX
  long long n;
  uint32_t* out;          // [n][W]
  int32_t* out_exp;       // [n]: the ciphertext's exponent (an int encodes at exponent 0)
  int32_t* status;        // [n] (nullable): ST_OK or ST_ENC_RANGE (|k| > max_int: factor 1, like k_mul)
  uint8_t* neg;           // [n]: 1 where the term still needs the inversion
  const uint32_t* N;      // n^2
  const uint32_t* R2;     // R^2 mod n^2
  const uint32_t* oneR;   // R mod n^2
  const uint32_t* maxint; // n // 3 - 1, limbs (S, zero padded)
  uint32_t mprime;
  int ct_words;
  uint32_t* scratch;      // per-lane tiles: (TROW << win) words per lane
};

// digit `d` (win bits from bit d win) of an exponent of xw words in LDS
__device__ __forceinline__ int big_digit(const uint32_t* ew, int xw, int win, int d) {
  const int b = d * win, wi = b >> 5, sh = b & 31;
  const uint64_t lo = wi < xw ? (uint64_t)ew[wi] : 0ull, hi = wi + 1 < xw ? (uint64_t)ew[wi + 1] : 0ull;
  return (int)((((hi << 32) | lo) >> sh) & ((1u << win) - 1u));
}

// dynamic LDS of k_mul_big: [GPB slots of S limbs][GPB exponents of xw words]
template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_mul_big(MulBigParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  const int xw = p.k.xw, win = p.win;
  uint32_t* slot = smem + gib * S;
  uint32_t* ew = smem + GPB * S + gib * xw;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  uint32_t* tw = p.scratch + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * ((size_t)TROW << win);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    const uint32_t* kv = p.k.x + t * p.k.xs * xw;
    // the exponent words, once per group; then the exact |k| > max_int over the limbs
    wave_lds_fence();
    for (int j = tig; j < xw; j += TPI) ew[j] = kv[j];
    wave_lds_fence();
    uint32_t a[L], tt[L];
    bool range;
    {
      uint32_t mx[L];
      load_limbs_g<TPI>(p.maxint, mx, tig);
      words_to_limbs(ew, xw, a, tig);
      range = sub_limbs<TPI>(mx, a, tt, lane, tig);
    }
    if (range) {                                                 // factor 1: every digit reads as zero
      wave_lds_fence();
      for (int j = tig; j < xw; j += TPI) ew[j] = 0u;
      wave_lds_fence();
    }
    const int ebits = big_bits<TPI>(ew, xw, tig);
    const bool negs = ebits != 0 && p.k.neg != nullptr && p.k.neg[t * p.k.xs] != 0;
    int nw = (ebits + win - 1) / win;                            // windows, wave maximum
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) nw = max(nw, __shfl_xor(nw, s));
    if (nw == 0) {
      load_limbs_g<TPI>(p.oneR, a, tig);                                   // c^0 = 1 (Montgomery R)
    } else {
      // x~ = c R mod n^2; tiles: 0 -> R, d -> x~^d (d = 1 .. 2^win - 1)
      words_to_limbs(p.ct + t * p.ct_words, p.ct_words, a, tig);
      copy_g_to_lds<TPI>(slot, p.R2, tig);
      montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
      load_limbs_g<TPI>(p.oneR, tt, tig);
      tile_store(tw, 0, tt, lane);
      tile_store(tw, 1, a, lane);
      write_limbs_lds<TPI>(slot, a, tig);
#pragma unroll
      for (int q = 0; q < L; ++q) tt[q] = a[q];
      for (int dd = 2; dd < (1 << win); ++dd) {
        montmul<TPI>(tt, tt, slot, TPI, m, p.mprime, lane, tig);
        tile_store(tw, dd, tt, lane);
      }
      tile_load(tw, big_digit(ew, xw, win, nw - 1), a, lane);
      for (int w = nw - 2; w >= 0; --w) {
#pragma unroll 1
        for (int s = 0; s < win; ++s) {
          write_limbs_lds<TPI>(slot, a, tig);
          montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
        }
        tile_load(tw, big_digit(ew, xw, win, w), tt, lane);
        write_limbs_lds<TPI>(slot, tt, tig);
        montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
      }
    }
    write_one_lds<TPI>(slot, tig);
    montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);                 // leave the Montgomery domain
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(slot, a, p.out + t * p.ct_words, p.ct_words, valid, tig);
    if (valid && tig == 0) {
      p.out_exp[t] = p.exp[t];
      p.neg[t] = negs ? 1 : 0;
      if (p.status) p.status[t] = range ? ST_ENC_RANGE : ST_OK;
    }
  }
}

}  // namespace fpai
