// k_modinv<K>: x_i^-1 mod m for a few dozen residues and one odd modulus of W <= 256 words, one value per wavefront,
// by the 31-steps-at-a-time binary extended GCD of modinv_step.hpp (which holds the algorithm and the round count).
//
// Layout. A block is one wave. Each of a, b, u, v and m lies across the 64 lanes, K = ceil(W / 64) consecutive words
// per lane in registers (lane l holds words l K .. l K + K - 1; words from W on are zero), so a number is 64 K words
// wide whatever W is, and W <= 64 runs one word per lane. No LDS.
//
// One round:
//   * top words: a ballot over the lanes with a non-zero word of a | b, then v_readlane of words jt, jt - 1, 1 and 0
//     of a and b; modinv_approx and modinv_steps31 run on wave-uniform values (scalar registers);
//   * each matrix row +-(cp P - cn N) is the unsigned sum cp P + cn ~N + cn: K v_mad_u64_u32 per term and lane, the
//     lane's high word handed to the lane above (ds_bpermute), the carries that this leaves resolved by one ballot
//     look-ahead over the full wave (bn_group.hpp's lookahead_carry_in without the group seams). The sign is the
//     wave-uniform top word: carry out of lane 63 less cn;
//   * the division by 2^31 takes bit 31 of each word and 31 bits of the next one, the lane's last word from the lane
//     above (ds_bpermute);
//   * a negative a' or b' is negated (carry in = every lane below is zero: one ballot) and its row is flipped;
//   * (u, v): the same sum with a third term k m or k ~m (modinv_row_k) that clears the low 31 bits, then + m when the
//     quotient is negative. The coefficients sum to at most 2^32, so every accumulator fits 64 bits.
// Per round and lane: 10 K multiply-accumulates (2 x 2 K for a and b, 2 x 3 K for u and v), four to eight look-aheads
// of two ballots each, and the 31 steps: about 12 scalar instructions each, the longest part of a round.
//
// Status: 0 and the inverse in [0, m) where gcd(x, m) = 1; otherwise 1, the output row untouched, and *any_noinv = 1.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "modinv_step.hpp"

namespace fpai {

constexpr int MODINV_MAX_WORDS = 256;

struct ModinvParams {
  const uint32_t* x;      // [count][W] residues below m
  const uint32_t* m;      // [W] odd modulus
  uint32_t* out;          // [count][W] (may be x)
  uint32_t* status;       // [count] (nullable)
  uint32_t* any_noinv;    // one word, cleared by the caller on the stream before (nullable)
  int W;
  int rounds;             // modinv_rounds(len(m))
  uint32_t ninv31;        // modinv_neg_minv31(m[0])
};

// Adds the carries that a lane-local pass left: `cin` (the word from the lane below, or a carry bit) goes into S, the
// carries out of that are resolved over the wave. Returns the carry out of lane 63.
template <int K>
__device__ __forceinline__ uint32_t modinv_carry(uint32_t (&S)[K], uint32_t cin, int lane) {
  uint64_t c = cin;
  bool ones = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    c += S[i];
    S[i] = (uint32_t)c;
    c >>= 32;
    ones = ones && S[i] == 0xffffffffu;
  }
  const uint64_t G = __ballot(c != 0);
  const uint64_t X = G | __ballot(ones);
  const uint64_t sum = X + G;
  uint32_t ci = (uint32_t)(((sum ^ X ^ G) >> lane) & 1ull);
#pragma unroll
  for (int i = 0; i < K; ++i) {
    S[i] += ci;
    ci = (ci && S[i] == 0u) ? 1u : 0u;
  }
  return sum < X ? 1u : 0u;
}

// out = (cp P + cn ~N + ck M' + c0 - 2^(2048 K) topsub) / 2^31 with M' = m or ~m; true when it is negative
template <int K, bool WITH_M>
__device__ __forceinline__ bool modinv_apply(const uint32_t (&P)[K], const uint32_t (&N)[K], uint32_t cp, uint32_t cn,
                                             const uint32_t (&m)[K], uint32_t ck, bool mneg, uint32_t c0, int64_t topsub,
                                             uint32_t (&out)[K], int lane) {
  uint32_t S[K];
  uint64_t t = lane == 0 ? c0 : 0u;
  const uint32_t mx = mneg ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    t += (uint64_t)cp * P[i];
    t += (uint64_t)cn * (uint32_t)~N[i];
    if (WITH_M) t += (uint64_t)ck * (m[i] ^ mx);
    S[i] = (uint32_t)t;
    t >>= 32;
  }
  const uint32_t hi = (uint32_t)t;
  const uint32_t below = __shfl_up(hi, 1);
  const uint32_t cout = modinv_carry<K>(S, lane == 0 ? 0u : below, lane);
  const int64_t top = (int64_t)(uint32_t)__builtin_amdgcn_readlane(hi, 63) + cout - topsub;   // (the builtin returns int)
  const uint32_t above = __shfl_down(S[0], 1);
  const uint32_t next = lane == 63 ? (uint32_t)top : above;
#pragma unroll
  for (int i = 0; i < K; ++i) out[i] = (S[i] >> 31) | ((i + 1 < K ? S[i + 1] : next) << 1);
  return top < 0;
}

// word j of a number (j wave-uniform)
template <int K>
__device__ __forceinline__ uint32_t modinv_word(const uint32_t (&z)[K], int j) {
  const int r = j % K;
  uint32_t sel = z[0];
#pragma unroll
  for (int i = 1; i < K; ++i) sel = r == i ? z[i] : sel;
  return __builtin_amdgcn_readlane(sel, j / K);
}

template <int K>
__global__ __launch_bounds__(64) void k_modinv(ModinvParams p) {
  const int lane = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * p.W;
  uint32_t a[K], b[K], u[K], v[K], m[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int j = lane * K + i;
    m[i] = j < p.W ? p.m[j] : 0u;
    a[i] = j < p.W ? p.x[row + j] : 0u;
    b[i] = m[i];
    u[i] = j == 0 ? 1u : 0u;
    v[i] = 0u;
  }
#pragma unroll 1
  for (int it = 0; it < p.rounds; ++it) {
    // the top non-zero word of a | b (b is odd, so there is one)
    uint32_t ow = 0;
    int ti = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const uint32_t o = a[i] | b[i];
      if (o) { ow = o; ti = i; }
    }
    const int tl = 63 - __builtin_clzll(__ballot(ow != 0));
    const int jt = tl * K + __builtin_amdgcn_readlane(ti, tl);
    const int s = 32 - __builtin_clz(__builtin_amdgcn_readlane(ow, tl));
    const int j1 = jt > 1 ? jt : 1;
    const uint64_t alo = ((uint64_t)modinv_word<K>(a, 1) << 32) | modinv_word<K>(a, 0);
    const uint64_t blo = ((uint64_t)modinv_word<K>(b, 1) << 32) | modinv_word<K>(b, 0);
    const uint64_t ahi = ((uint64_t)modinv_word<K>(a, j1) << 32) | modinv_word<K>(a, j1 - 1);
    const uint64_t bhi = ((uint64_t)modinv_word<K>(b, j1) << 32) | modinv_word<K>(b, j1 - 1);
    const ModinvMat M = modinv_steps31(modinv_approx(alo, ahi, jt, s), modinv_approx(blo, bhi, jt, s));
    uint32_t na[K], nb[K], nu[K], nv[K];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t f = r ? M.f1 : M.f0, g = r ? M.g1 : M.g0;
      uint32_t (&ab)[K] = r ? nb : na;
      uint32_t (&uv)[K] = r ? nv : nu;
      ModinvRow pl = modinv_row_plan(f, g, false);
      bool neg = pl.p_is_b ? modinv_apply<K, false>(b, a, pl.cp, pl.cn, m, 0u, false, pl.cn, (int64_t)pl.cn, ab, lane)
                           : modinv_apply<K, false>(a, b, pl.cp, pl.cn, m, 0u, false, pl.cn, (int64_t)pl.cn, ab, lane);
      if (neg) {
        bool zero = true;
#pragma unroll
        for (int i = 0; i < K; ++i) zero = zero && ab[i] == 0u;
        const uint64_t lower = (1ull << lane) - 1ull;
        uint32_t ci = (__ballot(zero) & lower) == lower ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          ab[i] = ~ab[i] + ci;
          ci = (ci && ab[i] == 0u) ? 1u : 0u;
        }
        pl = modinv_row_plan(f, g, true);
      }
      const uint32_t p0 = pl.p_is_b ? v[0] : u[0], n0 = pl.p_is_b ? u[0] : v[0];
      const uint32_t t0 = __builtin_amdgcn_readfirstlane(pl.cp * p0 + pl.cn * ~n0 + pl.cn);
      const ModinvK mk = modinv_row_k(t0, pl.cp, p.ninv31);
      const uint32_t sub = mk.neg ? mk.k : 0u;
      neg = pl.p_is_b ? modinv_apply<K, true>(v, u, pl.cp, pl.cn, m, mk.k, mk.neg, pl.cn + sub, (int64_t)pl.cn + sub, uv, lane)
                      : modinv_apply<K, true>(u, v, pl.cp, pl.cn, m, mk.k, mk.neg, pl.cn + sub, (int64_t)pl.cn + sub, uv, lane);
      if (neg) {
        uint64_t c = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          c += (uint64_t)uv[i] + m[i];
          uv[i] = (uint32_t)c;
          c >>= 32;
        }
        const uint32_t below = __shfl_up((uint32_t)c, 1);
        (void)modinv_carry<K>(uv, lane == 0 ? 0u : below, lane);
      }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
      a[i] = na[i];
      b[i] = nb[i];
      u[i] = nu[i];
      v[i] = nv[i];
    }
  }
  // b = gcd(x, m)
  bool one = true;
#pragma unroll
  for (int i = 0; i < K; ++i) one = one && b[i] == ((lane == 0 && i == 0) ? 1u : 0u);
  const bool unit = __ballot(one) == ~0ull;
  if (unit) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int j = lane * K + i;
      if (j < p.W) p.out[row + j] = v[i];
    }
  }
  if (lane == 0) {
    if (p.status) p.status[blockIdx.x] = unit ? 0u : 1u;
    if (!unit && p.any_noinv) *p.any_noinv = 1u;
  }
}

}  // namespace fpai
