// Public-key fixed-base obfuscators for n of 1009..1024 bits (64 ciphertext words; DESIGN.md §3 "Fixed bases without
// the private key", kernels_pfb.hpp for the 2048-bit sampler): the same r = g_0^e_0 g_1^e_1 ... g_32^e_32 mod n, the
// same exponents and digit stream (k_pfb_digits), so r^n mod n^2 = prod_k T_k[d_k] over K table rows. Here every
// product mod n^2 is a p-adic pair product in ONE lane over the S = 37 limbs of n (bn_pair.hpp: v = A + n B, 5 S^2
// MACs), as k_pe1_pow holds its operands, and a row is the plain Montgomery pair of T_k[d] R, R = 2^(28 S):
//
//   row = the 32 words of A, then the 32 words of B (A, B < n < 2^1024, canonical): 256 B, two aligned 128-B lines.
//   A lane reads its own row with 16-byte loads, so every line a wave touches is used whole.
//
//   k_pfb1_chain  once per key, one lane per base: h_j R = (g_j R)^n by square-and-multiply over n's bits, then the
//                 digit bases B_k R = (h_j R)^(2^(W pos)) by W squarings per position
//   k_pfb1_lohi   one lane per (k, half-digit entry): B_k^e R for e < 2^LO, and B_k^(e 2^LO) R for e < 2^HI
//   k_pfb1_fill   one lane per row: T_k[d] R = lo[d mod 2^LO] hi[d >> LO] R^-1, canonical, packed to words
//   k_pfb1        per element, one lane: (A, B) = the pair of R; for every non-zero digit the lane moves its
//                 row through its column of the block's LDS tile ([64 words][256 lanes]: conflict-free, no barrier -- a
//                 lane reads only what it wrote) and runs one pair product with the row's limbs cut from the LDS words
//                 digit by digit, so the row never occupies registers beside the two accumulator rows; at the end the
//                 product by the pair (1, 0) leaves the Montgomery form and the canonical pair goes to xw
//   k_pe1_fin     (kernels_pe1.hpp) c = r^n (1 + n M) -> ciphertext words, exponent, status
#pragma once
#include "kernels_pe1.hpp"

namespace fpai {

constexpr int PFB1_S = 37;                  // limbs of n (k_pe1_*'s: R = 2^1036 >= 2^12 n)
constexpr int PFB1_PW = 32;                 // 32-bit words of A and of B in a table row
constexpr int PFB1_ROW4 = 2 * PFB1_PW / 4;  // uint4 per table row
constexpr int PFB1_SETUP_BLOCK = 64;        // the per-key kernels: one wave per block (they keep two pairs in registers)

struct Pfb1Const {
  const uint32_t* nl;      // n, S limbs
  const uint32_t* oneR;    // pair of R mod n^2 [A: S][B: S]
  const uint32_t* gR;      // [nbases][2S] pairs of g_j R mod n^2
  const uint32_t* nw;      // n as 32-bit words (k_pfb1_chain's exponent)
  uint32_t* bases;         // [K][2S] digit bases B_k R (construction only)
  uint32_t* lohi;          // [K][2^LO + 2^HI][2S] half-digit powers (construction only)
  const uint4* table;      // [K][2^W] rows of PFB1_ROW4 uint4
  uint32_t mprime;         // -n^-1 mod 2^28
  int nbits, nbases;
  int K, W, K0, KS;        // digits: K = K0 + (nbases - 1) KS; base 0 owns slots [0, K0)
};

struct Pfb1Params {
  const Pfb1Const* c;
  long long n;
  const uint32_t* digits;  // [K][n]
  uint32_t* xw;            // [2S][n]: canonical pair limbs of r^n for k_pe1_fin
};

template <int S>
__device__ __forceinline__ void pfb1_load_pair(const uint32_t* src, uint32_t (&A)[S], uint32_t (&B)[S]) {
#pragma unroll
  for (int j = 0; j < S; ++j) {
    A[j] = src[j];
    B[j] = src[S + j];
  }
}

// (A, B) <- (A, B)(XA, XB) R^-1 with the multiplier in registers
template <int S>
__device__ __forceinline__ void pfb1_mul_regs(uint32_t (&A)[S], uint32_t (&B)[S], const uint32_t (&XA)[S],
                                              const uint32_t (&XB)[S], const uint32_t (&m)[S], uint32_t mprime) {
  pair::mont_mul<S>(A, B, [&](auto j) { return make_uint2(XA[decltype(j)::value], XB[decltype(j)::value]); }, m, mprime);
}

// ---------------------------------------------------------------- per-key table construction
template <int S>
__global__ __launch_bounds__(PFB1_SETUP_BLOCK) void k_pfb1_chain(const Pfb1Const* c) {
  const int j = blockIdx.x * PFB1_SETUP_BLOCK + threadIdx.x;
  if (j >= c->nbases) return;
  uint32_t m[S], A[S], B[S], xa[S], xb[S];
#pragma unroll
  for (int i = 0; i < S; ++i) m[i] = c->nl[i];
  const uint32_t mprime = c->mprime;
  pfb1_load_pair<S>(c->gR + (size_t)j * 2 * S, xa, xb);
  pfb1_load_pair<S>(c->gR + (size_t)j * 2 * S, A, B);
  for (int b = c->nbits - 2; b >= 0; --b) {   // n's top bit is the start value
    pair::mont_sqr<S>(A, B, m, mprime);
    if ((c->nw[b >> 5] >> (b & 31)) & 1u) pfb1_mul_regs<S>(A, B, xa, xb, m, mprime);
  }
  const int k0 = j == 0 ? 0 : c->K0 + (j - 1) * c->KS;
  const int len = j == 0 ? c->K0 : c->KS;
  for (int pos = 0; pos < len; ++pos) {
    uint32_t* dst = c->bases + (size_t)(k0 + pos) * 2 * S;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      dst[i] = A[i];
      dst[S + i] = B[i];
    }
    if (pos + 1 < len)
      for (int q = 0; q < c->W; ++q) pair::mont_sqr<S>(A, B, m, mprime);
  }
}

// lohi[k][e] = B_k^e R (e < 2^LO), lohi[k][2^LO + e] = B_k^(e 2^LO) R (e < 2^HI): left-to-right binary over the W bits
// of the exponent from the pair of R (operands and results < 2n, which the pair product takes)
template <int S>
__global__ __launch_bounds__(PFB1_SETUP_BLOCK) void k_pfb1_lohi(const Pfb1Const* c) {
  const int W = c->W, LO = W / 2, HI = W - LO;
  const int nent = (1 << LO) + (1 << HI);
  const int k = blockIdx.y;
  const int idx = blockIdx.x * PFB1_SETUP_BLOCK + threadIdx.x;
  if (idx >= nent || k >= c->K) return;
  const uint32_t E = idx < (1 << LO) ? (uint32_t)idx : (uint32_t)(idx - (1 << LO)) << LO;
  uint32_t m[S], A[S], B[S], xa[S], xb[S];
#pragma unroll
  for (int i = 0; i < S; ++i) m[i] = c->nl[i];
  const uint32_t mprime = c->mprime;
  pfb1_load_pair<S>(c->bases + (size_t)k * 2 * S, xa, xb);
  pfb1_load_pair<S>(c->oneR, A, B);
  for (int b = W - 1; b >= 0; --b) {
    pair::mont_sqr<S>(A, B, m, mprime);
    if ((E >> b) & 1u) pfb1_mul_regs<S>(A, B, xa, xb, m, mprime);
  }
  uint32_t* dst = c->lohi + ((size_t)k * nent + idx) * 2 * S;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    dst[i] = A[i];
    dst[S + i] = B[i];
  }
}

// the 32 words of a canonical S-limb value (< 2^1024), as four-word stores
template <int S, int... Qs>
__device__ __forceinline__ void pfb1_store_words(const uint32_t (&X)[S], uint4* dst, std::integer_sequence<int, Qs...>) {
  uint32_t w[PFB1_PW];
  pe1_words_out<S>(X, w, PFB1_PW, std::make_integer_sequence<int, PFB1_PW>{});
  ((dst[Qs] = make_uint4(w[4 * Qs], w[4 * Qs + 1], w[4 * Qs + 2], w[4 * Qs + 3])), ...);
}

template <int S>
__global__ __launch_bounds__(PFB1_SETUP_BLOCK) void k_pfb1_fill(const Pfb1Const* c, uint4* table) {
  const int W = c->W, LO = W / 2, HI = W - LO;
  const int nent = (1 << LO) + (1 << HI);
  const int k = blockIdx.y;
  const long long d = (long long)blockIdx.x * PFB1_SETUP_BLOCK + threadIdx.x;
  if (d >= (1ll << W) || k >= c->K) return;
  uint32_t m[S], A[S], B[S], xa[S], xb[S];
#pragma unroll
  for (int i = 0; i < S; ++i) m[i] = c->nl[i];
  const uint32_t* lo = c->lohi + ((size_t)k * nent + (size_t)(d & ((1 << LO) - 1))) * 2 * S;
  const uint32_t* hi = c->lohi + ((size_t)k * nent + (size_t)(1 << LO) + (size_t)(d >> LO)) * 2 * S;
  pfb1_load_pair<S>(lo, A, B);
  pfb1_load_pair<S>(hi, xa, xb);
  pfb1_mul_regs<S>(A, B, xa, xb, m, c->mprime);
  pair::canon<S>(A, B, m);
  uint4* row = table + (((size_t)k << W) + (size_t)d) * PFB1_ROW4;
  pfb1_store_words<S>(A, row, std::make_integer_sequence<int, PFB1_PW / 4>{});
  pfb1_store_words<S>(B, row + PFB1_PW / 4, std::make_integer_sequence<int, PFB1_PW / 4>{});
}

// ---------------------------------------------------------------- per element
// The multiplier of one row product: limb pair (A_r[J], B_r[J]) cut from the lane's LDS column (word w of the row at
// col[w * LANE_BLOCK]) when digit J needs it; the second wave of the SIMD covers the LDS latency.
template <int S>
struct Pfb1Row {
  const uint32_t* col;
  template <int J>
  __device__ __forceinline__ uint2 operator()(std::integral_constant<int, J>) const {
    const uint32_t* cl = col;
    return make_uint2(lane::limb_from_words([cl](int w) { return cl[w * LANE_BLOCK]; }, PFB1_PW, J),
                      lane::limb_from_words([cl](int w) { return cl[(PFB1_PW + w) * LANE_BLOCK]; }, PFB1_PW, J));
  }
};
template <int... Qs>
__device__ __forceinline__ void pfb1_row_to_lds(const uint4* row, uint32_t* col, std::integer_sequence<int, Qs...>) {
  uint4 q[sizeof...(Qs)];
  ((q[Qs] = row[Qs]), ...);
  ((col[(4 * Qs) * LANE_BLOCK] = q[Qs].x, col[(4 * Qs + 1) * LANE_BLOCK] = q[Qs].y,
    col[(4 * Qs + 2) * LANE_BLOCK] = q[Qs].z, col[(4 * Qs + 3) * LANE_BLOCK] = q[Qs].w), ...);
}

template <int S>
__global__ __launch_bounds__(LANE_BLOCK, 2) void k_pfb1(Pfb1Params p) {
  __shared__ uint32_t tile[2 * PFB1_PW * LANE_BLOCK];   // [word][lane]: 64 KB, two blocks per CU
  const Pfb1Const* C = p.c;
  uint32_t m[S];
#pragma unroll
  for (int j = 0; j < S; ++j) m[j] = C->nl[j];
  const uint32_t mprime = C->mprime;
  const int K = C->K, W = C->W;
  const uint4* table = C->table;
  uint32_t* col = tile + threadIdx.x;
  // no barrier below: a lane touches only its own column, so the lanes past n simply leave
  for (long long i = (long long)blockIdx.x * LANE_BLOCK + threadIdx.x; i < p.n; i += (long long)gridDim.x * LANE_BLOCK) {
    uint32_t A[S], B[S];
    pfb1_load_pair<S>(C->oneR, A, B);
    for (int k = 0; k < K; ++k) {
      const uint32_t d = p.digits[(size_t)k * p.n + i] & ((1u << W) - 1u);
      if (d == 0) continue;   // T_k[0] = 1
      pfb1_row_to_lds(table + (((size_t)k << W) + d) * PFB1_ROW4, col, std::make_integer_sequence<int, PFB1_ROW4>{});
      pair::mont_mul<S>(A, B, Pfb1Row<S>{col}, m, mprime);
    }
    // out of the Montgomery form: the product by the pair (1, 0)
    pair::mont_mul<S>(A, B, [](auto j) { return make_uint2(decltype(j)::value == 0 ? 1u : 0u, 0u); }, m, mprime);
    pair::canon<S>(A, B, m);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      p.xw[(size_t)j * p.n + i] = A[j];
      p.xw[(size_t)(S + j) * p.n + i] = B[j];
    }
  }
}

}  // namespace fpai
