// Public-key fixed-base obfuscators for n of 2049..4096 bits (DESIGN.md §3 "Fixed bases without the private key",
// kernels_pfb.hpp for the 2048-bit sampler, kernels_pfb1.hpp for the 1024-bit one): the same r = g_0^e_0 g_1^e_1 ...
// g_32^e_32 mod n, the same exponents and digit stream (k_pfb_digits), so r^n mod n^2 = prod_k T_k[d_k] over K table
// rows. Every product mod n^2 is a pair product on a pair group of k_pe4_* (bn_pgroup.hpp: TPI = 8 lanes x LL = 19
// limbs over the S = 152 limbs of n, v = A + n B), and a row is the canonical Montgomery pair of T_k[d] R, R = 2^(28 S),
// stored as the product reads it:
//
//   row = [A: S][B: S] 28-bit limbs, one per 32-bit word, in lane order: 1216 B = 76 uint4. Nothing is unpacked.
//   T_k[0] = R is stored like any other row: a zero digit costs its product, and no lane ever branches on a digit.
//
//   k_pfb4_chain  once per key, one group per base: h_j R = (g_j R)^n by square-and-multiply over n's bits, then the
//                 digit bases B_k R = (h_j R)^(2^(W pos)) by W squarings per position
//   k_pfb4_lohi   one group per (k, half-digit entry): B_k^e R for e < 2^LO, and B_k^(e 2^LO) R for e < 2^HI
//   k_pfb4_fill   one group per row: T_k[d] R = lo[d mod 2^LO] hi[d >> LO] R^-1, canonical
//   k_pfb4        per element, one group: encode; (A, B) = row T_0[d_0]; K - 1 pair products whose multiplier rows go
//                 HBM -> registers -> the group's LDS slot, double-buffered: while row k multiplies out of one buffer
//                 the group fetches row k + 1 in five rounds of two 16-byte loads per lane, one round per outer pass
//                 of the product, into the other; the digits come eight rows at a time, one per lane, a chunk ahead;
//                 the last product, by the pair of c0 = (1, M mod n), leaves the Montgomery form -> xw
//   k_pe4_fin     (kernels_pe4.hpp) the pair -> ciphertext words
// The groups of a wave run the same instruction stream throughout (the ballots and DPP moves of bn_pgroup.hpp want the
// whole wave): groups past the end of the work repeat the last item and store nothing.
#pragma once
#include "kernels_pe4.hpp"

namespace fpai {

constexpr int PFB4_ROW4 = 2 * PE4_S / 4;   // uint4 per table row
constexpr int PFB4_FETCH = (PFB4_ROW4 + 2 * PE4_TPI - 1) / (2 * PE4_TPI);   // rounds of two loads per lane: 5 <= TPI
constexpr int PFB4_SETUP_BLOCK = 64;       // the per-key kernels: one wave, eight groups per block
constexpr size_t PFB4_LDS = ((size_t)2 * PE4_GPB * 2 * PE4_S + PE4_S) * 4;   // k_pfb4: two row buffers per group, X1
static_assert(PFB4_FETCH <= PE4_TPI && (2 * PE4_S) % 4 == 0, "a row is fetched within one product, in whole uint4");

struct Pfb4Const {
  const uint32_t* nl;      // n, S limbs
  const uint32_t* X1;      // (1 - R) mod n
  const uint32_t* oneR;    // pair of R mod n^2 [A: S][B: S]
  const uint32_t* gR;      // [nbases][2S] pairs of g_j R mod n^2
  const uint32_t* nw;      // n as 32-bit words (k_pfb4_chain's exponent)
  uint32_t* bases;         // [K][2S] digit bases B_k R (construction only)
  uint32_t* lohi;          // [K][2^LO + 2^HI][2S] half-digit powers (construction only)
  const uint4* table;      // [K][2^W] rows of PFB4_ROW4 uint4
  uint32_t mprime;         // -n^-1 mod 2^28
  int nbits, nbases;
  int K, W, K0, KS;        // digits: K = K0 + (nbases - 1) KS; base 0 owns slots [0, K0)
};

struct Pfb4Params {
  const Pfb4Const* c;
  long long n;
  const uint32_t* digits;  // [K][n]
  const uint4* table;      // c->table again: a kernel argument is known to be global memory, so the row loads do not
                           // count against the LDS reads of the product they run beside
  EncPlain src;
  EncOut dst;              // exp and status (ct: k_pe4_fin's)
  uint32_t* xw;            // [n][2S] pairs for k_pe4_fin
};

// a pair in global memory -> the group's multiplier slot
template <int TPI, int LL>
__device__ __forceinline__ void pfb4_pair_to_slot(uint32_t* slot, const uint32_t* __restrict__ g, int tig) {
  uint32_t a[LL], b[LL];
  pe4_load<TPI, LL>(g, a, tig);
  pe4_load<TPI, LL>(g + TPI * LL, b, tig);
  pe4_regs_to_slot<TPI, LL>(slot, a, b, tig);
}
template <int TPI, int LL>
__device__ __forceinline__ void pfb4_store_pair(uint32_t* __restrict__ g, const uint32_t (&A)[LL], const uint32_t (&B)[LL], int tig) {
#pragma unroll
  for (int i = 0; i < LL; ++i) {
    g[tig * LL + i] = A[i];
    g[TPI * LL + tig * LL + i] = B[i];
  }
}

// what every per-key kernel starts with: the block's LDS (a slot per group, then X1), n's limbs
template <int TPI, int LL>
struct Pfb4Setup {
  static constexpr int S = TPI * LL, GPB = PFB4_SETUP_BLOCK / TPI;
  uint32_t *slot, *xs;
  uint32_t m[LL];
  int lane, tig, gib;
  __device__ __forceinline__ Pfb4Setup(uint32_t* smem, const Pfb4Const* c) {
    lane = threadIdx.x & 63;
    tig = threadIdx.x % TPI;
    gib = threadIdx.x / TPI;
    slot = smem + gib * 2 * S;
    xs = smem + GPB * 2 * S;
    for (int i = threadIdx.x; i < S; i += PFB4_SETUP_BLOCK) xs[i] = c->X1[i];
    __syncthreads();
    pe4_load<TPI, LL>(c->nl, m, tig);
  }
  __device__ __forceinline__ void sqr(uint32_t (&A)[LL], uint32_t (&B)[LL], uint32_t mprime) {
    pe4_regs_to_slot<TPI, LL>(slot, A, B, tig);
    pgrp::montmul<TPI, LL, true>(A, B, slot, xs, m, mprime, lane, tig);
  }
  __device__ __forceinline__ void mul(uint32_t (&A)[LL], uint32_t (&B)[LL], const uint32_t* g, uint32_t mprime) {
    pfb4_pair_to_slot<TPI, LL>(slot, g, tig);
    pgrp::montmul<TPI, LL, false>(A, B, slot, xs, m, mprime, lane, tig);
  }
};

// ---------------------------------------------------------------- per-key table construction
// Every group runs base 0's K0 positions (the bits of n and the position count are the same for all; a base with fewer
// positions stores only its own), so the chain's time is that of base 0.
template <int TPI, int LL>
__global__ __launch_bounds__(PFB4_SETUP_BLOCK) void k_pfb4_chain(const Pfb4Const* c) {
  constexpr int S = TPI * LL, GPB = PFB4_SETUP_BLOCK / TPI;
  __shared__ __attribute__((aligned(16))) uint32_t smem[GPB * 2 * S + S];
  Pfb4Setup<TPI, LL> u(smem, c);
  const int j0 = blockIdx.x * GPB + u.gib;
  const bool valid = j0 < c->nbases;
  const int j = valid ? j0 : c->nbases - 1;
  const uint32_t mprime = c->mprime;
  const uint32_t* g = c->gR + (size_t)j * 2 * S;
  uint32_t A[LL], B[LL];
  pe4_load<TPI, LL>(g, A, u.tig);
  pe4_load<TPI, LL>(g + S, B, u.tig);
  for (int b = c->nbits - 2; b >= 0; --b) {   // n's top bit is the start value
    u.sqr(A, B, mprime);
    if ((c->nw[b >> 5] >> (b & 31)) & 1u) u.mul(A, B, g, mprime);
  }
  const int k0 = j == 0 ? 0 : c->K0 + (j - 1) * c->KS;
  const int len = j == 0 ? c->K0 : c->KS;
  const int W = c->W, K0 = c->K0;
  for (int pos = 0; pos < K0; ++pos) {
    if (valid && pos < len) pfb4_store_pair<TPI, LL>(c->bases + (size_t)(k0 + pos) * 2 * S, A, B, u.tig);
    if (pos + 1 < K0)
      for (int q = 0; q < W; ++q) u.sqr(A, B, mprime);
  }
}

// lohi[k][e] = B_k^e R (e < 2^LO), lohi[k][2^LO + e] = B_k^(e 2^LO) R (e < 2^HI): left-to-right binary over the W bits
// of the exponent from the pair of R. The groups of a wave hold different exponents, so a clear bit multiplies by the
// pair of R (the identity) instead of branching.
template <int TPI, int LL>
__global__ __launch_bounds__(PFB4_SETUP_BLOCK) void k_pfb4_lohi(const Pfb4Const* c) {
  constexpr int S = TPI * LL, GPB = PFB4_SETUP_BLOCK / TPI;
  __shared__ __attribute__((aligned(16))) uint32_t smem[GPB * 2 * S + S];
  Pfb4Setup<TPI, LL> u(smem, c);
  const int W = c->W, LO = W / 2, HI = W - LO;
  const int nent = (1 << LO) + (1 << HI);
  const int k = blockIdx.y;
  const int idx0 = blockIdx.x * GPB + u.gib;
  const bool valid = idx0 < nent;
  const int idx = valid ? idx0 : nent - 1;
  const uint32_t E = idx < (1 << LO) ? (uint32_t)idx : (uint32_t)(idx - (1 << LO)) << LO;
  const uint32_t mprime = c->mprime;
  const uint32_t* base = c->bases + (size_t)k * 2 * S;
  uint32_t A[LL], B[LL];
  pe4_load<TPI, LL>(c->oneR, A, u.tig);
  pe4_load<TPI, LL>(c->oneR + S, B, u.tig);
  for (int b = W - 1; b >= 0; --b) {
    u.sqr(A, B, mprime);
    u.mul(A, B, ((E >> b) & 1u) ? base : c->oneR, mprime);
  }
  if (valid) pfb4_store_pair<TPI, LL>(c->lohi + ((size_t)k * nent + idx) * 2 * S, A, B, u.tig);
}

template <int TPI, int LL>
__global__ __launch_bounds__(PFB4_SETUP_BLOCK) void k_pfb4_fill(const Pfb4Const* c, uint32_t* table) {
  constexpr int S = TPI * LL, GPB = PFB4_SETUP_BLOCK / TPI;
  __shared__ __attribute__((aligned(16))) uint32_t smem[GPB * 2 * S + S];
  Pfb4Setup<TPI, LL> u(smem, c);
  const int W = c->W, LO = W / 2, HI = W - LO;
  const int nent = (1 << LO) + (1 << HI);
  const int k = blockIdx.y;
  const long long d0 = (long long)blockIdx.x * GPB + u.gib;
  const bool valid = d0 < (1ll << W);
  const size_t d = valid ? (size_t)d0 : ((size_t)1 << W) - 1;
  const uint32_t* lo = c->lohi + ((size_t)k * nent + (d & (((size_t)1 << LO) - 1))) * 2 * S;
  const uint32_t* hi = c->lohi + ((size_t)k * nent + ((size_t)1 << LO) + (d >> LO)) * 2 * S;
  uint32_t A[LL], B[LL];
  pe4_load<TPI, LL>(lo, A, u.tig);
  pe4_load<TPI, LL>(lo + S, B, u.tig);
  u.mul(A, B, hi, c->mprime);
  pgrp::canon<TPI, LL>(A, B, u.m, u.lane, u.tig);
  if (valid) pfb4_store_pair<TPI, LL>(table + (((size_t)k << W) + d) * 2 * S, A, B, u.tig);
}

// ---------------------------------------------------------------- per element
// Round o of a row's fetch: lane t of the group moves uint4 16 o + t and 16 o + 8 + t (the latter while inside the row).
template <int TPI>
__device__ __forceinline__ void pfb4_fetch(const uint4* __restrict__ row, int o, int tig, uint4& q0, uint4& q1) {
  const int i0 = 2 * TPI * o + tig, i1 = i0 + TPI;
  q0 = row[i0];
  if (i1 < PFB4_ROW4) q1 = row[i1];
}
template <int TPI>
__device__ __forceinline__ void pfb4_put(uint32_t* slot, int o, int tig, const uint4& q0, const uint4& q1) {
  uint4* s4 = reinterpret_cast<uint4*>(slot);
  const int i0 = 2 * TPI * o + tig, i1 = i0 + TPI;
  s4[i0] = q0;
  if (i1 < PFB4_ROW4) s4[i1] = q1;
}

// (A, B) <- (A, B)(row in `cur`) R^-1 as pgrp::montmul, while the row at `next` (global; null: none) moves into `nxt`:
// the loads of a round are issued ahead of an outer pass of LL digits and written to LDS behind it.
template <int TPI, int LL>
__device__ __forceinline__ void pfb4_mul_fetch(uint32_t (&A)[LL], uint32_t (&B)[LL], const uint32_t* cur, uint32_t* nxt,
                                               const uint4* __restrict__ next, const uint32_t* xs, const uint32_t (&m)[LL],
                                               uint32_t mprime, int lane, int tig) {
  constexpr int S = TPI * LL;
  uint64_t P1[LL], P2[LL];
#pragma unroll
  for (int i = 0; i < LL; ++i) {
    P1[i] = 0;
    P2[i] = xs[tig * LL + i];
  }
  for (int o = 0; o < TPI; ++o) {
    const bool fetch = next != nullptr && o < PFB4_FETCH;   // wave-uniform
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (fetch) pfb4_fetch<TPI>(next, o, tig, q0, q1);
    __builtin_amdgcn_sched_barrier(0);
    pgrp::outer<TPI, LL, false, false>(P1, P2, A, B, cur + o * LL, cur + S + o * LL, m, mprime, tig,
                                       std::make_integer_sequence<int, LL>{});
    if (fetch) pfb4_put<TPI>(nxt, o, tig, q0, q1);
  }
  pgrp::normalize<TPI, LL>(P1, A, lane, tig);
  pgrp::normalize<TPI, LL>(P2, B, lane, tig);
}

// the pair of c0 = 1 + n M = (1, M mod n) into the slot, as k_pe4_pow stages it (M < 0: n - |M|; the group's lane 0
// runs the borrow over all S limbs)
template <int TPI, int LL>
__device__ __forceinline__ void pfb4_c0_to_slot(uint32_t* slot, int64_t M, const uint32_t* __restrict__ nl, int tig) {
  constexpr int S = TPI * LL;
  wave_lds_fence();
#pragma unroll
  for (int j = 0; j < LL; ++j) slot[tig * LL + j] = (tig == 0 && j == 0) ? 1u : 0u;
  if (tig == 0) {
    const bool neg = M < 0;
    const uint64_t mag = neg ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
    int32_t br = 0;
    for (int j = 0; j < S; ++j) {
      const uint32_t mj = j < 3 ? (uint32_t)(mag >> (LB * j)) & LMASK : 0u;
      const int32_t v = neg ? (int32_t)nl[j] - (int32_t)mj + br : (int32_t)mj;
      slot[S + j] = (uint32_t)v & LMASK;
      br = v >> LB;
    }
  }
  wave_lds_fence();
}

template <int TPI, int LL>
__global__ __launch_bounds__(BLOCK, 2) void k_pfb4(Pfb4Params p) {
  constexpr int S = TPI * LL;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  auto buf = [&](int b) { return smem + ((b & 1) * GPB + gib) * 2 * S; };   // row k multiplies out of buf(k), row k + 1 arrives in buf(k + 1)
  uint32_t* xs = smem + 2 * GPB * 2 * S;
  const Pfb4Const* C = p.c;
  for (int i = threadIdx.x; i < S; i += BLOCK) xs[i] = C->X1[i];
  __syncthreads();
  uint32_t m[LL];
  pe4_load<TPI, LL>(C->nl, m, tig);
  const uint32_t mprime = C->mprime;
  const int K = C->K, W = C->W;
  const uint32_t dmask = (1u << W) - 1u;
  const uint4* table = p.table;
  const int peer = ((lane & ~(TPI - 1)) << 2);   // ds_bpermute address of the group's lane 0
  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long e = base + gib;
    const bool valid = e < p.n;
    const long long ee = valid ? e : p.n - 1;
    int64_t M = 0;
    if (valid && tig == 0) {   // encode (fixedpoint_number.py:46-90)
      int ex = 0;
      const int stt = encode_elem(p.src.x, p.src.dtype, p.src.exp_mode, p.src.fexp, ee, M, ex);
      p.dst.exp[e] = ex;
      if (p.dst.status) p.dst.status[e] = stt;
    }
    // digits of rows [8 c, 8 c + 8), one per lane (rows past K - 1 repeat the last: never used), the masked digit
    // keeps every row address inside the table whatever the buffer holds
    auto chunk = [&](int c) { return p.digits[(size_t)min(TPI * c + tig, K - 1) * p.n + ee] & dmask; };
    auto row_of = [&](int k, uint32_t dg) {
      const uint32_t d = (uint32_t)__builtin_amdgcn_ds_bpermute(peer + ((k % TPI) << 2), (int)dg);
      return table + (((size_t)k << W) + d) * PFB4_ROW4;
    };
    uint32_t dcur = chunk(0), dnext = chunk(1);
    uint32_t A[LL], B[LL];
    {
      const uint32_t* r0 = reinterpret_cast<const uint32_t*>(row_of(0, dcur));
      pe4_load<TPI, LL>(r0, A, tig);
      pe4_load<TPI, LL>(r0 + S, B, tig);
    }
    wave_lds_fence();   // the previous element's last product has read its slot
    if (K > 1) {
      const uint4* r1 = row_of(1, dcur);
      for (int o = 0; o < PFB4_FETCH; ++o) {
        uint4 q0, q1;
        pfb4_fetch<TPI>(r1, o, tig, q0, q1);
        pfb4_put<TPI>(buf(1), o, tig, q0, q1);
      }
    }
    for (int k = 1; k < K; ++k) {
      const uint4* next = nullptr;
      if (k + 1 < K) {
        if ((k + 1) % TPI == 0) {
          dcur = dnext;
          dnext = chunk((k + 1) / TPI + 1);
        }
        next = row_of(k + 1, dcur);
      }
      wave_lds_fence();   // row k is whole in buf(k); the other buffer's readers are done
      pfb4_mul_fetch<TPI, LL>(A, B, buf(k), buf(k + 1), next, xs, m, mprime, lane, tig);
    }
    pfb4_c0_to_slot<TPI, LL>(buf(0), M, C->nl, tig);
    pgrp::montmul<TPI, LL, false>(A, B, buf(0), xs, m, mprime, lane, tig);
    if (valid) pfb4_store_pair<TPI, LL>(p.xw + (size_t)e * 2 * S, A, B, tig);
  }
}

}  // namespace fpai
