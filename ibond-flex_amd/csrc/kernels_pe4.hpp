// Public-key encryption on pair groups (bn_pgroup.hpp) for n of 2049..4096 bits: c = c0 r^n mod n^2 with every
// product mod n^2 a pair product over the S = 152 limbs of n, v = A + n B (mod n^2), A and B spread over the
// TPI = 8 lanes of a group (LL = 19 limbs per lane; R = 2^(28 152) >= 2^24 n). kernels_pe.hpp's three stages on the
// group engine: a square costs 4 S^2 = 92 k lane-MACs and a product 5 S^2 = 116 k, against the 2 (296)^2 = 175 k of
// either in k_encrypt<8> (Montgomery over the 296 limbs of n^2). Same ciphertext bits.
//
//   k_pe4_pre   encode -> M, exponent, status; r's words (explicit, or the element's ChaCha20 stream exactly as
//               k_encrypt draws it) -> its 2 S 28-bit digits in the group's LDS slot; r R mod n^2 as a pair: the
//               constant pair of R^3 mod n^2 times those digits, one B-free pass of 2 S digits whose second row
//               starts at (1 - R^2) mod n
//   k_pe4_pow   (r R)^n by the lane machine's op list for the exponent n (build_lane_program: 16 odd-power tiles in
//               device scratch, sliding window 5), the current multiplier staged in the group's LDS slot
//               [A2: S][B2: S]; the final product with the pair of c0 = 1 + n M, i.e. (1, M mod n), leaves Montgomery
//               form: the plain pair of c
//   k_pe4_fin   the canonical pair -> c = A + n B (< n^2) on the L = 37 group engine (one Montgomery product by
//               n R' mod n^2, as k_fbgp_w) -> ciphertext words
// Every lane of a wave follows the same op list; all cross-lane traffic stays inside a 16-lane DPP row.
#pragma once
#include "bn_pgroup.hpp"
#include "kernels_crt.hpp"

namespace fpai {

constexpr int PE4_TPI = 8, PE4_LL = 19, PE4_S = PE4_TPI * PE4_LL;   // 152 limbs >= the 147 of a 4096-bit n
constexpr int PE4_GPB = BLOCK / PE4_TPI;                            // 32 groups (elements) per block
constexpr int PE4_TQ = (2 * PE4_LL + 3) / 4;                        // quads of a lane's share of a tile: A, B, 2 pad words
constexpr int PE4_FS = PE4_TPI * L;                                 // 296 limbs of n^2 (k_pe4_fin)
constexpr int PE4_FSLOT = 2 * PE4_S > PE4_FS ? 2 * PE4_S : PE4_FS;  // k_pe4_fin's slot: the pair, then the n^2 operand
constexpr size_t PE4_SCRATCH_WORDS = (size_t)LANE_NTILE * PE4_TQ * 4;   // per lane of the k_pe4_pow grid

struct Pe4Const {
  const uint32_t* nl;      // n, S limbs
  const uint32_t* X1;      // (1 - R) mod n
  const uint32_t* XK;      // (1 - R^2) mod n
  const uint32_t* cK;      // pair of R^3 mod n^2 ([A: S][B: S])
  const uint32_t* prog;    // op list for the exponent n
  int nprog;
  uint32_t mprime;         // -n^-1 mod 2^28
  const uint32_t* N2;      // n^2, PE4_FS limbs (k_pe4_fin)
  const uint32_t* nR;      // n R' mod n^2, R' = 2^(28 PE4_FS)
  uint32_t mprime2;        // -n^-2 mod 2^28
};

struct Pe4Params {
  const Pe4Const* k;
  EncPlain src;
  EncObf rnd;
  EncOut dst;
  long long n;
  uint32_t* xw;            // [n][2 S] pairs ([A: S][B: S] per element)
  int64_t* M;              // [n] encodings (k_pe4_pre -> k_pe4_pow)
  uint32_t* scratch;       // k_pe4_pow's tiles (LaneScratch, PE4_TQ quads per lane per tile)
};

template <int TPI, int LL>
__device__ __forceinline__ void pe4_load(const uint32_t* __restrict__ g, uint32_t (&x)[LL], int tig) {
#pragma unroll
  for (int i = 0; i < LL; ++i) x[i] = g[tig * LL + i];
}
template <int TPI, int LL>
__device__ __forceinline__ void pe4_regs_to_slot(uint32_t* slot, const uint32_t (&A)[LL], const uint32_t (&B)[LL], int tig) {
  constexpr int S = TPI * LL;
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < LL; ++i) {
    slot[tig * LL + i] = A[i];
    slot[S + tig * LL + i] = B[i];
  }
  wave_lds_fence();
}

// a lane's share of tile k: quads [k TQ, (k + 1) TQ) of its scratch column hold A[0..LL), B[0..LL), 0, 0
template <int LL>
__device__ __forceinline__ uint32_t pe4_tile_word(const uint32_t (&A)[LL], const uint32_t (&B)[LL], int j) {
  return j < LL ? A[j] : j < 2 * LL ? B[j - LL] : 0u;
}
// (an opaque copy of the lane index: LICM would otherwise hoist the TQ 64-bit quad addresses of a constant tile out
// of the element loop and keep them live across the products)
__device__ __forceinline__ LaneScratch pe4_opaque(const LaneScratch& t) {
  uint32_t l = t.lid;
  asm volatile("" : "+v"(l));
  return LaneScratch{t.scratch, t.nl, l};
}
template <int LL>
__device__ __forceinline__ void pe4_tile_store(const LaneScratch& t0, int k, const uint32_t (&A)[LL], const uint32_t (&B)[LL]) {
  constexpr int TQ = (2 * LL + 3) / 4;
  const LaneScratch t = pe4_opaque(t0);
#pragma unroll
  for (int g = 0; g < TQ; ++g)
    t.quad(k * TQ + g) = make_uint4(pe4_tile_word<LL>(A, B, 4 * g), pe4_tile_word<LL>(A, B, 4 * g + 1),
                                    pe4_tile_word<LL>(A, B, 4 * g + 2), pe4_tile_word<LL>(A, B, 4 * g + 3));
}
template <int LL>
__device__ __forceinline__ void pe4_tile_load(const LaneScratch& t0, int k, uint32_t (&A)[LL], uint32_t (&B)[LL]) {
  constexpr int TQ = (2 * LL + 3) / 4;
  const LaneScratch t = pe4_opaque(t0);
  uint4 v[TQ];
#pragma unroll
  for (int g = 0; g < TQ; ++g) v[g] = t.quad(k * TQ + g);
#pragma unroll
  for (int g = 0; g < TQ; ++g) {
    const uint32_t w[4] = {v[g].x, v[g].y, v[g].z, v[g].w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * g + q;
      if (j < LL) A[j] = w[q];
      else if (j < 2 * LL) B[j - LL] = w[q];
    }
  }
}
// tile k -> the group's multiplier slot [A2: S][B2: S]
template <int TPI, int LL>
__device__ __forceinline__ void pe4_tile_to_slot(const LaneScratch& t, int k, uint32_t* slot, int tig) {
  uint32_t a[LL], b[LL];
  pe4_tile_load<LL>(t, k, a, b);
  pe4_regs_to_slot<TPI, LL>(slot, a, b, tig);
}

template <int TPI, int LL>
__global__ __launch_bounds__(BLOCK) void k_pe4_pre(Pe4Params p) {
  constexpr int S = TPI * LL;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * 2 * S;   // r's words (<= 2 S of them), then its 2 S digits
  const Pe4Const* K = p.k;
  uint32_t m[LL];
  pe4_load<TPI, LL>(K->nl, m, tig);
  const uint32_t mprime = K->mprime;
  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long e = base + gib;
    const bool valid = e < p.n;
    const long long ee = valid ? e : p.n - 1;
    if (valid && tig == 0) {   // encode (fixedpoint_number.py:46-90): M for k_pe4_pow's final product
      int64_t M = 0;
      int ex = 0;
      const int stt = encode_elem(p.src.x, p.src.dtype, p.src.exp_mode, p.src.fexp, ee, M, ex);
      p.M[e] = M;
      p.dst.exp[e] = ex;
      if (p.dst.status) p.dst.status[e] = stt;
    }
    wave_lds_fence();
    int nw;
    if (p.rnd.obf == 1) {
      nw = p.rnd.r_words;
      const uint32_t* rg = p.rnd.r + ee * p.rnd.r_stride;
      for (int w = tig; w < nw; w += TPI) slot[w] = rg[w];
    } else {
      nw = p.rnd.r_words;
      const unsigned long long g = p.rnd.index_base + (unsigned long long)ee;
      for (int b = tig; b * 16 < nw; b += TPI) {
        uint32_t blk[16];
        obf_stream_block(p.rnd.rng_key, b, g, blk);
#pragma unroll
        for (int w = 0; w < 16; ++w)
          if (b * 16 + w < nw) slot[b * 16 + w] = blk[w];
      }
    }
    wave_lds_fence();
    // lane t cuts digits [2 LL t, 2 LL t + 2 LL) out of the words (registers first: the digits overwrite the words)
    {
      int t = tig;
      asm volatile("" : "+v"(t));
      uint32_t y[2 * LL];
#pragma unroll
      for (int i = 0; i < 2 * LL; ++i) {
        const int bit = (t * 2 * LL + i) * LB, wi = bit >> 5;
        const uint32_t lo = wi < nw ? slot[wi] : 0u, hi = wi + 1 < nw ? slot[wi + 1] : 0u;
        y[i] = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(bit & 31)) & LMASK;
      }
      wave_lds_fence();
#pragma unroll
      for (int i = 0; i < 2 * LL; ++i) slot[t * 2 * LL + i] = y[i];
      wave_lds_fence();
    }
    // (cA + n cB) r R^-2 = r R mod n^2: P1 = REDC(cA r), P2 = REDC(cB r - m1) from (1 - R^2) mod n, 2 S digits
    uint32_t A[LL], B[LL];
    pe4_load<TPI, LL>(K->cK, A, tig);
    pe4_load<TPI, LL>(K->cK + S, B, tig);
    uint64_t P1[LL], P2[LL];
#pragma unroll
    for (int i = 0; i < LL; ++i) {
      P1[i] = 0;
      P2[i] = K->XK[tig * LL + i];
    }
    for (int o = 0; o < 2 * TPI; ++o)
      pgrp::outer<TPI, LL, false, true>(P1, P2, A, B, slot + o * LL, slot, m, mprime, tig, std::make_integer_sequence<int, LL>{});
    pgrp::normalize<TPI, LL>(P1, A, lane, tig);
    pgrp::normalize<TPI, LL>(P2, B, lane, tig);
    if (valid) {
      uint32_t* xo = p.xw + (size_t)e * 2 * S + tig * LL;
#pragma unroll
      for (int i = 0; i < LL; ++i) {
        xo[i] = A[i];
        xo[S + i] = B[i];
      }
    }
  }
}

template <int TPI, int LL>
__global__ __launch_bounds__(BLOCK, 2) void k_pe4_pow(Pe4Params p) {
  constexpr int S = TPI * LL;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * 2 * S;   // the current multiplier [A2: S][B2: S]
  uint32_t* xs = smem + GPB * 2 * S;     // (1 - R) mod n: the second row's start
  const Pe4Const* K = p.k;
  for (int i = threadIdx.x; i < S; i += BLOCK) xs[i] = K->X1[i];
  __syncthreads();
  uint32_t m[LL];
  pe4_load<TPI, LL>(K->nl, m, tig);
  const uint32_t mprime = K->mprime;
  const int nprog = K->nprog;
  const uint32_t* prog = K->prog;
  const LaneScratch tl = lane_scratch(p.scratch);
  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long e = base + gib;
    const bool valid = e < p.n;
    const long long ee = valid ? e : p.n - 1;
    uint32_t A[LL], B[LL];
    pe4_load<TPI, LL>(p.xw + (size_t)ee * 2 * S, A, tig);
    pe4_load<TPI, LL>(p.xw + (size_t)ee * 2 * S + S, B, tig);
    pe4_tile_store<LL>(tl, 0, A, B);
    // The op list of kernels_crt.hpp on pair groups. A square reads (A, B) itself from the slot, so a multiplier is
    // staged when its product comes (LOP_PREFETCH is not used); `kept`: the slot still holds what LOP_B_SET left
    // there (the table's x~^2: no square runs between its products).
    // (a do-while: with a loop that may run zero times the first load of (A, B) stays live, spilled, to its end)
    bool kept = false;
    int i = 0;
    do {
      const uint32_t op = (i < nprog) ? lane_op(prog, i) : LOP_B_CONST;
      if (op & LOP_A_FROM_T) pe4_tile_load<LL>(tl, (op >> 16) & 0xFF, A, B);
      if (op & LOP_SQR) {
        pe4_regs_to_slot<TPI, LL>(slot, A, B, tig);
        pgrp::montmul<TPI, LL, true>(A, B, slot, xs, m, mprime, lane, tig);
        kept = false;
      } else {
        if (op & LOP_B_CONST) {
          // the final multiplier: the pair of c0 = 1 + n M = (1, M mod n) (M < 0: n - |M|, the group's lane 0
          // runs the borrow over all S limbs)
          wave_lds_fence();
#pragma unroll
          for (int j = 0; j < LL; ++j) slot[tig * LL + j] = (tig == 0 && j == 0) ? 1u : 0u;
          if (tig == 0) {
            const int64_t M = p.M[ee];
            const bool neg = M < 0;
            const uint64_t mag = neg ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
            const uint32_t* nlp = K->nl;
            int32_t br = 0;
            for (int j = 0; j < S; ++j) {
              const uint32_t mj = j < 3 ? (uint32_t)(mag >> (LB * j)) & LMASK : 0u;
              const int32_t v = neg ? (int32_t)nlp[j] - (int32_t)mj + br : (int32_t)mj;
              slot[S + j] = (uint32_t)v & LMASK;
              br = v >> LB;
            }
          }
          wave_lds_fence();
        } else if (!((op & LOP_B_READY) && kept)) {
          pe4_tile_to_slot<TPI, LL>(tl, (op >> 8) & 0xFF, slot, tig);
        }
        pgrp::montmul<TPI, LL, false>(A, B, slot, xs, m, mprime, lane, tig);
      }
      if (op & LOP_STORE) pe4_tile_store<LL>(tl, op >> 24, A, B);
      if (op & LOP_B_SET) {
        pe4_regs_to_slot<TPI, LL>(slot, A, B, tig);
        kept = true;
      }
    } while (++i <= nprog);
    if (valid) {
      uint32_t* xo = p.xw + (size_t)e * 2 * S + tig * LL;
#pragma unroll
      for (int i = 0; i < LL; ++i) {
        xo[i] = A[i];
        xo[S + i] = B[i];
      }
    }
  }
}

// c = A + (B (n R') R'^-1 mod n^2) from the canonical pair (A, B < n, so the sum is c itself, < n^2, after the two
// conditional subtractions of the Montgomery product's excess), then the ciphertext words
template <int TPI, int LL>
__global__ __launch_bounds__(BLOCK) void k_pe4_fin(Pe4Params p) {
  constexpr int S = TPI * LL;
  constexpr int FS = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  static_assert(2 * S <= PE4_FSLOT && FS <= PE4_FSLOT, "the pair and the n^2 operand fit the slot");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * PE4_FSLOT;
  const Pe4Const* K = p.k;
  uint32_t m2[L];
  load_limbs_g<TPI>(K->N2, m2, tig);
  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long e = base + gib;
    const bool valid = e < p.n;
    const long long ee = valid ? e : p.n - 1;
    {
      uint32_t m[LL], A[LL], B[LL];
      pe4_load<TPI, LL>(K->nl, m, tig);
      pe4_load<TPI, LL>(p.xw + (size_t)ee * 2 * S, A, tig);
      pe4_load<TPI, LL>(p.xw + (size_t)ee * 2 * S + S, B, tig);
      pgrp::canon<TPI, LL>(A, B, m, lane, tig);
      pe4_regs_to_slot<TPI, LL>(slot, A, B, tig);
    }
    // the LL = 19 layout -> the L = 37 layout of the n^2 engine (limbs >= S are zero)
    uint32_t a[L], b[L], t[L];
    {
      int tt = tig;
      asm volatile("" : "+v"(tt));
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const int idx = tt * L + i;
        a[i] = idx < S ? slot[idx] : 0u;
        b[i] = idx < S ? slot[S + idx] : 0u;
      }
    }
    copy_g_to_lds<TPI>(slot, K->nR, tig);
    montmul<TPI>(t, b, slot, TPI, m2, K->mprime2, lane, tig);   // n B mod n^2 (< 2 n^2)
    uint64_t P[L];
#pragma unroll
    for (int i = 0; i < L; ++i) P[i] = (uint64_t)t[i] + a[i];
    normalize<TPI>(P, t, lane, tig);
    cond_sub<TPI>(t, m2, lane, tig);
    cond_sub<TPI>(t, m2, lane, tig);
    emit_words<TPI>(slot, t, p.dst.ct + ee * p.dst.ct_words, p.dst.ct_words, valid, tig);
  }
}

}  // namespace fpai
