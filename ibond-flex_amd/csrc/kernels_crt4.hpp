// CRT encryption for holders of a 2049..4096-bit private key above the row kernels' range: kernels_crt.hpp's
// identity, r^n mod p_h^2 = (r^(q_h mod (p_h - 1)) mod p_h)^(p_h) mod p_h^2, over the S = 74 limbs of p_h, where
// the lane kernels (k_crt_a, k_crt_b_pair) stop at 37. Same ciphertext bits as k_encrypt<8>.
//
//   k_crt4_pre stage A, one element-half per lane: r R mod p_h by K CIOS passes over r's S-limb chunks against
//              R^(K+1) mod p_h (setup_rows4096's stage-A half)
//   k_crt4_a   the lane machine's op list over q_h mod (p_h - 1) (the list run_lane_program reads), in place. The operand and the 64-bit accumulator row stay in
//              registers, the modulus is wave-uniform (blockIdx.y is the half), and the multiplier is one LDS row
//              per lane, read a digit per CIOS step (kernels_dec4.hpp's d4_pass on a single lane); squares run
//              bn_lane.hpp's triangle (1.5 S^2 MACs). No closing product: y_h stays in Montgomery form.
//   k_crt4_b   stage B on split pairs (kernels_dec4.hpp's d4r_run, one element-half per lane pair): the pair
//              (y_h R mod p_h, 0) is the Montgomery form of some x == y_h (mod p_h), and x^(p_h) mod p_h^2 depends
//              on x mod p_h only. The op list over p_h, the closing product with the plain pair of the CRT
//              coefficient (which leaves Montgomery form), the canonical pair, and u_h = A + p_h B as 2 S limbs.
//   k_crt_fin<8> (kernels_crt.hpp) recombines, unchanged: it reads u as [2][2 S][n].
#pragma once
#include "kernels_dec4.hpp"

namespace fpai {

constexpr int C4_ROW = D4_S + 1;   // LDS words of a stage-A lane's multiplier row (odd stride: conflict-free reads)

struct Crt4Half {          // stage B
  const uint32_t* p;       // p_h, S limbs
  const uint32_t* X1;      // (1 - R) mod p_h
  const uint32_t* coef;    // plain pair of (q_h^2)^-1 mod p_h^2, resp. (p_h^2)^-1 mod q_h^2 ([A: S][B: S])
  const uint32_t* prog;    // op list over p_h
  int nprog;
  uint32_t mprime;
};

struct Crt4Params {
  const CrtHalf* ha;       // [2] stage A: p_h, R^(K+1) mod p_h, op list over q_h mod (p_h - 1)
  const Crt4Half* hb;      // [2] stage B
  long long n;             // elements
  EncObf rnd;              // PAI_OBF_GIVEN or PAI_OBF_RNG (then rnd.r_words <= RBUF_WORDS)
  int kchunks;             // ceil(32 rnd.r_words / (LB S)) <= KMAX_CHUNKS
  uint32_t* y;             // [2][S][n]: y_h R mod p_h (< 2 p_h)
  uint32_t* u;             // [2][2 S][n]
  uint32_t* scratch;       // per-lane tiles (LaneScratch, tile_quads<S> quads per tile)
};

// ---------------------------------------------------------------- stage A
// waves per SIMD the two chains are built for (measurement builds: tools/crt4_ab.py --lib). At two waves both spill to
// scratch (k_crt4_a 144 B, k_crt4_b 700 B per lane) and measured slower (stage B 1 657 -> 2 405 ms per 262 144 elements)
#ifndef FPAI_CRT4_OCC_A
#define FPAI_CRT4_OCC_A 1
#endif
#ifndef FPAI_CRT4_OCC_B
#define FPAI_CRT4_OCC_B 1
#endif
// (an opaque copy of the lane index: LICM would otherwise hoist the quad addresses of a constant tile out of the
// element loop and keep them live across the products; kernels_pe4.hpp)
__device__ __forceinline__ LaneScratch c4_opaque(const LaneScratch& t) {
  uint32_t l = t.lid;
  asm volatile("" : "+v"(l));
  return LaneScratch{t.scratch, t.nl, l};
}

// x~ = r R mod p_h, one element-half per lane: K passes over r's chunks of S digits (this lane's LDS row) with
// a = R^(K+1) mod p_h on one accumulator row (invariant T < a + p_h < 2 p_h for any digits < 2^LB)
template <int S>
__global__ __launch_bounds__(LANE_BLOCK, 1) void k_crt4_pre(Crt4Params p) {
  constexpr int TQ = tile_quads<S>();
  __shared__ uint32_t lds[LANE_BLOCK * C4_ROW];
  const int half = blockIdx.y;
  const CrtHalf* H = p.ha + half;
  uint32_t m[S];
#pragma unroll
  for (int j = 0; j < S; ++j) m[j] = (uint32_t)__builtin_amdgcn_readfirstlane(H->m[j]);   // SGPRs
  const uint32_t mprime = H->mprime;
  const uint32_t* cK = H->c0 + (size_t)(p.kchunks - 1) * S;    // R^(K+1) mod p_h
  uint32_t* row = lds + threadIdx.x * C4_ROW;
  const LaneScratch tl = lane_scratch(p.scratch);
  const bool given = p.rnd.obf == 1;
  const int nw = p.rnd.r_words;
  for (long long base = (long long)blockIdx.x * LANE_BLOCK; base < p.n; base += (long long)gridDim.x * LANE_BLOCK) {
    const long long i = base + threadIdx.x;
    const long long ii = i < p.n ? i : p.n - 1;
    // r's words: the caller's (GIVEN) or this element's ChaCha stream staged in the lane scratch (as k_crt_a)
    const uint32_t* rg = given ? p.rnd.r + ii * p.rnd.r_stride : nullptr;
    if (!given) {
      const unsigned long long g = p.rnd.index_base + (unsigned long long)ii;
      for (int b = 0; b * 16 < nw; ++b) {
        uint32_t blk[16];
        obf_stream_block(p.rnd.rng_key, b, g, blk);
#pragma unroll
        for (int w = 0; w < 4; ++w)
          tl.quad(LANE_NTILE * TQ + b * 4 + w) = make_uint4(blk[4 * w], blk[4 * w + 1], blk[4 * w + 2], blk[4 * w + 3]);
      }
    }
    auto rw = [&](int wi) -> uint32_t {
      if (wi >= nw) return 0u;
      if (given) return rg[wi];
      const uint4 v = tl.quad(LANE_NTILE * TQ + (wi >> 2));
      const int c = wi & 3;
      return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w;
    };
    uint32_t t[S];   // the running value, normalised between passes so that only S words live while a row is cut
#pragma unroll
    for (int j = 0; j < S; ++j) t[j] = 0u;
#pragma unroll 1
    for (int k = 0; k < p.kchunks; ++k) {
      d4_fence();
#pragma unroll 1
      for (int j = 0; j < S; ++j) {
        const int bit = (k * S + j) * lane::LB, wi = bit >> 5, sh = bit & 31;
        const uint64_t w2 = ((uint64_t)rw(wi + 1) << 32) | rw(wi);
        row[j] = (uint32_t)(w2 >> sh) & lane::LMASK;
      }
      d4_fence();
      uint32_t a[S];
#pragma unroll
      for (int j = 0; j < S; ++j) a[j] = cK[j];
      uint64_t P[S];
#pragma unroll
      for (int j = 0; j < S; ++j) P[j] = t[j];
      d4_pass<S>(P, a, row, 0, m, mprime, false, std::make_integer_sequence<int, S>{});
      lane::normalize<S>(P, t);
    }
    if (i < p.n) {
#pragma unroll
      for (int j = 0; j < S; ++j) p.y[((size_t)half * S + j) * p.n + i] = t[j];
    }
  }
}

// y_h R = (r R)^(e_h) mod p_h in place over p.y: the lane machine (kernels_crt.hpp's op list) without the closing
// product, so y_h stays in Montgomery form
template <int S>
__global__ __launch_bounds__(LANE_BLOCK, FPAI_CRT4_OCC_A) void k_crt4_a(Crt4Params p) {
  constexpr int TQ = tile_quads<S>();
  using Q = std::make_integer_sequence<int, TQ>;
  __shared__ uint32_t lds[LANE_BLOCK * C4_ROW];
  const int half = blockIdx.y;
  const CrtHalf* H = p.ha + half;
  uint32_t m[S];
#pragma unroll
  for (int j = 0; j < S; ++j) m[j] = (uint32_t)__builtin_amdgcn_readfirstlane(H->m[j]);   // SGPRs
  const uint32_t mprime = H->mprime;
  const int nprog = H->nprog;
  const uint32_t* prog = H->prog;
  uint32_t* row = lds + threadIdx.x * C4_ROW;                  // this lane's multiplier
  const LaneScratch tl = lane_scratch(p.scratch);
  for (long long base = (long long)blockIdx.x * LANE_BLOCK; base < p.n; base += (long long)gridDim.x * LANE_BLOCK) {
    const long long i = base + threadIdx.x;
    const long long ii = i < p.n ? i : p.n - 1;
    uint32_t a[S];
#pragma unroll
    for (int j = 0; j < S; ++j) a[j] = p.y[((size_t)half * S + j) * p.n + ii];
    d4r_tile_store<S>(c4_opaque(tl), 0, a, Q{});
#pragma unroll 1
    for (int o = 0; o < nprog; ++o) {
      const uint32_t op = lane_op(prog, o);
      if (op & LOP_A_FROM_T) d4r_tile_load<S>(tl, (op >> 16) & 0xFF, a, Q{});
      if (op & LOP_SQR) {
        if (op & LOP_PREFETCH) d4_tile_load<S>(tl, (op >> 8) & 0xFF, row, Q{});   // the next product's multiplier
        lane::mont_sqr<S>(a, m, mprime);
      } else {
        if (!(op & LOP_B_READY)) d4_tile_load<S>(tl, (op >> 8) & 0xFF, row, Q{});
        uint64_t P[S];
#pragma unroll
        for (int j = 0; j < S; ++j) P[j] = 0;
        d4_pass<S>(P, a, row, 0, m, mprime, false, std::make_integer_sequence<int, S>{});
        lane::normalize<S>(P, a);
      }
      if (op & LOP_STORE) d4r_tile_store<S>(tl, op >> 24, a, Q{});
      if (op & LOP_B_SET) {
        d4_fence();
#pragma unroll
        for (int j = 0; j < S; ++j) row[j] = a[j];
        d4_fence();
      }
    }
    if (i < p.n) {
#pragma unroll
      for (int j = 0; j < S; ++j) p.y[((size_t)half * S + j) * p.n + i] = a[j];
    }
  }
}

// ---------------------------------------------------------------- stage B: u_h = y_h^(p_h) coef_h mod p_h^2
// one row of the plain product A + p B: P += p B_J, limb J retires (written out), its carry moves up
template <int S, int J>
__device__ __forceinline__ void c4_wide_step(uint64_t (&P)[S], const uint32_t (&m)[S], const uint32_t* __restrict__ dig,
                                             uint32_t& cur, uint32_t* __restrict__ out, size_t stride, bool wr) {
  const uint32_t y = cur;
  if constexpr (J + 1 < S) cur = dig[J + 1];
#pragma unroll
  for (int i = 0; i < S; ++i) P[(i + J) % S] += (uint64_t)m[i] * y;
  if (wr) out[(size_t)J * stride] = (uint32_t)P[J] & lane::LMASK;
  P[(J + 1) % S] += P[J] >> lane::LB;
  P[J] = 0;
  lane::pin<S>(P);
  __builtin_amdgcn_sched_barrier(0);
}
template <int S, int... Js>
__device__ __forceinline__ void c4_wide(uint64_t (&P)[S], const uint32_t (&m)[S], const uint32_t* __restrict__ dig,
                                        uint32_t* __restrict__ out, size_t stride, bool wr, std::integer_sequence<int, Js...>) {
  uint32_t cur = dig[0];
  (c4_wide_step<S, Js>(P, m, dig, cur, out, stride, wr), ...);
}

template <int S>
__global__ __launch_bounds__(LANE_BLOCK, FPAI_CRT4_OCC_B) void k_crt4_b(Crt4Params p) {
  constexpr int TQ = tile_quads<S>();
  using Q = std::make_integer_sequence<int, TQ>;
  __shared__ uint32_t lds[D4_PAIRS * D4R_SLOT + S];
  const int half = blockIdx.y;
  const Crt4Half* H = p.hb + half;
  uint32_t m[S];
#pragma unroll
  for (int j = 0; j < S; ++j) m[j] = H->p[j];
  const uint32_t mprime = H->mprime;
  const int nprog = H->nprog;
  const uint32_t* prog = H->prog;
  const uint32_t* cf = H->coef;
  uint32_t* x1 = lds + D4_PAIRS * D4R_SLOT;   // (1 - R) mod p_h: the odd row's start in squares
  for (int i = threadIdx.x; i < S; i += blockDim.x) x1[i] = H->X1[i];
  __syncthreads();
  const int tig = threadIdx.x & 1;
  const bool odd = tig != 0;
  const int pib = threadIdx.x >> 1;
  uint32_t* st = lds + pib * D4R_SLOT;
  const LaneScratch tl = lane_scratch(p.scratch);
  for (long long base = (long long)blockIdx.x * D4_PAIRS; base < p.n; base += (long long)gridDim.x * D4_PAIRS) {
    const long long e = base + pib;
    const bool valid = e < p.n;
    const long long ee = valid ? e : p.n - 1;
    uint32_t a[S];   // this lane's component (the even lane A = y_h R mod p_h, the odd lane B = 0)
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const uint32_t v = p.y[((size_t)half * S + i) * p.n + ee];
      a[i] = odd ? 0u : v;
    }
    d4r_tile_store<S>(c4_opaque(tl), 0, a, Q{});
    d4r_run<S>(a, st, tl, prog, nprog, x1, m, mprime, tig, [=](uint32_t* dst) {
#pragma unroll
      for (int j = 0; j < S; ++j) dst[j] = cf[tig * S + j];
    });
    // the canonical pair of the plain (A < 2p, B < 4p): A >= p moves one p into B
    {
      uint32_t d[S];
      const bool lt = lane::sub<S>(a, m, d);
      const uint32_t ge = lt ? 0u : 1u;
      uint32_t c = __builtin_amdgcn_update_dpp(0u, ge, 0xA0, 0xF, 0xF, false) & (odd ? 1u : 0u);   // the even lane's
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const uint32_t v = ((odd || lt) ? a[j] : d[j]) + c;
        a[j] = v & lane::LMASK;
        c = v >> lane::LB;
      }
#pragma unroll 1
      for (int r = 0; r < 4; ++r) lane::cond_sub<S>(a, m);   // (the even lane's A < p already)
    }
    // u = A + p B over 2 S limbs: B's digits and A's limbs through the pair's LDS slot, both lanes run the rows
    d4_fence();
#pragma unroll
    for (int j = 0; j < S; ++j) st[tig * S + j] = a[j];
    d4_fence();
    {
      uint64_t P[S];
#pragma unroll
      for (int j = 0; j < S; ++j) P[j] = st[j];
      uint32_t* out = p.u + (size_t)half * 2 * S * p.n + ee;
      const bool wr = valid && !odd;
      c4_wide<S>(P, m, st + S, out, (size_t)p.n, wr, std::make_integer_sequence<int, S>{});
      uint32_t hi[S];
      lane::normalize<S>(P, hi);
      if (wr) {
#pragma unroll
        for (int j = 0; j < S; ++j) out[(size_t)(S + j) * p.n] = hi[j];
      }
    }
    d4_fence();
  }
}

}  // namespace fpai
