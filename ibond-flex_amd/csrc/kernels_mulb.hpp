// Broadcast multiply (pai_mul_bcast[_dev]): ciphertext i meets the F scalars of row i of a plain matrix and nothing is
// summed -- `enc[:, None] * X`, an outer product, per-sample residual x feature rows. Output (i, j) is what k_mul gives
// for ciphertext i and x[i][j] (kernels_mul.hpp): c_i^|M_ij| mod n^2, flagged for the batch inversion where M_ij < 0.
// The F outputs of a row are powers of ONE base, so the row shares a fixed-base comb instead of F window chains:
//
//   T_i[t][d] = c_i^(d 16^t) R mod n^2,  t = 0 .. 15, d = 0 .. 15   (Montgomery form; d = 0 is R, so a zero digit needs
//                                                                    no branch)
//   out[i][j] = prod_t T_i[t][digit t of |M_ij|]                     at most 16 products and NO squaring
//
//   k_mulb_plan      one wave per row: encodes the row's scalars ONCE (encode_elem, the encoder of k_mul) into |M|, the
//                    output exponent, the status and the inversion flag, and finds the row's window count top_i (the
//                    windows above it are neither built nor read)
//   k_mulb_tab<TPI>  phase 0, one lane group per ciphertext: x~ = c R, then T[t][1] from T[t-1][1] by four squarings;
//                    phase 1, one lane group per (ciphertext, window): T[t][0] = R and T[t][d] = T[t][d-1] T[t][1].
//                    The 4 top_i - 4 squarings are the only serial part; the 14 products of a window run beside those
//                    of the other windows, so a call of few ciphertexts still fills the chip.
//   k_mulb_acc<TPI>  one WAVE per (ciphertext, tile of 64 / TPI columns): the wave stages window t's 16 entries
//                    (16 S limbs) in its own LDS buffer with 16-byte loads, every lane group multiplies its register
//                    accumulator by the entry of its digit, read from that buffer as the product's B operand (no
//                    per-group copy); a window in which no group of the wave has a digit is neither staged nor
//                    multiplied. No block barrier: the four waves of a block may serve different rows with different
//                    window counts. Leaves the Montgomery domain, reduces, writes the words.
//
// Lane-group engine (bn_group.hpp, 28-bit limbs), table rows in the layout k_mm_tab writes.
#pragma once
#include "kernels.hpp"

namespace fpai {

constexpr int MULB_WIN = 16;    // 4-bit windows of a magnitude of up to 64 bits (INT64_MIN: digit 8 of window 15)

// limbs of one ciphertext's comb at group size tpi: [MULB_WIN][16][S]
constexpr size_t mulb_entry_limbs(int tpi) { return (size_t)MULB_WIN * 16 * tpi * L; }

struct MulbPlanParams {
  const int32_t* exp;     // ciphertext exponents [N]
  const void* x;          // scalars [N][F]
  int dtype;              // PAI_F32 / PAI_F64 / PAI_I64
  long long N, F;
  uint64_t* mag;          // [N][F] |M| (0 where the scalar does not encode)
  int32_t* exp_out;       // [N][F] exp_i + e_s
  int32_t* status;        // [N][F] (nullable)
  uint8_t* neg;           // [N][F] 1 where the output still needs the inversion
  int32_t* rowtop;        // [N] windows the row uses: 0 (every |M| is 0) .. 16
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_mulb_plan(MulbPlanParams p) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * 4;
  for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < p.N; i += nwaves) {
    const int e = p.exp[i];
    int top = 0;
    for (long long j = lane; j < p.F; j += 64) {
      const long long o = i * p.F + j;
      int64_t M = 0;
      int es = 0;
      const int st = encode_elem(p.x, p.dtype, 0, 0, o, M, es);
      if (st != ST_OK) M = 0;
      const uint64_t mg = M < 0 ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
      p.mag[o] = mg;
      p.exp_out[o] = e + es;
      p.neg[o] = M < 0 ? 1 : 0;
      if (p.status) p.status[o] = st;
      if (mg) top = max(top, (67 - __clzll(mg)) / 4);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) top = max(top, __shfl_xor(top, s));
    if (lane == 0) p.rowtop[i] = top;
  }
}

struct MulbTabParams {
  const uint32_t* ct;       // [N][W]
  const int32_t* rowtop;    // [N]
  long long i0, nb;         // the block of ciphertexts i0 .. i0 + nb
  int phase;                // 0: T[t][1]; 1: T[t][0] and T[t][2 .. 15]
  uint32_t* tab;            // [nb][MULB_WIN][16][S]
  const uint32_t* N;        // n^2
  const uint32_t* R2;       // R^2 mod n^2
  const uint32_t* oneR;     // R mod n^2
  uint32_t mprime;
  int ct_words;
};

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_mulb_tab(MulbTabParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long n = p.phase ? p.nb * MULB_WIN : p.nb;

  for (long long base = (long long)blockIdx.x * GPB; base < n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < n;
    const long long t = valid ? inst : n - 1;
    const long long il = p.phase ? t / MULB_WIN : t;
    const int top = valid ? p.rowtop[p.i0 + il] : 0;
    uint32_t* ent = p.tab + (size_t)il * (MULB_WIN * 16 * S);
    uint32_t tt[L];
    if (p.phase == 0) {
      int wtop = top;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) wtop = max(wtop, __shfl_xor(wtop, s));
      if (wtop == 0) continue;
      words_to_limbs(p.ct + (p.i0 + il) * p.ct_words, p.ct_words, tt, tig);
      copy_g_to_lds<TPI>(slot, p.R2, tig);
      montmul<TPI>(tt, tt, slot, TPI, m, p.mprime, lane, tig);       // x~ = c R
      for (int w = 0; w < wtop; ++w) {
        if (w < top) store_limbs_g<TPI>(ent + (size_t)(w * 16 + 1) * S, tt, tig);
        if (w + 1 == wtop) break;
#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
          write_limbs_lds<TPI>(slot, tt, tig);
          montmul<TPI>(tt, tt, slot, TPI, m, p.mprime, lane, tig);
        }
      }
    } else {
      const int w = (int)(t % MULB_WIN);
      const bool active = w < top;
      if (ballot(active) == 0ull) continue;                          // a wave of windows no scalar reaches
      uint32_t* rows = ent + (size_t)w * 16 * S;
      load_limbs_g<TPI>(p.oneR, tt, tig);
      if (active) store_limbs_g<TPI>(rows, tt, tig);                 // digit 0: R
      load_limbs_g<TPI>(active ? rows + S : p.oneR, tt, tig);        // T[w][1], phase 0's
      write_limbs_lds<TPI>(slot, tt, tig);
#pragma clang loop unroll(disable)
      for (int r = 2; r < 16; ++r) {
        montmul<TPI>(tt, tt, slot, TPI, m, p.mprime, lane, tig);
        if (active) store_limbs_g<TPI>(rows + (size_t)r * S, tt, tig);
      }
    }
  }
}

struct MulbAccParams {
  const uint64_t* mag;      // [N][F]
  const int32_t* rowtop;    // [N]
  long long F;
  long long i0, nb;         // the block of ciphertexts whose combs are in tab
  const uint32_t* tab;
  uint32_t* out;            // [N][F][W]
  const uint32_t* N;
  const uint32_t* oneR;
  uint32_t mprime;
  int ct_words;
};

// LDS of k_mulb_acc: per wave ONE stage buffer of 16 S limbs, which after the last window doubles as the output slots
// of the wave's 64 / TPI groups (64 L limbs: more than 16 S at TPI 2 only). 37 KiB a block at TPI 2 and 4, 74 KiB at
// TPI 8: two blocks a CU at every size, which is what the registers allow (250 VGPRs, no spill, at TPI 2, 4 and 8 with
// mulb_stage below). The product leaves 6 registers over, so a second buffer filled through registers during the
// product spilled 22 VGPRs at TPI 2 and 76 at TPI 4 and was dropped: the copy of the next window is covered by the
// SIMD's other wave only. (A second buffer filled by direct global-to-LDS loads has not been tried.)
constexpr int mulb_wave_limbs(int tpi) { return (16 * tpi > 64 ? 16 * tpi : 64) * L; }
constexpr size_t mulb_acc_lds_bytes(int tpi) { return (size_t)(BLOCK / 64) * mulb_wave_limbs(tpi) * 4; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One window's 16 entries (ROW4 16-byte pieces) from global memory into the wave's LDS buffer, through the lane's
// registers, in passes of at most MULB_PASS pieces a lane (16 VGPRs: the loads of a pass are all issued before its
// first store waits for one). A lane past the end loads the last piece again and stores nothing. The lane index is an
// opaque copy: otherwise LICM hoists the per-piece 64-bit addresses out of the window loop and they stay live across
// the product, which has no register to spare (they spilled at TPI 4 and 8).
constexpr int MULB_PASS = 4;
template <int ROW4, int K0, int... Ks>
__device__ __forceinline__ void mulb_stage_pass(uint32_t* buf, const u32x4* __restrict__ g, int lane,
                                                std::integer_sequence<int, Ks...>) {
  u32x4 pf[sizeof...(Ks)];
  ((pf[Ks] = g[min(lane + 64 * (K0 + Ks), ROW4 - 1)]), ...);
  ((lane + 64 * (K0 + Ks) < ROW4 ? (void)(reinterpret_cast<u32x4*>(buf)[lane + 64 * (K0 + Ks)] = pf[Ks]) : (void)0), ...);
  __builtin_amdgcn_sched_barrier(0);              // one pass's registers at a time
}
template <int ROW4, int... Ps>
__device__ __forceinline__ void mulb_stage(uint32_t* buf, const u32x4* __restrict__ g, int lane,
                                           std::integer_sequence<int, Ps...>) {
  constexpr int PF = (ROW4 + 63) / 64;            // pieces per lane
  asm volatile("" : "+v"(lane));
  wave_lds_fence();
  (mulb_stage_pass<ROW4, Ps * MULB_PASS>(
       buf, g, lane, std::make_integer_sequence<int, (PF - Ps * MULB_PASS < MULB_PASS ? PF - Ps * MULB_PASS : MULB_PASS)>{}),
   ...);
  wave_lds_fence();
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_mulb_acc(MulbAccParams p) {
  constexpr int S = TPI * L;
  constexpr int CW = 64 / TPI;                    // columns of a wave's tile
  constexpr int ROW4 = 16 * S / 4;                // 16-byte pieces of one window's 16 entries
  constexpr auto KS = std::make_integer_sequence<int, ((ROW4 + 63) / 64 + MULB_PASS - 1) / MULB_PASS>{};   // passes
  static_assert(mulb_wave_limbs(TPI) >= 16 * S && mulb_wave_limbs(TPI) >= CW * S, "stage buffer / output slots");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = lane % TPI;
  const int gw = lane / TPI;
  uint32_t* wbuf = smem + (threadIdx.x >> 6) * mulb_wave_limbs(TPI);
  uint32_t* slot = wbuf + gw * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long ntw = (p.F + CW - 1) / CW, n = p.nb * ntw;
  const long long nwaves = (long long)gridDim.x * (BLOCK / 64);

  for (long long u = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); u < n; u += nwaves) {
    const long long il = u / ntw, j = (u % ntw) * CW + gw;
    const bool valid = j < p.F;                   // a tail tile's spare groups repeat the last column and write nothing
    const size_t o = (size_t)(p.i0 + il) * p.F + (valid ? j : p.F - 1);
    const uint64_t mg = p.mag[o];
    const int top = p.rowtop[p.i0 + il];          // wave-uniform: one row per wave
    const u32x4* rows = reinterpret_cast<const u32x4*>(p.tab + (size_t)il * (MULB_WIN * 16 * S));
    uint32_t a[L];
    load_limbs_g<TPI>(p.oneR, a, tig);
#pragma clang loop unroll(disable)
    for (int w = 0; w < top; ++w) {
      const int dig = (int)((mg >> (4 * w)) & 15u);
      if (ballot(dig != 0) == 0ull) continue;     // no group of the wave has a digit here: neither staged nor multiplied
      mulb_stage<ROW4>(wbuf, rows + (size_t)w * ROW4, lane, KS);
      montmul<TPI>(a, a, wbuf + dig * S, TPI, m, p.mprime, lane, tig);   // digit 0 reads R: the product keeps a
    }
    write_one_lds<TPI>(slot, tig);
    montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);           // leave the Montgomery domain
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(slot, a, p.out + o * p.ct_words, p.ct_words, valid, tig);
  }
}

}  // namespace fpai
