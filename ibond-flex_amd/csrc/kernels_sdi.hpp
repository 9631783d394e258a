// Segmented weighted sums over index lists that are device memory (pai_segment_dot_idx_dev): the sum of kernels_sd.hpp,
//
//   out_s = prod_{t in segment s} (c[index[t]]^+-1)^(|M_t| 16^(E_s - e_t)) mod n^2,   e_t = exp[index[t]] + e(x[t]),
//
// without the two things the host did for it there: no numbering of the call's distinct ciphertexts (the window tables
// of a row live in LDS and are built from ct[index[t]] as it comes) and no inversion per ciphertext (a row keeps the
// product P of its non-negative terms and the product N of the magnitudes of its negative ones, both at the row's E;
// the segment's N is inverted once at the end, out = P N^-1: the same residue, so the same bits).
//
//   k_sdi_rows<TPI>  ONE WAVE per row of k_seg_rows (at most 16 consecutive entries of one segment): the G = 64 / TPI
//                    lane groups of the wave are the row's team.
//     scalars   lanes 0 .. 15 encode one scalar each as k_mul does (status, |M|, sign, e = exp[index[t]] + e(x[t])) into
//               LDS; E = the largest e of the row's real operands, zero terms included.
//     tables    group kk % G builds c~ = c R, c~^2, c~^3 (Montgomery form) of operand kk in LDS: 3 rows of S limbs per
//               operand, 2-bit windows. Operands with |M| = 0 get none.
//     windows   the effective exponents |M_t| 4^(2 (E - e_t)) are never formed (window w of operand t is bits 2 sh, 2 sh
//               + 1 of |M_t|, sh = w - 2 (E - e_t)). Their range [0, wtop) is cut into G contiguous slices of len =
//               ceil(wtop / G) windows; group g walks slice g from its top window down: two squarings of each of its
//               two accumulators, then one product per operand with a non-zero digit, into P or N by the operand's
//               sign. Both accumulators of every group live in LDS, so an accumulator is chosen by address and the
//               table row is the product's register operand. A long exponent spread makes the slices longer.
//     join      Horner over the slices from the top one down, J = J^(4^len) R_g: group 0 runs the P chain, group 1 the
//               N chain at the same time (2 len squarings and one product per slice).
//     output    P and N leave the Montgomery domain and go out with E in k_add's operand layout ([rows][W], [rows]).
//               A row without operands (past the level's real count, or an empty segment) writes 1, 1 and INT32_MIN.
//   Every product of the kernel goes through one montmul site: the groups of the wave run in lock step, a group
//   without work in a step multiplies its own P accumulator into registers and stores nothing, and a step in which no
//   group has work is skipped.
//
//   k_sdi_fill       only when the lists are bad: the segments' N become 1, so that the batch inversion behind it works
//                    on defined values (its kernels are not gated on the check words).
//   k_sdi_out        the gated copy of the finished sums, exponents and statuses to the caller's arrays: nothing is
//                    written when a check word is set or the inversion found a value without inverse (bad[2] = 1 then).
//
// Lane-group engine (bn_group.hpp). Model count per full row at 64-bit magnitudes without spread (G = 16): 32 table
// products, 16 * 32 * 3/4 = 384 digit products and 2 * 2 * 32 squarings in the slices, (G - 1)(2 len + 1) = 75 per join
// chain; the dependent chain is len (4 + 16) + (G - 1)(2 len + 1) + 4 = 119 products, against 85 of one k_mul term.
#pragma once
#include "engine_res.hpp"
#include "kernels.hpp"

namespace fpai {

constexpr int SDI_WAVE = 64;                 // lanes per block: one wave, one row at a time
constexpr int SDI_META_WORDS = SEGPLAN_C * 6;   // |M| (64 bits), ciphertext row (64 bits), e and sign of 16 operands

// dynamic LDS of k_sdi_rows in 32-bit words: R^2, R, 1 | [16][3][S] tables | [G][2][S] accumulators | scalars
constexpr size_t sdi_lds_bytes(int tpi) {
  return ((size_t)(3 + 3 * SEGPLAN_C) * tpi * L + (size_t)2 * SDI_WAVE * L + SDI_META_WORDS) * 4;
}

struct SdiRowsParams {
  const uint32_t* ct;        // [N][W]
  const int32_t* exp;        // [N]
  const long long* index;    // [total], checked by k_check_idx
  const void* x;             // [total] scalars
  int dtype;
  const long long* gidx;     // [rows][16]: k_seg_rows of level 0 without an index, so POSITIONS t of the lists, -1 past
  long long rows;
  uint32_t* outP;            // [rows][W]
  uint32_t* outN;            // [rows][W]
  int32_t* pexp;             // [rows]
  int32_t* pexp2;            // nullable: a second copy of pexp (the N operands' exponents when the rows are the segments)
  int32_t* status;           // [total] nullable: k_mul's status of every entry
  unsigned long long* bad;   // the call's check words; bad[3] = the smallest t whose scalar does not encode
  const long long* gate;
  const uint32_t* N;         // n^2, R^2 mod n^2, R mod n^2: S limbs, group layout
  const uint32_t* R2;
  const uint32_t* oneR;
  uint32_t mprime;
  int ct_words;
};

template <int TPI>
__global__ __launch_bounds__(SDI_WAVE) void k_sdi_rows(SdiRowsParams p) {
  constexpr int S = TPI * L;
  constexpr int G = SDI_WAVE / TPI;
  constexpr int C = SEGPLAN_C;
  constexpr int ROUNDS = (C + G - 1) / G;
  static_assert(G >= 2 && (((3 + 3 * C) * S + 2 * SDI_WAVE * L) & 1) == 0, "two join workers; 8-byte aligned scalars");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  if (add_gate_shut(p.gate)) return;
  const int lane = threadIdx.x;
  const int tig = lane % TPI;
  const int gib = lane / TPI;
  uint32_t* cR2 = smem;
  uint32_t* cR = smem + S;
  uint32_t* cOne = smem + 2 * S;
  uint32_t* tab = smem + 3 * S;
  uint32_t* acc = tab + 3 * C * S;
  uint64_t* mags = reinterpret_cast<uint64_t*>(acc + 2 * G * S);
  long long* srcs = reinterpret_cast<long long*>(mags + C);
  int* eks = reinterpret_cast<int*>(srcs + C);
  int* negs = eks + C;
  uint32_t* myP = acc + (gib * 2) * S;
  uint32_t* myN = myP + S;
  const bool wkP = gib == 0, wkN = gib == 1;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  for (int i = lane; i < S; i += SDI_WAVE) {
    cR2[i] = p.R2[i];
    cR[i] = p.oneR[i];
    cOne[i] = i == 0 ? 1u : 0u;
  }
  const int W = p.ct_words;

  for (long long row = blockIdx.x; row < p.rows; row += gridDim.x) {
    wave_lds_fence();
    if (lane < C) {
      const long long t = p.gidx[row * C + lane];
      uint64_t mg = 0;
      long long src = -1;
      int ek = INT32_MIN, ng = 0;
      if (t >= 0) {
        int64_t M = 0;
        int es = 0;
        const int st = encode_elem(p.x, p.dtype, 0, 0, t, M, es);
        if (st != ST_OK) {
          M = 0;
          atomicMin(p.bad + 3, (unsigned long long)t);
        }
        if (p.status) p.status[t] = st;
        src = p.index[t];
        ek = p.exp[src] + es;
        ng = M < 0 ? 1 : 0;
        mg = M < 0 ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
      }
      mags[lane] = mg;
      srcs[lane] = src;
      eks[lane] = ek;
      negs[lane] = ng;
    }
    wave_lds_fence();
    int nreal = 0, E = INT32_MIN;
    bool hasneg = false;
    for (int kk = 0; kk < C; ++kk) {
      if (srcs[kk] < 0) break;                                       // the real operands come first
      ++nreal;
      E = max(E, eks[kk]);                                           // zero terms count: the value 1 with its exponent
      hasneg = hasneg || negs[kk] != 0;
    }
    if (nreal == 0) {
      for (int j = lane; j < W; j += SDI_WAVE) {
        p.outP[row * W + j] = j == 0 ? 1u : 0u;
        p.outN[row * W + j] = j == 0 ? 1u : 0u;
      }
      if (lane == 0) {
        p.pexp[row] = RES_EMPTY_EXP;
        if (p.pexp2) p.pexp2[row] = RES_EMPTY_EXP;
      }
      continue;
    }
    long long wtop = 0;                                              // 2-bit windows of the widest effective exponent
    for (int kk = 0; kk < nreal; ++kk) {
      const uint64_t mg = mags[kk];
      if (mg) wtop = max(wtop, (long long)((65 - __clzll(mg)) / 2) + 2 * ((long long)E - eks[kk]));
    }
    const long long len = (wtop + G - 1) / G;                        // windows per slice
    const int gtop = wtop > 0 ? (int)((wtop - 1) / len) : 0;         // the top slice that holds a window
    const long long wbase = (long long)gib * len + len - 1;          // this group's window at step 0

    // operands -> limbs, plain, into row 0 of their tables (the group's P slot is the staging area)
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
      const int kk = r * G + gib;
      const bool act = kk < nreal && mags[min(kk, C - 1)] != 0;
      // uniform over the group, and the staging touches the group's own slot only (its fences order LDS traffic for
      // the compiler and are no instructions), so a group without operand loads nothing
      if (act) {
        uint32_t xl[L];
        stage_words_to_limbs<TPI>(myP, p.ct + srcs[kk] * W, W, xl, tig);
#pragma unroll
        for (int i = 0; i < L; ++i) tab[(kk * 3) * S + tig * L + i] = xl[i];
      }
    }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < L; ++i) myP[tig * L + i] = myN[tig * L + i] = cR[tig * L + i];   // both accumulators: 1
    wave_lds_fence();

    uint32_t* const JP = acc + (gtop * 2) * S;                        // the join accumulators: the top slice's
    uint32_t* const myJ = wkN ? JP + S : JP;
    bool stP = false, stN = false;                                   // this group's P / N differs from 1
    uint64_t mP = 0, mN = 0;                                         // ... of all groups, once the slices are done
    bool jP = false, jN = false;                                     // the join accumulators differ from 1
    int phase = 0, op = 0, gcur = 0;
    long long j = 0, q = 0;
#pragma clang loop unroll(disable)
    for (;;) {
      // this group's next product: a <- limbs at srcA, a = a * B, limbs at dst <- a when active
      const uint32_t* srcA = myP;
      const uint32_t* Bp = myP;
      uint32_t* dst = myP;
      bool active = false;
      if (phase == 0) {                                              // tables: c~ = c R^2 R^-1, c~^2, c~^3
        if (op >= 3 * ROUNDS) {
          phase = 1;
          op = 0;
          continue;
        }
        const int kk = (op / 3) * G + gib, s = op % 3;
        uint32_t* row0 = tab + (min(kk, C - 1) * 3) * S;
        srcA = s == 2 ? row0 + S : row0;
        Bp = s == 0 ? cR2 : row0;
        dst = row0 + s * S;
        active = kk < nreal && mags[min(kk, C - 1)] != 0;
        ++op;
      } else if (phase == 1) {                                       // the slices
        if (j >= len) {
          mP = ballot(stP);
          mN = ballot(stN);
          jP = ((mP >> (gtop * TPI)) & 1ull) != 0;
          jN = ((mN >> (gtop * TPI)) & 1ull) != 0;
          gcur = gtop - 1;
          q = 0;
          phase = 2;
          continue;
        }
        if (op < 4) {                                                // two squarings of P, two of N
          uint32_t* a_ = op >= 2 ? myN : myP;
          srcA = Bp = dst = a_;
          active = op >= 2 ? stN : stP;
          ++op;
          if (op == 2 && !hasneg) op = 4;
        } else {
          const int kk = op - 4;
          const long long sh = (wbase - j) - 2 * ((long long)E - eks[kk]);   // window of |M_kk| at chain window w
          const int dig = (kk < nreal && sh >= 0 && sh < 32) ? (int)((mags[kk] >> (2 * (int)sh)) & 3u) : 0;
          const bool ng = negs[kk] != 0;
          uint32_t* a_ = ng ? myN : myP;
          srcA = tab + (kk * 3 + max(dig, 1) - 1) * S;
          Bp = dst = a_;
          active = dig != 0;
          stP = stP || (active && !ng);
          stN = stN || (active && ng);
          if (++op == 4 + C) {
            op = 0;
            ++j;
          }
        }
      } else if (phase == 2) {                                       // Horner over the slices below the top one
        if (gcur < 0) {
          phase = 3;
          continue;
        }
        if (q < 2 * len) {
          srcA = Bp = dst = myJ;
          active = (wkP && jP) || (wkN && jN);
          ++q;
        } else {
          const bool gP = ((mP >> (gcur * TPI)) & 1ull) != 0, gN = ((mN >> (gcur * TPI)) & 1ull) != 0;
          srcA = dst = myJ;
          Bp = acc + (gcur * 2 + (wkN ? 1 : 0)) * S;
          active = (wkP && gP) || (wkN && gN);
          jP = jP || gP;
          jN = jN || gN;
          q = 0;
          --gcur;
        }
      } else if (phase == 3) {                                       // leave the Montgomery domain
        srcA = dst = myJ;
        Bp = cOne;
        active = wkP || wkN;
        phase = 4;
      } else {
        break;
      }
      if (ballot(active) == 0ull) continue;
      wave_lds_fence();
      uint32_t a[L];
#pragma unroll
      for (int i = 0; i < L; ++i) a[i] = srcA[tig * L + i];
      montmul<TPI>(a, a, Bp, TPI, m, p.mprime, lane, tig);
      wave_lds_fence();
      if (active) {
#pragma unroll
        for (int i = 0; i < L; ++i) dst[tig * L + i] = a[i];
      }
      wave_lds_fence();
    }
    uint32_t a[L];
#pragma unroll
    for (int i = 0; i < L; ++i) a[i] = myJ[tig * L + i];
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(myP, a, (wkN ? p.outN : p.outP) + row * W, W, wkP || wkN, tig);
    if (lane == 0) {
      p.pexp[row] = E;
      if (p.pexp2) p.pexp2[row] = E;
    }
  }
}

struct SdiFinParams {
  const long long* gate;     // the two list words of k_check_idx
  const uint32_t* noinv;     // the batch inversion's word (k_sdi_out)
  uint32_t* nrows;           // [nseg][W] the segments' N (k_sdi_fill)
  const uint32_t* prod;      // [nseg][W] P N^-1
  const int32_t* pexp;       // [nseg]
  const int32_t* st;         // [total]
  long long nseg, total;
  int W;
  uint32_t* out;             // the caller's arrays
  int32_t* out_exp;
  int32_t* status;           // nullable
  long long* bad;
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_sdi_fill(SdiFinParams p) {
  if (!add_gate_shut(p.gate)) return;
  const long long n = p.nseg * p.W;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < n; u += (long long)gridDim.x * blockDim.x)
    p.nrows[u] = u % p.W == 0 ? 1u : 0u;
}

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_sdi_out(SdiFinParams p) {
  if (add_gate_shut(p.gate)) return;
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  if (*p.noinv != 0u) {
    if (first == 0) p.bad[2] = 1;
    return;
  }
  const long long n = p.nseg * p.W;
  for (long long u = first; u < n; u += step) p.out[u] = p.prod[u];
  for (long long s = first; s < p.nseg; s += step) p.out_exp[s] = p.pexp[s];
  if (p.status)
    for (long long t = first; t < p.total; t += step) p.status[t] = p.st[t];
}

}  // namespace fpai
