// Prefix sums of ciphertext arrays along an axis (pai_cumsum[_dev]): for a C-contiguous [outer][L][inner] array,
//
//   E_j = max over j' <= j of e_j' ;  out_j = prod over j' <= j of c_j'^(16^(E_j - e_j')) mod n^2   (canonical),
//
// entries with exponent PAD_EXP (the empty segments of pai_segment_add / pai_histogram: ciphertext 1) skipped.
//
//   k_scan<TPI>   one lane group per (o, tile, i): a sequential chain over the tile's positions j, forward or from the
//                 top down. Operands enter in plain form, as in k_add, and the Montgomery factor of the running
//                 product is tracked: acc = P R^rho, rho = 1 at the start (acc = R) and one less after every plain
//                 operand (P R^rho * c * R^-1). Every prefix leaves through a product by the constant R^(1 - rho)
//                 (k_add's RS table: P R^rho * R^(1 - rho) * R^-1 = P, then the conditional subtraction): two products
//                 per element, one of them on the dependent chain. As the constants end at R^(ADD_KMAX + 1), a product
//                 by R^(2 - rho) brings rho back to 1 after ADD_KMAX operands.
//                 Mixed exponents: an operand above the maximum first brings rho back to 1 and squares acc 4 (e - E)
//                 times; an operand below it is parked: acc goes to the group's second LDS slot, the operand is
//                 converted (R^2 * c * R^-1 = c R), squared 4 (E - e) times in the registers and multiplied by the
//                 parked acc, which keeps rho.
//                 With a carry (the blocked scan), the tile's chain starts from the scanned total of the tiles before
//                 it, entered like an operand at its own exponent. emit_all == 0 writes the tile's total only.
//
// The blocked scan (flexpai.hip) is k_scan over tiles for the totals, the same scan over [outer][tiles][inner], and
// k_scan again per tile with the carries. Products of canonical residues mod n^2 are associative and commutative, so
// every tiling gives the same bits.
//
// Every step is one Montgomery product acc * B with a per-group B, at ONE montmul site (k_add's scheme): the groups of
// a wave run in lock step, and a group with nothing to do multiplies by R and drops the result.
#pragma once
#include "kernels.hpp"

namespace fpai {

struct ScanParams {
  const uint32_t* ct;      // [outer][L][inner][W]
  const int32_t* exp;      // [outer][L][inner]
  long long outer, L, inner;
  long long T, tiles;      // tile length, ceil(L / T)
  int reverse;             // 1: positions run from the tile's top down, and the carry comes from tile t + 1
  int emit_all;            // 1: every prefix to out (array layout); 0: the tile's total to out[(o tiles + t) inner + i]
  const uint32_t* carry;   // nullable: [outer][tiles][inner][W], the inclusive scan of the tiles' totals
  const int32_t* carry_exp;
  uint32_t* out;
  int32_t* out_exp;
  const uint32_t* N;
  const uint32_t* R2;      // R^2 mod n^2, limbs
  const uint32_t* oneR;    // R mod n^2, limbs
  const uint32_t* RS;      // [ADD_KMAX + 2][ct_words]: R^s mod n^2, s = 0 .. ADD_KMAX + 1 (32-bit words)
  uint32_t mprime;
  int ct_words;
};

enum : int { SC_IDLE = 0, SC_MUL = 1, SC_SQ = 2, SC_PARK = 3, SC_JOIN = 4, SC_EMIT = 5, SC_NORM = 6 };
enum : int { SP_FETCH = 0, SP_ACCSQ = 1, SP_MUL = 2, SP_TMPSQ = 3, SP_JOIN = 4, SP_EMIT = 5 };

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_scan(ScanParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * 2 * S;
  uint32_t* park = slot + S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long ninst = p.outer * p.tiles * p.inner;

  for (long long base = (long long)blockIdx.x * GPB; base < ninst; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < ninst;
    const long long ii = valid ? inst : ninst - 1;
    const long long i = ii % p.inner, q = ii / p.inner, t = q % p.tiles, o = q / p.tiles;
    const long long j0 = t * p.T, j1 = min(p.L, j0 + p.T), len = j1 - j0;
    const long long ct_ = p.reverse ? t + 1 : t - 1;               // the tile whose scanned total is the carry
    const bool has_carry = p.carry != nullptr && ct_ >= 0 && ct_ < p.tiles;
    const long long cidx = (o * p.tiles + (has_carry ? ct_ : t)) * p.inner + i;

    uint32_t a[L];
    load_limbs_g<TPI>(p.oneR, a, tig);                              // acc = R: the empty product at rho = 1
    int E = PAD_EXP, phase = SP_FETCH, rho = 1;
    long long pos = has_carry ? -1 : 0, sq = 0, epos = 0;
    bool done = !valid;
#pragma clang loop unroll(disable)
    for (;;) {
      int op = SC_IDLE, s = 1;                                      // s: the constant R^s of an emit or a NORM
      long long osrc = -1;                                          // operand: element index, or -1 for the carry
      while (op == SC_IDLE && !done) {
        const long long j = p.reverse ? j1 - 1 - pos : j0 + pos;
        const long long idx = (o * p.L + j) * p.inner + i;
        if (phase == SP_FETCH) {
          const int e = pos < 0 ? p.carry_exp[cidx] : p.exp[idx];
          osrc = pos < 0 ? -1 : idx;
          if (e == PAD_EXP) {
            phase = SP_EMIT;
          } else if (E == PAD_EXP || e == E) {
            if (1 - rho >= ADD_KMAX) {                              // the constants end at R^(ADD_KMAX + 1): back to rho = 1
              op = SC_NORM;
              s = 2 - rho;
              rho = 1;
            } else {
              E = e;
              op = SC_MUL;
              --rho;
              phase = SP_EMIT;
            }
          } else if (e > E) {
            if (rho != 1) {                                         // squarings need acc = P R
              op = SC_NORM;
              s = 2 - rho;
              rho = 1;
            } else {
              sq = 4ll * ((long long)e - E);
              E = e;
              phase = SP_ACCSQ;
            }
          } else {
            sq = 4ll * ((long long)E - e);
            op = SC_PARK;
            phase = SP_TMPSQ;
          }
        } else if (phase == SP_ACCSQ || phase == SP_TMPSQ) {
          op = SC_SQ;
          if (--sq == 0) phase = phase == SP_ACCSQ ? SP_MUL : SP_JOIN;
        } else if (phase == SP_MUL) {
          op = SC_MUL;
          --rho;
          osrc = pos < 0 ? -1 : idx;
          phase = SP_EMIT;
        } else if (phase == SP_JOIN) {
          op = SC_JOIN;
          phase = SP_EMIT;
        } else {                                                    // SP_EMIT
          if (pos >= 0 && (p.emit_all || pos == len - 1)) {
            op = SC_EMIT;
            s = 1 - rho;
            epos = p.emit_all ? idx : ii;
          }
          ++pos;
          phase = SP_FETCH;
          if (pos >= len) done = true;
        }
      }
      if (ballot(op != SC_IDLE) == 0ull) break;
      if (ballot(op == SC_PARK) != 0ull) {                          // acc -> park, a <- R^2
        uint32_t x[L];
        load_limbs_g<TPI>(p.R2, x, tig);
        write_limbs_lds_if<TPI>(park, a, tig, op == SC_PARK);
#pragma unroll
        for (int k = 0; k < L; ++k) a[k] = op == SC_PARK ? x[k] : a[k];
      }
      {
        const bool operand = op == SC_MUL || op == SC_PARK;
        const uint32_t* src = !operand ? p.RS + (size_t)s * p.ct_words : osrc < 0 ? p.carry + cidx * p.ct_words : p.ct + osrc * p.ct_words;
        uint32_t b[L];
        stage_words_to_limbs<TPI>(slot, src, p.ct_words, b, tig);
        if (ballot(op == SC_JOIN) != 0ull) {
#pragma unroll
          for (int k = 0; k < L; ++k) b[k] = op == SC_JOIN ? park[tig * L + k] : b[k];
        }
#pragma unroll
        for (int k = 0; k < L; ++k) b[k] = op == SC_SQ ? a[k] : b[k];
        write_limbs_lds<TPI>(slot, b, tig);
      }
      uint32_t r[L];
      montmul<TPI>(r, a, slot, TPI, m, p.mprime, lane, tig);
      const bool keep = op == SC_IDLE || op == SC_EMIT;
#pragma unroll
      for (int k = 0; k < L; ++k) a[k] = keep ? a[k] : r[k];
      if (ballot(op == SC_EMIT) != 0ull) {
        cond_sub<TPI>(r, m, lane, tig);
#pragma unroll
        for (int k = 0; k < L; ++k) r[k] = E == PAD_EXP ? ((tig == 0 && k == 0) ? 1u : 0u) : r[k];   // nothing entered yet
        emit_words<TPI>(slot, r, p.out + epos * p.ct_words, p.ct_words, op == SC_EMIT, tig);
        if (op == SC_EMIT && tig == 0) p.out_exp[epos] = E;
      }
    }
  }
}

}  // namespace fpai
