// The fold of kernels_pack.hpp (k_pack_fold: pai_pack_ciphertexts, pai_repack) for calls of few outputs, one output per
// DPP row of 16 lanes instead of one per group of 2 / 4 / 8 lanes. An output is a chain of (k - 1) stride + 2 k + 1
// products mod n^2 that depend on each other; a call of a few thousand outputs leaves most of the chip idle on the group
// kernel and pays that chain at a group's pace. On a row a product is K digit steps of 2 LW multiply-accumulates per
// lane (kernels_crtw.hpp mont<K>, K = 74 / 148 / 296 limbs of n^2, LW = ceil((K + 1) / 16)) against 2 S L on a group.
//
//   k_pack_fold_w<K>  k_pack_fold's walk with crtw's machinery: the same (slot, step) schedule, wave-uniform over the
//                     four rows of the wave (the ballot at injection steps, the 16^D alignment folded into the
//                     squarings, PAD_EXP and slots past the last value as the factor 1). The accumulator stays in the
//                     row's lanes (LW limbs per lane: nothing is parked); the row's two LDS slots hold the squaring
//                     operand and the entering factor c_j R, one slot shared by the block holds R^2 mod n^2. R =
//                     2^(28 K) and the constants are k_pe_w's (and, since K = S, the group engine's). The walk ends with
//                     a product by 1, a conditional subtraction and the words out: the result is canonical, so the
//                     bits are k_pack_fold's.
#pragma once
#include "kernels_crtw.hpp"
#include "kernels_pack.hpp"

namespace fpai {
namespace crtw {

template <int K>
__global__ __launch_bounds__(BLOCK_W) void k_pack_fold_w(PackFoldParams p) {
  constexpr int LW = Geom<K>::LW, SW = Geom<K>::W;
  static_assert(SW % 4 == 0, "16-byte slots");
  __shared__ __attribute__((aligned(16))) uint32_t sm[(GPW * 2 + 1) * SW];
  const int lane = threadIdx.x, tig = lane & (TPI - 1), g = lane / TPI;
  uint32_t* SQ = sm + g * 2 * SW;                       // the squaring operand; the words on the way in and out
  uint32_t* FA = SQ + SW;                               // the entering factor c_j R (or R), then 1
  uint32_t* CR = sm + GPW * 2 * SW;                     // R^2 mod n^2
  for (int w = lane; w < SW; w += BLOCK_W) CR[w] = w < K ? p.R2[w] : 0u;
  uint32_t m[LW], oneR[LW];
  load_const<LW>(p.N, K, m, tig);
  load_const<LW>(p.oneR, K, oneR, tig);
  const uint32_t mprime = p.mprime;
  const int sb = p.stride, k = p.lay.k, nw = p.ct_words;   // nw <= K < SW: 32 nw < 2 nb + 32 <= 28 K + 32

  for (long long base = (long long)blockIdx.x * GPW; base < p.n; base += (long long)gridDim.x * GPW) {
    const long long inst = base + g;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    const int cnt = (int)min((long long)k, p.nvals - t * k);   // slots of this output that hold a value (>= 1)
    int jtop = cnt - 1;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) jtop = max(jtop, __shfl_xor(jtop, s));
    uint32_t acc[LW];
#pragma unroll
    for (int i = 0; i < LW; ++i) acc[i] = oneR[i];
    bool started = false;                                       // wave-uniform: some row has injected
    for (int j = jtop; j >= 0; --j) {
      const int d4 = j < cnt ? fold_shift(p, t, j, valid && tig == 0) : -1;
      int rtop = d4;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) rtop = max(rtop, __shfl_xor(rtop, s));
      if (started) rtop = sb - 1;
      const uint32_t* src = p.ct + (t * k + (j < cnt ? j : 0)) * nw;
#pragma unroll 1
      for (int r = rtop; r >= 0; --r) {
        if (started) {
          put<LW, SW>(SQ, acc, tig);
          mont<K>(acc, SQ, m, mprime, lane, tig);
        }
        const bool inj = d4 == r;
        if (ballot(inj) != 0ull) {
          // c_j: its words through the row's squaring slot (free between two squarings), cut into this lane's limbs
          wave_lds_fence();
          for (int w = tig; w < nw; w += TPI) SQ[w] = src[w];
          wave_lds_fence();
          uint32_t b[LW];
#pragma unroll
          for (int i = 0; i < LW; ++i) {
            const int bit = (tig * LW + i) * LB, wi = bit >> 5, sh = bit & 31;
            const uint64_t lo = wi < nw ? (uint64_t)SQ[wi] : 0ull;
            const uint64_t hi = wi + 1 < nw ? (uint64_t)SQ[wi + 1] : 0ull;
            const uint32_t v = (uint32_t)(((hi << 32) | lo) >> sh) & LMASK;
            b[i] = inj ? v : ((tig == 0 && i == 0) ? 1u : 0u);
          }
          mont<K>(b, CR, m, mprime, lane, tig);                 // c_j R, or R
          put<LW, SW>(FA, b, tig);
          mont<K>(acc, FA, m, mprime, lane, tig);
          started = true;
        }
      }
    }
    {
      uint32_t one[LW];
#pragma unroll
      for (int i = 0; i < LW; ++i) one[i] = (tig == 0 && i == 0) ? 1u : 0u;
      put<LW, SW>(FA, one, tig);
      mont<K>(acc, FA, m, mprime, lane, tig);                   // leave the Montgomery domain
      uint32_t d[LW];
      if (!sub<LW>(acc, m, d, lane, tig)) {
#pragma unroll
        for (int i = 0; i < LW; ++i) acc[i] = d[i];
      }
    }
    put<LW, SW>(SQ, acc, tig);
    if (valid) {
      for (int w = tig; w < nw; w += TPI) p.out[t * nw + w] = limbs_word(SQ, SW, w);
    }
    wave_lds_fence();
  }
}

}  // namespace crtw
}  // namespace fpai
