// The cut of the fixed-base exponent a_h < 2^kb into K digits (kernels_fb.hpp), host and device, no HIP needed.
//
// A cut is (K, W, nw): positions 0 .. nw-1 hold W + 1 bits, positions nw .. K-1 hold W bits (nw = 0: the uniform
// cut). G^a = prod_k T_k[d_k] is the same group element for every cut of the same a_h, so the cut moves the tables
// and the digits only, never a ciphertext bit. Widths that differ by at most one bit with the wider digits first make
// every per-position quantity arithmetic on (W, nw) -- no offset table for the kernels to read:
//   width(k) = W + (k < nw),  bit offset(k) = k W + min(k, nw),  first row(k) = (k + min(k, nw)) 2^W.
// The sampler's product loop is at its instruction floor, so it keeps forming the row as k 2^W + digit: k_fb_digits
// adds the shift min(k, nw) 2^W of the wider positions before k to the digit it stores (32 bits: fb_cut_plan keeps a
// half's rows below 2^32).
// Why uneven: bits(p_h - 1) = 1024 = 46 x 22 + 12 spends a whole row product of the uniform W = 22 cut on a 12-bit top
// digit; 12 digits of 23 bits and 34 of 22 are 46 digits, one product fewer, in 243 M rows per half instead of 193 M
// (uniform W = 23 would need 377 M).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FB_CUT_HD __host__ __device__ __forceinline__
#else
#define FB_CUT_HD inline
#endif

namespace fpai {

constexpr int FB_CUT_WMAX = 24;   // widest digit the table builder takes: lo/hi half-digit tables of 2^12 entries (FB_LO)

FB_CUT_HD int fb_cut_width(int k, int W, int nw) { return W + (k < nw ? 1 : 0); }
FB_CUT_HD int fb_cut_bit(int k, int W, int nw) { return k * W + (k < nw ? k : nw); }
// first table row of position k; at k = K the rows of one half
FB_CUT_HD uint64_t fb_cut_row(int k, int W, int nw) { return (uint64_t)(k + (k < nw ? k : nw)) << W; }
// ... less k 2^W: what a stored digit carries beside its value
FB_CUT_HD uint32_t fb_cut_shift(int k, int W, int nw) { return (uint32_t)(k < nw ? k : nw) << W; }

struct FbCut {
  int K = 0, W = 0, nw = 0;
  uint64_t rows() const { return fb_cut_row(K, W, nw); }   // per half
  uint64_t bytes(uint64_t row_bytes) const { return 2 * rows() * row_bytes; }   // both halves
};

inline FbCut fb_cut_uniform(int kb, int W) { return W > 0 ? FbCut{(kb + W - 1) / W, W, 0} : FbCut{}; }

// The uniform window of today's plan: the largest of the ladder <= Wmax whose tables fit the budget (0: none)
inline int fb_ladder_window(int kb, int Wmax, uint64_t row_bytes, uint64_t budget) {
  for (int w : {24, 23, 22, 21, 20, 16, 12, 8})
    if (w <= Wmax && fb_cut_uniform(kb, w).bytes(row_bytes) <= budget) return w;
  return 0;
}

// The cut of a kb-bit exponent beside the uniform window Wu = fb_ladder_window(...): the smallest K >= Kmin whose
// tables fit the budget with every digit of at most min(Wmax, FB_CUT_WMAX) bits, at the fewest rows that K allows
// (kb mod K digits of floor(kb / K) + 1 bits, the rest of floor(kb / K)). A cut that saves no digit against the
// uniform one is not taken: the plan is then exactly the uniform plan -- same W, K, rows and bytes.
inline FbCut fb_cut_plan(int kb, int Wu, int Wmax, uint64_t row_bytes, uint64_t budget, int Kmin) {
  const FbCut uni = fb_cut_uniform(kb, Wu);
  const int cap = Wmax < FB_CUT_WMAX ? Wmax : FB_CUT_WMAX;
  if (!Wu || cap < Wu) return uni;
  int K = (kb + cap - 1) / cap;
  for (K = K < Kmin ? Kmin : K; K < uni.K; ++K) {
    const FbCut c{K, kb / K, kb % K};
    if (c.bytes(row_bytes) <= budget && c.rows() <= 0xffffffffull) return c;
  }
  return uni;
}

}  // namespace fpai
