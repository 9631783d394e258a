// Packed plaintexts: k signed fixed-point values in disjoint bit fields of ONE Paillier plaintext (include/flexpai.h,
// "Packed plaintexts"). A layout is (slot_bits sb, value_bits vb, exponent e, slots k), B = 2^sb; value i
// of a call lives in ciphertext i / k, slot i % k (slot 0 least significant); the plaintext is the SIGNED integer
// M = sum_j t_j B^j with signed digits |t_j| <= 2^(vb-1) - 1, encrypted as m = M mod n like every other plaintext of
// the library (negatives are n - |M|).
//
//   k_pack_mul<TPI>  one ciphertext per group of TPI lanes (bn_group.hpp), like k_obf_mul. The lanes encode the group's
//                    k values (encode_elem at the fixed exponent), place the biased digits t + B/2 as byte fields into
//                    the group's LDS slot (sb is a multiple of 8: no two lanes write the same byte), cut the slot into
//                    28-bit limbs and subtract the layout constant H = sum_j (B/2) B^j, cut from the same slot filled
//                    with B/2 fields: the borrow is the sign of M, and a wrapped (negative) difference is negated.
//                    n |M| is a full-width schoolbook product by columns (make_c0's multiplier has three limbs): a
//                    column sums at most 147 products below 2^56, under 2^64, so plain 64-bit accumulators and one
//                    normalize do at every key size. c0 = 1 + n |M| or n^2 + 1 - n |M|; with an obfuscator the encrypt
//                    chain has already written s = r^n into the output row, and c0 s is k_obf_mul's two Montgomery
//                    products (c0 R^2 R^-1, then s R^-1) and one cond_sub.
//   k_pack_fold<TPI> k EXISTING ordinary ciphertexts -> one packed ciphertext (pai_pack_ciphertexts), one output per group:
//                    prod_j c_j^(16^D_j 2^(sb j)) by Horner from the top slot, the exponent alignment folded into the
//                    squarings (below, in front of the kernel).
//   k_unpack         raw plaintexts m = D(ct) in [0, n) -> the N values. A block takes UNPACK_CPB ciphertexts: all
//                    threads copy their words into LDS (coalesced), one thread per ciphertext does the multiword sign
//                    test against max_int = n / 3 - 1 and forms U = M + H in place (M = m, or m - n), then all
//                    threads cut the fields out of U and store val / mant / status of consecutive values (coalesced).
//                    U >= B^k or U < 0 is an overflow of the whole ciphertext, as is m in the gap between max_int and
//                    n - max_int.
#pragma once
#include "kernels.hpp"

namespace fpai {

struct PackLayout {
  int sb, vb, fexp, k;   // slot bits (a multiple of 8 in [16, 64]), value bits, base-16 exponent, slots per ciphertext
};

struct PackMulParams {
  const void* x;          // [nvals] values of dtype
  int dtype;
  long long nvals;
  PackLayout lay;
  int obf;                // PAI_OBF_*: 0 emits c0, else ct holds r^n on entry
  uint32_t* ct;           // [n][ct_words], in place
  int32_t* status;        // [nvals], nullable
  long long n;            // ciphertexts: ceil(nvals / k)
  const uint32_t* N;      // n^2, limbs (S)
  const uint32_t* R2;     // R^2 mod n^2
  const uint32_t* nl;     // n limbs (S, zero padded)
  uint32_t mprime;
  int ct_words;
  int n_limbs, m_limbs;   // limbs of n; limbs that hold |M| < 2^(k sb - 1)
};

// The value t of slot j of ciphertext ci (0 past the call's last value), its status written when `record`
__device__ __forceinline__ int64_t pack_encode(const PackMulParams& p, long long ci, int j, bool record) {
  const long long i = ci * p.lay.k + j;
  if (i >= p.nvals) return 0;
  int64_t t = 0;
  int e = 0;
  int st = encode_elem(p.x, p.dtype, 1, p.lay.fexp, i, t, e);
  const int64_t lim = p.lay.vb >= 64 ? INT64_MAX : ((int64_t)1 << (p.lay.vb - 1)) - 1;
  if (st != ST_OK || t > lim || t < -lim) {
    st = ST_ENC_RANGE;
    t = 0;
  }
  if (record && p.status) p.status[i] = st;
  return t;
}

// The group's slot, zeroed, then one sb-bit field per slot: the biased digits of ciphertext ci (digits), or B/2 in
// every field (the constant H); cut into this lane's L limbs. Bytes [0, k sb / 8) are written, k sb <= key bits - 2.
template <int TPI>
__device__ __forceinline__ void pack_fields_to_limbs(uint32_t* slot, const PackMulParams& p, long long ci, bool digits,
                                                     bool record, uint32_t (&x)[L], int tig) {
  const int nbytes = p.lay.sb >> 3;
  const uint64_t half = 1ull << (p.lay.sb - 1);
  wave_lds_fence();                                   // earlier readers of the slot are done
#pragma unroll
  for (int i = 0; i < L; ++i) slot[tig * L + i] = 0u;
  wave_lds_fence();
  uint8_t* sbytes = reinterpret_cast<uint8_t*>(slot);
  for (int j = tig; j < p.lay.k; j += TPI) {
    const uint64_t d = half + (digits ? (uint64_t)pack_encode(p, ci, j, record) : 0ull);   // sb = 64: wraps as meant
    for (int b = 0; b < nbytes; ++b) sbytes[j * nbytes + b] = (uint8_t)(d >> (8 * b));
  }
  wave_lds_fence();
  int t = tig;
  asm volatile("" : "+v"(t));
  const int base = t * L * LB;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int bit = base + i * LB, j = bit >> 5;      // j + 1 < S: ((S - 1) LB >> 5) + 1 < S for S >= 37
    x[i] = __builtin_amdgcn_alignbit(slot[j + 1], slot[j], bit & 31) & LMASK;
  }
  wave_lds_fence();
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pack_mul(PackMulParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t* nsh = smem + GPB * S;                     // n's S limbs, shared by the block's groups
  for (int i = threadIdx.x; i < S; i += BLOCK) nsh[i] = p.nl[i];
  __syncthreads();
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    uint32_t a[L];
    bool neg;
    {
      // |M| and its sign from D = M + H: the borrow of D - H is the sign, and a wrapped difference is negated
      // (0 - x mod 2^(LB S)), so that H and D are dead before the second subtraction
      uint32_t dh[L];
      {
        uint32_t h[L], d[L];
        pack_fields_to_limbs<TPI>(slot, p, t, false, false, h, tig);
        pack_fields_to_limbs<TPI>(slot, p, t, true, valid, d, tig);
        neg = sub_limbs<TPI>(d, h, dh, lane, tig);
      }
      uint32_t z[L];
#pragma unroll
      for (int i = 0; i < L; ++i) z[i] = 0u;
      (void)sub_limbs<TPI>(z, dh, a, lane, tig);
#pragma unroll
      for (int i = 0; i < L; ++i) a[i] = neg ? a[i] : dh[i];
    }
    // n |M| by columns: column c = sum_j n[c - j] |M|[j], at most min(n_limbs, m_limbs) <= 147 products
    write_limbs_lds<TPI>(slot, a, tig);
    {
      uint64_t P[L];
      // opaque copy: stops LICM from hoisting the L per-column loop bounds and addresses out of the element loop,
      // where they would stay live across the Montgomery products
      int tt = tig;
      asm volatile("" : "+v"(tt));
#pragma unroll
      for (int i = 0; i < L; ++i) {
        const int col = tt * L + i;
        const int jlo = max(0, col - (p.n_limbs - 1)), jhi = min(col, p.m_limbs - 1);
        uint64_t acc = 0;
        for (int j = jlo; j <= jhi; ++j) acc += (uint64_t)nsh[col - j] * slot[j];
        P[i] = acc;
      }
      uint32_t X[L], D[L];
      normalize<TPI>(P, X, lane, tig);
      (void)sub_limbs<TPI>(m, X, D, lane, tig);       // n^2 - n |M| (only used when M < 0)
#pragma unroll
      for (int i = 0; i < L; ++i) P[i] = (uint64_t)(neg ? D[i] : X[i]) + ((tig == 0 && i == 0) ? 1u : 0u);
      normalize<TPI>(P, a, lane, tig);
    }
    if (p.obf != 0) {
      // step 0: a <- c0 R^2 R^-1 = c0 R; step 1: a <- (c0 R) s R^-1 = c0 s, s = r^n read from the output row itself
      // (one montmul site, as in k_obf_mul)
#pragma unroll 1
      for (int step = 0; step < 2; ++step) {
        if (step == 0) {
          copy_g_to_lds<TPI>(slot, p.R2, tig);
        } else {
          uint32_t b[L];
          stage_words_to_limbs<TPI>(slot, p.ct + t * p.ct_words, p.ct_words, b, tig);
          write_limbs_lds<TPI>(slot, b, tig);
        }
        montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
      }
      cond_sub<TPI>(a, m, lane, tig);
    }
    emit_words<TPI>(slot, a, p.ct + t * p.ct_words, p.ct_words, valid, tig);
  }
}

// ================================================================= fold (pai_pack_ciphertexts)
// k existing ordinary ciphertexts -> one packed ciphertext, out = prod_j c_j^(2^(4 D_j + sb j)) mod n^2 with
// D_j = E - exp_j and 0 <= 4 D_j < sb. One output per group of TPI lanes, Horner from the top slot over the bit
// positions t = sb j + r: every step squares, and slot j enters at r = 4 D_j, where 4 D_j squarings of its own remain:
//   (acc^(2^(sb - 4D)) c_j)^(2^(4D)) = acc^(2^sb) c_j^(16^D).
// The slot a step can inject is j = t / sb for every group of the wave, so the walk over (j, r) is wave-uniform; only
// the step r at which a group injects differs. A step multiplies when some group of the wave injects there (ballot);
// the others multiply by 1 (R in the Montgomery domain). Nothing is squared before the wave's first injection, so the
// top slot costs its own 4 D squarings and a ragged output starts at its own top slot. Per slot: sb squarings, one
// product by R^2 that takes c_j into the Montgomery domain, one product into acc.
// pai_repack is the same walk over PACKED inputs: slot j of an output is a whole input ciphertext of s slots, so the
// distance between two slots is stride = s sb bits (not bounded by 64 like sb), there are no exponents (exp is null:
// every D_j = 0) and lay.k counts the inputs per output.
struct PackFoldParams {
  const uint32_t* ct;     // [nvals][ct_words] ciphertexts
  const int32_t* exp;     // [nvals]; PAD_EXP: the ciphertext 1 of an empty segment; null: every shift is 0
  long long nvals;
  PackLayout lay;
  int stride;             // bits between neighbouring slots of an output: lay.sb, or s sb for pai_repack
  uint32_t* out;          // [n][ct_words]
  int32_t* status;        // [nvals], nullable
  long long n;            // outputs: ceil(nvals / k)
  const uint32_t* N;      // n^2, limbs (S)
  const uint32_t* R2;     // R^2 mod n^2
  const uint32_t* oneR;   // R mod n^2
  uint32_t mprime;
  int ct_words;
};

// 4 D of slot j of output ci, or -1 where the slot contributes the factor 1; the status is written when `record`
__device__ __forceinline__ int fold_shift(const PackFoldParams& p, long long ci, int j, bool record) {
  const long long i = ci * p.lay.k + j;
  if (i >= p.nvals) return -1;
  if (!p.exp) return 0;
  const int32_t e = p.exp[i];
  int st = ST_OK, d4 = -1;
  if (e != PAD_EXP) {
    const long long d = (long long)p.lay.fexp - (long long)e;
    if (d < 0 || 4 * d >= p.lay.sb) st = ST_ENC_RANGE;
    else d4 = (int)(4 * d);
  }
  if (record && p.status) p.status[i] = st;
  return d4;
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pack_fold(PackFoldParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t* park = smem + (GPB + gib) * S;            // second slot of the group: acc during an injection
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const int sb = p.stride, k = p.lay.k;

  for (long long base = (long long)blockIdx.x * GPB; base < p.n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.n;
    const long long t = valid ? inst : p.n - 1;
    const int cnt = (int)min((long long)k, p.nvals - t * k);   // slots of this output that hold a value (>= 1)
    int jtop = cnt - 1;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) jtop = max(jtop, __shfl_xor(jtop, s));
    uint32_t acc[L];
    load_limbs_g<TPI>(p.oneR, acc, tig);
    bool started = false;                                       // wave-uniform: some group has injected
    for (int j = jtop; j >= 0; --j) {
      const int d4 = j < cnt ? fold_shift(p, t, j, valid && tig == 0) : -1;
      int rtop = d4;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) rtop = max(rtop, __shfl_xor(rtop, s));
      if (started) rtop = sb - 1;
      const uint32_t* src = p.ct + (t * k + (j < cnt ? j : 0)) * p.ct_words;
#pragma unroll 1
      for (int r = rtop; r >= 0; --r) {
        if (started) {
          write_limbs_lds<TPI>(slot, acc, tig);
          montmul<TPI>(acc, acc, slot, TPI, m, p.mprime, lane, tig);
        }
        const bool inj = d4 == r;
        if (ballot(inj) != 0ull) {
          // acc waits in the group's second LDS slot while c_j enters the Montgomery domain: acc, c_j, the modulus
          // and the product's 2 L accumulator registers together do not fit 256 VGPRs
          wave_lds_fence();
#pragma unroll
          for (int i = 0; i < L; ++i) park[tig * L + i] = acc[i];
          wave_lds_fence();
          uint32_t b[L];
          stage_words_to_limbs<TPI>(slot, src, p.ct_words, b, tig);
#pragma unroll
          for (int i = 0; i < L; ++i) b[i] = inj ? b[i] : ((tig == 0 && i == 0) ? 1u : 0u);
          copy_g_to_lds<TPI>(slot, p.R2, tig);
          montmul<TPI>(b, b, slot, TPI, m, p.mprime, lane, tig);        // c_j R, or R
          write_limbs_lds<TPI>(slot, b, tig);
#pragma unroll
          for (int i = 0; i < L; ++i) acc[i] = park[tig * L + i];
          montmul<TPI>(acc, acc, slot, TPI, m, p.mprime, lane, tig);
          started = true;
        }
      }
    }
    write_one_lds<TPI>(slot, tig);
    montmul<TPI>(acc, acc, slot, TPI, m, p.mprime, lane, tig);           // leave the Montgomery domain
    cond_sub<TPI>(acc, m, lane, tig);
    emit_words<TPI>(slot, acc, p.out + t * p.ct_words, p.ct_words, valid, tig);
  }
}

// ================================================================= unpack
constexpr int UNPACK_BLOCK = 256;
constexpr int UNPACK_CPB = 64;     // ciphertexts per block: one wave does the multiword step

struct UnpackParams {
  const uint32_t* raw;     // [n][pt_words] plaintexts in [0, n)
  long long n;             // ciphertexts
  long long nvals;
  PackLayout lay;
  double* val;             // [nvals]
  int64_t* mant;           // [nvals], nullable
  int32_t* status;         // [nvals]
  const uint32_t* consts;  // [3][pt_words] words: n, max_int, n - max_int
  int pt_words;
};

// sign(a - b) over nw words, most significant first
__device__ __forceinline__ int unpack_cmp(const uint32_t* a, const uint32_t* __restrict__ b, int nw) {
  for (int w = nw - 1; w >= 0; --w) {
    const uint32_t x = a[w], y = b[w];
    if (x != y) return x > y ? 1 : -1;
  }
  return 0;
}

template <int DUMMY = 0>
__global__ __launch_bounds__(UNPACK_BLOCK) void k_unpack(UnpackParams p) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int PW = p.pt_words, ROW = PW + 1;            // odd row stride: the per-ciphertext threads hit distinct banks
  uint32_t* U = smem;                                 // [UNPACK_CPB][ROW]
  uint32_t* Hs = smem + UNPACK_CPB * ROW;             // [PW] words of H
  int* ovf = reinterpret_cast<int*>(Hs + PW);         // [UNPACK_CPB]
  const int sb = p.lay.sb, k = p.lay.k;
  const int top = k * sb;                             // bits of B^k; top <= key bits - 2 < 32 PW
  for (int w = threadIdx.x; w < PW; w += UNPACK_BLOCK) {
    uint32_t hw = 0;
    for (int b = 0; b < 32; ++b) {
      const int bit = 32 * w + b;
      if (bit < top && bit % sb == sb - 1) hw |= 1u << b;
    }
    Hs[w] = hw;
  }
  const uint32_t* nw = p.consts;
  const uint32_t* maxint = p.consts + PW;
  const uint32_t* nmm = p.consts + 2 * PW;

  for (long long base = (long long)blockIdx.x * UNPACK_CPB; base < p.n; base += (long long)gridDim.x * UNPACK_CPB) {
    const int nc = (int)min((long long)UNPACK_CPB, p.n - base);
    __syncthreads();                                  // Hs is written; the previous round's readers of U are done
    for (int i = threadIdx.x; i < nc * PW; i += UNPACK_BLOCK) U[(i / PW) * ROW + i % PW] = p.raw[base * PW + i];
    __syncthreads();
    if (threadIdx.x < nc) {
      uint32_t* u = U + threadIdx.x * ROW;
      const bool pos = unpack_cmp(u, maxint, PW) <= 0;
      const bool neg = !pos && unpack_cmp(u, nmm, PW) >= 0;
      // U = m + H (- n when negative), two's complement over PW words and the carry out
      int64_t c = 0;
      uint32_t high = 0;                              // bits of U at and above B^k
      for (int w = 0; w < PW; ++w) {
        c += (int64_t)u[w] + (int64_t)Hs[w] - (neg ? (int64_t)nw[w] : 0);
        const uint32_t v = (uint32_t)c;
        c >>= 32;
        u[w] = v;
        const int lo = 32 * w;
        if (lo >= top) high |= v;
        else if (lo + 32 > top) high |= v >> (top - lo);
      }
      ovf[threadIdx.x] = (!pos && !neg) || c != 0 || high != 0;
    }
    __syncthreads();
    const long long v0 = base * k;
    const long long nv = min((long long)nc * k, p.nvals - v0);
    const int nbytes = sb >> 3;
    for (long long v = threadIdx.x; v < nv; v += UNPACK_BLOCK) {
      const int ci = (int)(v / k), j = (int)(v % k);
      const uint8_t* ub = reinterpret_cast<const uint8_t*>(U + ci * ROW) + j * nbytes;
      uint64_t d = 0;
      for (int b = 0; b < nbytes; ++b) d |= (uint64_t)ub[b] << (8 * b);
      const int64_t t = (int64_t)(d - (1ull << (sb - 1)));   // sb = 64: wraps as meant
      const bool bad = ovf[ci] != 0;
      p.val[v0 + v] = bad ? 0.0 : ldexp((double)t, -4 * p.lay.fexp);
      if (p.mant) p.mant[v0 + v] = bad ? 0 : t;
      p.status[v0 + v] = bad ? ST_OVERFLOW : ST_OK;
    }
  }
}

}  // namespace fpai
