// Fused encrypted-by-plain matrix product (pai_matmul[_dev], he_otp_lr_ft1/train.py:160 `enc_diff_y.dot(features)`):
// every output is a product of powers of the same K bases,
//
//   out[i][j] = prod_k (c[i][k]^+-1)^(|M_kj| 16^D_kij) mod n^2,   D_kij = E_ij - e_kij,
//
// where (M_kj, e_s) is the reference's encoding of x[k][j] (FixedPointNumber.encode, precision None), the sign of M
// selects c or invert(c) (encrypted_number.py:100-106), e_kij = exp[i][k] + e_s and E is the largest e over the
// operands (the alignment of __add__, encrypted_number.py:115-137: a shift of the exponent by whole 4-bit digits).
// A 4-bit interleaved (Straus) multi-exponentiation shares ONE squaring chain among the operands of an output and reads
// each base's window table once per digit; the alignment costs nothing but a longer chain:
//
//   k_mm_sign      x (K x d) -> neg_row[k] = 1 when some column holds M_kj < 0 (-0.0 and range failures are not negative)
//   k_mm_tab<TPI>  one ciphertext per lane group: x~ = c R mod n^2 and the Montgomery-form powers x~^0 .. x~^15
//                  ([16][S] limbs, group layout; entry 0 = R mod n^2, so a zero digit needs no branch); for the rows
//                  k with neg_row[k] the same 16 rows of c^-1 (taken from a copy of the inputs inverted in place by
//                  the batch inversion, kernels_mul.hpp k_inv_*). The inverse rows of other rows are neither built
//                  nor read.
//   k_mm_acc<TPI>  one instance per output (i, j) and per chunk of MM_KC consecutive k: encodes its scalars, walks the
//                  windows from the top one down -- four squarings, then one product per operand with the table row of
//                  its digit -- and writes the chunk's partial (an exact residue) and E in the operand layout of k_add
//                  ([chunk][m d][W], [chunk][m d]), which reduces the chunks as before.
//
// Lane-group engine (bn_group.hpp), like k_mul / k_add / k_inv_*: one montmul site per kernel.
#pragma once
#include "kernels.hpp"

namespace fpai {

// Operands per k_mm_acc instance: the chunk of the k_add reduction tree (flexpai.hip MATMUL_CHUNK). Their magnitudes
// and exponents live in LDS (12 bytes each): at TPI = 2 (128 groups per block) 16 operands keep the block at 61 KiB
// and two blocks per CU; 32 would need 85 KiB, one block per CU, for a squaring chain that is already shared by 16.
constexpr int MM_KC = 16;

// The reference's scalar encoding as k_mul applies it: status != OK -> M = 0.
__device__ __forceinline__ void mm_encode(int dtype, const void* x, long long xi, int64_t& M, int& es) {
  M = 0;
  es = 0;
  if (encode_elem(x, dtype, 0, 0, xi, M, es) != ST_OK) M = 0;
}

struct MmSignParams {
  const void* x;          // scalars [K][d]
  int dtype;              // PAI_F32 / PAI_F64 / PAI_I64
  long long K, d;
  uint8_t* neg_row;       // [K], zeroed by the caller
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_mm_sign(MmSignParams p) {
  const long long n = p.K * p.d;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    int64_t M;
    int es;
    mm_encode(p.dtype, p.x, t, M, es);
    if (M < 0) p.neg_row[t / p.d] = 1;
  }
}

struct MmTabParams {
  const uint32_t* ct;       // [m][K][W] ciphertexts
  const uint32_t* inv;      // the same layout with the ciphertexts of flagged rows inverted (null: has_neg = 0)
  const uint8_t* neg_row;   // [K]
  long long K;              // row length of ct / inv
  long long i0, k0;         // the block: rows i0 .. i0 + mb, columns k0 .. k0 + kb
  long long mb, kb;
  int has_neg;              // the block holds a flagged row: entries mb kb .. 2 mb kb are the inverses' tables
  uint32_t* tab;            // [(1 + has_neg) mb kb][16][S]
  const uint32_t* N;        // n^2
  const uint32_t* R2;       // R^2 mod n^2
  const uint32_t* oneR;     // R mod n^2
  uint32_t mprime;
  int ct_words;
};

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_mm_tab(MmTabParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long ne = p.mb * p.kb, n = ne * (p.has_neg ? 2 : 1);

  for (long long base = (long long)blockIdx.x * GPB; base < n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < n;
    const long long t = valid ? inst : n - 1;
    const bool sgn = t >= ne;
    const long long e = sgn ? t - ne : t;
    const long long il = e / p.kb, kl = e % p.kb;
    const bool active = valid && (!sgn || p.neg_row[p.k0 + kl] != 0);
    if (ballot(active) == 0ull) continue;                          // a wave of inverse rows nobody reads
    const uint32_t* src = (sgn ? p.inv : p.ct) + ((p.i0 + il) * p.K + p.k0 + kl) * p.ct_words;
    uint32_t* rows = p.tab + (size_t)t * 16 * S;
    uint32_t tt[L];
    load_limbs_g<TPI>(p.oneR, tt, tig);
    if (active) store_limbs_g<TPI>(rows, tt, tig);                 // x~^0 = R
    words_to_limbs(src, p.ct_words, tt, tig);
    copy_g_to_lds<TPI>(slot, p.R2, tig);
#pragma clang loop unroll(disable)
    for (int r = 1; r < 16; ++r) {
      montmul<TPI>(tt, tt, slot, TPI, m, p.mprime, lane, tig);     // r = 1: c R^2 R^-1 = x~; then x~^(r-1) x~
      if (active) store_limbs_g<TPI>(rows + r * S, tt, tig);
      if (r == 1) write_limbs_lds<TPI>(slot, tt, tig);
    }
  }
}

struct MmAccParams {
  const int32_t* exp;       // ciphertext exponents [m][K]
  const void* x;            // scalars [K][d]
  int dtype;
  long long K, d;
  long long i0, k0;         // the block (k0 a multiple of MM_KC)
  long long mb, kb;
  int has_neg;
  const uint32_t* tab;      // k_mm_tab's tables of this block
  uint32_t* part;           // [ceil(K / MM_KC)][Np][W]: this block writes chunks k0 / MM_KC .., outputs i0 d ..
  int32_t* pexp;            // [ceil(K / MM_KC)][Np]
  long long Np;             // m d
  const uint32_t* N;
  const uint32_t* oneR;
  uint32_t mprime;
  int ct_words;
};

// dynamic LDS of k_mm_acc: one S-limb slot per lane group, then |M| (64 bits) and e (32 bits) of its MM_KC operands
constexpr size_t mm_acc_lds_bytes(int tpi) { return (size_t)BLOCK * L * 4 + (size_t)(BLOCK / tpi) * MM_KC * 12; }

// The windows run from the wave's top one down (groups with a shorter chain hold R until their first digit: the
// squarings are skipped while no group of the wave has started, a product while every group's digit is 0).
template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_mm_acc(MmAccParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  static_assert(MM_KC % TPI == 0 && MM_KC <= 32, "operand rounds / sign mask");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint64_t* mags = reinterpret_cast<uint64_t*>(smem + BLOCK * L) + gib * MM_KC;
  int* eks = reinterpret_cast<int*>(reinterpret_cast<uint64_t*>(smem + BLOCK * L) + GPB * MM_KC) + gib * MM_KC;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long nch = (p.kb + MM_KC - 1) / MM_KC, ne = p.mb * p.kb, n = nch * p.mb * p.d;

  for (long long base = (long long)blockIdx.x * GPB; base < n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < n;
    const long long t = valid ? inst : n - 1;
    const long long j = t % p.d, r0 = t / p.d;
    const long long il = r0 % p.mb, q = r0 / p.mb;
    const long long kl0 = q * MM_KC;                               // first operand, relative to k0
    const int nreal = (int)min((long long)MM_KC, p.kb - kl0);
    // encode: lane tig takes the operands kk = tig, tig + TPI, ..; the signs travel by ballot
    uint32_t negmask = 0;
    wave_lds_fence();
#pragma unroll 1
    for (int r = 0; r < MM_KC / TPI; ++r) {
      const int kk = r * TPI + tig;
      const bool real = kk < nreal;
      const long long k = p.k0 + kl0 + (real ? kk : 0);
      int64_t M;
      int es;
      mm_encode(p.dtype, p.x, k * p.d + j, M, es);
      if (!real) M = 0;                                            // padding: digit 0 everywhere, not part of E
      mags[kk] = M < 0 ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
      eks[kk] = p.exp[(p.i0 + il) * p.K + k] + es;
      const uint64_t B = ballot(M < 0);
      negmask |= (uint32_t)((B >> (lane - tig)) & ((1u << TPI) - 1u)) << (r * TPI);
    }
    wave_lds_fence();
    int E = INT32_MIN;
    for (int kk = 0; kk < nreal; ++kk) E = max(E, eks[kk]);        // zero terms count: the value 1 with its exponent
    long long top = 0;
    for (int kk = 0; kk < nreal; ++kk) {
      const uint64_t mg = mags[kk];
      if (mg) top = max(top, (long long)((67 - __clzll(mg)) / 4) + ((long long)E - eks[kk]));
    }
    int wtop = (int)min(top, (long long)INT32_MAX);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) wtop = max(wtop, __shfl_xor(wtop, s));

    // 32-bit (the host checks both counts): two registers less across the chain, which has none to spare
    const int o = (int)((p.k0 / MM_KC + q) * p.Np + (p.i0 + il) * p.d + j);   // the partial's row in part / pexp
    const int ent0 = (int)(il * p.kb + kl0);                                  // the chunk's first table
    // opaque copy: stops LICM from hoisting the per-lane 64-bit bases of oneR, the tables and the output out of the
    // instance loop, which would pin them for the whole kernel (they spilled)
    int tg = tig;
    asm volatile("" : "+v"(tg));
    uint32_t a[L];
    load_limbs_g<TPI>(p.oneR, a, tg);
    bool started = false;                                          // a != R
    for (int w = wtop - 1; w >= 0; --w) {
#pragma clang loop unroll(disable)
      for (int op = 0; op < 4 + MM_KC; ++op) {
        // B goes to the slot inside each branch (no 37-limb value merges), the product follows the join
        if (op < 4) {
          if (ballot(started) == 0ull) continue;
          write_limbs_lds<TPI>(slot, a, tig);
        } else {
          const int kk = op - 4;
          const long long sh = (long long)w - ((long long)E - eks[kk]);   // window of |M_k| at chain window w
          const int dig = (sh >= 0 && sh < 16) ? (int)((mags[kk] >> (4 * (int)sh)) & 15u) : 0;
          if (ballot(dig != 0) == 0ull) continue;
          const size_t ent = (((negmask >> kk) & 1u) ? (size_t)ne : 0) + (size_t)(ent0 + min(kk, nreal - 1));
          copy_g_to_lds<TPI>(slot, p.tab + (ent * 16 + dig) * S, tg);
          started = started || dig != 0;
        }
        montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
      }
    }
    write_one_lds<TPI>(slot, tig);
    montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);         // leave the Montgomery domain
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(slot, a, p.part + (size_t)o * p.ct_words, p.ct_words, valid, tg);
    if (valid && tig == 0) p.pexp[o] = E;
  }
}

}  // namespace fpai
