// Segmented weighted sums of ciphertexts (pai_segment_dot[_dev]): the sparse encrypted-by-plain product,
//
//   out_s = prod_{t in segment s} (c[index[t]]^+-1)^(|M_t| 16^(E_s - e_t)) mod n^2,   e_t = exp[index[t]] + e(x[t]),
//
// with (M_t, e(x[t])) the reference's encoding of x[t] and E_s the largest e_t of the segment: pai_matmul's sum
// (kernels_mm.hpp) over an index list in which every term carries its own scalar. The chunk of MM_KC consecutive entries
// of one segment takes the place of the MM_KC consecutive k of an output; window tables (k_mm_tab, unchanged) are built
// once per DISTINCT ciphertext that a block of chunks references, so the cost follows the stored entries:
//
//   k_sd_sign      entries -> neg[uid[t]] = 1 where M_t < 0 (a scatter over the call's distinct ciphertexts; -0.0 and
//                  range failures are not negative, as in k_mm_sign), and k_mul's status of every entry
//   k_sd_gather    rows of the ciphertext array through an index: the distinct ciphertexts of a block in table-slot
//                  order (the input of k_mm_tab and of the batch inversion), or the entries of a slice (term path)
//   k_sd_acc<TPI>  one instance per chunk: k_mm_acc's window walk with every operand's table found through its slot
//                  (LDS, beside |M| and e); writes the chunk's partial and E into a flat list [chunk][W], [chunk] that
//                  the segmented add reduces (ceil(len_s / MM_KC) consecutive rows per segment).
//
// Lane-group engine (bn_group.hpp), one montmul site per kernel.
#pragma once
#include "kernels_mm.hpp"

namespace fpai {

struct SdSignParams {
  const void* x;            // scalars [nnz]
  int dtype;
  long long nnz;
  const int32_t* uid;       // [nnz]: the entry's ciphertext among the call's distinct ones
  uint8_t* neg;             // [distinct], zeroed by the caller
  int32_t* status;          // [nnz] (nullable): k_mul's status of every entry
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_sd_sign(SdSignParams p) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < p.nnz; t += (long long)gridDim.x * blockDim.x) {
    int64_t M = 0;
    int es = 0;
    const int st = encode_elem(p.x, p.dtype, 0, 0, t, M, es);
    if (p.status) p.status[t] = st;
    if (st == ST_OK && M < 0) p.neg[p.uid[t]] = 1;
  }
}

struct SdGatherParams {
  const uint32_t* ct;       // [N][W]
  const int32_t* exp;       // [N] (nullable with out_exp)
  const long long* rows;    // [n] rows of ct, each in [0, N)
  long long n;
  uint32_t* out;            // [n][W]
  int32_t* out_exp;         // [n] (nullable)
  int ct_words;
};

// one word per thread
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_sd_gather(SdGatherParams p) {
  const long long total = p.n * p.ct_words;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long long)gridDim.x * blockDim.x) {
    const long long r = u / p.ct_words, w = u % p.ct_words;
    const long long src = p.rows[r];
    p.out[u] = p.ct[src * p.ct_words + w];
    if (w == 0 && p.out_exp) p.out_exp[r] = p.exp[src];
  }
}

struct SdAccParams {
  const int32_t* exp;       // ciphertext exponents [N]
  const void* x;            // scalars [nnz]
  int dtype;
  const long long* index;   // [nnz] rows of exp
  const int32_t* tslot;     // [nnz] the entry's table among this block's (k_mm_tab entry, 0 .. ne)
  const long long* cstart;  // [chunks + 1] first entry of every chunk of the call; a chunk holds 1 .. MM_KC entries
  int q0, q1;               // the block: chunks q0 .. q1
  int ne;                   // tables of the block: the inverse of entry e is entry ne + e
  const uint32_t* tab;      // k_mm_tab's tables of this block
  uint32_t* part;           // [chunks][W]
  int32_t* pexp;            // [chunks]
  const uint32_t* N;
  const uint32_t* oneR;
  uint32_t mprime;
  int ct_words;
};

// dynamic LDS of k_sd_acc: k_mm_acc's, and the table slot (32 bits) of every operand
constexpr size_t sd_acc_lds_bytes(int tpi) { return mm_acc_lds_bytes(tpi) + (size_t)(BLOCK / tpi) * MM_KC * 4; }

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_sd_acc(SdAccParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  static_assert(MM_KC % TPI == 0, "operand rounds");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint64_t* mags = reinterpret_cast<uint64_t*>(smem + BLOCK * L) + gib * MM_KC;
  int* eks = reinterpret_cast<int*>(reinterpret_cast<uint64_t*>(smem + BLOCK * L) + GPB * MM_KC) + gib * MM_KC;
  int* ents = reinterpret_cast<int*>(reinterpret_cast<uint64_t*>(smem + BLOCK * L) + GPB * MM_KC) + GPB * MM_KC + gib * MM_KC;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const int n = p.q1 - p.q0;

  for (int base = blockIdx.x * GPB; base < n; base += gridDim.x * GPB) {
    const int inst = base + gib;
    const bool valid = inst < n;
    const int o = p.q0 + (valid ? inst : n - 1);                   // the chunk: its row in part / pexp
    const long long t0 = p.cstart[o];
    const int nreal = (int)(p.cstart[o + 1] - t0);
    // encode: lane tig takes the operands kk = tig, tig + TPI, ..; a negative operand's slot is its inverse's table
    wave_lds_fence();
#pragma unroll 1
    for (int r = 0; r < MM_KC / TPI; ++r) {
      const int kk = r * TPI + tig;
      const bool real = kk < nreal;
      const long long t = t0 + (real ? kk : 0);
      int64_t M;
      int es;
      mm_encode(p.dtype, p.x, t, M, es);
      if (!real) M = 0;                                            // padding: digit 0 everywhere, not part of E
      mags[kk] = M < 0 ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
      eks[kk] = p.exp[p.index[t]] + es;
      ents[kk] = p.tslot[t] + (M < 0 ? p.ne : 0);
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

    // opaque copy, as in k_mm_acc: keeps the per-lane 64-bit bases out of the instance loop's live registers
    int tg = tig;
    asm volatile("" : "+v"(tg));
    uint32_t a[L];
    load_limbs_g<TPI>(p.oneR, a, tg);
    bool started = false;                                          // a != R
    for (int w = wtop - 1; w >= 0; --w) {
#pragma clang loop unroll(disable)
      for (int op = 0; op < 4 + MM_KC; ++op) {
        if (op < 4) {
          if (ballot(started) == 0ull) continue;
          write_limbs_lds<TPI>(slot, a, tig);
        } else {
          const int kk = op - 4;
          const long long sh = (long long)w - ((long long)E - eks[kk]);   // window of |M_t| at chain window w
          const int dig = (sh >= 0 && sh < 16) ? (int)((mags[kk] >> (4 * (int)sh)) & 15u) : 0;
          if (ballot(dig != 0) == 0ull) continue;
          copy_g_to_lds<TPI>(slot, p.tab + ((size_t)ents[kk] * 16 + dig) * S, tg);
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
