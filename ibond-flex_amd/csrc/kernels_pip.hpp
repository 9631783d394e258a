// Bucket-method (Pippenger) multi-exponentiation for narrow encrypted-by-plain products (pai_matmul[_dev], d < 16):
//
//   out[i][j] = P N^-1 mod n^2,   P, N = prod over the k with M_kj > 0 / M_kj < 0 of c[i][k]^(|M_kj| 16^(E - e_kj)),
//
// with (M, e) and E as in kernels_mm.hpp. The effective exponents |M| 16^(E - e) are cut into windows of w bits; window
// t of sign s owns the buckets 1 .. 2^w - 1, bucket b the product B_b of the ciphertexts whose digit is b (no squaring
// while accumulating), the window the sum_b b B_b (running sum from the top bucket down), the sign the Horner join of
// its windows. The wide integer |M| << 4 (E - e) is never formed: pip_digit cuts window t out of it.
//
//   k_pip_scan       one block per output: E, whether a scalar is negative, and the widest effective exponent (bits)
//   k_pip_plan       one block per output: counting sort of the digits in LDS -- 2 nwin 2^w counters (sign, window,
//                    bucket), an exclusive scan, then every (term, window) with a non-zero digit drops its k into the
//                    cell's member list. A cell of more than PIP_RUN members is cut into runs; the block reserves its
//                    runs in the call's unit list with one atomicAdd and writes (first member, members, row i) of each.
//   k_pip_acc<TPI>   one lane group per run: the product of its members, gathered from the [m][K][W] input in plain
//                    form (every montmul drops one factor R; one product by R^(len + 1) restores the Montgomery form)
//   k_pip_red<TPI>   one lane group per (output, sign, window): for the non-empty buckets b_1 > b_2 > .. (b_last+1 = 0)
//                    run *= B_b (the bucket's run partials), sum *= run^(b_i - b_i+1); an empty bucket costs no product
//                    but its share of the squarings of that power, an empty window none
//   k_pip_horner<TPI> one lane group per (output, sign): w squarings per window below the first non-empty one, one
//                    product per non-empty window; leaves the Montgomery form and writes the canonical P / N with E in
//                    k_add's operand layout ([2][m d][W]), where the batch inversion and k_add finish out = P N^-1.
//
// Lane-group engine (bn_group.hpp); one montmul site per kernel, a group without work multiplies by R.
#pragma once
#include "kernels_mm.hpp"

namespace fpai {

constexpr int PIP_RUN = 32;          // members per run of a bucket (R^(PIP_RUN + 1) <= R^(ADD_KMAX + 1), the last constant)
constexpr int PIP_WMIN = 4, PIP_WMAX = 8;
// Cap on the bits of an output's effective exponents. The plan's counters take 2 ceil(cap / w) 2^w x 4 bytes of LDS:
// 128 KiB at w = 8, 16 KiB at w = 4, next to 3 KiB of scan scratch, inside the 160 KiB of a gfx950 CU.
constexpr int PIP_CAP_BITS = 512;
static_assert(PIP_RUN + 1 <= ADD_KMAX + 1, "R^s constants");

// window t (w bits) of mag << sh
__device__ __forceinline__ int pip_digit(uint64_t mag, int sh, int t, int w) {
  const int lo = t * w - sh;
  const uint64_t v = lo >= 64 ? 0ull : lo >= 0 ? mag >> lo : lo > -w ? mag << -lo : 0ull;
  return (int)(v & ((1u << w) - 1u));
}

// max over the block's 256 threads
__device__ __forceinline__ long long pip_block_max(long long v, long long* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

struct PipScanParams {
  const int32_t* exp;       // ciphertext exponents [m][K]
  const void* x;            // scalars [K][d]
  int dtype;
  long long K, d, Np;       // Np = m d outputs
  int32_t* E;               // [Np]
  uint8_t* neg;             // [Np] 1: the output has a negative term (the batch inversion's flags)
  int* summary;             // [0]: the widest effective exponent of the call in bits, zeroed by the caller
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_pip_scan(PipScanParams p) {
  __shared__ long long red[256];
  for (long long o = blockIdx.x; o < p.Np; o += gridDim.x) {
    const long long i = o / p.d, j = o % p.d;
    int E = INT32_MIN;                                             // zero terms count: the value 1 with its exponent
    for (long long k = threadIdx.x; k < p.K; k += 256) {
      int64_t M;
      int es;
      mm_encode(p.dtype, p.x, k * p.d + j, M, es);
      E = max(E, p.exp[i * p.K + k] + es);
    }
    E = (int)pip_block_max(E, red);
    long long bits = 0, neg = 0;
    for (long long k = threadIdx.x; k < p.K; k += 256) {
      int64_t M;
      int es;
      mm_encode(p.dtype, p.x, k * p.d + j, M, es);
      if (M == 0) continue;
      const uint64_t mag = M < 0 ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
      bits = max(bits, (long long)(64 - __clzll(mag)) + 4 * ((long long)E - (p.exp[i * p.K + k] + es)));
      neg |= M < 0;
    }
    bits = pip_block_max(bits, red);
    neg = pip_block_max(neg, red);
    if (threadIdx.x == 0) {
      p.E[o] = E;
      p.neg[o] = (uint8_t)neg;
      atomicMax(&p.summary[0], (int)min(bits, (long long)INT32_MAX));
    }
  }
}

struct PipPlanParams {
  const int32_t* exp;
  const void* x;
  int dtype;
  long long K, d;
  long long o0, nob;        // the outputs of this launch: o0 .. o0 + nob
  const int32_t* E;         // [Np]
  int w, nwin;              // cells = 2 nwin 2^w: (sign nwin + window) 2^w + digit
  long long Ms;             // member slots per output
  int32_t* members;         // [nob][Ms] the k of every cell's members, cell after cell
  int32_t* uoff;            // [nob][cells + 1] first unit of every cell (and the end of the last)
  int4* runs;               // the units: (first member in `members`, members, row i, 0)
  unsigned* nunits;         // units reserved so far, zeroed by the caller
};

// dynamic LDS of k_pip_plan: the counters, the per-thread sums of the scan (members, runs) and the reserved base
constexpr size_t pip_plan_lds_bytes(int w, int nwin) { return ((size_t)(2 * nwin) << w) * 4 + (2 * 256 + 1) * 4; }

// Term k of output (i, j): magnitude, sign, shift in bits and the windows tlo .. thi its digits fall into. False: M = 0.
__device__ __forceinline__ bool pip_term(const PipPlanParams& p, long long i, long long j, long long k, int E,
                                         uint64_t& mag, int& sgn, int& sh, int& tlo, int& thi) {
  int64_t M;
  int es;
  mm_encode(p.dtype, p.x, k * p.d + j, M, es);
  if (M == 0) return false;
  mag = M < 0 ? (uint64_t)0 - (uint64_t)M : (uint64_t)M;
  sgn = M < 0 ? 1 : 0;
  // the host has checked shift + bits(mag) <= PIP_CAP_BITS; scalars rewritten since then must not leave the counters
  const long long shl = 4 * ((long long)E - (p.exp[i * p.K + k] + es));
  if (shl < 0 || shl > PIP_CAP_BITS) return false;
  sh = (int)shl;
  tlo = sh / p.w;
  thi = min((sh + 63 - __clzll(mag)) / p.w, p.nwin - 1);
  return true;
}

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_pip_plan(PipPlanParams p) {
  extern __shared__ unsigned pip_cnt[];
  const int cells = (2 * p.nwin) << p.w;
  unsigned* tsum = pip_cnt + cells;                                // [256] members, [256] runs, [1] base
  const int tid = threadIdx.x;
  const int per = (cells + 255) / 256, c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
  for (long long ol = blockIdx.x; ol < p.nob; ol += gridDim.x) {
    const long long o = p.o0 + ol, i = o / p.d, j = o % p.d;
    const int E = p.E[o];
    __syncthreads();
    for (int t = tid; t < cells; t += 256) pip_cnt[t] = 0u;
    __syncthreads();
    for (long long k = tid; k < p.K; k += 256) {
      uint64_t mag;
      int sgn, sh, tlo, thi;
      if (!pip_term(p, i, j, k, E, mag, sgn, sh, tlo, thi)) continue;
      for (int t = tlo; t <= thi; ++t) {
        const int dig = pip_digit(mag, sh, t, p.w);
        if (dig) atomicAdd(&pip_cnt[((sgn * p.nwin + t) << p.w) + dig], 1u);
      }
    }
    __syncthreads();
    unsigned ms = 0, us = 0;
    for (int cI = c0; cI < c1; ++cI) {
      ms += pip_cnt[cI];
      us += (pip_cnt[cI] + PIP_RUN - 1) / PIP_RUN;
    }
    tsum[tid] = ms;
    tsum[256 + tid] = us;
    __syncthreads();
    if (tid == 0) {
      unsigned am = 0, au = 0;
      for (int t = 0; t < 256; ++t) {
        const unsigned vm = tsum[t], vu = tsum[256 + t];
        tsum[t] = am;
        tsum[256 + t] = au;
        am += vm;
        au += vu;
      }
      tsum[512] = atomicAdd(p.nunits, au);
      p.uoff[ol * (cells + 1) + cells] = (int32_t)(tsum[512] + au);
    }
    __syncthreads();
    {
      unsigned mo = tsum[tid], uo = tsum[512] + tsum[256 + tid];
      for (int cI = c0; cI < c1; ++cI) {
        const unsigned n = pip_cnt[cI];
        p.uoff[ol * (cells + 1) + cI] = (int32_t)uo;
        for (unsigned r = 0; r * PIP_RUN < n; ++r)
          p.runs[uo++] = make_int4((int)(ol * p.Ms + mo + r * PIP_RUN), (int)min((unsigned)PIP_RUN, n - r * PIP_RUN), (int)i, 0);
        pip_cnt[cI] = mo;                                          // from here on the cell's cursor
        mo += n;
      }
    }
    __syncthreads();
    for (long long k = tid; k < p.K; k += 256) {
      uint64_t mag;
      int sgn, sh, tlo, thi;
      if (!pip_term(p, i, j, k, E, mag, sgn, sh, tlo, thi)) continue;
      for (int t = tlo; t <= thi; ++t) {
        const int dig = pip_digit(mag, sh, t, p.w);
        if (!dig) continue;
        const unsigned pos = atomicAdd(&pip_cnt[((sgn * p.nwin + t) << p.w) + dig], 1u);
        if (pos < (unsigned long long)p.Ms) p.members[ol * p.Ms + pos] = (int32_t)k;   // (scalars rewritten between the passes)
      }
    }
  }
}

struct PipAccParams {
  const uint32_t* ct;       // [m][K][W]
  long long K;
  const int32_t* members;
  const int4* runs;
  const unsigned* nunits;
  uint32_t* part;           // [units][S] the runs' products, Montgomery form
  const uint32_t* N;
  const uint32_t* RS;       // [ADD_KMAX + 2][ct_words]: R^s mod n^2
  uint32_t mprime;
  int ct_words;
};

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pip_acc(PipAccParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long n = (long long)*p.nunits;

  for (long long base = (long long)blockIdx.x * GPB; base < n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < n;
    const long long el = valid ? inst : n - 1;
    const int4 run = p.runs[el];
    const int32_t* mem = p.members + run.x;
    const int len = valid ? run.y : 1;
    const uint32_t* row = p.ct + (long long)run.z * p.K * p.ct_words;
    int wlen = len;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) wlen = max(wlen, __shfl_xor(wlen, s));
    uint32_t a[L];
    stage_words_to_limbs<TPI>(slot, row + (long long)mem[0] * p.ct_words, p.ct_words, a, tig);   // plain: rho = 0
#pragma clang loop unroll(disable)
    for (int j = 1; j <= wlen; ++j) {
      // member j (rho -= 1), then R^(len + 1) (rho = 1 - len -> 1), then R (nothing) until the wave's longest run is done
      const uint32_t* src = j < len ? row + (long long)mem[j] * p.ct_words
                                    : p.RS + (size_t)(j == len ? len + 1 : 1) * p.ct_words;
      uint32_t t[L];
      stage_words_to_limbs<TPI>(slot, src, p.ct_words, t, tig);
      write_limbs_lds<TPI>(slot, t, tig);
      montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
    }
    if (valid) store_limbs_g<TPI>(p.part + el * S, a, tig);
  }
}

struct PipRedParams {
  const int32_t* uoff;      // [nob][cells + 1]
  long long nob;
  int w, nwin;
  const uint32_t* part;
  uint32_t* run;            // [nob 2 nwin][S] the instance's running product
  uint32_t* wsum;           // [nob 2 nwin][S] the window's sum, Montgomery form
  uint8_t* wflag;           // [nob 2 nwin] 1: the window has a member
  const uint32_t* N;
  const uint32_t* oneR;
  uint32_t mprime;
};

// the next non-empty bucket below b of the window whose unit offsets start at uo (0: none)
__device__ __forceinline__ int pip_next_bucket(const int32_t* uo, int b) {
  do --b;
  while (b > 0 && uo[b + 1] == uo[b]);
  return b;
}

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pip_red(PipRedParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  enum { PH_LOAD, PH_ACC, PH_POW, PH_SUM, PH_PUT, PH_DONE };
  enum { K_ID, K_MUL, K_SQ };
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long per = 2 * p.nwin, n = p.nob * per;
  const int cells = (2 * p.nwin) << p.w;

  for (long long base = (long long)blockIdx.x * GPB; base < n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < n;
    const long long el = valid ? inst : 0;
    const int32_t* uo = p.uoff + (el / per) * (cells + 1) + ((el % per) << p.w);   // bucket b: units uo[b] .. uo[b + 1]
    uint32_t* rung = p.run + el * S;
    uint32_t* sumg = p.wsum + el * S;
    int b = valid ? pip_next_bucket(uo, 1 << p.w) : 0;
    int ph = b ? PH_LOAD : PH_DONE;
    int u = b ? uo[b] : 0, u1 = b ? uo[b + 1] : 0;
    int nb = 0, g = 0, bit = -1;
    bool half = false, have_run = false, have_sum = false;
    uint32_t a[L];
    load_limbs_g<TPI>(p.oneR, a, tig);
#pragma clang loop unroll(disable)
    for (;;) {
      // this group's next product: a *= B with B from `bsrc` (K_MUL), a itself (K_SQ) or R (K_ID: no work left)
      int kind = K_ID;
      const uint32_t* bsrc = p.oneR;
      while (kind == K_ID && ph != PH_DONE) {
        if (ph == PH_LOAD) {                                       // a = run, or the first partial of the top bucket
          load_limbs_g<TPI>(have_run ? rung : p.part + (long long)u * S, a, tig);
          if (!have_run) ++u;
          have_run = true;
          ph = PH_ACC;
        } else if (ph == PH_ACC) {                                 // run *= the bucket's partials
          if (u < u1) {
            bsrc = p.part + (long long)u * S;
            ++u;
            kind = K_MUL;
          } else {
            store_limbs_g<TPI>(rung, a, tig);
            nb = pip_next_bucket(uo, b);
            g = b - nb;
            bit = 30 - __clz(g);
            half = false;
            ph = PH_POW;
          }
        } else if (ph == PH_POW) {                                 // a = run^g, left to right
          if (bit < 0) {
            ph = PH_SUM;
          } else if (!half) {
            half = true;
            kind = K_SQ;
          } else {
            half = false;
            if ((g >> bit) & 1) {
              bsrc = rung;
              kind = K_MUL;
            }
            --bit;
          }
        } else if (ph == PH_SUM) {                                 // a = sum run^g
          if (have_sum) {
            bsrc = sumg;
            kind = K_MUL;
          }
          ph = PH_PUT;
        } else {                                                   // PH_PUT
          store_limbs_g<TPI>(sumg, a, tig);
          have_sum = true;
          b = nb;
          if (b) {
            u = uo[b];
            u1 = uo[b + 1];
            ph = PH_LOAD;
          } else {
            ph = PH_DONE;
          }
        }
      }
      if (ballot(kind != K_ID) == 0ull) break;
      {
        uint32_t t[L];
        load_limbs_g<TPI>(bsrc, t, tig);
#pragma unroll
        for (int q = 0; q < L; ++q) t[q] = kind == K_SQ ? a[q] : t[q];
        write_limbs_lds<TPI>(slot, t, tig);
      }
      montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
    }
    if (valid && tig == 0) p.wflag[el] = have_sum ? 1 : 0;
  }
}

struct PipHornerParams {
  const uint32_t* wsum;     // [nob 2 nwin][S]
  const uint8_t* wflag;     // [nob 2 nwin]
  const int32_t* E;         // [Np]
  long long o0, nob, Np;
  int w, nwin;
  uint32_t* pn;             // [2][Np][W]: P, then N, canonical
  int32_t* pnexp;           // [2][Np]
  const uint32_t* N;
  const uint32_t* oneR;
  uint32_t mprime;
  int ct_words;
};

template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_pip_horner(PipHornerParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);
  const long long n = p.nob * 2;

  for (long long base = (long long)blockIdx.x * GPB; base < n; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < n;
    const long long el = valid ? inst : n - 1;
    const long long o = p.o0 + el / 2, row = (el % 2) * p.Np + o;
    const uint8_t* fl = p.wflag + el * p.nwin;
    const uint32_t* ws = p.wsum + el * p.nwin * S;
    int tg = tig;
    asm volatile("" : "+v"(tg));
    uint32_t a[L];
    load_limbs_g<TPI>(p.oneR, a, tg);
    bool started = false;                                          // a != R
    for (int t = p.nwin - 1; t >= 0; --t) {
#pragma clang loop unroll(disable)
      for (int op = 0; op <= p.w; ++op) {
        const uint32_t* bsrc = p.oneR;
        if (op < p.w) {                                            // w squarings (R stays R)
          if (ballot(started) == 0ull) continue;
        } else {                                                   // times the window's sum
          const bool on = fl[t] != 0;
          if (ballot(on) == 0ull) continue;
          if (on) bsrc = ws + (long long)t * S;
          started = started || on;
        }
        {
          uint32_t tt[L];
          load_limbs_g<TPI>(bsrc, tt, tg);
#pragma unroll
          for (int q = 0; q < L; ++q) tt[q] = op < p.w ? a[q] : tt[q];
          write_limbs_lds<TPI>(slot, tt, tig);
        }
        montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
      }
    }
    write_one_lds<TPI>(slot, tig);
    montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);         // leave the Montgomery domain
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(slot, a, p.pn + row * p.ct_words, p.ct_words, valid, tg);
    if (valid && tig == 0) p.pnexp[row] = p.E[o];
  }
}

}  // namespace fpai
