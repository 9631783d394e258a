// Encrypted histograms over a binned feature matrix (pai_histogram[_dev]): per-cell sums of one ciphertext vector,
//
//   out[(v F + f) B + b] = prod over the samples i with node[i] == v and bins[i][f] == b of c_i^(16^(E - e_i)) mod n^2,
//
// with everything the segmented add is told through index lists derived from the bin matrix on the device:
//
//   k_hist_count    members per cell. One block walks tiles of samples of one feature; the feature's nodes x B counters
//                   are privatised in LDS where they fit HIST_LDS_CELLS (one flush of the non-zero counters per block and
//                   feature), above that every pair goes to the global counter.
//   k_hist_scatter  sample ids (int32) into the cells' member lists. A block counts a tile of HIST_TILE samples in LDS,
//                   one lane per touched cell reserves the tile's share of the cell's list with ONE global atomicAdd, and
//                   every pair lands at the reserved base plus its rank in the tile. The order inside a list is free: the
//                   product of canonical residues does not depend on it.
//   k_hist_rows     k_add's gather rows from the member lists: run r of a cell (HIST_RUN consecutive members, the last
//                   one ragged) becomes one row of HIST_RUN sources, padded with -1.
//
//   k_hist_acc<TPI> one lane group per run: k_add's Horner product with the operands read straight from the member
//                   list (4 W contiguous bytes per member), one canonical partial at the run's largest exponent.
//
// The runs' partials are summed by the segmented add. k_hist_rows + k_add (HIST_RUN == ADD_KMAX operands per instance)
// is the same product over padded gather rows; the test build selects it with $FLEXPAI_HIST_ACC=0.
#pragma once
#include "kernels.hpp"

namespace fpai {

constexpr int HIST_RUN = 64;            // members per run (the fastest of 64, 128, 256: DESIGN.md section 5); k_add's ADD_KMAX
constexpr int HIST_LDS_CELLS = 8192;    // privatised counters of one feature: 32 KiB, so that 4 blocks share a CU's LDS
constexpr int HIST_SPT = 8;             // samples per thread and tile of k_hist_scatter
constexpr int HIST_TILE = 256 * HIST_SPT;

struct HistParams {
  const void* bins;            // [N][stride] bin ids
  int bin_u16;                 // 0: uint8, 1: uint16
  long long stride;            // elements per row
  const int32_t* node;         // [N] (nullable: every sample in node 0)
  int nodes, B;
  long long N, F;
  long long f0, f1;            // the features of this launch
  int lds;                     // 1: nodes * B <= HIST_LDS_CELLS, counters in LDS
  unsigned long long* count;   // [nodes F B] members per cell (k_hist_count adds; k_hist_scatter bounds the ranks by it)
  const int32_t* cell_off;     // [nodes F B] first member of the cell in `members`
  unsigned* cursor;            // [nodes F B] members placed so far, zeroed by the caller
  int32_t* members;            // the member lists of the features f0 .. f1
};

// cell of pair (i, f) within its feature (v B + b), or -1 when the sample or the bin id is skipped
__device__ __forceinline__ int hist_local(const HistParams& p, long long i, long long f) {
  const int v = p.node ? p.node[i] : 0;
  const unsigned b = p.bin_u16 ? (unsigned)static_cast<const uint16_t*>(p.bins)[i * p.stride + f]
                               : (unsigned)static_cast<const uint8_t*>(p.bins)[i * p.stride + f];
  return (v >= 0 && v < p.nodes && b < (unsigned)p.B) ? v * p.B + (int)b : -1;
}
__device__ __forceinline__ size_t hist_cell(const HistParams& p, int local, long long f) {
  return ((size_t)(local / p.B) * (size_t)p.F + (size_t)f) * (size_t)p.B + (size_t)(local % p.B);
}

// grid: x tiles of samples (grid stride), y features (grid stride)
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_hist_count(HistParams p) {
  extern __shared__ unsigned h_cnt[];
  const int nb = p.nodes * p.B;
  for (long long f = p.f0 + blockIdx.y; f < p.f1; f += gridDim.y) {
    if (p.lds) {
      for (int t = threadIdx.x; t < nb; t += 256) h_cnt[t] = 0u;
      __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.N; i += (long long)gridDim.x * 256) {
      const int l = hist_local(p, i, f);
      if (l < 0) continue;
      if (p.lds) atomicAdd(&h_cnt[l], 1u);
      else atomicAdd(&p.count[hist_cell(p, l, f)], 1ull);
    }
    if (p.lds) {
      __syncthreads();
      for (int t = threadIdx.x; t < nb; t += 256)
        if (h_cnt[t]) atomicAdd(&p.count[hist_cell(p, t, f)], (unsigned long long)h_cnt[t]);
      __syncthreads();
    }
  }
}

// grid: x tiles of HIST_TILE samples (grid stride), y features (grid stride)
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_hist_scatter(HistParams p) {
  extern __shared__ unsigned h_cnt[];   // per cell of the feature: the tile's count, then the reserved base
  const int nb = p.nodes * p.B;
  const long long tiles = (p.N + HIST_TILE - 1) / HIST_TILE;
  for (long long f = p.f0 + blockIdx.y; f < p.f1; f += gridDim.y) {
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      int loc[HIST_SPT];
      unsigned rank[HIST_SPT];
      if (p.lds) {
        for (int t = threadIdx.x; t < nb; t += 256) h_cnt[t] = 0u;
        __syncthreads();
      }
#pragma unroll
      for (int s = 0; s < HIST_SPT; ++s) {
        const long long i = tile * HIST_TILE + s * 256 + threadIdx.x;
        loc[s] = i < p.N ? hist_local(p, i, f) : -1;
        rank[s] = 0u;
        if (loc[s] >= 0) rank[s] = p.lds ? atomicAdd(&h_cnt[loc[s]], 1u) : atomicAdd(&p.cursor[hist_cell(p, loc[s], f)], 1u);
      }
      if (p.lds) {
        __syncthreads();
        for (int t = threadIdx.x; t < nb; t += 256)
          if (h_cnt[t]) h_cnt[t] = atomicAdd(&p.cursor[hist_cell(p, t, f)], h_cnt[t]);
        __syncthreads();
      }
#pragma unroll
      for (int s = 0; s < HIST_SPT; ++s) {
        if (loc[s] < 0) continue;
        const size_t cell = hist_cell(p, loc[s], f);
        const unsigned long long pos = (unsigned long long)rank[s] + (p.lds ? h_cnt[loc[s]] : 0u);
        // (a bin matrix rewritten between the two passes must not write outside the cell's list)
        if (pos < p.count[cell]) p.members[(long long)p.cell_off[cell] + (long long)pos] = (int32_t)(tile * HIST_TILE + s * 256 + threadIdx.x);
      }
      if (p.lds) __syncthreads();
    }
  }
}

struct HistRowsParams {
  const int32_t* members;
  const int2* runs;        // [nruns] (first member, members) of every run, 1 .. HIST_RUN members
  long long nruns;
  long long* gidx;         // [nruns][HIST_RUN]
};

// one source per thread
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_hist_rows(HistRowsParams p) {
  const long long total = p.nruns * HIST_RUN;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long long)gridDim.x * blockDim.x) {
    const int2 r = p.runs[u / HIST_RUN];
    const int j = (int)(u % HIST_RUN);
    p.gidx[u] = j < r.y ? (long long)p.members[(long long)r.x + j] : -1ll;
  }
}

struct HistAccParams {
  const uint32_t* cts;     // [N][W]
  const int32_t* exps;     // [N]
  const int32_t* members;
  const int2* runs;        // [nruns] (first member, members >= 1)
  long long nruns;
  uint32_t* out;           // [nruns][W]
  int32_t* out_exp;        // [nruns]
  const uint32_t* N;
  const uint32_t* RS;      // [ADD_KMAX + 2][ct_words]: R^s mod n^2
  uint32_t mprime;
  int ct_words;
};

// k_add's Horner product (kernels.hpp) over one run, read from the member list: operands enter in plain form, the
// Montgomery factor (rho = 1 - mcount) is restored with one product by R^s per level change and at the end, and, since
// the R^s constants end at s = ADD_KMAX + 1, once more inside a level whenever ADD_KMAX operands have entered; 4 (nl - cur)
// squarings between levels. One montmul site; a group that is done multiplies by R.
template <int TPI>
__global__ __launch_bounds__(BLOCK, 2) void k_hist_acc(HistAccParams p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const int tig = threadIdx.x % TPI;
  const int gib = threadIdx.x / TPI;
  uint32_t* slot = smem + gib * S;
  uint32_t m[L];
  load_limbs_g<TPI>(p.N, m, tig);

  for (long long base = (long long)blockIdx.x * GPB; base < p.nruns; base += (long long)gridDim.x * GPB) {
    const long long inst = base + gib;
    const bool valid = inst < p.nruns;
    const long long el = valid ? inst : p.nruns - 1;
    const int2 run = p.runs[el];
    const int32_t* mem = p.members + run.x;
    const int k = run.y;
    int E = PAD_EXP, cur = INT32_MAX;
    for (int j = 0; j < k; ++j) {
      const int ej = p.exps[mem[j]];
      E = max(E, ej);
      cur = min(cur, ej);
    }
    uint32_t a[L];
    int jc = 0, sq = 0, mcount = 1;
    bool done = false;
    while (p.exps[mem[jc]] != cur) ++jc;
    stage_words_to_limbs<TPI>(slot, p.cts + (long long)mem[jc] * p.ct_words, p.ct_words, a, tig);   // rho = 0
    ++jc;
#pragma clang loop unroll(disable)
    for (;;) {
      // this group's next step: 0 square, 1 times operand `osrc`, 2 times R^s, 3 nothing (times R)
      int op = 3, s = 1;
      long long osrc = 0;
      if (!done) {
        if (sq > 0) {
          op = 0;
          --sq;
        } else {
          while (jc < k && p.exps[mem[jc]] != cur) ++jc;
          if (jc < k) {
            if (mcount == ADD_KMAX) {                  // rho = 1 - mcount -> 0; the operand waits a step
              op = 2;
              s = mcount;
              mcount = 1;
            } else {
              op = 1;
              osrc = mem[jc];
              ++jc;
              ++mcount;
            }
          } else {
            int nl = INT32_MAX;
            for (int j = 0; j < k; ++j) {
              const int ej = p.exps[mem[j]];
              if (ej > cur && ej < nl) nl = ej;
            }
            if (nl != INT32_MAX) {
              op = 2;
              s = 1 + mcount;                          // back to rho = 1 for the squarings
              sq = 4 * (nl - cur);
              cur = nl;
              jc = 0;
              mcount = 0;
            } else {
              done = true;
              if (mcount >= 2) {                       // rho = 1 - mcount -> 0
                op = 2;
                s = mcount;
              }
            }
          }
        }
      }
      if (ballot(op != 3) == 0ull) break;
      {
        const uint32_t* src = op == 1 ? p.cts + osrc * p.ct_words : p.RS + (size_t)s * p.ct_words;
        uint32_t t[L];
        stage_words_to_limbs<TPI>(slot, src, p.ct_words, t, tig);
#pragma unroll
        for (int i = 0; i < L; ++i) t[i] = op == 0 ? a[i] : t[i];
        write_limbs_lds<TPI>(slot, t, tig);
      }
      montmul<TPI>(a, a, slot, TPI, m, p.mprime, lane, tig);
    }
    cond_sub<TPI>(a, m, lane, tig);
    emit_words<TPI>(slot, a, p.out + el * p.ct_words, p.ct_words, valid, tig);
    if (valid && tig == 0) p.out_exp[el] = E;
  }
}

}  // namespace fpai
