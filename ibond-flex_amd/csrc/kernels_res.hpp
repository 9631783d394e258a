// Kernels of the device-resident ciphertext buffers: k_take (rows gathered by an index) and k_check_below (the
// wire-ingest range check). Both move or compare words only: no arithmetic on ciphertexts, plain C++, vector loads
// and stores.
#pragma once
#include "engine_res.hpp"

namespace fpai {

// The two words of k_check_idx, read by every kernel that follows it: uniform over the grid.
__device__ __forceinline__ bool res_gate_shut(const long long* gate) { return gate && (gate[0] >= 0 || gate[1] >= 0); }

// out[j] = in[index[j]] (words and exponent); index[j] == -1 writes ciphertext 1 with exponent INT32_MIN. A work item
// is one VEC-word piece of an output row, consecutive lanes take consecutive pieces of a row (coalesced on both sides),
// and the grid strides over the pieces. VEC = 4 (16-byte loads and stores) needs W % 4 == 0 and 16-byte aligned bases:
// every row then starts on a 16-byte boundary; VEC = 1 serves every other width (W = 65 of a 1035-bit key).
template <int VEC>
__global__ void __launch_bounds__(RES_BLOCK) k_take(TakeParams p) {
  const long long per_row = p.W / VEC;
  const long long total = p.M * per_row;
  const long long step = (long long)gridDim.x * RES_BLOCK;
  if (res_gate_shut(p.gate)) return;
  for (long long t = (long long)blockIdx.x * RES_BLOCK + threadIdx.x; t < total; t += step) {
    const long long j = t / per_row;
    const int q = (int)(t - j * per_row);
    const long long src = p.index[j];
    if constexpr (VEC == 4) {
      uint4 v = make_uint4(q == 0 ? 1u : 0u, 0u, 0u, 0u);
      if (src >= 0) v = reinterpret_cast<const uint4*>(p.in + src * p.W)[q];
      reinterpret_cast<uint4*>(p.out + j * p.W)[q] = v;
    } else {
      uint32_t v = q == 0 ? 1u : 0u;
      if (src >= 0) v = p.in[src * p.W + q];
      p.out[j * p.W + q] = v;
    }
    if (q == 0) p.out_exp[j] = src >= 0 ? p.in_exp[src] : RES_EMPTY_EXP;
  }
}

// One lane per row, from the top limb down: the first limb that differs from the limit decides, so a row of a random
// residue costs one word. A row equal to the limit is not below it.
__global__ void __launch_bounds__(RES_BLOCK) k_check_below(CheckBelowParams p) {
  const long long step = (long long)gridDim.x * RES_BLOCK;
  for (long long i = (long long)blockIdx.x * RES_BLOCK + threadIdx.x; i < p.N; i += step) {
    const uint32_t* row = p.ct + i * p.W;
    bool bad = true;
    for (int w = p.W - 1; w >= 0; --w) {
      const uint32_t a = row[w], b = p.limit[w];
      if (a != b) {
        bad = a > b;
        break;
      }
    }
    if (bad) atomicMin(p.first, (unsigned long long)i);
  }
}

// One pass over a device index and, when given, the segment offsets; the smallest offender of each goes to bad[0] /
// bad[1] by a vector atomicMin on the unsigned word (-1 = ~0 is the largest). It dereferences nothing but the two lists.
__global__ void __launch_bounds__(RES_BLOCK) k_check_idx(CheckIdxParams p) {
  const long long step = (long long)gridDim.x * RES_BLOCK;
  const long long first = (long long)blockIdx.x * RES_BLOCK + threadIdx.x;
  for (long long t = first; t < p.total; t += step) {
    const long long v = p.index[t];
    if (v < p.lo || v >= p.N) atomicMin(p.bad, (unsigned long long)t);
  }
  if (!p.seg_off) return;
  for (long long s = first; s <= p.nseg; s += step) {
    const long long o = p.seg_off[s];
    bool bad = s == 0 ? o != 0 : o < p.seg_off[s - 1];
    if (s == p.nseg && o != p.total) bad = true;
    if (bad) atomicMin(p.bad + 1, (unsigned long long)s);
  }
}

__device__ __forceinline__ long long seg_ceil_pow(long long len, int k) {   // ceil(len / 16^k), len >= 0
  for (int i = 0; i < k; ++i) len = (len + SEGPLAN_C - 1) / SEGPLAN_C;
  return len;
}

// ONE block: thread t owns the segments [t per, (t + 1) per); it sums its part counts, the block scans the 1024 sums
// in LDS, and the thread writes its exclusive offsets. Every level's counts follow from the segment's length alone
// (ceil(len / 16^(k + 1))), so one launch plans them all. off[k][nseg] = the level's number of partial sums.
__global__ void __launch_bounds__(SEGPLAN_BLOCK) k_seg_offsets(SegPlanParams p) {
  __shared__ long long v[SEGPLAN_BLOCK];
  if (res_gate_shut(p.gate)) return;
  const int t = threadIdx.x;
  const long long per = (p.nseg + SEGPLAN_BLOCK - 1) / SEGPLAN_BLOCK;
  const long long s0 = min((long long)t * per, p.nseg), s1 = min(s0 + per, p.nseg);
  for (int k = 0; k + 1 < p.levels; ++k) {
    long long sum = 0;
    for (long long s = s0; s < s1; ++s) sum += seg_ceil_pow(p.seg_off[s + 1] - p.seg_off[s], k + 1);
    v[t] = sum;
    __syncthreads();
    for (int o = 1; o < SEGPLAN_BLOCK; o <<= 1) {
      const long long x = t >= o ? v[t - o] : 0ll;
      __syncthreads();
      v[t] += x;
      __syncthreads();
    }
    long long run = v[t] - sum;
    long long* off = p.off + (long long)k * (p.nseg + 1);
    for (long long s = s0; s < s1; ++s) {
      off[s] = run;
      run += seg_ceil_pow(p.seg_off[s + 1] - p.seg_off[s], k + 1);
    }
    if (t == SEGPLAN_BLOCK - 1) off[p.nseg] = v[t];
    __syncthreads();
  }
}

// One lane per gather entry: row r belongs to the segment s with out_off[s] <= r < out_off[s + 1] (binary search; the
// last level has row s = segment s), part q = r - out_off[s] of it, and entry j is member 16 q + j of the segment's
// input rows, or -1 past its end. Every position read from index lies in [0, total): seg_off passed k_check_idx.
__global__ void __launch_bounds__(RES_BLOCK) k_seg_rows(SegRowsParams p) {
  if (res_gate_shut(p.gate)) return;
  const long long step = (long long)gridDim.x * RES_BLOCK;
  const long long entries = p.rows * SEGPLAN_C;
  for (long long u = (long long)blockIdx.x * RES_BLOCK + threadIdx.x; u < entries; u += step) {
    const long long r = u / SEGPLAN_C;
    const int j = (int)(u - r * SEGPLAN_C);
    long long s = r, q = 0;
    bool live = true;
    if (p.out_off) {
      live = r < p.out_off[p.nseg];
      if (live) {
        long long lo = 0, hi = p.nseg;     // the largest s with out_off[s] <= r; segments without parts are skipped
        while (hi - lo > 1) {
          const long long mid = lo + (hi - lo) / 2;
          if (p.out_off[mid] <= r) lo = mid;
          else hi = mid;
        }
        s = lo;
        q = r - p.out_off[s];
      }
    }
    long long src = -1;
    if (live) {
      const long long a = p.in_off[s], len = p.in_off[s + 1] - a, m = q * SEGPLAN_C + j;
      if (m < len) src = p.index ? p.index[a + m] : a + m;
    }
    p.gidx[u] = src;
  }
}

}  // namespace fpai
