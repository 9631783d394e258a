// Encrypted histograms over a sparse (CSR) matrix of bin ids (pai_histogram_sparse[_dev]): the member lists of
// kernels_hist.hpp, built from the STORED entries instead of the (sample, feature) pairs, so that the work follows nnz.
//
// Every (node v, feature f) owns B + 1 slots: slot b < B is cell (v, f, b) of the histogram, slot B collects the stored
// missing values (bin id >= B), which enter S_{v,f} without entering a cell. A stored entry whose bin id is the
// feature's default bin is in no slot: the default cell is T_v - S_{v,f} (flexpai.hip). One further pseudo feature, F,
// holds in its slot 0 the list of ALL samples of node v, whose sum is T_v. The slot of (v, f, q) is
// (v (F + 1) + f) (B + 1) + q.
//
//   k_shist_indptr   indptr[0] == 0 and no offset decreases (error bits for the host).
//   k_shist_pass<0>  members per slot, and the checks of the indices: inside [0, F), strictly increasing inside a row.
//   k_shist_pass<1>  sample ids (int32) into the slots' member lists.
//
// The grid runs over tiles of SHIST_TILE units, unit u < nnz being stored entry u (its row by bisection of indptr) and
// unit nnz + i row i's entry in its node's list. A tile touches slots of many features, so the tile's counters are a hash
// table in LDS keyed by the slot (open addressing, twice the tile's units, so it never fills); as in k_hist_scatter one
// lane per touched slot flushes the tile's count, or reserves the tile's share of the slot's list, with ONE global atomic,
// and every unit lands at the reserved base plus its rank in the tile. The lists feed k_hist_acc unchanged.
#pragma once
#include "kernels_hist.hpp"

namespace fpai {

constexpr int SHIST_SPT = 8;                   // units per thread and tile
constexpr int SHIST_TILE = 256 * SHIST_SPT;
constexpr int SHIST_HASH = 2 * SHIST_TILE;     // LDS table slots (a power of two): 32 KiB of keys and counters
constexpr int SHIST_HASH_BITS = 12;
static_assert(SHIST_HASH == 1 << SHIST_HASH_BITS, "hash size");
constexpr unsigned SHIST_EMPTY = 0xffffffffu;

enum { SHIST_ERR_INDPTR = 1, SHIST_ERR_INDEX = 2, SHIST_ERR_ORDER = 4 };

struct SHistParams {
  const long long* indptr;     // [N + 1]
  const int32_t* indices;      // [nnz] feature of every stored entry
  const void* data;            // [nnz] its bin id
  int bin_u16;                 // 0: uint8, 1: uint16
  const int32_t* default_bin;  // [F]
  const int32_t* node;         // [N] (nullable: every sample in node 0)
  int nodes, B;
  long long N, F, nnz;
  long long f0, f1;            // the features of this launch, out of 0 .. F (F: the nodes' lists of all their samples)
  unsigned long long* count;   // [nodes (F + 1) (B + 1)] members per slot
  const int32_t* cell_off;     // first member of the slot in `members`
  unsigned* cursor;            // members placed so far, zeroed by the caller
  int32_t* members;            // the member lists of the features f0 .. f1
  unsigned* err;               // [1] SHIST_ERR_* bits (k_shist_pass<0>)
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_shist_indptr(const long long* indptr, long long N, unsigned* err) {
  unsigned e = 0u;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256)
    if (indptr[i + 1] < indptr[i] || indptr[i] < 0) e = SHIST_ERR_INDPTR;
  if (blockIdx.x == 0 && threadIdx.x == 0 && indptr[0] != 0) e = SHIST_ERR_INDPTR;
  if (e) atomicOr(err, e);
}

// slot of unit u, or -1 when it is in none (of this launch); CHECK adds the index checks of a stored entry to `err`
template <bool CHECK>
__device__ __forceinline__ int shist_slot(const SHistParams& p, long long u, int& sample, unsigned& err) {
  long long i, f;
  int q = 0;
  if (u < p.nnz) {
    const int fi = p.indices[u];
    if (fi < 0 || fi >= p.F) {
      if (CHECK) err |= SHIST_ERR_INDEX;
      return -1;
    }
    f = fi;
    if (!CHECK && (f < p.f0 || f >= p.f1)) return -1;
    // the row of entry u: the first i with indptr[i + 1] > u (any indptr keeps i inside 0 .. N - 1)
    long long lo = 0, hi = p.N - 1;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (p.indptr[mid + 1] > u) hi = mid;
      else lo = mid + 1;
    }
    i = lo;
    if (CHECK && u > p.indptr[i] && p.indices[u - 1] >= fi) err |= SHIST_ERR_ORDER;
    const unsigned b = p.bin_u16 ? (unsigned)static_cast<const uint16_t*>(p.data)[u] : (unsigned)static_cast<const uint8_t*>(p.data)[u];
    if (b < (unsigned)p.B && (int)b == p.default_bin[f]) return -1;
    q = (int)min(b, (unsigned)p.B);
  } else {
    i = u - p.nnz;
    f = p.F;
  }
  if (f < p.f0 || f >= p.f1) return -1;
  const int v = p.node ? p.node[i] : 0;
  if (v < 0 || v >= p.nodes) return -1;
  sample = (int)i;
  return (int)(((long long)v * (p.F + 1) + f) * (p.B + 1) + q);
}

// MODE 0 counts, MODE 1 scatters. grid: x tiles of SHIST_TILE units (grid stride)
template <int MODE>
__global__ __launch_bounds__(256) void k_shist_pass(SHistParams p) {
  __shared__ unsigned h_key[SHIST_HASH];
  __shared__ unsigned h_cnt[SHIST_HASH];   // per touched slot: the tile's count, then (MODE 1) the reserved base
  const long long units = p.nnz + p.N, tiles = (units + SHIST_TILE - 1) / SHIST_TILE;
  unsigned err = 0u;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int t = threadIdx.x; t < SHIST_HASH; t += 256) {
      h_key[t] = SHIST_EMPTY;
      h_cnt[t] = 0u;
    }
    __syncthreads();
    int at[SHIST_SPT], sample[SHIST_SPT];
    unsigned rank[SHIST_SPT];
#pragma unroll
    for (int s = 0; s < SHIST_SPT; ++s) {
      const long long u = tile * SHIST_TILE + s * 256 + threadIdx.x;
      at[s] = -1;
      sample[s] = 0;
      rank[s] = 0u;
      const int slot = u < units ? shist_slot<MODE == 0>(p, u, sample[s], err) : -1;
      if (slot < 0) continue;
      unsigned h = ((unsigned)slot * 2654435761u) >> (32 - SHIST_HASH_BITS);
      for (;;) {
        const unsigned prev = atomicCAS(&h_key[h], SHIST_EMPTY, (unsigned)slot);
        if (prev == SHIST_EMPTY || prev == (unsigned)slot) break;
        h = (h + 1) & (SHIST_HASH - 1);
      }
      at[s] = (int)h;
      rank[s] = atomicAdd(&h_cnt[h], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < SHIST_HASH; t += 256) {
      if (!h_cnt[t]) continue;
      if (MODE == 0) atomicAdd(&p.count[h_key[t]], (unsigned long long)h_cnt[t]);
      else h_cnt[t] = atomicAdd(&p.cursor[h_key[t]], h_cnt[t]);
    }
    if (MODE == 1) {
      __syncthreads();
#pragma unroll
      for (int s = 0; s < SHIST_SPT; ++s) {
        if (at[s] < 0) continue;
        const unsigned slot = h_key[at[s]];
        const unsigned long long pos = (unsigned long long)rank[s] + h_cnt[at[s]];
        // (a matrix rewritten between the two passes must not write outside the slot's list)
        if (pos < p.count[slot]) p.members[(long long)p.cell_off[slot] + (long long)pos] = sample[s];
      }
    }
    __syncthreads();
  }
  if (MODE == 0 && err) atomicOr(p.err, err);
}

}  // namespace fpai
