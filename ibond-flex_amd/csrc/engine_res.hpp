// Host interface of the resident-buffer translation unit (engine_res.hip; the kernels: kernels_res.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fpai {

constexpr int RES_BLOCK = 256;
constexpr int32_t RES_EMPTY_EXP = INT32_MIN;   // the exponent of the identity (ciphertext 1): an empty segment's

struct TakeParams {
  const uint32_t* in;      // [N][W]
  const int32_t* in_exp;   // [N]
  const long long* index;  // [M], every entry -1 or in [0, N): checked before the launch (on the host, or by k_check_idx
                           // earlier on the stream, with `gate` set)
  long long M;
  int W;
  uint32_t* out;           // [M][W]
  int32_t* out_exp;        // [M]
  const long long* gate;   // nullable: the two words of k_check_idx; nothing is read through index or written when
                           // either is >= 0
};

struct CheckBelowParams {
  const uint32_t* ct;         // [N][W]
  long long N;
  int W;
  const uint32_t* limit;      // [W] little-endian 32-bit words of n^2
  unsigned long long* first;  // set to ~0 before the launch; the smallest i with ct[i] >= limit
};

// Device-side index lists (pai_take_idx_dev, pai_segment_add_idx_dev). bad[0] = the smallest t with index[t] outside
// [lo, N), bad[1] = the smallest offending position of seg_off (0: seg_off[0] != 0; s + 1: seg_off[s + 1] <
// seg_off[s]; nseg: seg_off[nseg] != total); both set to ~0 (-1) before the launch. seg_off is nullable (take).
struct CheckIdxParams {
  const long long* index;    // [total]
  long long total;
  long long lo, N;           // a valid entry v: lo <= v < N (lo = -1 admits the identity entry of take)
  const long long* seg_off;  // [nseg + 1], nullable
  long long nseg;
  unsigned long long* bad;   // [2]
};

constexpr int SEGPLAN_C = 16;        // members per partial sum: SEG_CHUNK of pai_segment_add_dev
constexpr int SEGPLAN_MAXLEV = 10;   // 16^10 = 2^40 > every supported total
constexpr int SEGPLAN_BLOCK = 1024;

// The levels of the reduction tree of pai_segment_add_idx_dev. Level k < levels - 1 turns the len_k(s) =
// ceil(len(s) / 16^k) rows of segment s into ceil(len_k(s) / 16) partial sums; off[k] is the exclusive scan of those
// counts over the segments, [nseg + 1] words each, k = 0 .. levels - 2 (k_seg_offsets). The last level writes one row per
// segment.
struct SegPlanParams {
  const long long* seg_off;  // [nseg + 1], checked by k_check_idx
  long long nseg;
  int levels;
  long long* off;            // [levels - 1][nseg + 1]
  const long long* gate;
};

// The gather rows of one level (k_seg_rows): row r, entry j of [rows][16], -1 where the part has no such member.
struct SegRowsParams {
  const long long* in_off;   // [nseg + 1]: the segments' ranges among this level's input rows
  const long long* index;    // level 0: input row = index[in_off[s] + t]; null: input row = in_off[s] + t
  const long long* out_off;  // [nseg + 1]: the scan of this level's part counts; null on the last level (row s = segment s)
  long long nseg;
  long long rows;            // rows written; those past out_off[nseg] are all -1
  long long* gidx;           // [rows][16]
  const long long* gate;
};

// grids are capped at 8 blocks per CU and stride over the work
hipError_t take_launch(const TakeParams& p, int cus, hipStream_t st);
hipError_t check_below_launch(const CheckBelowParams& p, int cus, hipStream_t st);
hipError_t check_idx_launch(const CheckIdxParams& p, int cus, hipStream_t st);
hipError_t seg_offsets_launch(const SegPlanParams& p, hipStream_t st);
hipError_t seg_rows_launch(const SegRowsParams& p, int cus, hipStream_t st);

}  // namespace fpai
