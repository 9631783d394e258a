// Host interface of the packed-plaintext translation unit (engine_pack.hip, kernels_pack.hpp).
#pragma once
#include "kernels_pack.hpp"

namespace fpai {

// dynamic LDS bytes of k_pack_mul<tpi> (one S-limb slot per lane group, and n's S limbs)
constexpr size_t pack_lds_bytes(int tpi) { return ((size_t)BLOCK * L + (size_t)tpi * L) * 4; }
// blocks per CU of k_pack_mul<tpi> (-1: unsupported group size)
int pack_occupancy(int tpi, int* occ);
hipError_t pack_launch(int tpi, const PackMulParams& p, int grid, hipStream_t st);

// dynamic LDS bytes of k_pack_fold (two S-limb slots per lane group: the multiplicand, and acc during an injection)
constexpr size_t fold_lds_bytes() { return (size_t)2 * BLOCK * L * 4; }
// blocks per CU of k_pack_fold<tpi> (-1: unsupported group size)
int fold_occupancy(int tpi, int* occ);
hipError_t fold_launch(int tpi, const PackFoldParams& p, int grid, hipStream_t st);

// dynamic LDS bytes of k_unpack: UNPACK_CPB rows of pt_words + 1 words, the words of H, one flag per row
constexpr size_t unpack_lds_bytes(int pt_words) {
  return ((size_t)UNPACK_CPB * (pt_words + 1) + pt_words + UNPACK_CPB) * 4;
}
hipError_t unpack_launch(const UnpackParams& p, int grid, hipStream_t st);

}  // namespace fpai
