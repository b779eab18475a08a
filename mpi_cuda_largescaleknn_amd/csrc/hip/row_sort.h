// Sorting of neighbour rows by (d² bits << 32 | id) keys: the key packing and the LDS
// bitonic network of the fixed-k rows (knn_neighbors.hip) and the CSR rows (radius.hip).
#pragma once
#include "dev.h"

namespace lsk {

__device__ __forceinline__ uint64_t pack_key(uint32_t d2bits, int32_t id) {
  return ((uint64_t)d2bits << 32) | (uint32_t)id;
}
__device__ __forceinline__ uint32_t key_d2bits(uint64_t key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ int32_t key_id(uint64_t key) { return (int32_t)(uint32_t)key; }

// d² bits -> bits of the final distance
__device__ __forceinline__ uint32_t finalised(uint32_t d2bits) {
  return fbits(final_distance(bitsf(d2bits)));
}

// Bitonic network over every aligned kpad (a power of two) segment of key[0 .. nelem) in
// LDS, all ascending, by the block's nthreads threads. The caller fills `key` (padding:
// all-ones keys sort last) and syncs; every step here ends with __syncthreads.
__device__ __forceinline__ void sort_rows_lds(uint64_t *key, uint32_t nelem, uint32_t kpad, uint32_t nthreads) {
  for (uint32_t kk = 2; kk <= kpad; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < nelem / 2; t += nthreads) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
        const uint32_t p = i | j;
        const bool asc = ((i & (kpad - 1u)) & kk) == 0u;
        const uint64_t a = key[i], b = key[p];
        if ((a > b) == asc) {  // (equal keys are the same word: swapping them changes nothing)
          key[i] = b;
          key[p] = a;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace lsk
