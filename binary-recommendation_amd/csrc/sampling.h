// Pieces the samplers share (sampling.hip: batch construction before the fit loop; sampling_step.hip: the per-step negative sampler).
#pragma once
#include "common.h"
#include "philox.h"

namespace br {

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {      // murmur3 finaliser
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}

// uniform integer in [0, n) from one Philox call: floor(u32 * n / 2^32)
__device__ __forceinline__ uint32_t draw_below(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t stream, uint32_t n) {
  const Philox4 d = philox4x32_10(c0, c1, stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (uint32_t)(((uint64_t)d.x * (uint64_t)n) >> 32);
}

// membership of `item` in the sorted positive list of `user` (CSR)
template <typename IdT>
__device__ __forceinline__ bool is_positive(const int64_t* __restrict__ off, const IdT* __restrict__ pos_items, int64_t user, IdT item) {
  int64_t lo = off[user], hi = off[user + 1];
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const IdT v = pos_items[mid];
    if (v < item) lo = mid + 1; else hi = mid;
  }
  return lo < off[user + 1] && pos_items[lo] == item;
}

}  // namespace br
