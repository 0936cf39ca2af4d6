// Pieces the samplers share (sampling.hip: batch construction before the fit loop; sampling_step.hip: the per-step negative sampler of
// BPR; sampling_epoch.hip: the per-step batches of NeuMF).
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

// the positives of one customer for the rejection test: a list of up to 8 items is fetched ONCE, by independent loads (one round trip;
// the binary search of is_positive is a chain of dependent ones per attempt, and the launch is bound by such chains), a longer one is
// searched.  The same answer either way.
template <typename IdT>
struct Positives {
  const int64_t* off; const IdT* items; int64_t user; int64_t n; IdT v[8];
  __device__ __forceinline__ void load(const int64_t* __restrict__ o, const IdT* __restrict__ it, int64_t u) {
    off = o; items = it; user = u;
    const int64_t lo = o[u];
    n = o[u + 1] - lo;
    if (n >= 1 && n <= 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = it[lo + (k < n ? k : n - 1)];
    }
  }
  __device__ __forceinline__ bool has(IdT item) const {
    if (n <= 0) return false;
    if (n > 8) return is_positive(off, items, user, item);
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) hit |= v[k] == item;      // (entries past n repeat the last one)
    return hit;
  }
};

// the one candidate a Philox draw d names: slot = floor(d.x * n_cand / 2^32); with Walker's alias table (ops.alias_table) the slot is
// kept iff d.y < thresh[slot], else it is alias[slot]; the id is cand[slot], or the slot itself without a candidate list
template <typename IdT>
__device__ __forceinline__ int64_t candidate_of(const Philox4& d, const void* __restrict__ cand, const uint32_t* __restrict__ thresh,
                                                const int32_t* __restrict__ alias, uint32_t n_cand, int* err) {
  uint32_t slot = (uint32_t)(((uint64_t)d.x * (uint64_t)n_cand) >> 32);
  if (thresh && d.y >= thresh[slot]) {
    slot = (uint32_t)alias[slot];
    if (slot >= n_cand) { if (err) atomicOr(err, BR_ERRFLAG_RANGE); slot = 0; }      // (a table ops.alias_table did not build)
  }
  return cand ? (int64_t)((const IdT*)cand)[slot] : (int64_t)slot;
}

struct PermKey { uint32_t k[4]; };
__host__ __device__ __forceinline__ PermKey perm_key(uint64_t seed, uint32_t stream) {
  PermKey p;
  for (int r = 0; r < 4; ++r) p.k[r] = mix32((uint32_t)seed + 0x9E3779B9u * (uint32_t)(r + 1)) ^ mix32((uint32_t)(seed >> 32) ^ (stream * 0x85ebca6bu + (uint32_t)r));
  return p;
}
// keyed bijection of [0, M), M >= 1
__host__ __device__ __forceinline__ uint32_t feistel_perm(uint32_t x, uint32_t M, const PermKey& key) {
  if (M <= 1) return 0;
  int b = 1;
  while (b < 32 && (1ull << b) < (uint64_t)M) ++b;
  const int hb = (b + 1) >> 1;
  const uint32_t mask = (1u << hb) - 1u;
  do {
    uint32_t L = x >> hb, R = x & mask;
    for (int r = 0; r < 4; ++r) {
      const uint32_t F = mix32(R ^ key.k[r]) & mask;
      const uint32_t t = L ^ F;
      L = R; R = t;
    }
    x = (L << hb) | R;
  } while (x >= M);
  return x;
}

}  // namespace br
