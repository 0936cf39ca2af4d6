// Streaming top-k pieces shared by the catalogue kernels (recommend.hip: NeuMF, recommend_dot.hip: dot-product models).
// Order everywhere: (score desc, position asc), brTopKRows' rule: strict >, ties keep the lower position.  An empty entry is
// (-inf, kNoPos): it never beats anything and is written out as -1 by the final merge.
#pragma once
#include <math.h>

#include "common.h"

namespace br {
namespace {

constexpr int kRecWaves = 4;              // users (waves) per workgroup of the NeuMF kernel and of the merge
constexpr int kRecSlots = 4;              // list entries per lane: k <= 256
constexpr int kRecMaxK = 64 * kRecSlots;
constexpr int32_t kNoPos = 0x7FFFFFFF;    // empty list entry (score -inf): never beats anything, written out as -1

__device__ __forceinline__ bool beats(float s, int32_t p, float ts, int32_t tp) { return s > ts || (s == ts && p < tp); }

__device__ __forceinline__ uint64_t wave_or64(uint64_t m) {
  uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, off, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, off, 64);
  }
  return ((uint64_t)hi << 32) | lo;
}

// A running top-k list held by one wave: entry e at slot e >> 6 of lane e & 63, sorted by (score desc, position asc).
struct WaveList {
  float s[kRecSlots];
  int32_t p[kRecSlots];
  float ts;      // the k-th entry (wave-uniform): a candidate must beat it
  int32_t tp;

  __device__ void init() {
#pragma unroll
    for (int r = 0; r < kRecSlots; ++r) { s[r] = -INFINITY; p[r] = kNoPos; }
    ts = -INFINITY; tp = kNoPos;
  }

  // insert (cs, cp) (wave-uniform; the caller has checked that it beats the k-th entry)
  __device__ void insert(float cs, int32_t cp, int k, int lane) {
    int pos = 0;
#pragma unroll
    for (int r = 0; r < kRecSlots; ++r) {
      const int e = r * 64 + lane;
      pos += __popcll(__ballot(e < k && beats(s[r], p[r], cs, cp)));
    }
    float ps[kRecSlots];
    int32_t pp[kRecSlots];
#pragma unroll
    for (int r = 0; r < kRecSlots; ++r) {          // entry e - 1: lane - 1 of the same slot, or lane 63 of the slot before
      const float up_s = __shfl_up(s[r], 1, 64);
      const int32_t up_p = __shfl_up(p[r], 1, 64);
      const float wr_s = r ? __shfl(s[r - 1], 63, 64) : -INFINITY;
      const int32_t wr_p = r ? __shfl(p[r - 1], 63, 64) : kNoPos;
      ps[r] = lane ? up_s : wr_s;
      pp[r] = lane ? up_p : wr_p;
    }
#pragma unroll
    for (int r = 0; r < kRecSlots; ++r) {
      const int e = r * 64 + lane;
      if (e == pos) { s[r] = cs; p[r] = cp; }
      else if (e > pos) { s[r] = ps[r]; p[r] = pp[r]; }
    }
    const int last = k - 1, slot = last >> 6;
    float ls = s[0];
    int32_t lp = p[0];
#pragma unroll
    for (int r = 1; r < kRecSlots; ++r) if (r == slot) { ls = s[r]; lp = p[r]; }   // (no runtime register indexing)
    ts = __shfl(ls, last & 63, 64);
    tp = __shfl(lp, last & 63, 64);
  }

  // offer one candidate per lane (ok = lane has one); lanes are taken in ascending order
  __device__ void offer(float cs, int32_t cp, bool ok, int k, int lane) {
    uint64_t bal = __ballot(ok && beats(cs, cp, ts, tp));
    while (bal) {
      const int l = __ffsll((unsigned long long)bal) - 1;
      bal &= bal - 1;
      const float vs = __shfl(cs, l, 64);
      const int32_t vp = __shfl(cp, l, 64);
      if (beats(vs, vp, ts, tp)) insert(vs, vp, k, lane);
    }
  }

  __device__ void store(float* out_s, int32_t* out_p, int k, int lane, bool final_form) const {
#pragma unroll
    for (int r = 0; r < kRecSlots; ++r) {
      const int e = r * 64 + lane;
      if (e < k) {
        out_s[e] = s[r];
        out_p[e] = (final_form && p[r] == kNoPos) ? -1 : p[r];
      }
    }
  }
};

// Insert (cs, cp) (wave-uniform) into the k-entry list S/P in LDS (entry e at S[e]; lane holds entries lane + 64 r) unless it does
// not make the list.  Returns the new k-th entry through ts/tp (unchanged when the candidate is rejected).
template <int SLOTS>
__device__ void list_insert(float* S, int32_t* P, int k, int lane, float cs, int32_t cp, float& ts, int32_t& tp) {
  float s[SLOTS];
  int32_t p[SLOTS];
  int pos = 0;
#pragma unroll
  for (int r = 0; r < SLOTS; ++r) {
    const int e = r * 64 + lane;
    s[r] = e < k ? S[e] : -INFINITY;
    p[r] = e < k ? P[e] : kNoPos;
    pos += __popcll(__ballot(e < k && beats(s[r], p[r], cs, cp)));
  }
  if (pos >= k) return;                            // (every store below depends on pos, so all loads above come first)
  float ps[SLOTS];
  int32_t pp[SLOTS];
#pragma unroll
  for (int r = 0; r < SLOTS; ++r) {                // entry e - 1 of the old list: lane - 1 of the same slot, or lane 63 of the slot before
    const float up_s = __shfl_up(s[r], 1, 64);
    const int32_t up_p = __shfl_up(p[r], 1, 64);
    const float wr_s = r ? __shfl(s[r - 1], 63, 64) : -INFINITY;
    const int32_t wr_p = r ? __shfl(p[r - 1], 63, 64) : kNoPos;
    ps[r] = lane ? up_s : wr_s;
    pp[r] = lane ? up_p : wr_p;
  }
#pragma unroll
  for (int r = 0; r < SLOTS; ++r) {
    const int e = r * 64 + lane;
    if (e < k) {
      if (e == pos) { S[e] = cs; P[e] = cp; s[r] = cs; p[r] = cp; }
      else if (e > pos) { S[e] = ps[r]; P[e] = pp[r]; s[r] = ps[r]; p[r] = pp[r]; }
    }
  }
  const int last = k - 1, slot = last >> 6;
  float ls = s[0];
  int32_t lp = p[0];
#pragma unroll
  for (int r = 1; r < SLOTS; ++r) if (r == slot) { ls = s[r]; lp = p[r]; }   // (no runtime register indexing)
  ts = __shfl(ls, last & 63, 64);
  tp = __shfl(lp, last & 63, 64);
}

// one wave per user: the n_splits lists of k entries -> the final top-k
__global__ __launch_bounds__(256) void catalog_merge_kernel(const float* __restrict__ part_s, const int32_t* __restrict__ part_p,
                                                             int64_t n_users, int64_t n_splits, int k, float* __restrict__ out_s,
                                                             int32_t* __restrict__ out_p) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (u >= n_users) return;
  const int64_t n = n_splits * k;
  const float* s = part_s + u * n;
  const int32_t* p = part_p + u * n;
  WaveList list;
  list.init();
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t q = base + lane;
    const bool ok = q < n;
    list.offer(ok ? s[q] : -INFINITY, ok ? p[q] : kNoPos, ok, k, lane);
  }
  list.store(out_s + u * k, out_p + u * k, k, lane, true);
}

// bytes of one of the two per-split list arrays (scores, positions): n_users x n_splits x k entries, 256-B rounded
int64_t part_bytes(int64_t U, int64_t S, int k) { return (U * S * k * (int64_t)sizeof(float) + 255) / 256 * 256; }

}  // namespace
}  // namespace br
