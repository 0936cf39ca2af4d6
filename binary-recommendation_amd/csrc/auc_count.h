// The catalogue pass of the dot-product AUC, written twice: dot_auc_pass for whole rows (dim <= 128) and dot_auc_wide_pass for 128-feature
// blocks (dim <= 512).  Both serve the single-device kernels (auc_dot.hip) and the owner-side count of a row-sharded engine
// (auc_owner.hip); the two widths are copies of each other behind the scores, kept the same by hand, as their tile streams are copies of
// the top-k and rank kernels' (DESIGN.md 4e "One copy of the tile loop", 4i).  A pass has its two CSRs in two separate roles:
//   - (off, idx) is only what the cursor (dot_tile.h RowCursor) and the window mask skip: on an owner its own positives, ascending LOCAL
//     positions into C;
//   - loff says where a user's sorted list lies in `sorted` (loff[u], pcnt[u] entries): ALL the user's positives, of every owner.
// The single-device kernels pass loff = off: the truth CSR in both roles.  The kernels own the LDS arrays (tile, pos_s, xm_s) and hand
// them in.  Here too, once for every kernel that runs a pass: the tile shape, the LDS cap and the split plan.
#pragma once
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"

namespace br {
namespace {

constexpr int kAucRT = 2, kAucCT = 4;     // 32 users per wave (whole-row kernel; the block kernel: kWideUW), 64 items per step
constexpr int kAucUW = 16 * kAucRT, kAucNT = 16 * kAucCT;
constexpr int kAucLdsCap = 2048;          // sorted positives of a wave's users kept in LDS up to this many (8 KB per wave)

// the split plan of a pass: 4 waves of kAucUW (wide: kWideUW) users per workgroup, kAucNT items per step
void auc_plan(bool wide, int64_t n_users, int64_t n_items, int64_t* splits, int64_t* steps_per_split) {
  split_plan(ceil_div(n_items, kAucNT), n_users, 4 * (wide ? kWideUW : kAucUW), splits, steps_per_split);
}

// the whole-row pass (dim <= 128, 4 KB >= dim): tile float [kAucNT * (4 KB + 4)] 16-B aligned, pos_s float [4 * kAucLdsCap], xm_s uint64 [4 * kAucUW]
template <int KB>
__device__ __forceinline__ void dot_auc_pass(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C, int64_t ld_c, int64_t n_items, int dim,
                                             int vec, const int64_t* off, const int32_t* __restrict__ idx, const int64_t* loff, const float* __restrict__ sorted,
                                             const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split, int64_t n_splits, uint64_t* __restrict__ part,
                                             float* __restrict__ dump, float* tile, float* pos_s, uint64_t* xm_s) {
  constexpr int RT = kAucRT, CT = kAucCT, UW = kAucUW, NT = kAucNT;
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): KB even -> the B-fragment reads hit 64 distinct banks
  constexpr int CHUNKS = NT * KB;          // float4 chunks per item tile
  constexpr int CPT = (CHUNKS + 255) / 256;
  static_assert(NT <= 64 && KB % 2 == 0, "tile shape");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = ((int64_t)blockIdx.x * 4 + wave) * UW;         // first user of this wave
  const bool active = u0 < n_users;                                   // (inactive waves still take part in the barriers)
  const int64_t split = blockIdx.y;
  const int64_t p0 = split * steps_per_split * NT;
  const int64_t p1 = p0 + steps_per_split * NT < n_items ? p0 + steps_per_split * NT : n_items;
  float* const PS = pos_s + wave * kAucLdsCap;
  uint64_t* const XM = xm_s + wave * UW;

  // user rows as A fragments: lane l holds Q[u0 + 16 rt + (l & 15)][4 kb + (l >> 4)]
  float qa[RT][KB];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t u = u0 + 16 * rt + (lane & 15);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int f = 4 * kb + (lane >> 4);
      qa[rt][kb] = (u < n_users && f < dim) ? Q[u * ld_q + f] : 0.f;
    }
  }

  // the sorted positives of the wave's users: in LDS when they fit (and lie inside the workspace), else read from `sorted`
  const int64_t u_end = u0 + UW < n_users ? u0 + UW : n_users;
  const int64_t w0 = active ? loff[u0] : 0, w1 = active ? loff[u_end] : 0;
  const bool in_lds = active && w0 >= 0 && w1 >= w0 && w1 <= cap && w1 - w0 <= kAucLdsCap;
  if (in_lds)
    for (int64_t e = lane; e < w1 - w0; e += 64) PS[e] = sorted[w0 + e];
  // the lane's users (rt, r): user u0 + 16 rt + 4 (lane >> 4) + r: P', list start, smallest and largest positive
  int np[RT][4], lb[RT][4];                                           // (lb: relative to w0 or to `sorted`, < cap < 2^31)
  float mn[RT][4], mx[RT][4];
  uint64_t w2[RT][4];
  int top = 0;                                                        // largest P' of the lane's users
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t u = u0 + 16 * rt + 4 * (lane >> 4) + r;
      const int n = u < n_users ? pcnt[u] : 0;
      np[rt][r] = n > 0 ? n : 0;
      lb[rt][r] = n > 0 ? (int)(loff[u] - (in_lds ? w0 : 0)) : 0;      // (0 for an empty list: every load stays in bounds)
      mn[rt][r] = n > 0 ? sorted[loff[u]] : INFINITY;
      mx[rt][r] = n > 0 ? sorted[loff[u] + n - 1] : -INFINITY;
      w2[rt][r] = 0;
      top = np[rt][r] > top ? np[rt][r] : top;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(top, o, 64);
    top = t > top ? t : top;
  }
  int step0 = 0;                                                      // highest power of two <= top (wave-uniform)
  if (top > 0) step0 = 1 << (31 - __builtin_clz((unsigned)top));

  // skip cursor of user u0 + lane: the first entry of its (off, idx) row at or after p0, and that entry's position
  RowCursor xc;
  if (lane < UW && u0 + lane < n_users) xc = cursor_at(off, idx, u0 + lane, p0);

  float4 pre[CPT];
  auto load_tile = [&](int64_t start) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int chunk = c * 256 + tid;
      const int it = chunk / KB, f = 4 * (chunk % KB);
      const int64_t p = start + it;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (chunk < CHUNKS && p < p1 && f < dim) {
        const float* row = C + p * ld_c + f;
        if (vec) {
          v = *reinterpret_cast<const float4*>(row);
        } else {
          v.x = row[0];
          if (f + 1 < dim) v.y = row[1];
          if (f + 2 < dim) v.z = row[2];
          if (f + 3 < dim) v.w = row[3];
        }
      }
      pre[c] = v;
    }
  };
  load_tile(p0);

  for (int64_t base = p0; base < p1; base += NT) {
    __syncthreads();                                                  // the previous step's tile reads are done
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int chunk = c * 256 + tid;
      if (chunk < CHUNKS) *reinterpret_cast<float4*>(tile + (chunk / KB) * LD + 4 * (chunk % KB)) = pre[c];
    }
    __syncthreads();
    if (base + NT < p1) load_tile(base + NT);                         // in flight while this step is scored
    if (!active) continue;

    // this window's positive mask of user u0 + lane (lanes < UW), handed to the lanes that hold the user's scores through LDS
    const uint64_t xm = cursor_window(xc, idx, base, NT);
    const bool any_ex = __ballot(xm != 0) != 0;
    if (any_ex) {
      if (lane < UW) XM[lane] = xm;
      wave_lds_order();
    }

    f32x4 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float b = tile[(16 * ct + (lane & 15)) * LD + 4 * kb + (lane >> 4)];   // B[k][j] = C[item j][feature 4 kb + k]
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[rt][kb], b, acc[rt][ct], 0, 0, 0);
      }
    }

    // D: lane l, register r = score(user u0 + 16 rt + 4 (l >> 4) + r, item base + 16 ct + (l & 15)), user (rt, r) of the lane.
    // A score counts unless its item is one of the user's positives or lies past the split; fast paths first, then the scores
    // inside [min, max] of their user (never NaN, never a user without positives) search the sorted list, one row tile at a time
    const int pl = lane & 15;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      uint64_t m[4] = {0, 0, 0, 0};
      if (any_ex) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = XM[16 * rt + 4 * (lane >> 4) + r];
      }
      auto counts = [&](int ct, int r) { return base + 16 * ct + pl < p1 && !((m[r] >> (16 * ct + pl)) & 1); };
      auto inside = [&](int ct, int r) {
        const float s = acc[rt][ct][r];
        return counts(ct, r) && s >= mn[rt][r] && s <= mx[rt][r];
      };
      bool any_in = false;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[rt][ct][r];
          const int64_t p = base + 16 * ct + pl;
          const int row = 16 * rt + 4 * (lane >> 4) + r;
          if (dump && p < p1 && u0 + row < n_users) dump[(u0 + row) * n_items + p] = s;
          if (counts(ct, r) && s < mn[rt][r]) w2[rt][r] += 2 * (uint64_t)np[rt][r];
          any_in |= inside(ct, r);
        }
      if (__ballot(any_in) == 0) continue;

      // c = #{entries < s} (le: <= s) by binary lifting over the user's np entries: the 16 searches step in lockstep
      auto search = [&](const float* A, int (&c)[CT][4], bool le) __attribute__((always_inline)) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) c[ct][r] = 0;
        for (int step = step0; step > 0; step >>= 1) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = c[ct][r] + step;
              const bool in = j <= np[rt][r];
              const float v = A[lb[rt][r] + (in ? j - 1 : 0)];
              const float s = acc[rt][ct][r];
              if (in && (le ? v <= s : v < s)) c[ct][r] = j;
            }
        }
      };
      auto entry = [&](const float* A, int ct, int r, int l) __attribute__((always_inline)) {
        return A[lb[rt][r] + (l < np[rt][r] ? l : 0)];
      };
      int lo[CT][4], hi[CT][4];
      bool any_tie = false;
      if (in_lds) search(PS, lo, false); else search(sorted, lo, false);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = in_lds ? entry(PS, ct, r, lo[ct][r]) : entry(sorted, ct, r, lo[ct][r]);
          any_tie |= inside(ct, r) && lo[ct][r] < np[rt][r] && v == acc[rt][ct][r];
          hi[ct][r] = lo[ct][r];
        }
      if (__ballot(any_tie)) {
        if (in_lds) search(PS, hi, true); else search(sorted, hi, true);
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (inside(ct, r)) {                                        // 2 #{> s} + #{== s} of np < 2^31 entries: fits 32 bits
            const uint32_t n = (uint32_t)np[rt][r], l = (uint32_t)lo[ct][r], h = (uint32_t)hi[ct][r];
            w2[rt][r] += 2u * (n - h) + (h - l);
          }
    }
  }

  if (!active) return;
  // the 16 lanes of a lane group hold the same users: sum them, one partial per (user, split)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uint64_t v = w2[rt][r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      const int64_t u = u0 + 16 * rt + 4 * (lane >> 4) + r;
      if ((lane & 15) == 0 && u < n_users) part[u * n_splits + split] = v;
    }
}

// the block pass (dim <= 512, 128 NB >= dim): tile float [kAucNT * (4 kWideKB + 4)] 16-B aligned, pos_s float [4 * kAucLdsCap], xm_s uint64 [4 * kWideUW]
template <int NB>
__device__ __forceinline__ void dot_auc_wide_pass(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C, int64_t ld_c, int64_t n_items,
                                                  int dim, int vec, const int64_t* off, const int32_t* __restrict__ idx, const int64_t* loff,
                                                  const float* __restrict__ sorted, const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                  int64_t n_splits, uint64_t* __restrict__ part, float* __restrict__ dump, float* tile, float* pos_s, uint64_t* xm_s) {
  constexpr int CT = kAucCT, UW = kWideUW, NT = kAucNT, KB = kWideKB;
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): the B-fragment reads hit 64 distinct banks
  constexpr int CPT = NT * KB / 256;       // float4 chunks per thread and block
  static_assert(NT <= 64 && NT * KB % 256 == 0, "tile shape");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = ((int64_t)blockIdx.x * 4 + wave) * UW;         // first user of this wave
  const bool active = u0 < n_users;                                   // (inactive waves still take part in the barriers)
  const int64_t split = blockIdx.y;
  const int64_t p0 = split * steps_per_split * NT;
  const int64_t p1 = p0 + steps_per_split * NT < n_items ? p0 + steps_per_split * NT : n_items;
  float* const PS = pos_s + wave * kAucLdsCap;
  uint64_t* const XM = xm_s + wave * UW;

  // user rows as A fragments: lane l holds Q[u0 + (l & 15)][4 kb + (l >> 4)], kb over all NB blocks
  float qa[NB * KB];
  {
    const int64_t u = u0 + (lane & 15);
#pragma unroll
    for (int kb = 0; kb < NB * KB; ++kb) {
      const int f = 4 * kb + (lane >> 4);
      qa[kb] = (u < n_users && f < dim) ? Q[u * ld_q + f] : 0.f;
    }
  }

  // the sorted positives of the wave's users: in LDS when they fit (and lie inside the workspace), else read from `sorted`
  const int64_t u_end = u0 + UW < n_users ? u0 + UW : n_users;
  const int64_t w0 = active ? loff[u0] : 0, w1 = active ? loff[u_end] : 0;
  const bool in_lds = active && w0 >= 0 && w1 >= w0 && w1 <= cap && w1 - w0 <= kAucLdsCap;
  if (in_lds)
    for (int64_t e = lane; e < w1 - w0; e += 64) PS[e] = sorted[w0 + e];
  // the lane's users r: user u0 + 4 (lane >> 4) + r: P', list start, smallest and largest positive
  int np[4], lb[4];                                                   // (lb: relative to w0 or to `sorted`, < cap < 2^31)
  float mn[4], mx[4];
  uint64_t w2[4];
  int top = 0;                                                        // largest P' of the lane's users
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t u = u0 + 4 * (lane >> 4) + r;
    const int n = u < n_users ? pcnt[u] : 0;
    np[r] = n > 0 ? n : 0;
    lb[r] = n > 0 ? (int)(loff[u] - (in_lds ? w0 : 0)) : 0;            // (0 for an empty list: every load stays in bounds)
    mn[r] = n > 0 ? sorted[loff[u]] : INFINITY;
    mx[r] = n > 0 ? sorted[loff[u] + n - 1] : -INFINITY;
    w2[r] = 0;
    top = np[r] > top ? np[r] : top;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(top, o, 64);
    top = t > top ? t : top;
  }
  int step0 = 0;                                                      // highest power of two <= top (wave-uniform)
  if (top > 0) step0 = 1 << (31 - __builtin_clz((unsigned)top));

  // skip cursor of user u0 + lane: the first entry of its (off, idx) row at or after p0, and that entry's position
  RowCursor xc;
  if (lane < UW && u0 + lane < n_users) xc = cursor_at(off, idx, u0 + lane, p0);

  // features [f0, f0 + 128) of the items [start, start + NT) -> pre
  float4 pre[CPT];
  auto load_block = [&](int64_t start, int f0) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int chunk = c * 256 + tid;
      const int it = chunk / KB, f = f0 + 4 * (chunk % KB);
      const int64_t p = start + it;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < p1 && f < dim) {
        const float* row = C + p * ld_c + f;
        if (vec) {
          v = *reinterpret_cast<const float4*>(row);
        } else {
          v.x = row[0];
          if (f + 1 < dim) v.y = row[1];
          if (f + 2 < dim) v.z = row[2];
          if (f + 3 < dim) v.w = row[3];
        }
      }
      pre[c] = v;
    }
  };
  load_block(p0, 0);

  for (int64_t base = p0; base < p1; base += NT) {
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      __syncthreads();                                                // the previous block's tile reads are done
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int chunk = c * 256 + tid;
        *reinterpret_cast<float4*>(tile + (chunk / KB) * LD + 4 * (chunk % KB)) = pre[c];
      }
      __syncthreads();
      if (s + 1 < NB) load_block(base, 4 * KB * (s + 1));             // in flight while this block is scored
      else if (base + NT < p1) load_block(base + NT, 0);
      if (active) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const float b = tile[(16 * ct + (lane & 15)) * LD + 4 * kb + (lane >> 4)];   // B[k][j] = C[item j][feature 128 s + 4 kb + k]
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s * KB + kb], b, acc[ct], 0, 0, 0);
          }
        }
      }
    }
    if (!active) continue;

    // this window's positive mask of user u0 + lane (lanes < UW), handed to the lanes that hold the user's scores through LDS
    const uint64_t xm = cursor_window(xc, idx, base, NT);
    const bool any_ex = __ballot(xm != 0) != 0;
    uint64_t m[4] = {0, 0, 0, 0};
    if (any_ex) {
      wave_lds_order();                                               // (the previous step's reads of XM)
      if (lane < UW) XM[lane] = xm;
      wave_lds_order();
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] = XM[4 * (lane >> 4) + r];
    }

    // D: lane l, register r = score(user u0 + 4 (l >> 4) + r, item base + 16 ct + (l & 15)), user r of the lane.
    // A score counts unless its item is one of the user's positives or lies past the split; fast paths first, then the scores
    // inside [min, max] of their user (never NaN, never a user without positives) search the sorted list
    const int pl = lane & 15;
    auto counts = [&](int ct, int r) { return base + 16 * ct + pl < p1 && !((m[r] >> (16 * ct + pl)) & 1); };
    auto inside = [&](int ct, int r) {
      const float s = acc[ct][r];
      return counts(ct, r) && s >= mn[r] && s <= mx[r];
    };
    bool any_in = false;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[ct][r];
        const int64_t p = base + 16 * ct + pl;
        const int row = 4 * (lane >> 4) + r;
        if (dump && p < p1 && u0 + row < n_users) dump[(u0 + row) * n_items + p] = s;
        if (counts(ct, r) && s < mn[r]) w2[r] += 2 * (uint64_t)np[r];
        any_in |= inside(ct, r);
      }
    if (__ballot(any_in) == 0) continue;

    // c = #{entries < s} (le: <= s) by binary lifting over the user's np entries: the 16 searches step in lockstep
    auto search = [&](const float* A, int (&c)[CT][4], bool le) __attribute__((always_inline)) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[ct][r] = 0;
      for (int step = step0; step > 0; step >>= 1) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = c[ct][r] + step;
            const bool in = j <= np[r];
            const float v = A[lb[r] + (in ? j - 1 : 0)];
            const float s = acc[ct][r];
            if (in && (le ? v <= s : v < s)) c[ct][r] = j;
          }
      }
    };
    auto entry = [&](const float* A, int r, int l) __attribute__((always_inline)) { return A[lb[r] + (l < np[r] ? l : 0)]; };
    int lo[CT][4], hi[CT][4];
    bool any_tie = false;
    if (in_lds) search(PS, lo, false); else search(sorted, lo, false);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = in_lds ? entry(PS, r, lo[ct][r]) : entry(sorted, r, lo[ct][r]);
        any_tie |= inside(ct, r) && lo[ct][r] < np[r] && v == acc[ct][r];
        hi[ct][r] = lo[ct][r];
      }
    if (__ballot(any_tie)) {
      if (in_lds) search(PS, hi, true); else search(sorted, hi, true);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (inside(ct, r)) {                                          // 2 #{> s} + #{== s} of np < 2^31 entries: fits 32 bits
          const uint32_t n = (uint32_t)np[r], l = (uint32_t)lo[ct][r], h = (uint32_t)hi[ct][r];
          w2[r] += 2u * (n - h) + (h - l);
        }
  }

  if (!active) return;
  // the 16 lanes of a lane group hold the same users: sum them, one partial per (user, split)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    uint64_t v = w2[r];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int64_t u = u0 + 4 * (lane >> 4) + r;
    if ((lane & 15) == 0 && u < n_users) part[u * n_splits + split] = v;
  }
}

}  // namespace
}  // namespace br
