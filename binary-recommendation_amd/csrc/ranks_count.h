// The catalogue pass of the dot-product ranks with its CSRs in separate roles: the one text of the tile loop behind brDotCatalogRanks
// (ranks_dot.hip) and behind brDotRankCount, the owner-side count of a row-sharded engine (ranks_owner.hip), as
// auc_count.h serves auc_dot.hip and auc_owner.hip.  The tile streams are those of dot_auc_pass and dot_auc_wide_pass (auc_count.h),
// copies kept the same by hand (DESIGN.md 4e "One copy of the tile loop").  The roles:
//   - the skip CSRs (soff, sidx) and (xoff, xidx; optional) are only what the two cursors (dot_tile.h RowCursor) and the window mask
//     read: positions into C that are no candidates of the user.  One device: the truth CSR and the exclusion CSR.  An owner: one CSR,
//     its truth and excluded positions merged, ascending LOCAL positions (xoff == nullptr folds the second cursor away);
//   - the list CSR loff says where user u's sorted positives lie in `sorted` (loff[u], pcnt[u] entries: ALL of them, of every owner)
//     and where its n + 1 bins and tie bins start (loff[u] + u).  `cap`: the floats `sorted` holds; a list that does not lie inside
//     is left alone (the rank_bins.h convention).
// With loff == soff the passes are the single-device kernels: the same pointer in both roles costs them no register.  The kernels own
// the LDS arrays (tile, pos_s, bin_s, xm_s) and hand them in.  The passes ADD into bins / ties; zeroing and finalizing is the caller's.
// Here too, once for every kernel that runs a pass: the tile shape, the LDS cap and the split plan.
#pragma once
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"

namespace br {
namespace {

constexpr int kRankRT = 2, kRankCT = 4;   // 32 users per wave (whole-row kernel; the block kernel: kWideUW), 64 items per step
constexpr int kRankUW = 16 * kRankRT, kRankNT = 16 * kRankCT;
constexpr int kRankLdsCap = 2048;         // sorted positives of a wave's users kept in LDS up to this many (8 KB per wave, the AUC's
                                          // kAucLdsCap) ...
constexpr int kRankBins = kRankLdsCap + kRankUW;   // ... and their n + 1 bins each beside them (8.1 KB per wave).  With the widest
// tile that is 98.5 KB of the CU's 160 KB: one workgroup per CU, which is what the kernels' registers (256 VGPRs and AGPRs on top,
// as the AUC kernels) allow anyway

void ranks_plan(int64_t n_users, int64_t n_items, int users_per_wave, int64_t* splits, int64_t* steps_per_split) {
  split_plan(ceil_div(n_items, kRankNT), n_users, 4 * users_per_wave, splits, steps_per_split);
}

// One row tile's 16 scores of a lane (CT column tiles x the lane's 4 users r) against their users' sorted lists.  ok: bit 4 ct + r
// set where the score counts (a candidate inside the split).  np / lb / hb: the users' P', list start in A and first bin in H and T;
// mn / mx: smallest and largest positive (NaN for an empty list: nothing compares).  A: PS or `sorted`; H: the LDS bins or the global
// ones; T: the global tie bins.
template <int CT>
__device__ __forceinline__ void rank_count(const f32x4 (&acc)[CT], uint32_t ok, const int (&np)[4], const int (&lb)[4], const int (&hb)[4],
                                           const float (&mn)[4], const float (&mx)[4], int (&over)[4], int step0, const float* A, int* H,
                                           int* T) {
  uint32_t in = 0;                                                    // bit 4 ct + r: the score lies inside [min, max] of its user
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = acc[ct][r];
      const bool c = (ok >> (4 * ct + r)) & 1;
      over[r] += c && s > mx[r];
      in |= (uint32_t)(c && s >= mn[r] && s <= mx[r]) << (4 * ct + r);
    }
  if (__ballot(in != 0) == 0) return;

  // c = #{entries < s} (le: <= s) by binary lifting over the user's np entries: the 16 searches step in lockstep
  auto search = [&](int (&c)[CT][4], bool le) __attribute__((always_inline)) {
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
          const bool inb = j <= np[r];
          const float v = A[lb[r] + (inb ? j - 1 : 0)];
          const float s = acc[ct][r];
          if (inb && (le ? v <= s : v < s)) c[ct][r] = j;
        }
    }
  };
  int lo[CT][4], hi[CT][4];
  bool any_tie = false;
  search(lo, false);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = A[lb[r] + (lo[ct][r] < np[r] ? lo[ct][r] : 0)];
      any_tie |= ((in >> (4 * ct + r)) & 1) && lo[ct][r] < np[r] && v == acc[ct][r];
      hi[ct][r] = lo[ct][r];
    }
  if (__ballot(any_tie)) search(hi, true);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((in >> (4 * ct + r)) & 1) {
        atomicAdd(&H[hb[r] + lo[ct][r]], 1);
        if (hi[ct][r] > lo[ct][r]) atomicAdd(&T[hb[r] + lo[ct][r]], 1);
      }
}

// the whole-row pass (dim <= 128, 4 KB >= dim): tile float [kRankNT * (4 KB + 4)] 16-B aligned, pos_s float [4 * kRankLdsCap], bin_s
// int [4 * kRankBins], xm_s uint64 [4 * kRankUW]
template <int KB>
__device__ __forceinline__ void dot_ranks_pass(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                               int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* soff,
                                               const int32_t* __restrict__ sidx, const int64_t* xoff, const int32_t* __restrict__ xidx,
                                               const int64_t* loff, const float* __restrict__ sorted, const int32_t* __restrict__ pcnt,
                                               int64_t cap, int64_t steps_per_split, int32_t* bins, int32_t* ties, float* __restrict__ dump,
                                               float* tile, float* pos_s, int* bin_s, uint64_t* xm_s) {
  constexpr int RT = kRankRT, CT = kRankCT, UW = kRankUW, NT = kRankNT;
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
  float* const PS = pos_s + wave * kRankLdsCap;
  int* const BN = bin_s + wave * kRankBins;
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

  // the sorted positives of the wave's users and their bins: in LDS when they fit (and lie inside the workspace), else in global memory
  const int64_t u_end = u0 + UW < n_users ? u0 + UW : n_users;
  const int64_t w0 = active ? loff[u0] : 0, w1 = active ? loff[u_end] : 0;
  const bool in_lds = active && w0 >= 0 && w1 >= w0 && w1 <= cap && w1 - w0 <= kRankLdsCap;
  if (in_lds) {
    for (int64_t e = lane; e < w1 - w0; e += 64) PS[e] = sorted[w0 + e];
    for (int e = lane; e < kRankBins; e += 64) BN[e] = 0;
  }
  const int64_t g0 = in_lds ? w0 + u0 : 0;                            // global bin of local bin 0
  // the lane's users (rt, r): user u0 + 16 rt + 4 (lane >> 4) + r: P', list start, first bin, smallest and largest positive
  int np[RT][4], lb[RT][4], hb[RT][4], over[RT][4];                   // (lb, hb: relative to w0 / g0, or absolute: < 2^31, checked by the entry)
  float mn[RT][4], mx[RT][4];
  int top = 0;                                                        // largest P' of the lane's users
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t u = u0 + 16 * rt + 4 * (lane >> 4) + r;
      const int n = u < n_users ? pcnt[u] : 0;                       // (-1 of brAucSortPieces for a list outside `cap`: empty)
      np[rt][r] = n > 0 ? n : 0;
      lb[rt][r] = n > 0 ? (int)(loff[u] - (in_lds ? w0 : 0)) : 0;     // (0 for an empty list: every load stays in bounds)
      hb[rt][r] = n > 0 ? (int)(loff[u] + u - g0) : 0;
      mn[rt][r] = n > 0 ? sorted[loff[u]] : __builtin_nanf("");
      mx[rt][r] = n > 0 ? sorted[loff[u] + n - 1] : __builtin_nanf("");
      over[rt][r] = 0;
      top = np[rt][r] > top ? np[rt][r] : top;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(top, o, 64);
    top = t > top ? t : top;
  }
  int step0 = 0;                                                      // highest power of two <= top (wave-uniform)
  if (top > 0) step0 = 1 << (31 - __builtin_clz((unsigned)top));

  // the cursors of user u0 + lane over its rows of the two skip CSRs
  RowCursor tc, xc;
  if (lane < UW && u0 + lane < n_users) {
    tc = cursor_at(soff, sidx, u0 + lane, p0);
    if (xoff) xc = cursor_at(xoff, xidx, u0 + lane, p0);
  }

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

    // this window's mask (the skipped positions) of user u0 + lane (lanes < UW), handed to the lanes that hold the user's scores through LDS
    const uint64_t xm = cursor_window(tc, sidx, base, NT) | cursor_window(xc, xidx, base, NT);
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
    // A score counts unless its item is masked for the user or lies past the split
    const int pl = lane & 15;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      uint64_t m[4] = {0, 0, 0, 0};
      if (any_ex) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = XM[16 * rt + 4 * (lane >> 4) + r];
      }
      uint32_t ok = 0;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t p = base + 16 * ct + pl;
          const int row = 16 * rt + 4 * (lane >> 4) + r;
          if (dump && p < p1 && u0 + row < n_users) dump[(u0 + row) * n_items + p] = acc[rt][ct][r];
          ok |= (uint32_t)(p < p1 && !((m[r] >> (16 * ct + pl)) & 1)) << (4 * ct + r);
        }
      if (in_lds) rank_count<CT>(acc[rt], ok, np[rt], lb[rt], hb[rt], mn[rt], mx[rt], over[rt], step0, PS, BN, ties + g0);
      else rank_count<CT>(acc[rt], ok, np[rt], lb[rt], hb[rt], mn[rt], mx[rt], over[rt], step0, sorted, bins, ties);
    }
  }

  if (!active) return;
  if (in_lds) {                                                       // the wave's LDS bins into the global ones
    wave_lds_order();
    const int nb = (int)(w1 - w0) + (int)(u_end - u0);
    for (int e = lane; e < nb; e += 64) {
      const int v = BN[e];
      if (v) atomicAdd(&bins[g0 + e], v);
    }
  }
  // the 16 lanes of a lane group hold the same users: the scores above the user's largest positive into its last bin
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int v = over[rt][r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((lane & 15) == 0 && np[rt][r] > 0 && v) atomicAdd(&bins[g0 + hb[rt][r] + np[rt][r]], v);
    }
}

// the block pass (dim <= 512, 128 NB >= dim): tile float [kRankNT * (4 kWideKB + 4)] 16-B aligned, pos_s float [4 * kRankLdsCap], bin_s
// int [4 * kRankBins], xm_s uint64 [4 * kWideUW]
template <int NB>
__device__ __forceinline__ void dot_ranks_wide_pass(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                    int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* soff,
                                                    const int32_t* __restrict__ sidx, const int64_t* xoff, const int32_t* __restrict__ xidx,
                                                    const int64_t* loff, const float* __restrict__ sorted, const int32_t* __restrict__ pcnt,
                                                    int64_t cap, int64_t steps_per_split, int32_t* bins, int32_t* ties,
                                                    float* __restrict__ dump, float* tile, float* pos_s, int* bin_s, uint64_t* xm_s) {
  constexpr int CT = kRankCT, UW = kWideUW, NT = kRankNT, KB = kWideKB;
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): the B-fragment reads hit 64 distinct banks
  constexpr int CPT = NT * KB / 256;       // float4 chunks per thread and block
  static_assert(NT <= 64 && NT * KB % 256 == 0 && UW <= kRankUW, "tile shape");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = ((int64_t)blockIdx.x * 4 + wave) * UW;         // first user of this wave
  const bool active = u0 < n_users;                                   // (inactive waves still take part in the barriers)
  const int64_t split = blockIdx.y;
  const int64_t p0 = split * steps_per_split * NT;
  const int64_t p1 = p0 + steps_per_split * NT < n_items ? p0 + steps_per_split * NT : n_items;
  float* const PS = pos_s + wave * kRankLdsCap;
  int* const BN = bin_s + wave * kRankBins;
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

  // the sorted positives of the wave's users and their bins: in LDS when they fit (and lie inside the workspace), else in global memory
  const int64_t u_end = u0 + UW < n_users ? u0 + UW : n_users;
  const int64_t w0 = active ? loff[u0] : 0, w1 = active ? loff[u_end] : 0;
  const bool in_lds = active && w0 >= 0 && w1 >= w0 && w1 <= cap && w1 - w0 <= kRankLdsCap;
  if (in_lds) {
    for (int64_t e = lane; e < w1 - w0; e += 64) PS[e] = sorted[w0 + e];
    for (int e = lane; e < kRankBins; e += 64) BN[e] = 0;
  }
  const int64_t g0 = in_lds ? w0 + u0 : 0;                            // global bin of local bin 0
  // the lane's users r: user u0 + 4 (lane >> 4) + r: P', list start, first bin, smallest and largest positive
  int np[4], lb[4], hb[4], over[4];                                   // (lb, hb: relative to w0 / g0, or absolute: < 2^31, checked by the entry)
  float mn[4], mx[4];
  int top = 0;                                                        // largest P' of the lane's users
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t u = u0 + 4 * (lane >> 4) + r;
    const int n = u < n_users ? pcnt[u] : 0;                         // (-1 of brAucSortPieces for a list outside `cap`: empty)
    np[r] = n > 0 ? n : 0;
    lb[r] = n > 0 ? (int)(loff[u] - (in_lds ? w0 : 0)) : 0;           // (0 for an empty list: every load stays in bounds)
    hb[r] = n > 0 ? (int)(loff[u] + u - g0) : 0;
    mn[r] = n > 0 ? sorted[loff[u]] : __builtin_nanf("");
    mx[r] = n > 0 ? sorted[loff[u] + n - 1] : __builtin_nanf("");
    over[r] = 0;
    top = np[r] > top ? np[r] : top;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(top, o, 64);
    top = t > top ? t : top;
  }
  int step0 = 0;                                                      // highest power of two <= top (wave-uniform)
  if (top > 0) step0 = 1 << (31 - __builtin_clz((unsigned)top));

  // the cursors of user u0 + lane over its rows of the two skip CSRs
  RowCursor tc, xc;
  if (lane < UW && u0 + lane < n_users) {
    tc = cursor_at(soff, sidx, u0 + lane, p0);
    if (xoff) xc = cursor_at(xoff, xidx, u0 + lane, p0);
  }

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

    // this window's mask (the skipped positions) of user u0 + lane (lanes < UW), handed to the lanes that hold the user's scores through LDS
    const uint64_t xm = cursor_window(tc, sidx, base, NT) | cursor_window(xc, xidx, base, NT);
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
    // A score counts unless its item is masked for the user or lies past the split
    const int pl = lane & 15;
    uint32_t ok = 0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t p = base + 16 * ct + pl;
        const int row = 4 * (lane >> 4) + r;
        if (dump && p < p1 && u0 + row < n_users) dump[(u0 + row) * n_items + p] = acc[ct][r];
        ok |= (uint32_t)(p < p1 && !((m[r] >> (16 * ct + pl)) & 1)) << (4 * ct + r);
      }
    if (in_lds) rank_count<CT>(acc, ok, np, lb, hb, mn, mx, over, step0, PS, BN, ties + g0);
    else rank_count<CT>(acc, ok, np, lb, hb, mn, mx, over, step0, sorted, bins, ties);
  }

  if (!active) return;
  if (in_lds) {                                                       // the wave's LDS bins into the global ones
    wave_lds_order();
    const int nb = (int)(w1 - w0) + (int)(u_end - u0);
    for (int e = lane; e < nb; e += 64) {
      const int v = BN[e];
      if (v) atomicAdd(&bins[g0 + e], v);
    }
  }
  // the 16 lanes of a lane group hold the same users: the scores above the user's largest positive into its last bin
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int v = over[r];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((lane & 15) == 0 && np[r] > 0 && v) atomicAdd(&bins[g0 + hb[r] + np[r]], v);
  }
}

}  // namespace
}  // namespace br
