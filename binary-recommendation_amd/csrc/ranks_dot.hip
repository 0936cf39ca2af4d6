// Exact full-catalogue ranks of the positives for dot-product models (include/binrec.h "Catalogue ranks"): for every truth entry
// e = (u, p), over score(u, i) = sum_j Q[u][j] C[i][j] in fp32 and the candidates i != p that the exclusion CSR leaves to u,
//
//   above[e] = #{i: score(u, i) > score(u, p)},   tied[e] = #{i: score(u, i) == score(u, p)}
//
// without the U x I score matrix, and from those integers NDCG@k, recall@k, hit@k and MRR (brRankMetrics).  DESIGN.md 4k.
//
// The launches of brDotCatalogRanks:
//   - rank_init_kernel (rank_bins.h, as the excluded and the finalize kernels below: one text with ranks_neumf.hip): the bins zeroed,
//     the outputs -1;
//   - auc_pos_kernel (auc_pos.h), as the AUC entries launch it: a positive's score bit for bit the catalogue pass's, the user's
//     non-NaN positives sorted ascending v_0 <= ... <= v_{n-1};
//   - dot_ranks_kernel / dot_ranks_wide_kernel: the tile streams of dot_auc_pass and dot_auc_wide_pass (auc_count.h), copies kept the
//     same by hand (DESIGN.md 4e "One copy of the tile loop"), with two cursors (dot_tile.h RowCursor) behind the
//     window mask (truth and exclusion).  Behind the scores, per candidate score s of a user with n sorted positives (rank_count): s below
//     v_0 or NaN touches nothing; s above v_{n-1} bumps a register counter; s inside searches lo = #{v < s} as the AUC does and adds
//     1 to the user's bin lo (n + 1 bins per user: the candidate outranks the positives 0 .. lo - 1), and on the rare tie path
//     (hi = #{v <= s} > lo) 1 to the tie bin lo.  The bins of a wave's users sit in LDS beside their sorted lists while those fit
//     (kRankLdsCap) and are added to the global bins at the end of the split; longer lists count into the global bins directly.
//     Integer atomics only: the result does not depend on the plan or on the order of arrival;
//   - rank_excluded_kernel (only with an exclusion CSR): a positive that is also excluded is ranked but is no candidate of the user's
//     other positives: -1 in its bin and its tie bin;
//   - rank_finalize_kernel: one wave per user: suffix sums over the bins in place, then per entry above = S[hi] + (n - hi) and
//     tied = T[lo] + (hi - lo) - [the entry is a candidate itself], the second terms being the user's other positives read off the
//     sorted list.  A NaN positive keeps (-1, -1).
#include <math.h>

#include "auc_pos.h"
#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"
#include "rank_bins.h"

namespace br {
namespace {

constexpr int kRankRT = 2, kRankCT = 4;   // 32 users per wave (whole-row kernel; the block kernel: kWideUW), 64 items per step
constexpr int kRankUW = 16 * kRankRT, kRankNT = 16 * kRankCT;
constexpr int kRankLdsCap = 2048;         // sorted positives of a wave's users kept in LDS up to this many (8 KB per wave, the AUC's
                                          // kAucLdsCap) ...
constexpr int kRankBins = kRankLdsCap + kRankUW;   // ... and their n + 1 bins each beside them (8.1 KB per wave).  With the widest
// tile that is 98.5 KB of the CU's 160 KB: one workgroup per CU, which is what the kernels' registers (256 VGPRs and AGPRs on top,
// as the AUC kernels) allow anyway
constexpr int kRankMaxKs = 8;

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

// the whole-row pass (dim <= 128, 4 KB >= dim)
template <int KB>
__global__ __launch_bounds__(256) void dot_ranks_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                         int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ idx, const int64_t* __restrict__ xoff,
                                                         const int32_t* __restrict__ xidx, const float* __restrict__ sorted,
                                                         const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split, int32_t* bins,
                                                         int32_t* ties, float* __restrict__ dump) {
  constexpr int RT = kRankRT, CT = kRankCT, UW = kRankUW, NT = kRankNT;
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): KB even -> the B-fragment reads hit 64 distinct banks
  constexpr int CHUNKS = NT * KB;          // float4 chunks per item tile
  constexpr int CPT = (CHUNKS + 255) / 256;
  static_assert(NT <= 64 && KB % 2 == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) float tile[NT * LD];
  __shared__ float pos_s[4 * kRankLdsCap];
  __shared__ int bin_s[4 * kRankBins];
  __shared__ uint64_t xm_s[4 * UW];

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
  const int64_t w0 = active ? off[u0] : 0, w1 = active ? off[u_end] : 0;
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
      const int n = u < n_users ? pcnt[u] : 0;
      np[rt][r] = n > 0 ? n : 0;
      lb[rt][r] = n > 0 ? (int)(off[u] - (in_lds ? w0 : 0)) : 0;      // (0 for an empty list: every load stays in bounds)
      hb[rt][r] = n > 0 ? (int)(off[u] + u - g0) : 0;
      mn[rt][r] = n > 0 ? sorted[off[u]] : __builtin_nanf("");
      mx[rt][r] = n > 0 ? sorted[off[u] + n - 1] : __builtin_nanf("");
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

  // the cursors of user u0 + lane over its truth row and its exclusion row
  RowCursor tc, xc;
  if (lane < UW && u0 + lane < n_users) {
    tc = cursor_at(off, idx, u0 + lane, p0);
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

    // this window's mask (positives and excluded) of user u0 + lane (lanes < UW), handed to the lanes that hold the user's scores through LDS
    const uint64_t xm = cursor_window(tc, idx, base, NT) | cursor_window(xc, xidx, base, NT);
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

// the block pass (dim <= 512, 128 NB >= dim)
template <int NB>
__global__ __launch_bounds__(256) void dot_ranks_wide_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                              int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                              const int32_t* __restrict__ idx, const int64_t* __restrict__ xoff,
                                                              const int32_t* __restrict__ xidx, const float* __restrict__ sorted,
                                                              const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                              int32_t* bins, int32_t* ties, float* __restrict__ dump) {
  constexpr int CT = kRankCT, UW = kWideUW, NT = kRankNT, KB = kWideKB;
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): the B-fragment reads hit 64 distinct banks
  constexpr int CPT = NT * KB / 256;       // float4 chunks per thread and block
  static_assert(NT <= 64 && NT * KB % 256 == 0 && UW <= kRankUW, "tile shape");
  __shared__ __attribute__((aligned(16))) float tile[NT * LD];
  __shared__ float pos_s[4 * kRankLdsCap];
  __shared__ int bin_s[4 * kRankBins];
  __shared__ uint64_t xm_s[4 * UW];

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
  const int64_t w0 = active ? off[u0] : 0, w1 = active ? off[u_end] : 0;
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
    const int n = u < n_users ? pcnt[u] : 0;
    np[r] = n > 0 ? n : 0;
    lb[r] = n > 0 ? (int)(off[u] - (in_lds ? w0 : 0)) : 0;            // (0 for an empty list: every load stays in bounds)
    hb[r] = n > 0 ? (int)(off[u] + u - g0) : 0;
    mn[r] = n > 0 ? sorted[off[u]] : __builtin_nanf("");
    mx[r] = n > 0 ? sorted[off[u] + n - 1] : __builtin_nanf("");
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

  // the cursors of user u0 + lane over its truth row and its exclusion row
  RowCursor tc, xc;
  if (lane < UW && u0 + lane < n_users) {
    tc = cursor_at(off, idx, u0 + lane, p0);
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

    // this window's mask (positives and excluded) of user u0 + lane (lanes < UW), handed to the lanes that hold the user's scores through LDS
    const uint64_t xm = cursor_window(tc, idx, base, NT) | cursor_window(xc, xidx, base, NT);
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

struct RankKs {
  int32_t k[kRankMaxKs];
};

// one wave per user: r = 1 + above + tied per positive with a rank, sums in double
__global__ __launch_bounds__(256) void rank_metrics_kernel(const int32_t* __restrict__ above, const int32_t* __restrict__ tied,
                                                            const int64_t* __restrict__ off, int64_t n_users, RankKs ks, int n_ks,
                                                            float* __restrict__ mrr, float* __restrict__ ndcg, float* __restrict__ recall,
                                                            float* __restrict__ hit) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int64_t o0 = off[u], o1 = off[u + 1], P = o1 - o0;
  if (P <= 0) {
    const float nan = __builtin_nanf("");
    if (lane == 0) mrr[u] = nan;
    if (lane < n_ks) ndcg[lane * n_users + u] = recall[lane * n_users + u] = hit[lane * n_users + u] = nan;
    return;
  }
  double dcg[kRankMaxKs];
  int64_t cnt[kRankMaxKs];
#pragma unroll
  for (int j = 0; j < kRankMaxKs; ++j) { dcg[j] = 0.0; cnt[j] = 0; }
  int64_t best = INT64_MAX;
  for (int64_t e = o0 + lane; e < o1; e += 64) {
    const int32_t a = above[e], t = tied[e];
    if (a < 0 || t < 0) continue;                                     // a positive without a rank: a miss that still counts in P
    const int64_t r = 1 + (int64_t)a + (int64_t)t;
    const double g = 1.0 / log2((double)(1 + r));
    best = r < best ? r : best;
#pragma unroll
    for (int j = 0; j < kRankMaxKs; ++j)
      if (j < n_ks && r <= (int64_t)ks.k[j]) { dcg[j] += g; ++cnt[j]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t b = __shfl_xor(best, o, 64);
    best = b < best ? b : best;
  }
  if (lane == 0) mrr[u] = best == INT64_MAX ? 0.f : (float)(1.0 / (double)best);
#pragma unroll
  for (int j = 0; j < kRankMaxKs; ++j) {
    if (j >= n_ks) break;
    const int64_t k = ks.k[j], top = P < k ? P : k;
    double ideal = 0.0;
    for (int64_t i = 1 + lane; i <= top; i += 64) ideal += 1.0 / log2((double)(1 + i));
    const double d = wave_sum_d(dcg[j]), id = wave_sum_d(ideal);
    int64_t c = cnt[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) {
      ndcg[j * n_users + u] = (float)(d / id);
      recall[j * n_users + u] = (float)((double)c / (double)P);
      hit[j * n_users + u] = best <= k ? 1.f : 0.f;
    }
  }
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brDotCatalogRanksWorkspaceBytes(int64_t n_users, int64_t n_items, int dim, int64_t n_truth) {
  if (n_users < 0 || n_items < 1 || n_items >= ((int64_t)1 << 31) || n_truth < 0 || dim < 1 || dim > kDotWideMaxDim) return -1;
  if (n_truth + n_users > INT32_MAX) return -1;
  return ranks_ws(n_users, n_truth).total;
}

extern "C" int brDotCatalogRanks(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                                 const int64_t* truth_off, const int32_t* truth_idx, int64_t n_truth, const int64_t* excl_off,
                                 const int32_t* excl_idx, int32_t* out_above, int32_t* out_tied, float* dump_scores, int flags, void* ws,
                                 int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && truth_off && truth_idx && out_above && out_tied && ws, "brDotCatalogRanks: null pointer");
  BR_CHECK_ARG(!excl_off == !excl_idx, "brDotCatalogRanks: excl_off and excl_idx go together");
  if (const int rc = dot_check_args("brDotCatalogRanks", ld_q, n_users, ld_c, n_items, dim, kDotWideMaxDim)) return rc;
  BR_CHECK_ARG((flags & ~BR_DOT_FORCE_WIDE) == 0, "brDotCatalogRanks: unknown flags 0x%x", flags);
  BR_CHECK_ARG(n_truth >= 0 && n_truth + n_users <= INT32_MAX, "brDotCatalogRanks: n_truth = %lld: 0 <= n_truth, n_truth + n_users < 2^31",
               (long long)n_truth);
  const RanksWs w = ranks_ws(n_users, n_truth);
  if (ws_bytes < w.total) {
    br::set_error("brDotCatalogRanks: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)w.total);
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  int32_t* pcnt = (int32_t*)((char*)ws + w.pcnt);
  float* raw = (float*)((char*)ws + w.raw);
  float* sorted = (float*)((char*)ws + w.sorted);
  int32_t* bins = (int32_t*)((char*)ws + w.bins);
  int32_t* ties = (int32_t*)((char*)ws + w.ties);
  const int64_t cap = n_truth;                                       // truth entries [0, cap) fit; a user past them keeps (-1, -1)
  const int vec = rows_vec4(C, ld_c, dim);
  hipStream_t st = (hipStream_t)stream;
  launch_rank_init(st, w, ws, out_above, out_tied, n_truth);
  BR_CHECK_LAUNCH("brDotCatalogRanks init");
  const unsigned per_user = (unsigned)ceil_div(n_users, 4);
  int64_t S, sps;
  if (!dot_use_wide(dim, flags)) {
    ranks_plan(n_users, n_items, kRankUW, &S, &sps);
    const dim3 grid((unsigned)ceil_div(n_users, 4 * kRankUW), (unsigned)S);
    dispatch_kb(dim, [&](auto kb) {
      constexpr int KB = decltype(kb)::value;
      auc_pos_kernel<KB><<<per_user, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, truth_off, truth_idx, raw, sorted, pcnt, cap);
      dot_ranks_kernel<KB><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, truth_off, truth_idx, excl_off, excl_idx, sorted,
                                                 pcnt, cap, sps, bins, ties, dump_scores);
    });
  } else {
    ranks_plan(n_users, n_items, kWideUW, &S, &sps);
    const dim3 grid((unsigned)ceil_div(n_users, 4 * kWideUW), (unsigned)S);
    dispatch_nb(dim, [&](auto nb) {
      constexpr int NB = decltype(nb)::value;
      auc_pos_kernel<NB * kWideKB><<<per_user, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, truth_off, truth_idx, raw, sorted, pcnt,
                                                              cap);
      dot_ranks_wide_kernel<NB><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, truth_off, truth_idx, excl_off, excl_idx,
                                                      sorted, pcnt, cap, sps, bins, ties, dump_scores);
    });
  }
  BR_CHECK_LAUNCH("brDotCatalogRanks");
  if (excl_off) {
    rank_excluded_kernel<<<per_user, 256, 0, st>>>(truth_off, truth_idx, excl_off, excl_idx, raw, truth_off, sorted, pcnt, cap, n_users, bins,
                                                   ties);
    BR_CHECK_LAUNCH("brDotCatalogRanks excluded positives");
  }
  rank_finalize_kernel<<<per_user, 256, 0, st>>>(truth_off, truth_idx, excl_off, excl_idx, raw, truth_off, sorted, pcnt, cap, n_users, bins, ties,
                                                 out_above, out_tied);
  BR_CHECK_LAUNCH("brDotCatalogRanks finalize");
  return BR_OK;
}

extern "C" int brRankMetrics(const int32_t* above, const int32_t* tied, const int64_t* truth_off, int64_t n_users, const int32_t* ks, int n_ks,
                             float* out_mrr, float* out_ndcg, float* out_recall, float* out_hit, brStream stream) {
  BR_CHECK_ARG(above && tied && truth_off && ks && out_mrr && out_ndcg && out_recall && out_hit, "brRankMetrics: null pointer");
  BR_CHECK_ARG(n_users >= 0, "brRankMetrics: n_users = %lld < 0", (long long)n_users);
  BR_CHECK_ARG(n_ks >= 1 && n_ks <= kRankMaxKs, "brRankMetrics: %d cutoffs: 1 <= n_ks <= %d", n_ks, kRankMaxKs);
  RankKs k{};
  for (int j = 0; j < n_ks; ++j) {
    BR_CHECK_ARG(ks[j] >= 1, "brRankMetrics: ks[%d] = %d < 1", j, ks[j]);
    k.k[j] = ks[j];
  }
  if (n_users == 0) return BR_OK;
  rank_metrics_kernel<<<(unsigned)ceil_div(n_users, 4), 256, 0, (hipStream_t)stream>>>(above, tied, truth_off, n_users, k, n_ks, out_mrr, out_ndcg,
                                                                                       out_recall, out_hit);
  BR_CHECK_LAUNCH("brRankMetrics");
  return BR_OK;
}
