// Catalogue recommendation for dot-product models with rows wider than 128 features (include/binrec.h "Catalogue top-k and AUC
// for wide rows"): the contract of recommend_dot.hip - exact fp32 scores that depend on the two rows only, the selection of
// brTopKRows, no U x I matrix - for 129 <= dim <= 512 (a BPR model at the reference's latent_dim = 350).
//
//   - the feature axis is cut into NB blocks of 128 features (32 k-steps of v_mfma_f32_16x16x4_f32); the instantiated width is
//     128 NB (256, 384 or 512), features in natural order, zero padded;
//   - a step's NT = 16 CT items go through LDS one block at a time, so the tile array is the whole-row kernel's at KB = 32
//     (NT x 132 floats) whatever the width; the accumulators are CARRIED across the blocks of a step: block s's MFMAs take the
//     accumulators block s - 1 left, one chain from 0 over the padded width, bit for bit the fmaf chain of the whole-row kernel (no
//     per-block partial sums, the feature axis is never split across waves);
//   - the next block (the next step's first block after a step's last) is in flight while the current one is scored;
//   - a wave owns 16 users (one row tile), their A fragments in registers for the whole launch: 32 NB VGPRs;
//   - everything after the scores - threshold compare, candidate queue, LDS lists, exclusion cursor, split plan, merge - is
//     recommend_dot.hip's (topk_list.h, dot_tile.h); that part of the tile loop is a copy kept the same by hand, as the AUC passes' (auc_count.h) is
//     (DESIGN.md 4e "One copy of the tile loop", 4h).
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"
#include "topk_list.h"

namespace br {
namespace {

constexpr int kDotQueue = 128;            // candidate queue entries per wave (flushed before it can overflow)

// list capacity and column tiles per step by k (one row tile per wave): the lists of a workgroup's 64 users live in LDS
struct WideCfg {
  int kmax, ct;
};
WideCfg wide_cfg(int k) {
  if (k <= 16) return {16, 4};
  if (k <= 64) return {64, 4};
  if (k <= 128) return {128, 4};
  return {256, 2};
}

void wide_plan(int64_t n_users, int64_t n_items, int k, int64_t* splits, int64_t* steps_per_split) {
  split_plan(ceil_div(n_items, 16 * wide_cfg(k).ct), n_users, 4 * kWideUW, splits, steps_per_split);
}

template <int NB, int KMAX, int CT>
__global__ __launch_bounds__(256) void dot_topk_wide_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users,
                                                             const float* __restrict__ C, int64_t ld_c, int64_t n_items, int dim, int vec,
                                                             const int64_t* __restrict__ ex_off, const int32_t* __restrict__ ex_idx, int k,
                                                             int64_t steps_per_split, int64_t n_splits, float* __restrict__ part_s,
                                                             int32_t* __restrict__ part_p, float* __restrict__ dump) {
  constexpr int UW = kWideUW;              // users per wave
  constexpr int NT = 16 * CT;              // items per step (<= 64: one exclusion mask word)
  constexpr int KB = kWideKB;              // k-steps per feature block
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): the B-fragment reads hit 64 distinct banks
  constexpr int CPT = NT * KB / 256;       // float4 chunks per thread and block
  constexpr int SLOTS = (KMAX + 63) / 64;
  static_assert(NT <= 64 && NT * KB % 256 == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) float tile[NT * LD];
  __shared__ float lst_s[4 * UW * KMAX];
  __shared__ int32_t lst_p[4 * UW * KMAX];
  __shared__ float thr_s[4 * UW];
  __shared__ int32_t thr_p[4 * UW];
  __shared__ float q_s[4 * kDotQueue];
  __shared__ int32_t q_p[4 * kDotQueue];
  __shared__ int32_t q_r[4 * kDotQueue];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = ((int64_t)blockIdx.x * 4 + wave) * UW;         // first user of this wave
  const bool active = u0 < n_users;                                   // (inactive waves still take part in the barriers)
  const int64_t split = blockIdx.y;
  const int64_t p0 = split * steps_per_split * NT;
  const int64_t p1 = p0 + steps_per_split * NT < n_items ? p0 + steps_per_split * NT : n_items;
  float* const LS = lst_s + wave * UW * KMAX;
  int32_t* const LP = lst_p + wave * UW * KMAX;
  float* const TS = thr_s + wave * UW;
  int32_t* const TP = thr_p + wave * UW;
  float* const QS = q_s + wave * kDotQueue;
  int32_t* const QP = q_p + wave * kDotQueue;
  int32_t* const QR = q_r + wave * kDotQueue;

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
  for (int i = lane; i < UW * KMAX; i += 64) { LS[i] = -INFINITY; LP[i] = kNoPos; }
  if (lane < UW) {                                                    // users past the end: a threshold nothing beats
    const bool ok = u0 + lane < n_users;
    TS[lane] = ok ? -INFINITY : INFINITY;
    TP[lane] = ok ? kNoPos : -1;
  }

  // exclusion cursor of user u0 + lane: the first entry of its list at or after p0, and that entry's position
  int64_t ex_cur = 0, ex_end = 0, ex_nxt = INT64_MAX;
  if (ex_off && lane < UW && u0 + lane < n_users) {
    int64_t lo = ex_off[u0 + lane], hi = ex_off[u0 + lane + 1];
    ex_end = hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)ex_idx[mid] < p0) lo = mid + 1; else hi = mid;
    }
    ex_cur = lo;
    if (ex_cur < ex_end) ex_nxt = ex_idx[ex_cur];
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

    // this window's exclusion mask of user u0 + lane (lanes < UW)
    uint64_t xm = 0;
    while (ex_nxt < base + NT) {
      if (ex_nxt >= base) xm |= 1ull << (ex_nxt - base);
      ++ex_cur;
      ex_nxt = ex_cur < ex_end ? (int64_t)ex_idx[ex_cur] : INT64_MAX;
    }
    const bool any_ex = __ballot(xm != 0) != 0;

    // D: lane l, register r = score(user u0 + 4 (l >> 4) + r, item base + 16 ct + (l & 15))
    float ts[4];
    int32_t tp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ts[r] = TS[4 * (lane >> 4) + r];
      tp[r] = TP[4 * (lane >> 4) + r];
    }
    int qn = 0;
    auto flush = [&]() {
      wave_lds_order();
      for (int i = 0; i < qn; ++i) {
        const int row = QR[i];
        const float cs = QS[i];
        const int32_t cp = QP[i];
        if (any_ex) {
          const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)xm, row, 64), hi = (uint32_t)__shfl((int)(uint32_t)(xm >> 32), row, 64);
          const uint64_t m = ((uint64_t)hi << 32) | lo;
          if ((m >> (cp - base)) & 1) continue;
        }
        float nts = TS[row];
        int32_t ntp = TP[row];
        if (!beats(cs, cp, nts, ntp)) continue;
        list_insert<SLOTS>(LS + row * KMAX, LP + row * KMAX, k, lane, cs, cp, nts, ntp);
        wave_lds_order();
        if (lane == 0) { TS[row] = nts; TP[row] = ntp; }
        wave_lds_order();
      }
      qn = 0;
    };
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int64_t p = base + 16 * ct + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[ct][r];
        const int row = 4 * (lane >> 4) + r;
        if (dump && p < p1 && u0 + row < n_users) dump[(u0 + row) * n_items + p] = s;
        const bool pass = p < p1 && beats(s, (int32_t)p, ts[r], tp[r]);
        const uint64_t bal = __ballot(pass);
        if (bal) {
          if (qn > kDotQueue - 64) flush();
          if (pass) {
            const int slot = qn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
            QS[slot] = s; QP[slot] = (int32_t)p; QR[slot] = row;
          }
          qn += __popcll(bal);
        }
      }
    }
    if (qn) flush();
  }

  __syncthreads();
  if (!active) return;
  for (int row = 0; row < UW; ++row) {
    const int64_t u = u0 + row;
    if (u >= n_users) break;
    const int64_t o = (u * n_splits + split) * k;
    for (int e = lane; e < k; e += 64) { part_s[o + e] = LS[row * KMAX + e]; part_p[o + e] = LP[row * KMAX + e]; }
  }
}

template <int NB>
void launch_dot_topk_wide(int kmax, dim3 grid, hipStream_t st, const float* Q, int64_t ld_q, int64_t U, const float* C, int64_t ld_c, int64_t I,
                          int dim, int vec, const int64_t* ex_off, const int32_t* ex_idx, int k, int64_t sps, int64_t S, float* ps, int32_t* pp,
                          float* dump) {
#define BR_DOT_ARGS Q, ld_q, U, C, ld_c, I, dim, vec, ex_off, ex_idx, k, sps, S, ps, pp, dump
  switch (kmax) {
    case 16: dot_topk_wide_kernel<NB, 16, 4><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
    case 64: dot_topk_wide_kernel<NB, 64, 4><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
    case 128: dot_topk_wide_kernel<NB, 128, 4><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
    default: dot_topk_wide_kernel<NB, 256, 2><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
  }
#undef BR_DOT_ARGS
}

bool topk_sizes_ok(int64_t n_users, int64_t n_items, int dim, int k) {
  return n_users >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31) && dim >= 1 && dim <= kDotWideMaxDim && k >= 1 && k <= kRecMaxK;
}

int64_t wide_ws_bytes(int64_t n_users, int64_t n_items, int k) {
  int64_t S, sps;
  wide_plan(n_users, n_items, k, &S, &sps);
  return 2 * part_bytes(n_users, S, k);
}

}  // namespace
}  // namespace br

using namespace br;

// the larger of the two plans' needs where both can run (dim <= 128: BR_DOT_FORCE_WIDE is not known here)
extern "C" int64_t brDotCatalogTopKWideWorkspaceBytes(int64_t n_users, int64_t n_items, int dim, int k) {
  if (!topk_sizes_ok(n_users, n_items, dim, k)) return -1;
  const int64_t wide = wide_ws_bytes(n_users, n_items, k);
  if (dim > kDotMaxDim) return wide;
  const int64_t narrow = brDotCatalogTopKWorkspaceBytes(n_users, n_items, k);
  return narrow > wide ? narrow : wide;
}

extern "C" int brDotCatalogTopKWide(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                                    const int64_t* excl_off, const int32_t* excl_idx, int k, float* out_scores, int32_t* out_index,
                                    float* dump_scores, int flags, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && out_scores && out_index && ws, "brDotCatalogTopKWide: null pointer");
  BR_CHECK_ARG(k >= 1 && k <= kRecMaxK, "brDotCatalogTopKWide: k = %d outside [1, %d]", k, kRecMaxK);
  if (const int rc = dot_check_args("brDotCatalogTopKWide", ld_q, n_users, ld_c, n_items, dim, kDotWideMaxDim)) return rc;
  BR_CHECK_ARG((excl_off == nullptr) == (excl_idx == nullptr), "brDotCatalogTopKWide: exclusion needs both excl_off and excl_idx");
  BR_CHECK_ARG((flags & ~BR_DOT_FORCE_WIDE) == 0, "brDotCatalogTopKWide: unknown flags 0x%x", flags);
  const int64_t need = brDotCatalogTopKWideWorkspaceBytes(n_users, n_items, dim, k);
  if (ws_bytes < need) {
    br::set_error("brDotCatalogTopKWide: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)need);
    return BR_ERR_WORKSPACE;
  }
  if (dim <= kDotMaxDim && !(flags & BR_DOT_FORCE_WIDE))            // the whole-row launches: same kernels, same plan, same bits
    return brDotCatalogTopK(Q, ld_q, n_users, C, ld_c, n_items, dim, excl_off, excl_idx, k, out_scores, out_index, dump_scores, ws, ws_bytes,
                            stream);
  if (n_users == 0) return BR_OK;
  int64_t S, sps;
  wide_plan(n_users, n_items, k, &S, &sps);
  const int64_t pb = part_bytes(n_users, S, k);
  float* ps = (float*)ws;
  int32_t* pp = (int32_t*)((char*)ws + pb);
  const WideCfg c = wide_cfg(k);
  const dim3 grid((unsigned)ceil_div(n_users, 4 * kWideUW), (unsigned)S);
  const int vec = rows_vec4(C, ld_c, dim);
  hipStream_t st = (hipStream_t)stream;
  dispatch_nb(dim, [&](auto nb) {
    launch_dot_topk_wide<decltype(nb)::value>(c.kmax, grid, st, Q, ld_q, n_users, C, ld_c, n_items, dim, vec, excl_off, excl_idx, k, sps, S, ps,
                                              pp, dump_scores);
  });
  BR_CHECK_LAUNCH("brDotCatalogTopKWide");
  catalog_merge_kernel<<<(unsigned)ceil_div(n_users, kRecWaves), 256, 0, st>>>(ps, pp, n_users, S, k, out_scores, out_index);
  BR_CHECK_LAUNCH("brDotCatalogTopKWide merge");
  return BR_OK;
}
