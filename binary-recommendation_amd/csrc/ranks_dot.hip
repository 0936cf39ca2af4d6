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
//   - dot_ranks_kernel / dot_ranks_wide_kernel: dot_ranks_pass / dot_ranks_wide_pass (ranks_count.h: one text with the owner-side
//     count brDotRankCount, ranks_owner.hip) with the truth CSR in both roles: the tile streams of dot_auc_pass and dot_auc_wide_pass
//     (auc_count.h), with two cursors (dot_tile.h RowCursor) behind the window mask (truth and exclusion).  Behind the scores, per
//     candidate score s of a user with n sorted positives (rank_count): s below
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
#include "ranks_count.h"

namespace br {
namespace {

constexpr int kRankMaxKs = 8;

// the whole-row pass (dim <= 128, 4 KB >= dim): the truth CSR in both roles of dot_ranks_pass (ranks_count.h), the exclusion CSR behind the
// second cursor
template <int KB>
__global__ __launch_bounds__(256) void dot_ranks_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                         int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ idx, const int64_t* __restrict__ xoff,
                                                         const int32_t* __restrict__ xidx, const float* __restrict__ sorted,
                                                         const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split, int32_t* bins,
                                                         int32_t* ties, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kRankNT * (4 * KB + 4)];
  __shared__ float pos_s[4 * kRankLdsCap];
  __shared__ int bin_s[4 * kRankBins];
  __shared__ uint64_t xm_s[4 * kRankUW];
  dot_ranks_pass<KB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, xoff, xidx, off, sorted, pcnt, cap, steps_per_split, bins, ties, dump,
                     tile, pos_s, bin_s, xm_s);
}

// the block pass (dim <= 512, 128 NB >= dim)
template <int NB>
__global__ __launch_bounds__(256) void dot_ranks_wide_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                              int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                              const int32_t* __restrict__ idx, const int64_t* __restrict__ xoff,
                                                              const int32_t* __restrict__ xidx, const float* __restrict__ sorted,
                                                              const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                              int32_t* bins, int32_t* ties, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kRankNT * (4 * kWideKB + 4)];
  __shared__ float pos_s[4 * kRankLdsCap];
  __shared__ int bin_s[4 * kRankBins];
  __shared__ uint64_t xm_s[4 * kWideUW];
  dot_ranks_wide_pass<NB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, xoff, xidx, off, sorted, pcnt, cap, steps_per_split, bins, ties,
                          dump, tile, pos_s, bin_s, xm_s);
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
