// Exact catalogue ranks of dot-product models on row-sharded engines, counted where the item rows live (include/binrec.h "Catalogue
// ranks at the item owners"; parallel.py ranks_at_owners).  brDotRankCount is the catalogue pass of brDotCatalogRanks
// alone (ranks_count.h: the same text, the same bits) over the candidates one owner holds, the dot-product counterpart of
// brNeumfRankCount: one skip CSR (the owner's truth and excluded positions, LOCAL), the users' FULL lists of brAucSortPieces behind
// the list CSR, and bins laid out by the list CSR that the call adds into.  The phases around it are model-independent:
// brDotAucOwnerPositives and brAucSortPieces (auc_owner.hip), brRankBinsExcluded and brRankBinsFinalize (ranks_neumf.hip).
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"
#include "ranks_count.h"

namespace br {
namespace {

template <int KB>
__global__ __launch_bounds__(256) void dot_rank_count_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                              int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ soff,
                                                              const int32_t* __restrict__ sidx, const int64_t* __restrict__ loff,
                                                              const float* __restrict__ sorted, const int32_t* __restrict__ pcnt, int64_t cap,
                                                              int64_t steps_per_split, int32_t* bins, int32_t* ties, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kRankNT * (4 * KB + 4)];
  __shared__ float pos_s[4 * kRankLdsCap];
  __shared__ int bin_s[4 * kRankBins];
  __shared__ uint64_t xm_s[4 * kRankUW];
  dot_ranks_pass<KB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, soff, sidx, nullptr, nullptr, loff, sorted, pcnt, cap, steps_per_split, bins,
                     ties, dump, tile, pos_s, bin_s, xm_s);
}

template <int NB>
__global__ __launch_bounds__(256) void dot_rank_count_wide_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users,
                                                                   const float* __restrict__ C, int64_t ld_c, int64_t n_items, int dim, int vec,
                                                                   const int64_t* __restrict__ soff, const int32_t* __restrict__ sidx,
                                                                   const int64_t* __restrict__ loff, const float* __restrict__ sorted,
                                                                   const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                                   int32_t* bins, int32_t* ties, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kRankNT * (4 * kWideKB + 4)];
  __shared__ float pos_s[4 * kRankLdsCap];
  __shared__ int bin_s[4 * kRankBins];
  __shared__ uint64_t xm_s[4 * kWideUW];
  dot_ranks_wide_pass<NB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, soff, sidx, nullptr, nullptr, loff, sorted, pcnt, cap, steps_per_split,
                          bins, ties, dump, tile, pos_s, bin_s, xm_s);
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int brDotRankCount(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                              const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off, const float* sorted,
                              const int32_t* pcnt, int64_t cap, int32_t* bins, int32_t* ties, float* dump_scores, int flags, brStream stream) {
  BR_CHECK_ARG(Q && C && skip_off && skip_idx && list_off && sorted && pcnt && bins && ties, "brDotRankCount: null pointer");
  if (const int rc = dot_check_args("brDotRankCount", ld_q, n_users, ld_c, n_items, dim, kDotWideMaxDim)) return rc;
  BR_CHECK_ARG((flags & ~BR_DOT_FORCE_WIDE) == 0, "brDotRankCount: unknown flags 0x%x", flags);
  BR_CHECK_ARG(cap >= 0 && n_users <= INT32_MAX && cap <= INT32_MAX - n_users, "brDotRankCount: cap = %lld: 0 <= cap, cap + n_users < 2^31",
               (long long)cap);
  if (n_users == 0) return BR_OK;
  const int vec = rows_vec4(C, ld_c, dim);
  hipStream_t st = (hipStream_t)stream;
  int64_t S, sps;
  if (!dot_use_wide(dim, flags)) {
    ranks_plan(n_users, n_items, kRankUW, &S, &sps);
    const dim3 grid((unsigned)ceil_div(n_users, 4 * kRankUW), (unsigned)S);
    dispatch_kb(dim, [&](auto kb) {
      dot_rank_count_kernel<decltype(kb)::value><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, skip_off, skip_idx, list_off,
                                                                       sorted, pcnt, cap, sps, bins, ties, dump_scores);
    });
  } else {
    ranks_plan(n_users, n_items, kWideUW, &S, &sps);
    const dim3 grid((unsigned)ceil_div(n_users, 4 * kWideUW), (unsigned)S);
    dispatch_nb(dim, [&](auto nb) {
      dot_rank_count_wide_kernel<decltype(nb)::value><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, skip_off, skip_idx,
                                                                            list_off, sorted, pcnt, cap, sps, bins, ties, dump_scores);
    });
  }
  BR_CHECK_LAUNCH("brDotRankCount");
  return BR_OK;
}
