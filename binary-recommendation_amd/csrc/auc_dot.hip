// Full-catalogue AUC for dot-product models (include/binrec.h "Catalogue AUC"): per user the Mann-Whitney statistic of brFullAuc
// (eval.hip) over score(u, i) = sum_j Q[u][j] C[i][j] in fp32, without the U x I score matrix:
//
//   AUC(u) = W / (P N),  2W = sum over positives p and negatives i of 2 [s_i < s_p] + [s_i == s_p]
//
// Three launches (the first and the last in auc_pos.h), for rows of up to 128 features (brDotCatalogAuc):
//   - auc_pos_kernel: one wave per user scores the user's truth entries on the same v_mfma_f32_16x16x4_f32, with the same feature
//     order and zero padding, as the catalogue pass (so a positive's score is bit for bit the one the catalogue pass sees), then
//     sorts them ascending by counting rank (O(P^2) compares per user), NaN scores dropped; the count P' of the rest goes beside;
//   - dot_auc_kernel: dot_auc_pass (auc_count.h, the one text shared with the owners' count in auc_owner.hip) with the truth CSR in both
//     of its roles; the kernel owns the LDS arrays.  The pass's tile loop is a copy of dot_topk_kernel's (recommend_dot.hip; kept the same
//     by hand, dot_tile.h): 4 waves, 32 users per wave with their A fragments in
//     registers, 64-item steps streamed through LDS with the next step in flight.  Each lane takes its 32 scores per step: a
//     positive (the truth CSR walked with a cursor and a 64-bit window mask, as the exclusion there) or a NaN score adds 0, a
//     score below the user's smallest positive 2P', above the largest 0, and one inside [min, max] 2 #{positives > s} +
//     #{positives == s} by a branchless binary search of the sorted list (the 16 searches of a lane's row tile step in lockstep, so
//     their loads are issued together).  The sorted lists of a wave's users sit in LDS when they fit (kAucLdsCap), in global memory
//     (L2) otherwise.  Per user and item split one 64-bit partial 2W;
//   - auc_finalize_kernel: 2W summed over the splits in integers, then (float)((double)W / ((double)P (double)N)), brFullAuc's
//     rounding: the result equals brFullAuc on the same scores bit for bit (exact while P N < 2^53), whatever the plan.
//
// Rows of 129 to 512 features (brDotCatalogAucWide; include/binrec.h "Catalogue top-k and AUC for wide rows") take the same three launches:
//   - auc_pos_kernel at the width 128 NB the catalogue pass is instantiated at (dot_wide.h): one accumulator chain from 0 over the
//     padded width, which is what the block chain below is, so a positive's score stays the catalogue pass's bit for bit;
//   - dot_auc_wide_kernel: dot_auc_wide_pass (auc_count.h, shared with the owners in the same way): the block stream of
//     dot_topk_wide_kernel (recommend_dot_wide.hip: 128-feature
//     blocks through the NT x 132 float LDS tile, accumulators carried across a step's blocks, the next block in flight) with 16 users
//     per wave, and behind the scores the integer Mann-Whitney count of dot_auc_pass, a copy kept the same by hand;
//   - auc_finalize_kernel.
// One host helper (run_auc) carves the workspace and makes the three launches for either width.
#include <math.h>

#include <string>

#include "auc_count.h"
#include "auc_pos.h"
#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"

namespace br {
namespace {

// workspace of a plan: partials uint64 [n_users][splits], P' int32 [n_users], then the raw and the sorted positive scores, float
// [n_truth + 1] each (the tail behind `fixed` is split in two halves; its size bounds the truth entries a call can take)
struct AucWs {
  int64_t splits, steps_per_split;          // the plan
  int64_t part, pcnt, raw, sorted, fixed;   // byte offsets; fixed: the bytes in front of the tail
  int64_t cap;                              // truth entries [0, cap) fit; a user past them gets NaN
};
AucWs auc_ws(bool wide, int64_t n_users, int64_t n_items, int64_t ws_bytes) {
  AucWs w;
  auc_plan(wide, n_users, n_items, &w.splits, &w.steps_per_split);
  w.part = 0;
  w.pcnt = align256(n_users * w.splits * 8);
  w.fixed = w.pcnt + align256(n_users * 4);
  const int64_t half = ws_bytes > w.fixed ? (ws_bytes - w.fixed) / 2 / 256 * 256 : 0;   // >= align256(4) in a call: one float of padding at least
  w.raw = w.fixed;
  w.sorted = w.fixed + half;
  w.cap = half / 4 - 1;
  if (w.cap > INT32_MAX) w.cap = INT32_MAX;
  return w;
}
int64_t auc_ws_bytes(bool wide, int64_t n_users, int64_t n_items, int64_t n_truth) {
  return auc_ws(wide, n_users, n_items, 0).fixed + 2 * align256(4 * (n_truth + 1));
}

template <int KB>
__global__ __launch_bounds__(256) void dot_auc_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                       int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ idx, const float* __restrict__ sorted,
                                                       const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                       int64_t n_splits, uint64_t* __restrict__ part, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kAucNT * (4 * KB + 4)];
  __shared__ float pos_s[4 * kAucLdsCap];
  __shared__ uint64_t xm_s[4 * kAucUW];
  dot_auc_pass<KB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, off, sorted, pcnt, cap, steps_per_split, n_splits, part, dump, tile,
                   pos_s, xm_s);
}

template <int NB>
__global__ __launch_bounds__(256) void dot_auc_wide_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                            int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ sorted,
                                                            const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                            int64_t n_splits, uint64_t* __restrict__ part, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kAucNT * (4 * kWideKB + 4)];
  __shared__ float pos_s[4 * kAucLdsCap];
  __shared__ uint64_t xm_s[4 * kWideUW];
  dot_auc_wide_pass<NB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, off, sorted, pcnt, cap, steps_per_split, n_splits, part, dump,
                        tile, pos_s, xm_s);
}

// positives -> catalogue pass -> finalize over the checked arguments of `name`, with the whole-row or the block kernels
int run_auc(const char* name, bool wide, const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
            const int64_t* off, const int32_t* idx, float* out_auc, float* dump, void* ws, int64_t ws_bytes, hipStream_t st) {
  const AucWs w = auc_ws(wide, n_users, n_items, ws_bytes);
  uint64_t* part = (uint64_t*)((char*)ws + w.part);
  int32_t* pcnt = (int32_t*)((char*)ws + w.pcnt);
  float* raw = (float*)((char*)ws + w.raw);
  float* sorted = (float*)((char*)ws + w.sorted);
  const int vec = rows_vec4(C, ld_c, dim);
  const unsigned per_user = (unsigned)ceil_div(n_users, 4);
  const dim3 grid((unsigned)ceil_div(n_users, 4 * (wide ? kWideUW : kAucUW)), (unsigned)w.splits);
  if (wide)
    dispatch_nb(dim, [&](auto nb) {
      constexpr int NB = decltype(nb)::value;
      auc_pos_kernel<NB * kWideKB><<<per_user, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, off, idx, raw, sorted, pcnt, w.cap);
      dot_auc_wide_kernel<NB><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, sorted, pcnt, w.cap,
                                                    w.steps_per_split, w.splits, part, dump);
    });
  else
    dispatch_kb(dim, [&](auto kb) {
      constexpr int KB = decltype(kb)::value;
      auc_pos_kernel<KB><<<per_user, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, off, idx, raw, sorted, pcnt, w.cap);
      dot_auc_kernel<KB><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, sorted, pcnt, w.cap, w.steps_per_split,
                                               w.splits, part, dump);
    });
  BR_CHECK_LAUNCH(name);
  auc_finalize_kernel<<<(unsigned)ceil_div(n_users, 256), 256, 0, st>>>(part, w.splits, off, pcnt, n_users, n_items, out_auc);
  BR_CHECK_LAUNCH((std::string(name) + " finalize").c_str());
  return BR_OK;
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brDotCatalogAucWorkspaceBytes(int64_t n_users, int64_t n_items, int64_t n_truth) {
  if (n_users < 0 || n_items < 1 || n_items >= ((int64_t)1 << 31) || n_truth < 0) return -1;
  return auc_ws_bytes(false, n_users, n_items, n_truth);
}

extern "C" int brDotCatalogAuc(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                               const int64_t* truth_off, const int32_t* truth_idx, float* out_auc, float* dump_scores, void* ws,
                               int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && truth_off && truth_idx && out_auc && ws, "brDotCatalogAuc: null pointer");
  if (const int rc = dot_check_args("brDotCatalogAuc", ld_q, n_users, ld_c, n_items, dim)) return rc;
  const int64_t least = brDotCatalogAucWorkspaceBytes(n_users, n_items, 0);
  if (ws_bytes < least) {
    br::set_error("brDotCatalogAuc: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)least);
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  return run_auc("brDotCatalogAuc", false, Q, ld_q, n_users, C, ld_c, n_items, dim, truth_off, truth_idx, out_auc, dump_scores, ws, ws_bytes,
                 (hipStream_t)stream);
}

// the larger of the two plans' needs where both can run (dim <= 128: BR_DOT_FORCE_WIDE is not known here)
extern "C" int64_t brDotCatalogAucWideWorkspaceBytes(int64_t n_users, int64_t n_items, int dim, int64_t n_truth) {
  if (n_users < 0 || n_items < 1 || n_items >= ((int64_t)1 << 31) || n_truth < 0 || dim < 1 || dim > kDotWideMaxDim) return -1;
  const int64_t wide = auc_ws_bytes(true, n_users, n_items, n_truth);
  if (dim > kDotMaxDim) return wide;
  const int64_t narrow = auc_ws_bytes(false, n_users, n_items, n_truth);
  return narrow > wide ? narrow : wide;
}

extern "C" int brDotCatalogAucWide(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                                   const int64_t* truth_off, const int32_t* truth_idx, float* out_auc, float* dump_scores, int flags, void* ws,
                                   int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && truth_off && truth_idx && out_auc && ws, "brDotCatalogAucWide: null pointer");
  if (const int rc = dot_check_args("brDotCatalogAucWide", ld_q, n_users, ld_c, n_items, dim, kDotWideMaxDim)) return rc;
  BR_CHECK_ARG((flags & ~BR_DOT_FORCE_WIDE) == 0, "brDotCatalogAucWide: unknown flags 0x%x", flags);
  const int64_t least = brDotCatalogAucWideWorkspaceBytes(n_users, n_items, dim, 0);
  if (ws_bytes < least) {
    br::set_error("brDotCatalogAucWide: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)least);
    return BR_ERR_WORKSPACE;
  }
  if (!dot_use_wide(dim, flags))                                      // the whole-row launches: same kernels, same plan, same bits
    return brDotCatalogAuc(Q, ld_q, n_users, C, ld_c, n_items, dim, truth_off, truth_idx, out_auc, dump_scores, ws, ws_bytes, stream);
  if (n_users == 0) return BR_OK;
  return run_auc("brDotCatalogAucWide", true, Q, ld_q, n_users, C, ld_c, n_items, dim, truth_off, truth_idx, out_auc, dump_scores, ws, ws_bytes,
                 (hipStream_t)stream);
}
