// Exact full-catalogue ranks of the positives for NeuMF (include/binrec.h "Catalogue ranks for NeuMF"): for every truth
// entry e = (u, p), over the head probability prob(u, i) brNeumfCatalogAuc / brNeumfCatalogTopK form and dump (neumf_score.h: the same
// text, the same bits) and the candidates i != p that the exclusion CSR leaves to u,
//
//   above[e] = #{i: prob(u, i) > prob(u, p)},   tied[e] = #{i: prob(u, i) == prob(u, p)}
//
// without the U x I matrix; brRankMetrics (ranks_dot.hip) turns the integers into MRR, NDCG@k, recall@k and hit@k.  The contract is
// brDotCatalogRanks' (DESIGN.md 4k).  The launches of brNeumfCatalogRanks:
//   - rank_init_kernel (rank_bins.h): the bins zeroed, the outputs -1;
//   - neumf_positives (auc_neumf.hip's neumf_auc_pos_kernel) and brAucSortPieces with one piece, as brNeumfCatalogAuc: the user's
//     non-NaN positives ascending v_0 <= ... <= v_{n-1}, their number n in pcnt;
//   - neumf_rank_count_kernel: neumf_auc_count_kernel's grid and split plan (4 users per workgroup, one wave per user, lane = item, 64
//     items per step); the window mask is the union of two WaveCursors (truth and exclusion).  Per valid unmasked score s: below v_0 or NaN
//     touches nothing; above v_{n-1} bumps a per-lane register counter (wave-reduced into bin n at the end of the split); inside,
//     lo = #{v < s} by binary lifting and bin lo gets +1 (the candidate outranks the positives 0 .. lo - 1), and where v_lo == s tie bin
//     lo too.  The list is wave-uniform: it sits in LDS up to kNeumfRankLdsCap entries with the wave's n + 1 bins beside it (LDS integer
//     adds, the non-zero bins added to the global ones at the end of the split); longer lists count straight into the global bins.
//     Integer atomics only: the result does not depend on the plan or on the order of arrival;
//   - rank_excluded_kernel (only with an exclusion CSR) and rank_finalize_kernel (rank_bins.h): the text brDotCatalogRanks launches.
// brNeumfRankCount is the catalogue pass alone, for the item owners of a row-sharded engine (parallel.py ranks_at_owners), and
// brRankBinsExcluded / brRankBinsFinalize the two shared kernels behind C entries: model-independent, as brAucSortPieces is.
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "neumf_score.h"
#include "neumf_tower.h"
#include "rank_bins.h"
#include "topk_list.h"

namespace br {
namespace {

// sorted positives of a wave's user kept in LDS up to this many, its n + 1 bins beside them: 2 KB + 2052 B per wave, 16 400 B per
// workgroup, so nine workgroups fit the 160 KB of a compute unit - more than the seven (28 waves) the registers of the narrowest tower
// allow: LDS never bounds the occupancy (at the AUC kernel's 1024 it would: four workgroups)
constexpr int kNeumfRankLdsCap = 512;

template <int W, int ACT>
__global__ __launch_bounds__(256) void neumf_rank_count_kernel(const float* __restrict__ pu, int64_t ld_u, const float* __restrict__ pit,
                                                                int64_t ld_i, int64_t n_users, int64_t n_items, int dim, int n1, int n3,
                                                                const float* __restrict__ tower, TowerLayout L,
                                                                const int64_t* __restrict__ t_off, const int32_t* __restrict__ t_idx,
                                                                const int64_t* __restrict__ x_off, const int32_t* __restrict__ x_idx,
                                                                const int64_t* __restrict__ loff, const float* __restrict__ sorted,
                                                                const int32_t* __restrict__ pcnt, int64_t cap, int64_t chunks_per_split,
                                                                int32_t* bins, int32_t* ties, float* __restrict__ dump_probs) {
  __shared__ float pos_s[kRecWaves * kNeumfRankLdsCap];
  __shared__ int bin_s[kRecWaves * (kNeumfRankLdsCap + 1)];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wave;
  if (u >= n_users) return;                                  // (no workgroup barrier below: a wave may leave alone)
  const auto [p0, p1] = split_items(blockIdx.y, chunks_per_split, n_items);

  // the user's sorted positives (wave-uniform): n entries from lb, in LDS with their bins when they fit, else read from `sorted`.  A
  // list that does not lie inside sorted's `cap` floats counts as empty (its entries keep (-1, -1): pcnt < 0)
  const int64_t lb = loff[u];
  int np = pcnt[u];
  if (np < 0 || lb < 0 || lb + np > cap) np = 0;
  if (np == 0 && !dump_probs) return;                        // nothing to rank against: no candidate of this user touches a bin
  const bool in_lds = np <= kNeumfRankLdsCap;
  float* const PS = pos_s + wave * kNeumfRankLdsCap;
  int* const BN = bin_s + wave * (kNeumfRankLdsCap + 1);
  const float* __restrict__ GS = sorted + (np > 0 ? lb : 0);
  int32_t* const GB = bins + (np > 0 ? lb + u : 0);          // the user's n + 1 global bins, the tie bins likewise
  int32_t* const GT = ties + (np > 0 ? lb + u : 0);
  if (in_lds) {
    for (int e = lane; e < np; e += 64) PS[e] = GS[e];
    for (int e = lane; e <= np; e += 64) BN[e] = 0;
    wave_lds_order();
  }
  const float mn = np > 0 ? GS[0] : INFINITY, mx = np > 0 ? GS[np - 1] : -INFINITY;
  int step0 = 0;                                             // highest power of two <= n
  if (np > 0) step0 = 1 << (31 - __builtin_clz((unsigned)np));

  const float* __restrict__ urow = pu + u * ld_u;            // [Pu (b1 included) | user mf]
  const TowerView t = tower_view(tower, L);

  // the two cursors: first entry of the user's truth row and of its exclusion row at or after p0 (no exclusion CSR: an empty row)
  WaveCursor tc = wave_cursor_at(t_off, t_idx, u, p0), xc;
  if (x_off) xc = wave_cursor_at(x_off, x_idx, u, p0);

  int over = 0;                                              // this lane's candidates above the user's largest positive
  for (int64_t base = p0; base < p1; base += 64) {
    const int64_t p = base + lane;
    const bool valid = p < p1;
    const int64_t pc = valid ? p : p1 - 1;                   // tail lanes recompute the last item (never read past the list)

    uint64_t m = wave_cursor_window(tc, t_idx, base, lane);
    if (xc.cur < xc.end) m |= wave_cursor_window(xc, x_idx, base, lane);         // (wave-uniform)
    const bool skipped = (wave_or64(m) >> lane) & 1;

    const float s = neumf_score<W, ACT>(urow, pit + pc, ld_i, dim, n1, n3, t);
    if (valid && dump_probs) dump_probs[u * n_items + p] = s;

    // fast paths first (a NaN score fails every compare: nothing); the scores inside [min, max] search the list
    const bool counts = valid && !skipped;
    over += counts && s > mx;
    const bool inside = counts && s >= mn && s <= mx;
    if (__ballot(inside) == 0) continue;

    // lo = #{entries < s} by binary lifting over the n entries; inside: s <= max, so lo < n
    auto search = [&](const float* A) __attribute__((always_inline)) {
      int c = 0;
      for (int step = step0; step > 0; step >>= 1) {
        const int j = c + step;
        const bool in = j <= np;
        const float v = A[in ? j - 1 : 0];
        if (in && v < s) c = j;
      }
      return c;
    };
    if (in_lds) {
      const int lo = search(PS);
      if (inside) {
        atomicAdd(&BN[lo], 1);
        if (PS[lo] == s) atomicAdd(&GT[lo], 1);
      }
    } else {
      const int lo = search(GS);
      if (inside) {
        atomicAdd(&GB[lo], 1);
        if (GS[lo] == s) atomicAdd(&GT[lo], 1);
      }
    }
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o, 64);
  if (np == 0) return;
  if (lane == 0 && over) atomicAdd(&GB[np], over);
  if (in_lds) {                                              // the wave's LDS bins into the global ones
    wave_lds_order();
    for (int e = lane; e <= np; e += 64) {
      const int v = BN[e];
      if (v) atomicAdd(&GB[e], v);
    }
  }
}

int rank_count(const char* name, const Operands& a, const int64_t* t_off, const int32_t* t_idx, const int64_t* x_off, const int32_t* x_idx,
               const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap, int32_t* bins, int32_t* ties, float* dump,
               hipStream_t st) {
  int64_t S, cps;
  catalog_plan(a.U, a.I, &S, &cps);
  const dim3 grid((unsigned)ceil_div(a.U, kRecWaves), (unsigned)S);
  if (const int rc = dispatch_tower(name, a.n2, a.act, [&](auto w, auto ac) {
        neumf_rank_count_kernel<decltype(w)::value, decltype(ac)::value><<<grid, 256, 0, st>>>(
            a.pu, a.ld_u, a.pit, a.ld_i, a.U, a.I, a.dim, a.n1, a.n3, a.tower, tower_layout(a.n1, a.n2, a.n3), t_off, t_idx, x_off, x_idx,
            list_off, sorted, pcnt, cap, cps, bins, ties, dump);
      }))
    return rc;
  BR_CHECK_LAUNCH(name);
  return BR_OK;
}

bool ranks_sizes_ok(int64_t n_users, int64_t n_truth) { return n_users >= 0 && n_truth >= 0 && n_truth + n_users <= INT32_MAX; }

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brNeumfCatalogRanksWorkspaceBytes(int64_t n_users, int64_t n_items, int64_t n_truth) {
  if (!catalog_sizes_ok(n_users, n_items) || !ranks_sizes_ok(n_users, n_truth)) return -1;
  return ranks_ws(n_users, n_truth).total + brAucSortPiecesWorkspaceBytes(1, n_truth);
}

extern "C" int brNeumfCatalogRanks(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim,
                                   int n1, int n2, int n3, int act, const float* tower, const int64_t* truth_off, const int32_t* truth_idx,
                                   int64_t n_truth, const int64_t* excl_off, const int32_t* excl_idx, int32_t* out_above, int32_t* out_tied,
                                   float* dump_probs, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(pu && pit && tower && truth_off && truth_idx && out_above && out_tied && ws, "brNeumfCatalogRanks: null pointer");
  BR_CHECK_ARG(!excl_off == !excl_idx, "brNeumfCatalogRanks: excl_off and excl_idx go together");
  if (const int rc = catalog_check_args("brNeumfCatalogRanks", ld_u, n_users, ld_i, n_items, dim, n1, n2, n3, act)) return rc;
  BR_CHECK_ARG(ranks_sizes_ok(n_users, n_truth), "brNeumfCatalogRanks: n_truth = %lld: 0 <= n_truth, n_truth + n_users < 2^31",
               (long long)n_truth);
  const RanksWs w = ranks_ws(n_users, n_truth);
  const int64_t tmp_bytes = brAucSortPiecesWorkspaceBytes(1, n_truth);
  if (ws_bytes < w.total + tmp_bytes) {
    br::set_error("brNeumfCatalogRanks: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)(w.total + tmp_bytes));
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  int32_t* pcnt = (int32_t*)((char*)ws + w.pcnt);
  float* raw = (float*)((char*)ws + w.raw);
  float* sorted = (float*)((char*)ws + w.sorted);
  int32_t* bins = (int32_t*)((char*)ws + w.bins);
  int32_t* ties = (int32_t*)((char*)ws + w.ties);
  void* tmp = (char*)ws + w.total;
  const int64_t cap = n_truth;                                       // truth entries [0, cap) fit; a user past them keeps (-1, -1)
  hipStream_t st = (hipStream_t)stream;
  launch_rank_init(st, w, ws, out_above, out_tied, n_truth);
  BR_CHECK_LAUNCH("brNeumfCatalogRanks init");
  const Operands a{pu, ld_u, pit, ld_i, n_users, n_items, dim, n1, n2, n3, act, tower};
  if (const int rc = neumf_positives("brNeumfCatalogRanks positives", a, truth_off, truth_idx, raw, cap, st)) return rc;
  // one piece per user, where the positives' kernel wrote it: piece_off = list_off = truth_off
  if (const int rc = brAucSortPieces(raw, cap, truth_off, 1, n_users, truth_off, sorted, cap, pcnt, tmp, tmp_bytes, stream)) return rc;
  if (const int rc = rank_count("brNeumfCatalogRanks count", a, truth_off, truth_idx, excl_off, excl_idx, truth_off, sorted, pcnt, cap,
                                bins, ties, dump_probs, st))
    return rc;
  const unsigned per_user = (unsigned)ceil_div(n_users, 4);
  if (excl_off) {
    rank_excluded_kernel<<<per_user, 256, 0, st>>>(truth_off, truth_idx, excl_off, excl_idx, raw, truth_off, sorted, pcnt, cap, n_users, bins,
                                                   ties);
    BR_CHECK_LAUNCH("brNeumfCatalogRanks excluded positives");
  }
  rank_finalize_kernel<<<per_user, 256, 0, st>>>(truth_off, truth_idx, excl_off, excl_idx, raw, truth_off, sorted, pcnt, cap, n_users, bins, ties,
                                                 out_above, out_tied);
  BR_CHECK_LAUNCH("brNeumfCatalogRanks finalize");
  return BR_OK;
}

extern "C" int brNeumfRankCount(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1,
                                int n2, int n3, int act, const float* tower, const int64_t* skip_off, const int32_t* skip_idx,
                                const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap, int32_t* bins, int32_t* ties,
                                float* dump_probs, brStream stream) {
  BR_CHECK_ARG(pu && pit && tower && skip_off && skip_idx && list_off && sorted && pcnt && bins && ties, "brNeumfRankCount: null pointer");
  if (const int rc = catalog_check_args("brNeumfRankCount", ld_u, n_users, ld_i, n_items, dim, n1, n2, n3, act)) return rc;
  BR_CHECK_ARG(ranks_sizes_ok(n_users, cap), "brNeumfRankCount: cap = %lld: 0 <= cap, cap + n_users < 2^31", (long long)cap);
  if (n_users == 0) return BR_OK;
  const Operands a{pu, ld_u, pit, ld_i, n_users, n_items, dim, n1, n2, n3, act, tower};
  return rank_count("brNeumfRankCount", a, skip_off, skip_idx, nullptr, nullptr, list_off, sorted, pcnt, cap, bins, ties, dump_probs,
                    (hipStream_t)stream);
}

extern "C" int brRankBinsExcluded(const int64_t* entry_off, const int32_t* entry_idx, const int64_t* excl_off, const int32_t* excl_idx,
                                  const float* raw, const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap,
                                  int64_t n_users, int32_t* bins, int32_t* ties, brStream stream) {
  BR_CHECK_ARG(entry_off && entry_idx && excl_off && excl_idx && raw && list_off && sorted && pcnt && bins && ties,
               "brRankBinsExcluded: null pointer");
  BR_CHECK_ARG(ranks_sizes_ok(n_users, cap), "brRankBinsExcluded: cap = %lld: 0 <= cap, cap + n_users < 2^31", (long long)cap);
  if (n_users == 0) return BR_OK;
  rank_excluded_kernel<<<(unsigned)ceil_div(n_users, 4), 256, 0, (hipStream_t)stream>>>(entry_off, entry_idx, excl_off, excl_idx, raw, list_off,
                                                                                         sorted, pcnt, cap, n_users, bins, ties);
  BR_CHECK_LAUNCH("brRankBinsExcluded");
  return BR_OK;
}

extern "C" int brRankBinsFinalize(const int64_t* entry_off, const int32_t* entry_idx, const int64_t* excl_off, const int32_t* excl_idx,
                                  const float* raw, const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap,
                                  int64_t n_users, int32_t* bins, const int32_t* ties, int32_t* above, int32_t* tied, brStream stream) {
  BR_CHECK_ARG(entry_off && entry_idx && raw && list_off && sorted && pcnt && bins && ties && above && tied, "brRankBinsFinalize: null pointer");
  BR_CHECK_ARG(!excl_off == !excl_idx, "brRankBinsFinalize: excl_off and excl_idx go together");
  BR_CHECK_ARG(ranks_sizes_ok(n_users, cap), "brRankBinsFinalize: cap = %lld: 0 <= cap, cap + n_users < 2^31", (long long)cap);
  if (n_users == 0) return BR_OK;
  rank_finalize_kernel<<<(unsigned)ceil_div(n_users, 4), 256, 0, (hipStream_t)stream>>>(entry_off, entry_idx, excl_off, excl_idx, raw, list_off,
                                                                                         sorted, pcnt, cap, n_users, bins, ties, above, tied);
  BR_CHECK_LAUNCH("brRankBinsFinalize");
  return BR_OK;
}
