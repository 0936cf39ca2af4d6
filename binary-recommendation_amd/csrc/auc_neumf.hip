// Full-catalogue AUC for NeuMF (include/binrec.h "Catalogue AUC for NeuMF"): per user the Mann-Whitney statistic of
// brFullAuc (eval.hip) over the head probability sigmoidf_acc(z) of every (user, item) pair in inference mode - the value predict returns
// and catalog_topk_kernel (recommend.hip) ranks by - without the U x I matrix:
//
//   AUC(u) = W / (P N),  2W = sum over positives p and the other items i of 2 [s_i < s_p] + [s_i == s_p]
//
// The scoring loop is neumf_score.h's (neumf_logit: acc = b2', the fmaf chain over n1 with act(urow[i] + x), the W3'^T chain, the head
// with w4mf . dot; neumf_score: sigmoidf_acc of it), the one text catalog_topk_kernel and the ranks (ranks_neumf.hip) call too, so a
// pair's probability depends on its user row, its item column and the folded tower only - not on the lane, the split or the kernel that
// forms it; a test compares the kernels' dumps bit for bit (tests/test_gpu_neumf_auc.py).  This unit also owns the positives' kernel
// and its launch (neumf_positives, declared in neumf_score.h), which the ranks call: its instantiations are compiled here only.  Four
// phases, the two in the middle and at the end shared with the dot-product models (auc_owner.hip):
//   - neumf_auc_pos_kernel: one wave per user, lane = one of the user's truth entries, 64 at a time: raw[pos_off[u] + j];
//   - brAucSortPieces: per user one ascending list, NaN dropped, the count P' beside;
//   - neumf_auc_count_kernel: catalog_topk_kernel's grid and split plan (4 users per workgroup, lane = item, 64 items per step).  The
//     user's own positives among the candidates are skipped with the exclusion cursor and its 64-bit window mask; every other valid
//     score s adds 2P' below the list's minimum, 0 above its maximum (or when NaN), and 2 #{> s} + #{== s} inside, by binary lifting
//     over the sorted list with a second search only when a tie is met.  A wave has one user, so the list is wave-uniform: it sits in
//     LDS up to kNeumfAucLdsCap entries and is read from `sorted` past that.  Per lane a uint64 count, summed over the wave at the
//     end: one partial per (user, split), the splits summed in integers by a small launch.  No float atomics;
//   - brAucFinalizeLists: the one division in double.
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "neumf_score.h"
#include "neumf_tower.h"
#include "topk_list.h"

namespace br {
namespace {

// sorted positives of a wave's user kept in LDS up to this many: 4 KB per wave, 16 KB per workgroup, so ten workgroups fit the 160 KB
// of a compute unit - more than the eight (32 waves) it can hold at all: LDS never bounds the occupancy
constexpr int kNeumfAucLdsCap = 1024;

// one wave per user: raw[off[u] + j] = the probability of (u, the user's j-th entry) (neumf_score.h neumf_positives)
template <int W, int ACT>
__global__ __launch_bounds__(256) void neumf_auc_pos_kernel(const float* __restrict__ pu, int64_t ld_u, const float* __restrict__ pit,
                                                             int64_t ld_i, int64_t n_users, int64_t n_items, int dim, int n1, int n3,
                                                             const float* __restrict__ tower, TowerLayout L,
                                                             const int64_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                             float* __restrict__ raw, int64_t cap) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wave;
  if (u >= n_users) return;
  const int64_t o0 = off[u], o1 = off[u + 1], P = o1 - o0;
  if (P <= 0 || o0 < 0 || o1 > cap) return;

  const float* __restrict__ urow = pu + u * ld_u;            // [Pu (b1 included) | user mf]
  const TowerView t = tower_view(tower, L);
  for (int64_t j0 = 0; j0 < P; j0 += 64) {
    const int64_t j = j0 + lane;
    const int64_t p = j < P ? (int64_t)idx[o0 + j] : -1;
    const bool ok = p >= 0 && p < n_items;
    const int64_t pc = ok ? p : 0;                           // (a lane without an entry scores item 0: every load stays in bounds)
    const float prob = neumf_score<W, ACT>(urow, pit + pc, ld_i, dim, n1, n3, t);
    if (j < P) raw[o0 + j] = ok ? prob : __builtin_nanf("");
  }
}

template <int W, int ACT>
__global__ __launch_bounds__(256) void neumf_auc_count_kernel(const float* __restrict__ pu, int64_t ld_u, const float* __restrict__ pit,
                                                               int64_t ld_i, int64_t n_users, int64_t n_items, int dim, int n1, int n3,
                                                               const float* __restrict__ tower, TowerLayout L,
                                                               const int64_t* __restrict__ ex_off, const int32_t* __restrict__ ex_idx,
                                                               const int64_t* __restrict__ loff, const float* __restrict__ sorted,
                                                               const int32_t* __restrict__ pcnt, int64_t cap, int64_t chunks_per_split,
                                                               int64_t n_splits, uint64_t* __restrict__ part,
                                                               float* __restrict__ dump_probs) {
  __shared__ float pos_s[kRecWaves * kNeumfAucLdsCap];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wave;
  if (u >= n_users) return;                                  // (no workgroup barrier below: a wave may leave alone)
  const int64_t split = blockIdx.y;
  const auto [p0, p1] = split_items(split, chunks_per_split, n_items);
  const float* __restrict__ urow = pu + u * ld_u;            // [Pu (b1 included) | user mf]
  const TowerView t = tower_view(tower, L);

  // the user's sorted positives (wave-uniform): P' entries from lb, in LDS when they fit, else read from `sorted`.  A list that does
  // not lie inside sorted's `cap` floats counts as empty (its user gets NaN from the finalize: pcnt < 0)
  const int64_t lb = loff[u];
  int np = pcnt[u];
  if (np < 0 || lb < 0 || lb + np > cap) np = 0;
  const bool in_lds = np <= kNeumfAucLdsCap;
  float* const PS = pos_s + wave * kNeumfAucLdsCap;
  const float* __restrict__ GS = sorted + (np > 0 ? lb : 0);
  if (in_lds) {
    for (int e = lane; e < np; e += 64) PS[e] = GS[e];
    wave_lds_order();
  }
  const float mn = np > 0 ? GS[0] : INFINITY, mx = np > 0 ? GS[np - 1] : -INFINITY;
  int step0 = 0;                                             // highest power of two <= P'
  if (np > 0) step0 = 1 << (31 - __builtin_clz((unsigned)np));

  WaveCursor ex = wave_cursor_at(ex_off, ex_idx, u, p0);     // skip cursor: first entry of the user's list at or after p0

  uint64_t w2 = 0;
  for (int64_t base = p0; base < p1; base += 64) {
    const int64_t p = base + lane;
    const bool valid = p < p1;
    const int64_t pc = valid ? p : p1 - 1;                   // tail lanes recompute the last item (never read past the list)

    const bool skipped = (wave_or64(wave_cursor_window(ex, ex_idx, base, lane)) >> lane) & 1;

    const float s = neumf_score<W, ACT>(urow, pit + pc, ld_i, dim, n1, n3, t);
    if (valid && dump_probs) dump_probs[u * n_items + p] = s;

    // fast paths first (a NaN score fails every compare: 0); the scores inside [min, max] search the list
    const bool counts = valid && !skipped;
    if (counts && s < mn) w2 += 2 * (uint64_t)np;
    const bool inside = counts && s >= mn && s <= mx;
    if (__ballot(inside) == 0) continue;

    // c = #{entries < s} (le: <= s) by binary lifting over the np entries
    auto search = [&](const float* A, bool le) __attribute__((always_inline)) {
      int c = 0;
      for (int step = step0; step > 0; step >>= 1) {
        const int j = c + step;
        const bool in = j <= np;
        const float v = A[in ? j - 1 : 0];
        if (in && (le ? v <= s : v < s)) c = j;
      }
      return c;
    };
    const int lo = in_lds ? search(PS, false) : search(GS, false);
    const float at = in_lds ? PS[lo < np ? lo : 0] : GS[lo < np ? lo : 0];
    const bool tie = inside && lo < np && at == s;
    int hi = lo;
    if (__ballot(tie)) hi = in_lds ? search(PS, true) : search(GS, true);
    if (inside) w2 += 2u * ((uint32_t)np - (uint32_t)hi) + ((uint32_t)hi - (uint32_t)lo);   // np < 2^31: fits 32 bits
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w2 += __shfl_xor(w2, o, 64);
  if (lane == 0) part[u * n_splits + split] = w2;
}

// out[u] = the user's 2W over these candidates: its item splits summed in integers
__global__ __launch_bounds__(256) void neumf_auc_sum_splits_kernel(const uint64_t* __restrict__ part, int64_t n_splits, int64_t n_users,
                                                                    uint64_t* __restrict__ out) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  uint64_t w2 = 0;
  for (int64_t s = 0; s < n_splits; ++s) w2 += part[u * n_splits + s];
  out[u] = w2;
}

int64_t count_part_bytes(int64_t n_users, int64_t n_items) {
  int64_t S, cps;
  catalog_plan(n_users, n_items, &S, &cps);
  return align256(n_users * S * 8);
}

// brNeumfCatalogAuc's workspace ahead of the three float arrays: the count's partials, 2W uint64 [n_users], P' int32 [n_users]
int64_t auc_fixed_bytes(int64_t n_users, int64_t n_items) {
  return count_part_bytes(n_users, n_items) + align256(n_users * 8) + align256(n_users * 4);
}

int count(const char* name, const Operands& a, const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off,
          const float* sorted, const int32_t* pcnt, int64_t cap, uint64_t* part, uint64_t* out_w2, float* dump, hipStream_t st) {
  int64_t S, cps;
  catalog_plan(a.U, a.I, &S, &cps);
  if (cap > INT32_MAX) cap = INT32_MAX;
  const dim3 grid((unsigned)ceil_div(a.U, kRecWaves), (unsigned)S);
  if (const int rc = dispatch_tower(name, a.n2, a.act, [&](auto w, auto ac) {
        neumf_auc_count_kernel<decltype(w)::value, decltype(ac)::value><<<grid, 256, 0, st>>>(
            a.pu, a.ld_u, a.pit, a.ld_i, a.U, a.I, a.dim, a.n1, a.n3, a.tower, tower_layout(a.n1, a.n2, a.n3), skip_off, skip_idx, list_off,
            sorted, pcnt, cap, cps, S, part, dump);
      }))
    return rc;
  BR_CHECK_LAUNCH(name);
  neumf_auc_sum_splits_kernel<<<(unsigned)ceil_div(a.U, 256), 256, 0, st>>>(part, S, a.U, out_w2);
  BR_CHECK_LAUNCH(name);
  return BR_OK;
}

}  // namespace

int neumf_positives(const char* name, const Operands& a, const int64_t* off, const int32_t* idx, float* raw, int64_t cap, hipStream_t st) {
  if (const int rc = dispatch_tower(name, a.n2, a.act, [&](auto w, auto ac) {
        neumf_auc_pos_kernel<decltype(w)::value, decltype(ac)::value><<<(unsigned)ceil_div(a.U, kRecWaves), 256, 0, st>>>(
            a.pu, a.ld_u, a.pit, a.ld_i, a.U, a.I, a.dim, a.n1, a.n3, a.tower, tower_layout(a.n1, a.n2, a.n3), off, idx, raw, cap);
      }))
    return rc;
  BR_CHECK_LAUNCH(name);
  return BR_OK;
}

}  // namespace br

using namespace br;

extern "C" int brNeumfAucPositives(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim,
                                   int n1, int n2, int n3, int act, const float* tower, const int64_t* pos_off, const int32_t* pos_idx,
                                   float* raw, brStream stream) {
  BR_CHECK_ARG(pu && pit && tower && pos_off && pos_idx && raw, "brNeumfAucPositives: null pointer");
  if (const int rc = catalog_check_args("brNeumfAucPositives", ld_u, n_users, ld_i, n_items, dim, n1, n2, n3, act)) return rc;
  if (n_users == 0) return BR_OK;
  const Operands a{pu, ld_u, pit, ld_i, n_users, n_items, dim, n1, n2, n3, act, tower};
  return neumf_positives("brNeumfAucPositives", a, pos_off, pos_idx, raw, INT64_MAX, (hipStream_t)stream);
}

extern "C" int64_t brNeumfAucCountWorkspaceBytes(int64_t n_users, int64_t n_items) {
  if (!catalog_sizes_ok(n_users, n_items)) return -1;
  return count_part_bytes(n_users, n_items);
}

extern "C" int brNeumfAucCount(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1,
                               int n2, int n3, int act, const float* tower, const int64_t* skip_off, const int32_t* skip_idx,
                               const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap, uint64_t* out_w2,
                               float* dump_probs, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(pu && pit && tower && skip_off && skip_idx && list_off && sorted && pcnt && out_w2 && ws, "brNeumfAucCount: null pointer");
  if (const int rc = catalog_check_args("brNeumfAucCount", ld_u, n_users, ld_i, n_items, dim, n1, n2, n3, act)) return rc;
  BR_CHECK_ARG(cap >= 0, "brNeumfAucCount: cap = %lld < 0", (long long)cap);
  const int64_t least = count_part_bytes(n_users, n_items);
  if (ws_bytes < least) {
    br::set_error("brNeumfAucCount: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)least);
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  const Operands a{pu, ld_u, pit, ld_i, n_users, n_items, dim, n1, n2, n3, act, tower};
  return count("brNeumfAucCount", a, skip_off, skip_idx, list_off, sorted, pcnt, cap, (uint64_t*)ws, out_w2, dump_probs,
               (hipStream_t)stream);
}

extern "C" int64_t brNeumfCatalogAucWorkspaceBytes(int64_t n_users, int64_t n_items, int64_t n_truth) {
  if (!catalog_sizes_ok(n_users, n_items) || n_truth < 0) return -1;
  return auc_fixed_bytes(n_users, n_items) + 3 * align256(4 * (n_truth + 1));
}

extern "C" int brNeumfCatalogAuc(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1,
                                 int n2, int n3, int act, const float* tower, const int64_t* truth_off, const int32_t* truth_idx,
                                 float* out_auc, float* dump_probs, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(pu && pit && tower && truth_off && truth_idx && out_auc && ws, "brNeumfCatalogAuc: null pointer");
  if (const int rc = catalog_check_args("brNeumfCatalogAuc", ld_u, n_users, ld_i, n_items, dim, n1, n2, n3, act)) return rc;
  const int64_t fixed = auc_fixed_bytes(n_users, n_items), least = brNeumfCatalogAucWorkspaceBytes(n_users, n_items, 0);
  if (ws_bytes < least) {
    br::set_error("brNeumfCatalogAuc: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)least);
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  // the tail in three equal parts: the raw scores, the sorted lists and the sort's scratch; its size bounds the truth entries a call takes
  const int64_t third = (ws_bytes - fixed) / 3 / 256 * 256;          // >= align256(4): one float of padding at least
  char* const base = (char*)ws;
  uint64_t* part = (uint64_t*)base;
  uint64_t* w2 = (uint64_t*)(base + count_part_bytes(n_users, n_items));
  int32_t* pcnt = (int32_t*)(base + count_part_bytes(n_users, n_items) + align256(n_users * 8));
  float* raw = (float*)(base + fixed);
  float* sorted = (float*)(base + fixed + third);
  void* tmp = base + fixed + 2 * third;
  int64_t cap = third / 4 - 1;                                       // truth entries [0, cap) fit; a user past them gets NaN
  if (cap > INT32_MAX) cap = INT32_MAX;
  hipStream_t st = (hipStream_t)stream;
  const Operands a{pu, ld_u, pit, ld_i, n_users, n_items, dim, n1, n2, n3, act, tower};
  if (const int rc = neumf_positives("brNeumfCatalogAuc positives", a, truth_off, truth_idx, raw, cap, st)) return rc;
  // one piece per user, where the positives' kernel wrote it: piece_off = list_off = truth_off
  if (const int rc = brAucSortPieces(raw, cap, truth_off, 1, n_users, truth_off, sorted, cap, pcnt, tmp, third, stream)) return rc;
  if (const int rc = count("brNeumfCatalogAuc count", a, truth_off, truth_idx, truth_off, sorted, pcnt, cap, part, w2, dump_probs, st))
    return rc;
  return brAucFinalizeLists(w2, n_users, 1, truth_off, pcnt, n_users, n_items, out_auc, stream);
}
