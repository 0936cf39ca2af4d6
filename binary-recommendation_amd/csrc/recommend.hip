// Catalogue recommendation for NeuMF (include/binrec.h "Catalogue top-k"): every user of a list scored against every item of a
// list in inference mode, only the k best per user written out, seen items excluded on the way.
//
// The first tower layer is separable: z1 = concat(mlp halves) . W1 + b1 = Pu[user] + Pi[item] with Pu = user_mlp . W1[user rows] + b1
// and Pi = item_mlp . W1[item rows] (brNeumfCatalogProject: two small products over the lists instead of 2*dim x n1 MACs per pair).
// BatchNorm in inference mode is an affine map a -> a * g rstd + (be - g mm rstd), folded into the next layer (brNeumfCatalogFold).
// Per pair what is left is act(Pu + Pi) -> n1 x n2 -> act -> n2 x n3 -> act -> head with the GMF dot, on the fp32 VALU with the
// weights as scalar (wave-uniform) operands, then sigmoid and a streaming top-k per user:
//   - one wave scores one user against 64 consecutive items per step (lane = item; the item side is stored feature-major, so each
//     feature is one coalesced 256-B load per wave); the user's row and the weights are scalar loads;
//   - a workgroup is 4 users (4 waves) over the same item range, the item axis is cut into splits so that small user lists still fill
//     the device (predictForUser: one user, up to 2048 splits);
//   - each wave keeps its user's running top-k of its split in registers (entry e = slot e / 64 of lane e % 64, sorted by (score desc,
//     position asc)); a pair enters only if it beats the k-th entry (one compare); the exclusion list of the user is walked with a
//     cursor as the item window advances (it is ascending), one 64-bit mask per window;
//   - the score, the tower view, the cursor and the dispatch over (tower width, activation) are neumf_score.h's, the one text the AUC
//     (auc_neumf.hip) and the ranks (ranks_neumf.hip) use too: this kernel calls neumf_logit and dumps z and sigmoidf_acc(z);
//   - a merge launch combines the splits' lists with the same order (ties keep the lower position, as brTopKRows) and pads with
//     (-inf, -1) where fewer than k candidates remain.
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "neumf_score.h"
#include "neumf_tower.h"
#include "topk_list.h"

namespace br {
namespace {

template <typename IdT>
__global__ __launch_bounds__(256) void catalog_project_kernel(const float* __restrict__ table, int64_t ld, int64_t rows,
                                                               const IdT* __restrict__ ids, int64_t n, int dim,
                                                               const float* __restrict__ W1, int n1, int w_row0,
                                                               const float* __restrict__ b1, int cols, float* __restrict__ out,
                                                               int64_t ld_out, int col_major, int* __restrict__ err) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * cols) return;
  int64_t r, c;
  if (col_major) { c = t / n; r = t - c * n; }
  else { r = t / cols; c = t - r * cols; }
  const int64_t id = load_id(ids, r);
  float v = 0.f;
  if (id < 0 || id >= rows) {
    if (c == 0 && err) atomicOr(err, BR_ERRFLAG_RANGE);
  } else {
    const float* row = table + id * ld;
    if (c < n1) {
      float acc = b1 ? b1[c] : 0.f;
      for (int d = 0; d < dim; ++d) acc = fmaf(row[d], W1[(int64_t)(w_row0 + d) * n1 + c], acc);
      v = acc;
    } else {
      v = row[dim + (c - n1)];
    }
  }
  out[col_major ? c * ld_out + r : r * ld_out + c] = v;
}

// one thread per folded element; double accumulation for the shifts (a sum over n1 / n2 terms)
__global__ __launch_bounds__(256) void catalog_fold_kernel(const float* __restrict__ W2, const float* __restrict__ b2,
                                                            const float* __restrict__ g1, const float* __restrict__ be1,
                                                            const float* __restrict__ mm1, const float* __restrict__ mv1,
                                                            const float* __restrict__ W3, const float* __restrict__ b3,
                                                            const float* __restrict__ g2, const float* __restrict__ be2,
                                                            const float* __restrict__ mm2, const float* __restrict__ mv2,
                                                            const float* __restrict__ W4, const float* __restrict__ b4, int n1, int n2,
                                                            int n3, int W, int mf_first, float eps, TowerLayout L,
                                                            float* __restrict__ tower) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L.total) return;
  auto scale1 = [&](int i) { return (double)g1[i] / sqrt((double)mv1[i] + (double)eps); };
  auto scale2 = [&](int j) { return (double)g2[j] / sqrt((double)mv2[j] + (double)eps); };
  float v = 0.f;
  if (t < L.b2) {                                   // W2'[i][j] = g1[i] rstd1[i] W2[i][j]
    const int i = (int)(t / W), j = (int)(t % W);
    if (j < n2) v = (float)(scale1(i) * (double)W2[(int64_t)i * n2 + j]);
  } else if (t < L.w3t) {                           // b2'[j] = b2[j] + sum_i (be1[i] - g1[i] mm1[i] rstd1[i]) W2[i][j]
    const int j = (int)(t - L.b2);
    if (j < n2) {
      double acc = b2[j];
      for (int i = 0; i < n1; ++i) acc += ((double)be1[i] - scale1(i) * (double)mm1[i]) * (double)W2[(int64_t)i * n2 + j];
      v = (float)acc;
    }
  } else if (t < L.b3) {                            // W3'^T[m][j] = g2[j] rstd2[j] W3[j][m]
    const int m = (int)((t - L.w3t) / W), j = (int)((t - L.w3t) % W);
    if (j < n2) v = (float)(scale2(j) * (double)W3[(int64_t)j * n3 + m]);
  } else if (t < L.w4) {
    const int m = (int)(t - L.b3);
    double acc = b3[m];
    for (int j = 0; j < n2; ++j) acc += ((double)be2[j] - scale2(j) * (double)mm2[j]) * (double)W3[(int64_t)j * n3 + m];
    v = (float)acc;
  } else if (t < L.w4mf) {                          // head: concat [dot, a3] (mf_first) or [a3, dot]
    const int m = (int)(t - L.w4);
    v = W4[mf_first ? 1 + m : m];
  } else if (t < L.b4) {
    v = W4[mf_first ? 0 : n3];
  } else {
    v = b4[0];
  }
  tower[t] = v;
}

template <int W, int ACT>
__global__ __launch_bounds__(256) void catalog_topk_kernel(const float* __restrict__ pu, int64_t ld_u, const float* __restrict__ pit,
                                                            int64_t ld_i, int64_t n_users, int64_t n_items, int dim, int n1, int n3,
                                                            const float* __restrict__ tower, TowerLayout L,
                                                            const int64_t* __restrict__ ex_off, const int32_t* __restrict__ ex_idx,
                                                            int k, int64_t chunks_per_split, int64_t n_splits,
                                                            float* __restrict__ part_s, int32_t* __restrict__ part_p,
                                                            float* __restrict__ dump_logits, float* __restrict__ dump_probs) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + wave;
  if (u >= n_users) return;
  const int64_t split = blockIdx.y;
  const auto [p0, p1] = split_items(split, chunks_per_split, n_items);
  const float* __restrict__ urow = pu + u * ld_u;            // [Pu (b1 included) | user mf]
  const TowerView t = tower_view(tower, L);
  WaveCursor ex;                                             // exclusion cursor: first entry of the user's list at or after p0
  if (ex_off) ex = wave_cursor_at(ex_off, ex_idx, u, p0);

  WaveList list;
  list.init();
  for (int64_t base = p0; base < p1; base += 64) {
    const int64_t p = base + lane;
    const bool valid = p < p1;
    const int64_t pc = valid ? p : p1 - 1;                   // tail lanes recompute the last item (never read past the list)

    bool excluded = false;
    if (ex_off) excluded = (wave_or64(wave_cursor_window(ex, ex_idx, base, lane)) >> lane) & 1;

    const float z = neumf_logit<W, ACT>(urow, pit + pc, ld_i, dim, n1, n3, t);
    const float prob = sigmoidf_acc(z);                      // the engine's head probability (predict)
    if (valid) {
      if (dump_logits) dump_logits[u * n_items + p] = z;
      if (dump_probs) dump_probs[u * n_items + p] = prob;
    }
    list.offer(prob, (int32_t)p, valid && !excluded, k, lane);
  }
  const int64_t o = (u * n_splits + split) * k;
  list.store(part_s + o, part_p + o, k, lane, false);
}

// brTopKRows with the exclusion CSR: one score row per workgroup, k passes, excluded columns skipped, (-inf, -1) past the end
__global__ __launch_bounds__(256) void topk_rows_exclude_kernel(const float* __restrict__ scores, int64_t n_items, int k,
                                                                 const int64_t* __restrict__ ex_off, const int32_t* __restrict__ ex_idx,
                                                                 float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  const float* row = scores + (int64_t)blockIdx.x * n_items;
  const int64_t e0 = ex_off ? ex_off[blockIdx.x] : 0, e1 = ex_off ? ex_off[blockIdx.x + 1] : 0;
  __shared__ float bs[4];
  __shared__ int bi[4];
  __shared__ float sel_s;
  __shared__ int sel_i;
  float prev_s = INFINITY;
  int prev_i = -1;
  for (int t = 0; t < k; ++t) {
    float best = -INFINITY;
    int besti = 0x7FFFFFFF;
    for (int64_t i = threadIdx.x; i < n_items; i += blockDim.x) {
      const float s = row[i];
      const bool after = (s < prev_s) || (s == prev_s && (int)i > prev_i);
      if (after && (s > best || (s == best && (int)i < besti))) {
        int64_t lo = e0, hi = e1;                          // excluded? (binary search in the ascending list)
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if ((int64_t)ex_idx[mid] < i) lo = mid + 1; else hi = mid;
        }
        if (!(lo < e1 && (int64_t)ex_idx[lo] == i)) { best = s; besti = (int)i; }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(besti, off, 64);
      if (os > best || (os == best && oi < besti)) { best = os; besti = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bs[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float b = bs[0]; int ix = bi[0];
      for (int w = 1; w < 4; ++w) if (bs[w] > b || (bs[w] == b && bi[w] < ix)) { b = bs[w]; ix = bi[w]; }
      sel_s = b; sel_i = ix;
      out_s[(int64_t)blockIdx.x * k + t] = ix == 0x7FFFFFFF ? -INFINITY : b;
      out_i[(int64_t)blockIdx.x * k + t] = ix == 0x7FFFFFFF ? -1 : ix;
    }
    __syncthreads();
    prev_s = sel_s; prev_i = sel_i;
    __syncthreads();
  }
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brNeumfCatalogTowerFloats(int n1, int n2, int n3) {
  if (!tower_shape_ok(n1, n2, n3)) return -1;
  return tower_layout(n1, n2, n3).total;
}

extern "C" int brNeumfCatalogFold(const float* W2, const float* b2, const float* g1, const float* be1, const float* mm1, const float* mv1,
                                  const float* W3, const float* b3, const float* g2, const float* be2, const float* mm2, const float* mv2,
                                  const float* W4, const float* b4, int n1, int n2, int n3, int mf_first, float bn_eps, float* tower,
                                  brStream stream) {
  BR_CHECK_ARG(W2 && b2 && g1 && be1 && mm1 && mv1 && W3 && b3 && g2 && be2 && mm2 && mv2 && W4 && b4 && tower,
               "brNeumfCatalogFold: null pointer");
  BR_CHECK_ARG(tower_shape_ok(n1, n2, n3), "brNeumfCatalogFold: tower widths n1, n2 <= 128, n3 <= 32 (got %d, %d, %d)", n1, n2, n3);
  const TowerLayout L = tower_layout(n1, n2, n3);
  catalog_fold_kernel<<<(unsigned)ceil_div(L.total, 256), 256, 0, (hipStream_t)stream>>>(
      W2, b2, g1, be1, mm1, mv1, W3, b3, g2, be2, mm2, mv2, W4, b4, n1, n2, n3, tower_width(n2), mf_first, bn_eps, L, tower);
  BR_CHECK_LAUNCH("brNeumfCatalogFold");
  return BR_OK;
}

extern "C" int brNeumfCatalogProject(const float* table, int64_t ld, int64_t rows, const void* ids, int id_type, int64_t n, int dim,
                                     const float* W1, int n1, int item_first, int user_side, const float* b1, int copy_mf, float* out,
                                     int64_t ld_out, int col_major, int* err_flag, brStream stream) {
  BR_CHECK_ARG(table && W1 && out, "brNeumfCatalogProject: null pointer");
  BR_CHECK_ARG(dim >= 1 && 2 * dim <= 256 && n1 >= 1 && n1 <= 128 && ld >= 2 * dim && rows >= 0 && n >= 0,
               "brNeumfCatalogProject: bad shape (1 <= dim, 2*dim <= 256, 1 <= n1 <= 128, ld >= 2*dim)");
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brNeumfCatalogProject: bad id_type");
  const int cols = n1 + (copy_mf ? dim : 0);
  BR_CHECK_ARG(col_major ? ld_out >= n : ld_out >= cols, "brNeumfCatalogProject: ld_out too small");
  if (n == 0) return BR_OK;
  // concat order: item_first -> [item, user] (W1 rows [0, dim) = item half), else [user, item]
  const int w_row0 = (user_side != 0) == (item_first != 0) ? dim : 0;
  const unsigned blocks = (unsigned)ceil_div(n * cols, 256);
  if (id_type == BR_IDS_I64)
    catalog_project_kernel<int64_t><<<blocks, 256, 0, (hipStream_t)stream>>>(table, ld, rows, (const int64_t*)ids, n, dim, W1, n1, w_row0,
                                                                              b1, cols, out, ld_out, col_major, err_flag);
  else
    catalog_project_kernel<int32_t><<<blocks, 256, 0, (hipStream_t)stream>>>(table, ld, rows, (const int32_t*)ids, n, dim, W1, n1, w_row0,
                                                                              b1, cols, out, ld_out, col_major, err_flag);
  BR_CHECK_LAUNCH("brNeumfCatalogProject");
  return BR_OK;
}

extern "C" int64_t brNeumfCatalogTopKWorkspaceBytes(int64_t n_users, int64_t n_items, int k) {
  if (n_users < 0 || n_items < 1 || k < 1 || k > kRecMaxK) return -1;
  int64_t S, cps;
  catalog_plan(n_users, n_items, &S, &cps);
  return 2 * part_bytes(n_users, S, k);
}

extern "C" int brNeumfCatalogTopK(const float* pu, int64_t ld_u, const float* pit, int64_t ld_i, int64_t n_users, int64_t n_items, int dim,
                                  int n1, int n2, int n3, int act, const float* tower, const int64_t* excl_off, const int32_t* excl_idx, int k,
                                  float* out_scores, int32_t* out_index, float* dump_logits, float* dump_probs, void* ws, int64_t ws_bytes,
                                  brStream stream) {
  BR_CHECK_ARG(pu && pit && tower && out_scores && out_index && ws, "brNeumfCatalogTopK: null pointer");
  BR_CHECK_ARG(k >= 1 && k <= kRecMaxK, "brNeumfCatalogTopK: k = %d outside [1, %d]", k, kRecMaxK);
  if (const int rc = catalog_check_args("brNeumfCatalogTopK", ld_u, n_users, ld_i, n_items, dim, n1, n2, n3, act)) return rc;
  BR_CHECK_ARG((excl_off == nullptr) == (excl_idx == nullptr), "brNeumfCatalogTopK: exclusion needs both excl_off and excl_idx");
  int64_t S, cps;
  catalog_plan(n_users, n_items, &S, &cps);
  const int64_t pb = part_bytes(n_users, S, k);
  if (ws_bytes < 2 * pb) {
    br::set_error("brNeumfCatalogTopK: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)(2 * pb));
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  float* ps = (float*)ws;
  int32_t* pp = (int32_t*)((char*)ws + pb);
  const TowerLayout L = tower_layout(n1, n2, n3);
  const dim3 grid((unsigned)ceil_div(n_users, kRecWaves), (unsigned)S);
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = dispatch_tower("brNeumfCatalogTopK", n2, act, [&](auto w, auto ac) {
        catalog_topk_kernel<decltype(w)::value, decltype(ac)::value><<<grid, 256, 0, st>>>(
            pu, ld_u, pit, ld_i, n_users, n_items, dim, n1, n3, tower, L, excl_off, excl_idx, k, cps, S, ps, pp, dump_logits, dump_probs);
      }))
    return rc;
  BR_CHECK_LAUNCH("brNeumfCatalogTopK");
  catalog_merge_kernel<<<(unsigned)ceil_div(n_users, kRecWaves), 256, 0, st>>>(ps, pp, n_users, S, k, out_scores, out_index);
  BR_CHECK_LAUNCH("brNeumfCatalogTopK merge");
  return BR_OK;
}

extern "C" int brTopKRowsExclude(const float* scores, int64_t n_users, int64_t n_items, int k, const int64_t* excl_off,
                                 const int32_t* excl_idx, float* out_scores, int32_t* out_index, brStream stream) {
  BR_CHECK_ARG(scores && out_scores && out_index && n_users >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31) && k >= 1,
               "brTopKRowsExclude: bad args (k >= 1, 1 <= n_items < 2^31)");
  BR_CHECK_ARG((excl_off == nullptr) == (excl_idx == nullptr), "brTopKRowsExclude: exclusion needs both excl_off and excl_idx");
  if (n_users == 0) return BR_OK;
  topk_rows_exclude_kernel<<<(unsigned)n_users, 256, 0, (hipStream_t)stream>>>(scores, n_items, k, excl_off, excl_idx, out_scores, out_index);
  BR_CHECK_LAUNCH("brTopKRowsExclude");
  return BR_OK;
}
