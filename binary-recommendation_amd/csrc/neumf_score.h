// The one text of the NeuMF catalogue kernels (recommend.hip: top-k, auc_neumf.hip: AUC, ranks_neumf.hip: ranks):
// the folded tower as the device sees it (TowerView), the score of one (user row, item column) pair (neumf_logit, neumf_score), a
// split's item range, the per-wave cursor over an ascending CSR row (WaveCursor) and, on the host, the operands and the dispatch over
// (tower width, activation).  A pair's probability depends on its user row, its item column and the folded tower only, and every
// kernel of the family forms it by calling neumf_logit: what one of them dumps or counts is what the others rank by.  Templates,
// structs and forceinline device functions only: including this header instantiates nothing.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"
#include "dot_tile.h"
#include "neumf_tower.h"
#include "topk_list.h"

namespace br {

// what every launch of the family takes: the projected users and items, the model's widths and activation, the folded tower
struct Operands {
  const float* pu; int64_t ld_u; const float* pit; int64_t ld_i; int64_t U, I; int dim, n1, n2, n3, act; const float* tower;
};

// one wave per user: raw[off[u] + j] = the probability of (u, the user's j-th entry), NaN for an entry outside [0, n_items).  A user
// whose entries lie past `cap` floats of raw is left alone (brAucSortPieces gives it pcnt -1).  `name`: the entry point, for the
// message (auc_neumf.hip has the kernel: it is compiled there only)
int neumf_positives(const char* name, const Operands& a, const int64_t* off, const int32_t* idx, float* raw, int64_t cap, hipStream_t st);

namespace {

struct TowerView {
  const float* __restrict__ W2; const float* __restrict__ b2; const float* __restrict__ W3t; const float* __restrict__ b3;
  const float* __restrict__ w4; float w4mf, b4;
};
__device__ __forceinline__ TowerView tower_view(const float* __restrict__ tower, const TowerLayout& L) {
  return {tower + L.w2, tower + L.b2, tower + L.w3t, tower + L.b3, tower + L.w4, tower[L.w4mf], tower[L.b4]};
}

// the head's logit of (urow = [Pu (b1 included) | user mf], the item column pcol (lane-private)); the weights are wave-uniform
template <int W, int ACT>
__device__ __forceinline__ float neumf_logit(const float* __restrict__ urow, const float* __restrict__ pcol, int64_t ld_i, int dim, int n1,
                                             int n3, const TowerView& t) {
  float acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = t.b2[j];
  float xn = pcol[0];
#pragma unroll 1
  for (int i = 0; i < n1; ++i) {                             // the next feature's load is in flight while this one is consumed
    const float x = xn;
    xn = pcol[(int64_t)(i + 1 < n1 ? i + 1 : i) * ld_i];
    const float h = act_apply(urow[i] + x, ACT);
    const float* __restrict__ w = t.W2 + (int64_t)i * W;
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = fmaf(h, w[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = act_apply(acc[j], ACT);     // padded columns: W3' rows are zero there
  float z = t.b4;
  for (int m = 0; m < n3; ++m) {
    const float* __restrict__ w = t.W3t + (int64_t)m * W;
    float s = t.b3[m];
#pragma unroll
    for (int j = 0; j < W; ++j) s = fmaf(acc[j], w[j], s);
    z = fmaf(act_apply(s, ACT), t.w4[m], z);
  }
  float dot = 0.f;
  for (int d = 0; d < dim; ++d) dot = fmaf(urow[n1 + d], pcol[(int64_t)(n1 + d) * ld_i], dot);
  return fmaf(t.w4mf, dot, z);
}

// the engine's head probability (predict)
template <int W, int ACT>
__device__ __forceinline__ float neumf_score(const float* __restrict__ urow, const float* __restrict__ pcol, int64_t ld_i, int dim, int n1,
                                             int n3, const TowerView& t) {
  return sigmoidf_acc(neumf_logit<W, ACT>(urow, pcol, ld_i, dim, n1, n3, t));
}

// the items [p0, p1) of split `split` (catalog_plan: chunks of 64 items)
struct ItemRange {
  int64_t p0, p1;
};
__device__ __forceinline__ ItemRange split_items(int64_t split, int64_t chunks_per_split, int64_t n_items) {
  const int64_t p0 = split * chunks_per_split * 64, p1 = p0 + chunks_per_split * 64;
  return {p0, p1 > n_items ? n_items : p1};
}

// a wave's cursor over one ascending CSR row as the item window advances: entries [cur, end) are still ahead.  Default: an empty row
struct WaveCursor {
  int64_t cur = 0, end = 0;
};
// the first entry of row u at or after p0
__device__ __forceinline__ WaveCursor wave_cursor_at(const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int64_t u, int64_t p0) {
  int64_t lo = off[u], hi = off[u + 1];
  WaveCursor c;
  c.end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)idx[mid] < p0) lo = mid + 1; else hi = mid;
  }
  c.cur = lo;
  return c;
}
// the row's entries inside [base, base + 64), 64 at a time (they are a prefix of the rest): this lane's share of the window mask
// (wave_or64 over the lanes gives the mask); the cursor moves past them
__device__ __forceinline__ uint64_t wave_cursor_window(WaveCursor& c, const int32_t* __restrict__ idx, int64_t base, int lane) {
  uint64_t m = 0;
  for (;;) {
    const int64_t q = c.cur + lane;
    const int64_t e = q < c.end ? (int64_t)idx[q] : INT64_MAX;
    const bool in = e < base + 64;
    if (in && e >= base) m |= 1ull << (e - base);
    const int n_in = __popcll(__ballot(in));
    c.cur += n_in;
    if (n_in < 64) break;
  }
  return m;
}

// f(integral_constant<W>, integral_constant<ACT>) at the instantiated tower width and activation; no kernel for n2: the error set in
// `name`'s name and returned
template <typename F>
int dispatch_tower(const char* name, int n2, int act, F&& f) {
  auto with_act = [&](auto w) {
    if (act == BR_ACT_SIGMOID) f(w, std::integral_constant<int, BR_ACT_SIGMOID>{});
    else if (act == BR_ACT_RELU) f(w, std::integral_constant<int, BR_ACT_RELU>{});
    else f(w, std::integral_constant<int, BR_ACT_LINEAR>{});
  };
#define BR_TOWER_W(WW) case WW: with_act(std::integral_constant<int, WW>{}); return BR_OK;
  switch (tower_width(n2)) {
    BR_TOWER_W(8) BR_TOWER_W(16) BR_TOWER_W(24) BR_TOWER_W(32) BR_TOWER_W(40) BR_TOWER_W(48) BR_TOWER_W(56)
    BR_TOWER_W(64) BR_TOWER_W(96) BR_TOWER_W(128)
  }
#undef BR_TOWER_W
  br::set_error("%s: no kernel for n2 = %d", name, n2);
  return BR_ERR_UNSUPPORTED;
}

}  // namespace
}  // namespace br
