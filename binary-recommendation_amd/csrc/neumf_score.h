// The one text of the NeuMF catalogue score outside recommend.hip: what the AUC (auc_neumf.hip) and the ranks (ranks_neumf.hip) share on
// the device - neumf_score, the scoring loop of catalog_topk_kernel<W, ACT> restated statement for statement, and the positives' kernel
// around it - and on the host: the operands, the dispatch over (tower width, activation) and the positives' launch.  A pair's
// probability depends on its user row, its item column and the folded tower only, so both files dump and count the same bits;
// recommend.hip keeps its own text because it is the measured kernel, held equal by a bit-equality test.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"
#include "dot_tile.h"
#include "neumf_tower.h"
#include "topk_list.h"

namespace br {
namespace {

// catalog_topk_kernel's scoring loop for the item column pcol (lane-private), restated: the head probability of (urow, pcol)
template <int W, int ACT>
__device__ __forceinline__ float neumf_score(const float* __restrict__ urow, const float* __restrict__ pcol, int64_t ld_i, int dim, int n1,
                                             int n3, const float* __restrict__ W2, const float* __restrict__ b2,
                                             const float* __restrict__ W3t, const float* __restrict__ b3, const float* __restrict__ w4,
                                             float w4mf, float b4) {
  float acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = b2[j];
  float xn = pcol[0];
#pragma unroll 1
  for (int i = 0; i < n1; ++i) {                             // the next feature's load is in flight while this one is consumed
    const float x = xn;
    xn = pcol[(int64_t)(i + 1 < n1 ? i + 1 : i) * ld_i];
    const float h = act_apply(urow[i] + x, ACT);
    const float* __restrict__ w = W2 + (int64_t)i * W;
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = fmaf(h, w[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = act_apply(acc[j], ACT);     // padded columns: W3' rows are zero there
  float z = b4;
  for (int m = 0; m < n3; ++m) {
    const float* __restrict__ w = W3t + (int64_t)m * W;
    float s = b3[m];
#pragma unroll
    for (int j = 0; j < W; ++j) s = fmaf(acc[j], w[j], s);
    z = fmaf(act_apply(s, ACT), w4[m], z);
  }
  float dot = 0.f;
  for (int d = 0; d < dim; ++d) dot = fmaf(urow[n1 + d], pcol[(int64_t)(n1 + d) * ld_i], dot);
  z = fmaf(w4mf, dot, z);
  return sigmoidf_acc(z);                                    // the engine's head probability (predict)
}

// one wave per user: raw[off[u] + j] = the probability of (u, the user's j-th entry), NaN for an entry outside [0, n_items).  A user
// whose entries lie past `cap` floats of raw is left alone (brAucSortPieces gives it pcnt -1)
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
  const float* __restrict__ W2 = tower + L.w2;
  const float* __restrict__ b2 = tower + L.b2;
  const float* __restrict__ W3t = tower + L.w3t;
  const float* __restrict__ b3 = tower + L.b3;
  const float* __restrict__ w4 = tower + L.w4;
  const float w4mf = tower[L.w4mf], b4 = tower[L.b4];

  for (int64_t j0 = 0; j0 < P; j0 += 64) {
    const int64_t j = j0 + lane;
    const int64_t p = j < P ? (int64_t)idx[o0 + j] : -1;
    const bool ok = p >= 0 && p < n_items;
    const int64_t pc = ok ? p : 0;                           // (a lane without an entry scores item 0: every load stays in bounds)
    const float prob = neumf_score<W, ACT>(urow, pit + pc, ld_i, dim, n1, n3, W2, b2, W3t, b3, w4, w4mf, b4);
    if (j < P) raw[o0 + j] = ok ? prob : __builtin_nanf("");
  }
}

struct Operands {
  const float* pu; int64_t ld_u; const float* pit; int64_t ld_i; int64_t U, I; int dim, n1, n3; const float* tower; TowerLayout L;
};

template <int W, int ACT>
void launch_pos(hipStream_t st, const Operands& a, const int64_t* off, const int32_t* idx, float* raw, int64_t cap) {
  neumf_auc_pos_kernel<W, ACT><<<(unsigned)ceil_div(a.U, kRecWaves), 256, 0, st>>>(a.pu, a.ld_u, a.pit, a.ld_i, a.U, a.I, a.dim, a.n1, a.n3,
                                                                                   a.tower, a.L, off, idx, raw, cap);
}

// f(integral_constant<W>, integral_constant<ACT>) at the instantiated tower width and activation; false: no kernel for n2
template <typename F>
bool dispatch_tower(int n2, int act, F&& f) {
  auto with_act = [&](auto w) {
    if (act == BR_ACT_SIGMOID) f(w, std::integral_constant<int, BR_ACT_SIGMOID>{});
    else if (act == BR_ACT_RELU) f(w, std::integral_constant<int, BR_ACT_RELU>{});
    else f(w, std::integral_constant<int, BR_ACT_LINEAR>{});
  };
#define BR_TOWER_W(WW) case WW: with_act(std::integral_constant<int, WW>{}); return true;
  switch (tower_width(n2)) {
    BR_TOWER_W(8) BR_TOWER_W(16) BR_TOWER_W(24) BR_TOWER_W(32) BR_TOWER_W(40) BR_TOWER_W(48) BR_TOWER_W(56)
    BR_TOWER_W(64) BR_TOWER_W(96) BR_TOWER_W(128)
  }
#undef BR_TOWER_W
  return false;
}

int positives(const char* name, const Operands& a, int n2, int act, const int64_t* off, const int32_t* idx, float* raw, int64_t cap,
              hipStream_t st) {
  if (!dispatch_tower(n2, act, [&](auto w, auto ac) { launch_pos<decltype(w)::value, decltype(ac)::value>(st, a, off, idx, raw, cap); })) {
    br::set_error("%s: no kernel for n2 = %d", name, n2);
    return BR_ERR_UNSUPPORTED;
  }
  BR_CHECK_LAUNCH(name);
  return BR_OK;
}

}  // namespace
}  // namespace br
