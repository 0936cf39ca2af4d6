// What the dot-product catalogue AUC entry points (auc_dot.hip, either width) and the ranks (ranks_dot.hip) launch around their catalogue pass: the positives'
// kernel (templated on the instantiated width 4 KB; one accumulator chain over all of it, so a positive's score is the catalogue
// pass's whatever way that pass streams the features) and the finalize.
#pragma once
#include <math.h>

#include "common.h"
#include "dot_tile.h"

namespace br {
namespace {

// one wave per user: score its truth entries, sort them ascending (NaN dropped) into sorted[off[u] ...], P' into pcnt[u] (-1: the
// user's entries lie past the workspace's capacity `cap`)
template <int KB>
__global__ __launch_bounds__(256) void auc_pos_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                       int64_t ld_c, int64_t n_items, int dim, const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ idx, float* raw, float* __restrict__ sorted,
                                                       int32_t* __restrict__ pcnt, int64_t cap) {
  __shared__ float chunk[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= n_users) return;
  const int64_t o0 = off[u], o1 = off[u + 1], P = o1 - o0;
  if (P <= 0 || o0 < 0 || o1 > cap) {
    if (lane == 0) pcnt[u] = P <= 0 ? 0 : -1;
    return;
  }
  // A: the user's row in all 16 rows (lane l: feature 4 kb + (l >> 4)), as the catalogue pass holds its users
  float qa[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int f = 4 * kb + (lane >> 4);
    qa[kb] = f < dim ? Q[u * ld_q + f] : 0.f;
  }
  for (int64_t c0 = 0; c0 < P; c0 += 16) {
    const int64_t j = c0 + (lane & 15);
    const int64_t p = j < P ? (int64_t)idx[o0 + j] : -1;
    const bool ok = p >= 0 && p < n_items;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int f = 4 * kb + (lane >> 4);
      const float b = ok && f < dim ? C[p * ld_c + f] : 0.f;      // B[k][j] = C[positive j][feature 4 kb + k]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[kb], b, acc, 0, 0, 0);
    }
    // D: lane l < 16, register 0 = row 0, column l = score(u, positive c0 + l); an entry outside [0, n_items) scores NaN (no credit)
    if (lane < 16 && j < P) raw[o0 + j] = ok ? acc[0] : __builtin_nanf("");
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");           // this wave's raw stores before its loads below
  __builtin_amdgcn_wave_barrier();

  // counting rank: rank(i) = #{j: s_j < s_i} + #{j < i: s_j == s_i}; NaN compares false, so NaN entries take no rank
  float* const ch = chunk[wave];
  int64_t nn = 0;
  for (int64_t i0 = 0; i0 < P; i0 += 64) {
    const int64_t i = i0 + lane;
    const float si = i < P ? raw[o0 + i] : __builtin_nanf("");
    int64_t rank = 0;
    for (int64_t j0 = 0; j0 < P; j0 += 64) {
      wave_lds_order();
      ch[lane] = j0 + lane < P ? raw[o0 + j0 + lane] : __builtin_nanf("");
      wave_lds_order();
      const int m = P - j0 < 64 ? (int)(P - j0) : 64;
      uint32_t r = 0;
      for (int t = 0; t < m; ++t) {
        const float v = ch[t];
        r += (v < si) | ((v == si) & (j0 + t < i));
      }
      rank += r;
    }
    if (si == si) sorted[o0 + rank] = si;
    nn += __popcll(__ballot(si == si));
  }
  if (lane == 0) pcnt[u] = (int32_t)nn;
}
__global__ __launch_bounds__(256) void auc_finalize_kernel(const uint64_t* __restrict__ part, int64_t n_splits, const int64_t* __restrict__ off,
                                                            const int32_t* __restrict__ pcnt, int64_t n_users, int64_t n_items,
                                                            float* __restrict__ auc) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  const int64_t P = off[u + 1] - off[u], N = n_items - P;
  if (P <= 0 || N <= 0 || pcnt[u] < 0) {
    auc[u] = __builtin_nanf("");
    return;
  }
  uint64_t w2 = 0;
  for (int64_t s = 0; s < n_splits; ++s) w2 += part[u * n_splits + s];
  auc[u] = (float)((double)w2 * 0.5 / ((double)P * (double)N));
}

}  // namespace
}  // namespace br
