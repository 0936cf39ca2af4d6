// Full-catalogue AUC of dot-product models on row-sharded engines, counted where the item rows live (include/binrec.h "Catalogue AUC on
// row-sharded engines"; parallel.py auc_at_owners).  brDotCatalogAuc[Wide]'s three launches (auc_dot.hip) cut into four phases, so that
// W owners, each holding a share of the candidates, together compute what one launch over all candidates computes, bit for bit:
//
//   - brDotAucOwnerPositives: auc_pos_kernel's scoring half (auc_pos.h) over the owner's candidates: the same v_mfma_f32_16x16x4_f32,
//     the same padded width and one chain from 0, so a positive's score is the one the catalogue pass of ANY owner layout sees;
//   - brAucSortPieces: auc_pos_kernel's sorting half over the pieces of all owners, read in place from an all-gather's receive buffer:
//     per user one ascending list, NaN dropped, the count P' beside.  A multiset is sorted, so the order of the pieces cannot matter;
//   - brDotAucOwnerCount: the catalogue pass (auc_count.h) over the owner's candidates: its own positives are skipped, every other
//     score is counted against the user's FULL list.  The item splits are summed in integers here: one uint64 2W per user;
//   - brAucFinalizeLists: auc_finalize_kernel over the W owners' partial 2W, read in place from an all-to-all's receive buffer:
//     integers add exactly, then the one division in double.
#include <math.h>

#include "auc_count.h"
#include "common.h"
#include "dot_tile.h"
#include "dot_wide.h"

namespace br {
namespace {

constexpr int kMaxLists = 4096;           // pieces per user of brAucSortPieces, lists per user of brAucFinalizeLists (brTopKListsMerge's limit)

// one wave per user: raw[off[u] + j] = score(u, the user's j-th entry), NaN for an entry outside [0, n_items); auc_pos_kernel's first half
template <int KB>
__global__ __launch_bounds__(256) void auc_pos_scores_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                              int64_t ld_c, int64_t n_items, int dim, const int64_t* __restrict__ off,
                                                              const int32_t* __restrict__ idx, float* __restrict__ raw) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= n_users) return;
  const int64_t o0 = off[u], o1 = off[u + 1], P = o1 - o0;
  if (P <= 0 || o0 < 0) return;
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
    // D: lane l < 16, register 0 = row 0, column l = score(u, positive c0 + l)
    if (lane < 16 && j < P) raw[o0 + j] = ok ? acc[0] : __builtin_nanf("");
  }
}

// one wave per user: the user's pieces raw[piece_off[w][u] ... piece_off[w][u + 1]), w < n_pieces, side by side into
// tmp[list_off[u] ...], then auc_pos_kernel's counting rank into sorted[list_off[u] ...], P' into pcnt[u].  -1: the list lies past
// `cap`, or the pieces do not fit the list or lie outside raw's n_raw entries (nothing of the user is read or written then)
__global__ __launch_bounds__(256) void auc_sort_pieces_kernel(const float* __restrict__ raw, int64_t n_raw, const int64_t* __restrict__ piece_off,
                                                               int n_pieces, int64_t n_users, const int64_t* __restrict__ list_off, float* tmp,
                                                               float* __restrict__ sorted, int32_t* __restrict__ pcnt, int64_t cap) {
  __shared__ float chunk[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t u = (int64_t)blockIdx.x * 4 + wave;
  if (u >= n_users) return;
  const int64_t o0 = list_off[u], o1 = list_off[u + 1], room = o1 - o0;
  if (room <= 0 || o0 < 0 || o1 > cap) {
    if (lane == 0) pcnt[u] = room <= 0 ? 0 : -1;
    return;
  }
  int64_t P = 0;                                                    // entries of all pieces (wave-uniform)
  for (int w = 0; w < n_pieces; ++w) {
    const int64_t a = piece_off[(int64_t)w * (n_users + 1) + u], b = piece_off[(int64_t)w * (n_users + 1) + u + 1];
    if (a < 0 || b < a || b > n_raw || P + (b - a) > room) {
      if (lane == 0) pcnt[u] = -1;
      return;
    }
    for (int64_t e = lane; e < b - a; e += 64) tmp[o0 + P + e] = raw[a + e];
    P += b - a;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");           // this wave's tmp stores before its loads below
  __builtin_amdgcn_wave_barrier();

  // counting rank: rank(i) = #{j: s_j < s_i} + #{j < i: s_j == s_i}; NaN compares false, so NaN entries take no rank
  float* const ch = chunk[wave];
  int64_t nn = 0;
  for (int64_t i0 = 0; i0 < P; i0 += 64) {
    const int64_t i = i0 + lane;
    const float si = i < P ? tmp[o0 + i] : __builtin_nanf("");
    int64_t rank = 0;
    for (int64_t j0 = 0; j0 < P; j0 += 64) {
      wave_lds_order();
      ch[lane] = j0 + lane < P ? tmp[o0 + j0 + lane] : __builtin_nanf("");
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

template <int KB>
__global__ __launch_bounds__(256) void dot_auc_owner_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users, const float* __restrict__ C,
                                                             int64_t ld_c, int64_t n_items, int dim, int vec, const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ idx, const int64_t* __restrict__ loff,
                                                             const float* __restrict__ sorted, const int32_t* __restrict__ pcnt, int64_t cap,
                                                             int64_t steps_per_split, int64_t n_splits, uint64_t* __restrict__ part,
                                                             float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kAucNT * (4 * KB + 4)];
  __shared__ float pos_s[4 * kAucLdsCap];
  __shared__ uint64_t xm_s[4 * kAucUW];
  dot_auc_pass<KB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, loff, sorted, pcnt, cap, steps_per_split, n_splits, part, dump, tile,
                   pos_s, xm_s);
}

template <int NB>
__global__ __launch_bounds__(256) void dot_auc_owner_wide_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users,
                                                                  const float* __restrict__ C, int64_t ld_c, int64_t n_items, int dim, int vec,
                                                                  const int64_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                                  const int64_t* __restrict__ loff, const float* __restrict__ sorted,
                                                                  const int32_t* __restrict__ pcnt, int64_t cap, int64_t steps_per_split,
                                                                  int64_t n_splits, uint64_t* __restrict__ part, float* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) float tile[kAucNT * (4 * kWideKB + 4)];
  __shared__ float pos_s[4 * kAucLdsCap];
  __shared__ uint64_t xm_s[4 * kWideUW];
  dot_auc_wide_pass<NB>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, off, idx, loff, sorted, pcnt, cap, steps_per_split, n_splits, part, dump,
                        tile, pos_s, xm_s);
}

// out[u] = the user's 2W over this owner's candidates: its item splits summed in integers
__global__ __launch_bounds__(256) void auc_sum_splits_kernel(const uint64_t* __restrict__ part, int64_t n_splits, int64_t n_users,
                                                              uint64_t* __restrict__ out) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  uint64_t w2 = 0;
  for (int64_t s = 0; s < n_splits; ++s) w2 += part[u * n_splits + s];
  out[u] = w2;
}

// auc_finalize_kernel (auc_pos.h) over n_lists partial 2W per user, list w of user u at part[w * list_stride + u]
__global__ __launch_bounds__(256) void auc_finalize_lists_kernel(const uint64_t* __restrict__ part, int64_t list_stride, int n_lists,
                                                                  const int64_t* __restrict__ off, const int32_t* __restrict__ pcnt,
                                                                  int64_t n_users, int64_t n_items, float* __restrict__ auc) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  const int64_t P = off[u + 1] - off[u], N = n_items - P;
  if (P <= 0 || N <= 0 || pcnt[u] < 0) {
    auc[u] = __builtin_nanf("");
    return;
  }
  uint64_t w2 = 0;
  for (int w = 0; w < n_lists; ++w) w2 += part[(int64_t)w * list_stride + u];
  auc[u] = (float)((double)w2 * 0.5 / ((double)P * (double)N));
}

int64_t owner_part_bytes(bool wide, int64_t n_users, int64_t n_items) {
  int64_t S, sps;
  auc_plan(wide, n_users, n_items, &S, &sps);
  return align256(n_users * S * 8);
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int brDotAucOwnerPositives(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                                      const int64_t* pos_off, const int32_t* pos_idx, float* raw, int flags, brStream stream) {
  BR_CHECK_ARG(Q && C && pos_off && pos_idx && raw, "brDotAucOwnerPositives: null pointer");
  if (const int rc = dot_check_args("brDotAucOwnerPositives", ld_q, n_users, ld_c, n_items, dim, kDotWideMaxDim)) return rc;
  BR_CHECK_ARG((flags & ~BR_DOT_FORCE_WIDE) == 0, "brDotAucOwnerPositives: unknown flags 0x%x", flags);
  if (n_users == 0) return BR_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)ceil_div(n_users, 4);
  if (dot_use_wide(dim, flags))
    dispatch_nb(dim, [&](auto nb) {
      auc_pos_scores_kernel<decltype(nb)::value * kWideKB><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, pos_off, pos_idx, raw);
    });
  else
    dispatch_kb(dim, [&](auto kb) {
      auc_pos_scores_kernel<decltype(kb)::value><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, pos_off, pos_idx, raw);
    });
  BR_CHECK_LAUNCH("brDotAucOwnerPositives");
  return BR_OK;
}

extern "C" int64_t brAucSortPiecesWorkspaceBytes(int n_pieces, int64_t cap) {
  if (n_pieces < 1 || n_pieces > kMaxLists || cap < 0) return -1;
  return align256(4 * ((cap > INT32_MAX ? INT32_MAX : cap) + 1));
}

extern "C" int brAucSortPieces(const float* raw, int64_t n_raw, const int64_t* piece_off, int n_pieces, int64_t n_users,
                               const int64_t* list_off, float* sorted, int64_t cap, int32_t* pcnt, void* ws, int64_t ws_bytes,
                               brStream stream) {
  BR_CHECK_ARG(raw && piece_off && list_off && sorted && pcnt && ws, "brAucSortPieces: null pointer");
  BR_CHECK_ARG(n_pieces >= 1 && n_pieces <= kMaxLists, "brAucSortPieces: n_pieces = %d outside [1, %d]", n_pieces, kMaxLists);
  BR_CHECK_ARG(n_users >= 0 && n_raw >= 0 && cap >= 0, "brAucSortPieces: bad sizes (n_users, n_raw, cap >= 0)");
  const int64_t least = brAucSortPiecesWorkspaceBytes(n_pieces, cap);
  if (ws_bytes < least) {
    br::set_error("brAucSortPieces: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)least);
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  if (cap > INT32_MAX) cap = INT32_MAX;                              // (the count pass keeps list positions in 32 bits)
  auc_sort_pieces_kernel<<<(unsigned)ceil_div(n_users, 4), 256, 0, (hipStream_t)stream>>>(raw, n_raw, piece_off, n_pieces, n_users, list_off,
                                                                                           (float*)ws, sorted, pcnt, cap);
  BR_CHECK_LAUNCH("brAucSortPieces");
  return BR_OK;
}

// the larger of the two plans' needs where both can run (dim <= 128: BR_DOT_FORCE_WIDE is not known here)
extern "C" int64_t brDotAucOwnerCountWorkspaceBytes(int64_t n_users, int64_t n_items, int dim) {
  if (n_users < 0 || n_items < 1 || n_items >= ((int64_t)1 << 31) || dim < 1 || dim > kDotWideMaxDim) return -1;
  const int64_t wide = owner_part_bytes(true, n_users, n_items);
  if (dim > kDotMaxDim) return wide;
  const int64_t narrow = owner_part_bytes(false, n_users, n_items);
  return narrow > wide ? narrow : wide;
}

extern "C" int brDotAucOwnerCount(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                                  const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off, const float* sorted,
                                  const int32_t* pcnt, int64_t cap, uint64_t* out_w2, float* dump_scores, int flags, void* ws,
                                  int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && skip_off && skip_idx && list_off && sorted && pcnt && out_w2 && ws, "brDotAucOwnerCount: null pointer");
  if (const int rc = dot_check_args("brDotAucOwnerCount", ld_q, n_users, ld_c, n_items, dim, kDotWideMaxDim)) return rc;
  BR_CHECK_ARG((flags & ~BR_DOT_FORCE_WIDE) == 0, "brDotAucOwnerCount: unknown flags 0x%x", flags);
  BR_CHECK_ARG(cap >= 0, "brDotAucOwnerCount: cap = %lld < 0", (long long)cap);
  const int64_t least = brDotAucOwnerCountWorkspaceBytes(n_users, n_items, dim);
  if (ws_bytes < least) {
    br::set_error("brDotAucOwnerCount: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)least);
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  const bool wide = dot_use_wide(dim, flags);
  int64_t S, sps;
  auc_plan(wide, n_users, n_items, &S, &sps);
  if (cap > INT32_MAX) cap = INT32_MAX;
  uint64_t* part = (uint64_t*)ws;
  const int vec = rows_vec4(C, ld_c, dim);
  hipStream_t st = (hipStream_t)stream;
  if (wide) {
    const dim3 grid((unsigned)ceil_div(n_users, 4 * kWideUW), (unsigned)S);
    dispatch_nb(dim, [&](auto nb) {
      dot_auc_owner_wide_kernel<decltype(nb)::value><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, skip_off, skip_idx,
                                                                           list_off, sorted, pcnt, cap, sps, S, part, dump_scores);
    });
  } else {
    const dim3 grid((unsigned)ceil_div(n_users, 4 * kAucUW), (unsigned)S);
    dispatch_kb(dim, [&](auto kb) {
      dot_auc_owner_kernel<decltype(kb)::value><<<grid, 256, 0, st>>>(Q, ld_q, n_users, C, ld_c, n_items, dim, vec, skip_off, skip_idx, list_off,
                                                                      sorted, pcnt, cap, sps, S, part, dump_scores);
    });
  }
  BR_CHECK_LAUNCH("brDotAucOwnerCount");
  auc_sum_splits_kernel<<<(unsigned)ceil_div(n_users, 256), 256, 0, st>>>(part, S, n_users, out_w2);
  BR_CHECK_LAUNCH("brDotAucOwnerCount sum");
  return BR_OK;
}

extern "C" int brAucFinalizeLists(const uint64_t* part, int64_t list_stride, int n_lists, const int64_t* truth_off, const int32_t* pcnt,
                                  int64_t n_users, int64_t n_items, float* out_auc, brStream stream) {
  BR_CHECK_ARG(part && truth_off && pcnt && out_auc, "brAucFinalizeLists: null pointer");
  BR_CHECK_ARG(n_lists >= 1 && n_lists <= kMaxLists, "brAucFinalizeLists: n_lists = %d outside [1, %d]", n_lists, kMaxLists);
  BR_CHECK_ARG(n_users >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31) && list_stride >= n_users,
               "brAucFinalizeLists: bad sizes (1 <= n_items < 2^31, list_stride >= n_users)");
  if (n_users == 0) return BR_OK;
  auc_finalize_lists_kernel<<<(unsigned)ceil_div(n_users, 256), 256, 0, (hipStream_t)stream>>>(part, list_stride, n_lists, truth_off, pcnt,
                                                                                                n_users, n_items, out_auc);
  BR_CHECK_LAUNCH("brAucFinalizeLists");
  return BR_OK;
}
