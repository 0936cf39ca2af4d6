// What the dot-product catalogue kernels (recommend_dot.hip / recommend_dot_wide.hip: top-k, auc_count.h: AUC, ranks_dot.hip: ranks)
// share outside their tile loops: the split plan (recommend.hip's too), wave_lds_order, the CSR row cursor (RowCursor: the AUC and the
// rank passes) and what the entry points check and choose alike.  The tile loop itself is still written out once per family and width
// (top-k, AUC pass, rank pass) and kept the same by hand: see DESIGN.md 4e "One copy of the tile loop".
#pragma once
#include <type_traits>

#include "common.h"

namespace br {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }   // workspace sections start on 256 bytes

constexpr int64_t kSplitTargetWgs = 2048;   // splits are added until the grid has about this many workgroups

// `units` steps of the item axis, users_per_wg users per workgroup -> the number of splits (grid.y, <= 65535) and the steps each takes
void split_plan(int64_t units, int64_t n_users, int64_t users_per_wg, int64_t* splits, int64_t* units_per_split) {
  int64_t s = ceil_div(kSplitTargetWgs, ceil_div(n_users > 0 ? n_users : 1, users_per_wg));
  if (s > units) s = units;
  if (s > 65535) s = 65535;
  if (s < 1) s = 1;
  const int64_t ups = ceil_div(units, s);
  *units_per_split = ups;
  *splits = ceil_div(units, ups);
}

// compiler barrier between one lane's LDS stores and another lane's loads of the same words (a wave's LDS accesses execute in order)
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the cursor of one CSR row over the item axis: the first entry at or after p0 (cur), the row's end and that entry's position
struct RowCursor {
  int64_t cur = 0, end = 0, nxt = INT64_MAX;
};
__device__ __forceinline__ RowCursor cursor_at(const int64_t* off, const int32_t* __restrict__ idx, int64_t u, int64_t p0) {
  RowCursor c;
  int64_t lo = off[u], hi = off[u + 1];
  c.end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)idx[mid] < p0) lo = mid + 1; else hi = mid;
  }
  c.cur = lo;
  if (c.cur < c.end) c.nxt = idx[c.cur];
  return c;
}
// the row's entries inside the window [base, base + NT) as a mask; the cursor moves past them
__device__ __forceinline__ uint64_t cursor_window(RowCursor& c, const int32_t* __restrict__ idx, int64_t base, int NT) {
  uint64_t m = 0;
  while (c.nxt < base + NT) {
    if (c.nxt >= base) m |= 1ull << (c.nxt - base);
    ++c.cur;
    c.nxt = c.cur < c.end ? (int64_t)idx[c.cur] : INT64_MAX;
  }
  return m;
}

// float4 item loads: every row of C 16-B aligned and whole chunks only
int rows_vec4(const float* C, int64_t ld_c, int dim) { return dim % 4 == 0 && ld_c % 4 == 0 && ((uintptr_t)C & 15) == 0; }

// f(std::integral_constant<int, KB>) for the instantiated feature width 4 KB >= dim
template <typename F>
void dispatch_kb(int dim, F&& f) {
  const int kb = (dim + 3) / 4;
  if (kb <= 4) f(std::integral_constant<int, 4>{}); else if (kb <= 8) f(std::integral_constant<int, 8>{});
  else if (kb <= 16) f(std::integral_constant<int, 16>{}); else if (kb <= 24) f(std::integral_constant<int, 24>{});
  else f(std::integral_constant<int, 32>{});
}

constexpr int kDotMaxDim = 128;            // widest rows of the whole-row kernels (recommend_dot.hip, auc_count.h dot_auc_pass)
constexpr int kDotWideMaxDim = 512;        // ... of the block kernels (recommend_dot_wide.hip, auc_count.h dot_auc_wide_pass)

// the checks the entry points make on (Q, C); `name`: the entry point, for the message
int dot_check_args(const char* name, int64_t ld_q, int64_t n_users, int64_t ld_c, int64_t n_items, int dim, int max_dim = kDotMaxDim) {
  BR_CHECK_ARG(dim >= 1 && dim <= max_dim, "%s: dim = %d outside [1, %d]", name, dim, max_dim);
  BR_CHECK_ARG(n_users >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31), "%s: bad sizes (1 <= n_items < 2^31)", name);
  BR_CHECK_ARG(ld_q >= dim && ld_c >= dim, "%s: ld_q, ld_c >= dim (got %lld, %lld, dim %d)", name, (long long)ld_q, (long long)ld_c, dim);
  return BR_OK;
}

}  // namespace
}  // namespace br
