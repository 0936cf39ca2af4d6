// What the NeuMF catalogue kernels (recommend.hip: top-k, auc_neumf.hip: AUC, ranks_neumf.hip: ranks) share on the host: the folded
// tower's layout, the padded width their kernels are instantiated at, the limits and the split plan.  What they share on the device
// (the scoring loop, the tower view, the wave cursor) and the dispatch over the instantiations: neumf_score.h.
#pragma once
#include "common.h"
#include "dot_tile.h"
#include "topk_list.h"

namespace br {
namespace {

// padded width of the second layer (the per-lane accumulator count): one instantiation per width
int tower_width(int n2) {
  if (n2 <= 64) return (n2 + 7) / 8 * 8;
  return n2 <= 96 ? 96 : 128;
}

// folded tower layout (floats): W2' [n1][W] | b2' [W] | W3'^T [n3][W] | b3' [n3] | w4 of the tower outputs [n3] | w4 of the GMF dot | b4
struct TowerLayout {
  int64_t w2, b2, w3t, b3, w4, w4mf, b4, total;
};
TowerLayout tower_layout(int n1, int n2, int n3) {
  const int W = tower_width(n2);
  TowerLayout t;
  t.w2 = 0;
  t.b2 = (int64_t)n1 * W;
  t.w3t = t.b2 + W;
  t.b3 = t.w3t + (int64_t)n3 * W;
  t.w4 = t.b3 + n3;
  t.w4mf = t.w4 + n3;
  t.b4 = t.w4mf + 1;
  t.total = t.b4 + 1;
  return t;
}

void catalog_plan(int64_t n_users, int64_t n_items, int64_t* splits, int64_t* chunks_per_split) {
  split_plan(ceil_div(n_items, 64), n_users, kRecWaves, splits, chunks_per_split);   // (dot_tile.h: the one plan of the catalogue kernels)
}

bool tower_shape_ok(int n1, int n2, int n3) { return n1 >= 1 && n1 <= 128 && n2 >= 1 && n2 <= 128 && n3 >= 1 && n3 <= 32; }

bool catalog_sizes_ok(int64_t n_users, int64_t n_items) { return n_users >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31); }

// what every entry point over (projected users, projected items, folded tower) checks on those operands; `name`: the entry, for the message
int catalog_check_args(const char* name, int64_t ld_u, int64_t n_users, int64_t ld_i, int64_t n_items, int dim, int n1, int n2, int n3, int act) {
  BR_CHECK_ARG(tower_shape_ok(n1, n2, n3), "%s: tower widths n1, n2 <= 128, n3 <= 32 (got %d, %d, %d)", name, n1, n2, n3);
  BR_CHECK_ARG(dim >= 1 && 2 * dim <= 256, "%s: 1 <= dim, 2*dim <= 256 (got %d)", name, dim);
  BR_CHECK_ARG(catalog_sizes_ok(n_users, n_items), "%s: bad sizes (1 <= n_items < 2^31)", name);
  BR_CHECK_ARG(ld_u >= n1 + dim && ld_i >= n_items, "%s: ld_u >= n1 + dim and ld_i >= n_items", name);
  BR_CHECK_ARG(act == BR_ACT_LINEAR || act == BR_ACT_SIGMOID || act == BR_ACT_RELU, "%s: bad act", name);
  return BR_OK;
}

}  // namespace
}  // namespace br
