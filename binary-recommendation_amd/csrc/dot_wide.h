// What the block kernels for wide rows (recommend_dot_wide.hip: top-k, auc_count.h dot_auc_wide_pass: AUC, ranks_dot.hip: ranks) share:
// the block shape, the choice between the whole-row and the block kernels and the choice of the instantiated width.  Every entry point
// must pick the same kernels and width for the same (dim, flags) (a positive's score in the AUC is the catalogue pass's bit for bit only
// then), so the choices live here.
#pragma once
#include <type_traits>

#include "common.h"
#include "dot_tile.h"

namespace br {
namespace {

constexpr int kWideKB = 32;               // k-steps per feature block: 128 features, the whole-row kernel's widest tile
constexpr int kWideUW = 16;               // users per wave: one row tile, 32 NB VGPRs of A fragments

// the block kernels for these rows?  (the positives, the catalogue pass and the owners' count must take the same ones)
bool dot_use_wide(int dim, int flags) { return dim > kDotMaxDim || (flags & BR_DOT_FORCE_WIDE); }

// f(std::integral_constant<int, NB>) for the instantiated width 128 NB >= dim: 256, 384 or 512 (dim <= 128, forced: 256, so the carry
// across blocks is exercised there too)
template <typename F>
void dispatch_nb(int dim, F&& f) {
  const int nb = (dim + 4 * kWideKB - 1) / (4 * kWideKB);
  if (nb <= 2) f(std::integral_constant<int, 2>{}); else if (nb == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace
}  // namespace br
