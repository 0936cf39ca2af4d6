// What the block kernels for wide rows (recommend_dot_wide.hip: top-k, auc_dot_wide.hip: AUC) share: the block shape and the choice
// of the instantiated width.  Both entry points must pick the same width for the same dim (a positive's score in the AUC is the
// catalogue pass's bit for bit only then), so the choice lives here.
#pragma once
#include <type_traits>

#include "common.h"

namespace br {
namespace {

constexpr int kWideKB = 32;               // k-steps per feature block: 128 features, the whole-row kernel's widest tile
constexpr int kWideUW = 16;               // users per wave: one row tile, 32 NB VGPRs of A fragments

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
