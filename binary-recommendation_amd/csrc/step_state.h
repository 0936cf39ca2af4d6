// The step-state advance as a workgroup: a launch of its own (step_state.hip), an extra workgroup of the chunk-rank launch
// (row_index.hip) or of the segment-partials launch (sparse_opt.hip: the later steps of a multi-step group have no rank launch).
#pragma once
#include "common.h"

#include <math.h>

namespace br {

// top of a training step: step += 1, alpha_t (thread 0), and the step's double scratch zeroed (all threads) -
// one launch instead of a memset node plus a kernel
__device__ __forceinline__ void step_state_advance_block(const StepAdvance& a) {
  for (int64_t i = threadIdx.x; i < a.n_zero; i += blockDim.x) a.zero[i] = 0.0;
  if (threadIdx.x == 0) {
    StepStateDev* st = a.st;
    const uint32_t t = st->step + 1;
    const double p1 = st->pow_b1 * a.b1, p2 = st->pow_b2 * a.b2;
    const float al = (float)(a.lr * sqrt(1.0 - p2) / (1.0 - p1));
    st->step = t;
    st->pow_b1 = p1;
    st->pow_b2 = p2;
    st->alpha_t = al;
    st->alpha_hist[t & (BR_ALPHA_RING - 1)] = al;
    if ((t & (BR_ALPHA_RING - 1)) < (uint32_t)BR_RING_MIRROR) st->alpha_hist[BR_ALPHA_RING + (t & (BR_ALPHA_RING - 1))] = al;   // the mirror behind the ring's end
  }
}

// the double scratch of later step `which` of a multi-step group, zeroed by one workgroup (its last reader - the previous group's
// finalize of that step - is behind the launch on the stream, its next writer - this group's fwd L1 of that step - in front)
__device__ __forceinline__ void step_state_zero_more(const StepAdvance& a, int which) {
  double* __restrict__ z = a.zero_more[which];
  for (int64_t i = threadIdx.x; i < a.n_zero; i += blockDim.x) z[i] = 0.0;
}

}  // namespace br
