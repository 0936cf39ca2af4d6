// The device-resident step state (step counter, alpha_t and its ring, the replay form's constants: common.h StepStateDev) and the
// staging copy of a batch into the step's fixed buffers.
#include "common.h"
#include "rows.h"
#include "step_state.h"

#include <vector>
#include <math.h>
#include <stddef.h>

namespace br {

__global__ __launch_bounds__(256) void step_state_advance_kernel(StepAdvance a) { step_state_advance_block(a); }

template <typename IdT>
__global__ __launch_bounds__(256) void stage_batch_kernel(IdT* __restrict__ du, IdT* __restrict__ di, float* __restrict__ dy,
                                                           const IdT* __restrict__ su, const IdT* __restrict__ si,
                                                           const float* __restrict__ sy, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const IdT u = su[i], it = si[i];
  const float y = sy ? sy[i] : 0.f;
  du[i] = u; di[i] = it;
  if (dy) dy[i] = y;
}

}  // namespace br

using namespace br;

extern "C" int64_t brStepStateBytes(void) { return (int64_t)sizeof(StepStateDev); }

extern "C" int brStepStateAdvance(void* step_state, double lr, double beta1, double beta2, double* zero, int64_t n_zero, brStream stream) {
  BR_CHECK_ARG(step_state != nullptr && n_zero >= 0 && (zero || n_zero == 0), "brStepStateAdvance: bad args");
  StepAdvance a;
  a.st = (StepStateDev*)step_state; a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.zero = zero; a.n_zero = n_zero;
  step_state_advance_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a);
  BR_CHECK_LAUNCH("brStepStateAdvance");
  return BR_OK;
}

extern "C" int brStepStateInit(void* step_state, double beta1, double beta2, double eps, int replay_mode, brStream stream) {
  BR_CHECK_ARG(step_state != nullptr, "brStepStateInit: null state");
  BR_CHECK_ARG(replay_mode == BR_REPLAY_EXACT || replay_mode == BR_REPLAY_FAST, "brStepStateInit: bad replay_mode %d", replay_mode);
  BR_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 > 0.0 && beta2 < 1.0 && eps >= 0.0, "brStepStateInit: beta1 in [0,1), beta2 in (0,1), eps >= 0");
  constexpr size_t off = offsetof(StepStateDev, fast);
  static_assert(offsetof(StepStateDev, pow2) + sizeof(float) * BR_ALPHA_RING == sizeof(StepStateDev), "StepStateDev tail layout");
  std::vector<StepStateDev> img(1);                            // a host image of the state; only its tail [fast, end) is copied
  StepStateDev* h = img.data();
  // the kernels multiply by the fp32 roundings of beta1 / beta2 (AdamHp): the closed forms below are powers of THOSE numbers - over a lag of
  // 1000 steps pow(0.999, k) and pow((float)0.999, k) are 1.3e-5 apart
  beta1 = (double)(float)beta1; beta2 = (double)(float)beta2;
  const double c = sqrt(beta2), rho = beta1 / c;
  h->fast = replay_mode == BR_REPLAY_FAST ? 1u : 0u;
  // theta is replayed over the first `trunc` steps of a lag: the steps behind it move theta by at most 7 rho^trunc / (1 - rho) of the first
  // step's update (alpha_j varies by less than 7x over any lag, m decays by beta1 and 1 / d grows by at most 1 / c per step); below 2^-23
  // of it they are under one ulp.  A multiple of 8 (the replay takes eight alphas per scalar load); rho >= 1: never truncated.
  uint32_t trunc = BR_ALPHA_RING;
  if (rho < 1.0) {
    const double need = log(ldexp(1.0, -23) * (1.0 - rho) / 7.0) / log(rho);
    if (need < (double)BR_ALPHA_RING) trunc = (uint32_t)((((int64_t)ceil(need < 1.0 ? 1.0 : need)) + 7) / 8 * 8);
  }
  h->trunc = trunc;
  h->sqrt_b2 = (float)c;
  h->eps_c = (float)(eps * (1.0 - c));
  for (int k = 0; k < BR_ALPHA_RING; ++k) { h->pow1[k] = (float)pow(beta1, (double)k); h->pow2[k] = (float)pow(beta2, (double)k); }
  const hipError_t ce = hipMemcpyAsync((char*)step_state + off, (const char*)h + off, sizeof(StepStateDev) - off, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (ce != hipSuccess) {
    set_error("brStepStateInit: copy failed: %s", hipGetErrorString(ce));
    return BR_ERR_HIP;
  }
  (void)hipStreamSynchronize((hipStream_t)stream);
  return BR_OK;
}

extern "C" int brStepStateSet(void* step_state, uint32_t step, double lr, double beta1, double beta2, brStream stream) {
  BR_CHECK_ARG(step_state != nullptr, "brStepStateSet: null state");
  struct { uint32_t step; float alpha_t; double p1, p2; } h;
  static_assert(sizeof(h) == offsetof(StepStateDev, alpha_hist), "StepStateDev head layout");
  h.step = step;
  h.p1 = pow(beta1, (double)step);
  h.p2 = pow(beta2, (double)step);
  const double tt = step > 0 ? (double)step : 1.0;
  h.alpha_t = (float)(lr * sqrt(1.0 - pow(beta2, tt)) / (1.0 - pow(beta1, tt)));
  // pageable source: hipMemcpyAsync returns after the copy has been staged, `h` may leave scope
  const hipError_t ce = hipMemcpyAsync(step_state, &h, sizeof(h), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (ce != hipSuccess) {
    set_error("brStepStateSet: copy failed: %s", hipGetErrorString(ce));
    return BR_ERR_HIP;
  }
  (void)hipStreamSynchronize((hipStream_t)stream);
  return BR_OK;
}

extern "C" int brStageBatch(void* dst_users, void* dst_items, float* dst_labels, const void* users, const void* items,
                            const float* labels, int id_type, int64_t n, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brStageBatch: bad id_type");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(dst_users && dst_items && users && items && n > 0, "brStageBatch: bad args");
  const unsigned grid = (unsigned)ceil_div(n, 256);
  BR_DISPATCH_ID(id_type, (stage_batch_kernel<IdT><<<grid, 256, 0, (hipStream_t)stream>>>((IdT*)dst_users, (IdT*)dst_items, dst_labels, (const IdT*)users, (const IdT*)items, labels, n)));
  BR_CHECK_LAUNCH("brStageBatch");
  return BR_OK;
}
