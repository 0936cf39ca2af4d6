// L4: the entries of the in-batch softmax and of E1 full-catalogue scoring; the sweep kernel they launch is softmax_kernel.h.
#include "softmax_kernel.h"

namespace br {

// combine the per-split (max, sum, diag) of every query: lse, loss_sum += sum_i (lse_i - diag_i)
__global__ __launch_bounds__(256) void lse_combine_kernel(const float* __restrict__ part, int n_split, int64_t n_r, float* __restrict__ lse_out,
                                                           double* __restrict__ loss_sum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double mine = 0.0;
  if (i < n_r) {
    float m = -INFINITY, d = 0.f;
    for (int s = 0; s < n_split; ++s) m = fmaxf(m, part[(0 * (int64_t)n_split + s) * n_r + i]);
    float l = 0.f;
    for (int s = 0; s < n_split; ++s) {
      const float ms = part[(0 * (int64_t)n_split + s) * n_r + i];
      if (ms > -INFINITY) l += part[(1 * (int64_t)n_split + s) * n_r + i] * exp_hw(ms - m);
      d += part[(2 * (int64_t)n_split + s) * n_r + i];
    }
    const float lse = m + logf(l);
    lse_out[i] = lse;
    mine = (double)lse - (double)d;
  }
  mine = wave_sum_d(mine);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0 && loss_sum) atomicAdd(loss_sum + (blockIdx.x & (BR_SUM_SLOTS - 1)), red[0] + red[1] + red[2] + red[3]);
}

// fused sweep with splits: per row M = max_s m_s, l = sum_s l_s e^(m_s - M), lse = M + log l, loss_sum += lse - diag;
// dQ[i][f] = sum_s slab[s][i][f] e^(m_s - M) / l - C[i + diag][f]
__global__ __launch_bounds__(256) void lse_grad_combine_kernel(const float* __restrict__ part, const float* __restrict__ slabs, int n_split, int64_t n_r,
                                                                int dim, int64_t ldo, const float* __restrict__ C, int64_t n_c, int64_t diag,
                                                                float* __restrict__ lse_out, double* __restrict__ loss_sum, float* __restrict__ dQ) {
  // one 64-lane wave per row: lane -> features lane, lane + 64
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  double mine = 0.0;
  if (i < n_r) {
    float M = -INFINITY, d = 0.f;
    for (int s = 0; s < n_split; ++s) M = fmaxf(M, part[(0 * (int64_t)n_split + s) * n_r + i]);
    float l = 0.f;
    for (int s = 0; s < n_split; ++s) {
      const float ms = part[(0 * (int64_t)n_split + s) * n_r + i];
      if (ms > -INFINITY) l += part[(1 * (int64_t)n_split + s) * n_r + i] * exp_hw(ms - M);
      d += part[(2 * (int64_t)n_split + s) * n_r + i];
    }
    const float lse = M + logf(l);
    if (lane == 0) { lse_out[i] = lse; mine = (double)lse - (double)d; }
    const float inv_l = 1.f / l;
    const int64_t pr = i + diag;
    const bool has_diag = pr >= 0 && pr < n_c;
    for (int f = lane; f < dim; f += 64) {
      float acc = 0.f;
      for (int s = 0; s < n_split; ++s) {
        const float ms = part[(0 * (int64_t)n_split + s) * n_r + i];
        if (ms > -INFINITY) acc += slabs[((int64_t)s * n_r + i) * ldo + f] * exp_hw(ms - M);
      }
      dQ[i * ldo + f] = acc * inv_l - (has_diag ? C[pr * dim + f] : 0.f);
    }
  }
  mine = wave_sum_d(mine);
  __shared__ double red[4];
  if (lane == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0 && loss_sum) atomicAdd(loss_sum + (blockIdx.x & (BR_SUM_SLOTS - 1)), red[0] + red[1] + red[2] + red[3]);
}

// out[i] = sum_s slabs[s][i] in split order (n = rows * ld floats, n % 4 == 0 or scalar tail)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ slabs, int n_split, int64_t n, float* __restrict__ out) {
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 + 3 < n && ((reinterpret_cast<uintptr_t>(slabs) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 && (n & 3) == 0) {
    float4 acc = *reinterpret_cast<const float4*>(slabs + i4);
    for (int s = 1; s < n_split; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(slabs + (int64_t)s * n + i4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(out + i4) = acc;
  } else {
    for (int64_t i = i4; i < n && i < i4 + 4; ++i) {
      float acc = slabs[i];
      for (int s = 1; s < n_split; ++s) acc += slabs[(int64_t)s * n + i];
      out[i] = acc;
    }
  }
}

// threshold sweep with splits: the M-th best key of the union of a query's per-split lists, one wave per query.  The keys are held in
// LDS and the M best are taken one after the other, each the best key ranked strictly after the one before (the order is total:
// real keys have distinct columns, and the fillers (-inf, kThrNone) of a short list are never ranked after themselves) -
// no atomics, the same result whatever the split count.
__global__ __launch_bounds__(64) void thr_combine_kernel(const uint2* __restrict__ lists, int n_keys, int M, int64_t n_t, int64_t diag,
                                                          float* __restrict__ thr_s, int32_t* __restrict__ thr_p) {
  extern __shared__ __attribute__((aligned(16))) uint2 keys[];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  for (int k = lane; k < n_keys; k += 64) keys[k] = lists[i * n_keys + k];
  __syncthreads();
  float prev_s = INFINITY;
  int prev_j = -1;
  for (int t = 0; t < M; ++t) {
    float best = -INFINITY;
    int bestj = kThrNone;
    for (int k = lane; k < n_keys; k += 64) {
      const float s = __uint_as_float(keys[k].x);
      const int j = (int)keys[k].y;
      if (key_worse(s, j, prev_s, prev_j) && key_worse(best, bestj, s, j)) { best = s; bestj = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(best, off, 64);
      const int oj = __shfl_xor(bestj, off, 64);
      if (key_worse(best, bestj, os, oj)) { best = os; bestj = oj; }
    }
    prev_s = best; prev_j = bestj;
  }
  if (lane == 0) {
    const int64_t partner = i + diag;
    const int64_t n_neg = n_t - ((partner >= 0 && partner < n_t) ? 1 : 0);
    thr_s[i] = n_neg > M ? prev_s : -INFINITY;
    thr_p[i] = n_neg > M ? prev_j : kThrNone;
  }
}

// E1: stable top-k of one score row per workgroup (ties keep the lower item position).
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ scores, int64_t n_items, int k,
                                                         float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  const float* row = scores + (int64_t)blockIdx.x * n_items;
  __shared__ float bs[4];
  __shared__ int bi[4];
  __shared__ float sel_s;
  __shared__ int sel_i;
  float prev_s = INFINITY;
  int prev_i = -1;
  for (int t = 0; t < k; ++t) {
    // best (score desc, index asc) strictly after (prev_s, prev_i)
    float best = -INFINITY;
    int besti = 0x7FFFFFFF;
    for (int64_t i = threadIdx.x; i < n_items; i += blockDim.x) {
      const float s = row[i];
      const bool after = (s < prev_s) || (s == prev_s && (int)i > prev_i);
      if (after && (s > best || (s == best && (int)i < besti))) { best = s; besti = (int)i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(besti, off, 64);
      if (os > best || (os == best && oi < besti)) { best = os; besti = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bs[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float b = bs[0]; int ix = bi[0];
      for (int w = 1; w < 4; ++w) if (bs[w] > b || (bs[w] == b && bi[w] < ix)) { b = bs[w]; ix = bi[w]; }
      sel_s = b; sel_i = ix;
      out_s[(int64_t)blockIdx.x * k + t] = b;
      out_i[(int64_t)blockIdx.x * k + t] = (ix == 0x7FFFFFFF) ? -1 : ix;
    }
    __syncthreads();
    prev_s = sel_s; prev_i = sel_i;
    __syncthreads();
  }
}

}  // namespace br

using namespace br;

namespace {
constexpr int kTargetWgs = 512;      // two workgroups per CU

// splits of the streamed axis so that row_blocks * splits ~ kTargetWgs (each split: a whole number of 64-row steps)
int choose_splits(int64_t n_r, int64_t n_t, int64_t max_splits) {
  const int64_t rb = ceil_div(n_r, (int64_t)kOwn), steps = ceil_div(n_t, (int64_t)kTs);
  int64_t s = ceil_div((int64_t)kTargetWgs, rb);
  if (s > steps) s = steps;
  if (s > max_splits) s = max_splits;
  if (s > 64) s = 64;
  return (int)(s < 1 ? 1 : s);
}

template <int MODE, int KQ, typename IdT, bool EMU>
void launch_inbatch_e(const InbatchArgs& a, int n_split, hipStream_t s) {
  constexpr int Kp = 8 * KQ, FT = (Kp + 31) / 32, KB = (Kp + 15) / 16;
  constexpr bool GRAD = MODE == MODE_GRAD_R || MODE == MODE_GRAD_C || MODE == MODE_LSE_GRAD_R;
  const size_t img = EMU ? (size_t)2 * KB * 3 * 2 * kGs * 4 + (GRAD ? (size_t)2 * 2 * FT * 3 * 2 * kGs * 4 : 0)
                         : (size_t)kTs * (Kp + 4) + (GRAD ? (size_t)FT * 32 * kLdT : 0);
  const size_t shmem = (img + kTs) * sizeof(float) + kTs * sizeof(IdT);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)inbatch_kernel<MODE, KQ, IdT, EMU>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    attr = true;
  }
  const dim3 grid((unsigned)ceil_div(a.n_r, (int64_t)kOwn), (unsigned)n_split);
  inbatch_kernel<MODE, KQ, IdT, EMU><<<grid, 256, shmem, s>>>(a);
}
template <int MODE, int KQ, typename IdT>
void launch_inbatch_k(const InbatchArgs& a, int n_split, hipStream_t s) {
  // bf16x6 where it measured faster (8 192 x 8 192 x 64: lse 120 -> 93 us, lse + dQ one sweep 185 -> 145, dC 163 -> 125): not for short streamed
  // axes (2 048: the piece staging costs more than the MFMAs save), not for the gradient modes past 64 features (the stationary pieces +
  // the accumulators of four feature tiles spill: 264 -> 340 us at 100 features)
  constexpr bool GRAD = MODE == MODE_GRAD_R || MODE == MODE_GRAD_C || MODE == MODE_LSE_GRAD_R;
  if (mlp_bf16x6() && a.n_t >= 4096 && (KQ <= 8 || !GRAD)) launch_inbatch_e<MODE, KQ, IdT, true>(a, n_split, s);
  else launch_inbatch_e<MODE, KQ, IdT, false>(a, n_split, s);
}

template <int MODE, typename IdT>
void launch_inbatch_t(const InbatchArgs& a, int n_split, hipStream_t s) {
  const int kq = (a.dim + 7) / 8;
  if (kq <= 4) launch_inbatch_k<MODE, 4, IdT>(a, n_split, s);
  else if (kq <= 7) launch_inbatch_k<MODE, 7, IdT>(a, n_split, s);
  else if (kq <= 8) launch_inbatch_k<MODE, 8, IdT>(a, n_split, s);
  else if (kq <= 13) launch_inbatch_k<MODE, 13, IdT>(a, n_split, s);
  else launch_inbatch_k<MODE, 16, IdT>(a, n_split, s);
}

template <int MODE>
void launch_inbatch(InbatchArgs a, int n_split, int id_type, hipStream_t s) {
  const int64_t steps = ceil_div(a.n_t, (int64_t)kTs);
  a.t_per_split = ceil_div(steps, (int64_t)n_split) * kTs;
  n_split = (int)ceil_div(a.n_t, a.t_per_split);       // no empty split
  if (id_type == BR_IDS_I64) launch_inbatch_t<MODE, int64_t>(a, n_split, s);
  else launch_inbatch_t<MODE, int32_t>(a, n_split, s);
}
// ---- hard negatives: the threshold sweep (MODE_THR) and the HARD forms.  ONE arithmetic per call: the body is chosen from the
// candidate count and the width alone and handed to every sweep of the call, whichever operand it streams - the selection is
// only reproducible on the same score bits (the plain rule above picks per mode and per streamed length).
bool hard_emu(int64_t Bc, int dim) { return mlp_bf16x6() && Bc >= 4096 && (dim + 7) / 8 <= 8; }

InbatchHardArgs hard_args(const InbatchArgs& b, const float* thr_s, const int32_t* thr_p) {
  InbatchHardArgs h;
  static_cast<InbatchArgs&>(h) = b;
  h.thr_s = thr_s; h.thr_p = thr_p; h.thr_s_out = nullptr; h.thr_p_out = nullptr; h.lists = nullptr; h.M = 0; h.col0 = 0;
  return h;
}
}  // namespace

extern "C" int64_t brInBatchSoftmaxWorkspaceBytes(int64_t Bq, int64_t Bc, int dim) {
  if (Bq <= 0 || Bc <= 0 || dim <= 0) return 0;
  const int64_t lse = (int64_t)3 * choose_splits(Bq, Bc, 64) * Bq;
  const int64_t gq = choose_splits(Bq, Bc, 64) > 1 ? (int64_t)choose_splits(Bq, Bc, 64) * Bq * dim : 0;
  const int64_t gc = choose_splits(Bc, Bq, 64) > 1 ? (int64_t)choose_splits(Bc, Bq, 64) * Bc * dim : 0;
  const int64_t fused = gq ? gq + lse : 0;             // brInBatchSoftmaxLseGradQ: slabs + (max, sum, diag)
  int64_t fl = lse > gq ? (lse > gc ? lse : gc) : (gq > gc ? gq : gc);
  fl = fused > fl ? fused : fl;
  return fl * (int64_t)sizeof(float);
}

extern "C" int brInBatchSoftmaxLse(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                   int64_t Bc, int dim, int64_t diag_offset, float* row_lse, double* loss_sum, void* ws, int64_t ws_bytes,
                                   brStream stream) {
  BR_CHECK_ARG(Q && C && row_lse && Bq >= 0 && Bc >= 1 && dim >= 1 && dim <= 128, "brInBatchSoftmaxLse: bad args (dim <= 128)");
  BR_CHECK_ARG((q_pos_ids == nullptr) == (cand_ids == nullptr), "brInBatchSoftmaxLse: ids both or neither");
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brInBatchSoftmaxLse: bad id_type");
  BR_CHECK_ARG(ws_bytes >= 0 && (ws != nullptr || ws_bytes == 0), "brInBatchSoftmaxLse: bad workspace");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / (int64_t)(3 * Bq * sizeof(float)) : 1);
  InbatchArgs a{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, nullptr, 0, n_split > 1 ? (float*)ws : nullptr, row_lse, loss_sum, 0};
  launch_inbatch<MODE_LSE>(a, n_split, id_type, s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxLse");
  if (n_split > 1) {
    const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
    lse_combine_kernel<<<(unsigned)ceil_div(Bq, (int64_t)256), 256, 0, s>>>((const float*)ws, (int)ceil_div(Bc, tps), Bq, row_lse, loss_sum);
    BR_CHECK_LAUNCH("brInBatchSoftmaxLse(combine)");
  }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxLseGradQ(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                        int64_t Bc, int dim, int64_t diag_offset, float* row_lse, double* loss_sum, float* dQ, void* ws,
                                        int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && row_lse && dQ && Bq >= 0 && Bc >= 1 && dim >= 1 && dim <= 128, "brInBatchSoftmaxLseGradQ: bad args (dim <= 128)");
  BR_CHECK_ARG((q_pos_ids == nullptr) == (cand_ids == nullptr), "brInBatchSoftmaxLseGradQ: ids both or neither");
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brInBatchSoftmaxLseGradQ: bad id_type");
  BR_CHECK_ARG(ws_bytes >= 0 && (ws != nullptr || ws_bytes == 0), "brInBatchSoftmaxLseGradQ: bad workspace");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dim > 64) {      // the fused sweep's registers (stationary rows + two score tiles + the dQ accumulator + 32 probabilities) only fit up to 64 features
    const int rc = brInBatchSoftmaxLse(Q, C, q_pos_ids, cand_ids, id_type, Bq, Bc, dim, diag_offset, row_lse, loss_sum, ws, ws_bytes, stream);
    if (rc != BR_OK) return rc;
    return brInBatchSoftmaxGrad(Q, C, q_pos_ids, cand_ids, id_type, Bq, Bc, dim, diag_offset, row_lse, dQ, nullptr, ws, ws_bytes, stream);
  }
  // workspace per split: the unnormalised dQ slab (Bq x dim) + (max, sum, diag) per row
  const int64_t per_split = (Bq * dim + 3 * Bq) * (int64_t)sizeof(float);
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / per_split : 1);
  const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
  const int ns = (int)ceil_div(Bc, tps);                 // splits actually launched (launch_inbatch recomputes the same)
  float* slabs = (float*)ws;
  float* part = n_split > 1 ? slabs + (int64_t)ns * Bq * dim : nullptr;
  InbatchArgs a{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, n_split > 1 ? slabs : dQ, dim, part, row_lse, loss_sum, 0};
  launch_inbatch<MODE_LSE_GRAD_R>(a, n_split, id_type, s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxLseGradQ");
  if (n_split > 1) {
    lse_grad_combine_kernel<<<(unsigned)ceil_div(Bq, (int64_t)4), 256, 0, s>>>(part, slabs, ns, Bq, dim, dim, C, Bc, diag_offset, row_lse, loss_sum, dQ);
    BR_CHECK_LAUNCH("brInBatchSoftmaxLseGradQ(combine)");
  }
  return BR_OK;
}

// one gradient sweep: rows of `own` are owned, `str` is streamed; direct or through slabs in ws
template <int MODE>
static int grad_sweep(const float* own, const float* str, int64_t n_own, int64_t n_str, int dim, const void* own_ids, const void* str_ids, int id_type,
                      int64_t diag, const float* lse, float* out, void* ws, int64_t ws_bytes, hipStream_t s) {
  const int n_split = choose_splits(n_own, n_str, ws ? ws_bytes / (int64_t)(n_own * dim * sizeof(float)) : 1);
  InbatchArgs a{own, str, n_own, n_str, dim, own_ids, str_ids, diag, lse, n_split > 1 ? (float*)ws : out, dim, nullptr, nullptr, nullptr, 0};
  launch_inbatch<MODE>(a, n_split, id_type, s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxGrad");
  if (n_split > 1) {
    const int64_t tps = ceil_div(ceil_div(n_str, (int64_t)kTs), (int64_t)n_split) * kTs;
    const int64_t n = n_own * dim;
    slab_sum_kernel<<<(unsigned)ceil_div(ceil_div(n, (int64_t)4), (int64_t)256), 256, 0, s>>>((const float*)ws, (int)ceil_div(n_str, tps), n, out);
    BR_CHECK_LAUNCH("brInBatchSoftmaxGrad(slab sum)");
  }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxGrad(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                    int64_t Bc, int dim, int64_t diag_offset, const float* row_lse, float* dQ, float* dC, void* ws,
                                    int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && row_lse && Bq >= 0 && Bc >= 1 && dim >= 1 && dim <= 128, "brInBatchSoftmaxGrad: bad args (dim <= 128)");
  BR_CHECK_ARG(dQ || dC, "brInBatchSoftmaxGrad: nothing to compute");
  BR_CHECK_ARG((q_pos_ids == nullptr) == (cand_ids == nullptr), "brInBatchSoftmaxGrad: ids both or neither");
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brInBatchSoftmaxGrad: bad id_type");
  BR_CHECK_ARG(ws_bytes >= 0 && (ws != nullptr || ws_bytes == 0), "brInBatchSoftmaxGrad: bad workspace");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  // dQ: queries own, candidates stream; the partner of query i is candidate i + diag_offset
  if (dQ) { const int rc = grad_sweep<MODE_GRAD_R>(Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, id_type, diag_offset, row_lse, dQ, ws, ws_bytes, s); if (rc) return rc; }
  // dC: candidates own, queries stream; the partner of candidate j is query j - diag_offset (the slabs of dQ are consumed by then)
  if (dC) { const int rc = grad_sweep<MODE_GRAD_C>(C, Q, Bc, Bq, dim, cand_ids, q_pos_ids, id_type, -diag_offset, row_lse, dC, ws, ws_bytes, s); if (rc) return rc; }
  return BR_OK;
}

// ---- hard negatives: C-ABI ----
#define BR_CHECK_HARD_COMMON(name)                                                                                                                  \
  BR_CHECK_ARG(Q && C && Bq >= 0 && Bc >= 1 && Bc < ((int64_t)1 << 31) && dim >= 1 && dim <= 128, name ": bad args (dim <= 128, Bc < 2^31)");      \
  BR_CHECK_ARG((q_pos_ids == nullptr) == (cand_ids == nullptr), name ": ids both or neither");                                                       \
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, name ": bad id_type");                                                                \
  BR_CHECK_ARG(ws_bytes >= 0 && (ws != nullptr || ws_bytes == 0), name ": bad workspace")

extern "C" int64_t brInBatchSoftmaxHardWorkspaceBytes(int64_t Bq, int64_t Bc, int dim, int M) {
  if (Bq <= 0 || Bc <= 0 || dim <= 0 || M < 1 || M > 64) return 0;
  const int64_t plain = brInBatchSoftmaxWorkspaceBytes(Bq, Bc, dim);
  const int64_t ns = choose_splits(Bq, Bc, 64);
  const int64_t lists = ns > 1 ? ns * Bq * M * (int64_t)sizeof(uint2) : 0;
  return plain > lists ? plain : lists;
}

extern "C" int brInBatchSoftmaxHardThreshold(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                             int64_t Bc, int dim, int64_t diag_offset, int M, float* thr_score, int32_t* thr_pos, void* ws,
                                             int64_t ws_bytes, brStream stream) {
  BR_CHECK_HARD_COMMON("brInBatchSoftmaxHardThreshold");
  BR_CHECK_ARG(M >= 1 && M <= 64, "brInBatchSoftmaxHardThreshold: 1 <= M <= 64");
  BR_CHECK_ARG(thr_score && thr_pos, "brInBatchSoftmaxHardThreshold: thr_score and thr_pos are required");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / (Bq * M * (int64_t)sizeof(uint2)) : 1);
  const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
  const int ns = (int)ceil_div(Bc, tps);                 // splits actually launched (launch_hard recomputes the same)
  InbatchHardArgs a = hard_args(InbatchArgs{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0}, nullptr, nullptr);
  a.M = M;
  if (n_split > 1) a.lists = (uint2*)ws; else { a.thr_s_out = thr_score; a.thr_p_out = thr_pos; }
  launch_hard<MODE_THR>(a, n_split, id_type, hard_emu(Bc, dim), s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxHardThreshold");
  if (n_split > 1) {
    thr_combine_kernel<<<(unsigned)Bq, 64, (size_t)ns * M * sizeof(uint2), s>>>((const uint2*)ws, ns * M, M, Bc, diag_offset, thr_score, thr_pos);
    BR_CHECK_LAUNCH("brInBatchSoftmaxHardThreshold(combine)");
  }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxLseHard(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                       int64_t Bc, int dim, int64_t diag_offset, float* row_lse, double* loss_sum, const float* thr_score,
                                       const int32_t* thr_pos, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_HARD_COMMON("brInBatchSoftmaxLseHard");
  BR_CHECK_ARG(row_lse && thr_score && thr_pos, "brInBatchSoftmaxLseHard: row_lse, thr_score and thr_pos are required");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / (int64_t)(3 * Bq * sizeof(float)) : 1);
  const InbatchHardArgs a = hard_args(InbatchArgs{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, nullptr, 0, n_split > 1 ? (float*)ws : nullptr, row_lse, loss_sum, 0},
                                      thr_score, thr_pos);
  launch_hard<MODE_LSE>(a, n_split, id_type, hard_emu(Bc, dim), s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxLseHard");
  if (n_split > 1) {
    const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
    lse_combine_kernel<<<(unsigned)ceil_div(Bq, (int64_t)256), 256, 0, s>>>((const float*)ws, (int)ceil_div(Bc, tps), Bq, row_lse, loss_sum);
    BR_CHECK_LAUNCH("brInBatchSoftmaxLseHard(combine)");
  }
  return BR_OK;
}

// one hard gradient sweep (grad_sweep with the thresholds of the QUERIES, owned or streamed)
template <int MODE>
static int grad_sweep_hard(const float* own, const float* str, int64_t n_own, int64_t n_str, int dim, const void* own_ids, const void* str_ids, int id_type,
                           int64_t diag, const float* lse, const float* thr_s, const int32_t* thr_p, bool emu, int64_t col0, float* out, void* ws,
                           int64_t ws_bytes, hipStream_t s) {
  const int n_split = choose_splits(n_own, n_str, ws ? ws_bytes / (int64_t)(n_own * dim * sizeof(float)) : 1);
  InbatchHardArgs a = hard_args(InbatchArgs{own, str, n_own, n_str, dim, own_ids, str_ids, diag, lse, n_split > 1 ? (float*)ws : out, dim, nullptr, nullptr, nullptr, 0},
                                thr_s, thr_p);
  a.col0 = col0;                                         // candidates own: their first column in the count of thr_p
  launch_hard<MODE>(a, n_split, id_type, emu, s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxGradHard");
  if (n_split > 1) {
    const int64_t tps = ceil_div(ceil_div(n_str, (int64_t)kTs), (int64_t)n_split) * kTs;
    const int64_t n = n_own * dim;
    slab_sum_kernel<<<(unsigned)ceil_div(ceil_div(n, (int64_t)4), (int64_t)256), 256, 0, s>>>((const float*)ws, (int)ceil_div(n_str, tps), n, out);
    BR_CHECK_LAUNCH("brInBatchSoftmaxGradHard(slab sum)");
  }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxGradHard(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                        int64_t Bc, int dim, int64_t diag_offset, const float* row_lse, float* dQ, float* dC, const float* thr_score,
                                        const int32_t* thr_pos, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_HARD_COMMON("brInBatchSoftmaxGradHard");
  BR_CHECK_ARG(row_lse && thr_score && thr_pos, "brInBatchSoftmaxGradHard: row_lse, thr_score and thr_pos are required");
  BR_CHECK_ARG(dQ || dC, "brInBatchSoftmaxGradHard: nothing to compute");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool emu = hard_emu(Bc, dim);
  if (dQ) { const int rc = grad_sweep_hard<MODE_GRAD_R>(Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, id_type, diag_offset, row_lse, thr_score, thr_pos, emu, 0, dQ, ws, ws_bytes, s); if (rc) return rc; }
  if (dC) { const int rc = grad_sweep_hard<MODE_GRAD_C>(C, Q, Bc, Bq, dim, cand_ids, q_pos_ids, id_type, -diag_offset, row_lse, thr_score, thr_pos, emu, 0, dC, ws, ws_bytes, s); if (rc) return rc; }
  return BR_OK;
}

// dC of a SLICE of the candidates the thresholds were taken over (the data-parallel step: every rank owns B of the world * B gathered
// candidates).  The body is chosen from the candidate count of the threshold sweep, Bc_total, not from the slice's: the keys are only
// meaningful against scores of the arithmetic that formed them.
extern "C" int brInBatchSoftmaxGradHardSlice(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                             int64_t Bc, int dim, int64_t diag_offset, const float* row_lse, float* dC, const float* thr_score,
                                             const int32_t* thr_pos, int64_t c0, int64_t Bc_total, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_HARD_COMMON("brInBatchSoftmaxGradHardSlice");
  BR_CHECK_ARG(row_lse && dC && thr_score && thr_pos, "brInBatchSoftmaxGradHardSlice: row_lse, dC, thr_score and thr_pos are required");
  BR_CHECK_ARG(c0 >= 0 && c0 + Bc <= Bc_total && Bc_total < ((int64_t)1 << 31), "brInBatchSoftmaxGradHardSlice: the slice [c0, c0 + Bc) must lie in [0, Bc_total), Bc_total < 2^31");
  if (Bq == 0) return BR_OK;
  return grad_sweep_hard<MODE_GRAD_C>(C, Q, Bc, Bq, dim, cand_ids, q_pos_ids, id_type, -diag_offset, row_lse, thr_score, thr_pos, hard_emu(Bc_total, dim), c0, dC, ws,
                                      ws_bytes, (hipStream_t)stream);
}

extern "C" int brInBatchSoftmaxLseGradQHard(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                            int64_t Bc, int dim, int64_t diag_offset, float* row_lse, double* loss_sum, float* dQ,
                                            const float* thr_score, const int32_t* thr_pos, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_HARD_COMMON("brInBatchSoftmaxLseGradQHard");
  BR_CHECK_ARG(row_lse && dQ && thr_score && thr_pos, "brInBatchSoftmaxLseGradQHard: row_lse, dQ, thr_score and thr_pos are required");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dim > 64) {      // as brInBatchSoftmaxLseGradQ: the fused sweep's registers only fit up to 64 features
    const int rc = brInBatchSoftmaxLseHard(Q, C, q_pos_ids, cand_ids, id_type, Bq, Bc, dim, diag_offset, row_lse, loss_sum, thr_score, thr_pos, ws, ws_bytes, stream);
    if (rc != BR_OK) return rc;
    return brInBatchSoftmaxGradHard(Q, C, q_pos_ids, cand_ids, id_type, Bq, Bc, dim, diag_offset, row_lse, dQ, nullptr, thr_score, thr_pos, ws, ws_bytes, stream);
  }
  const int64_t per_split = (Bq * dim + 3 * Bq) * (int64_t)sizeof(float);
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / per_split : 1);
  const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
  const int ns = (int)ceil_div(Bc, tps);
  float* slabs = (float*)ws;
  float* part = n_split > 1 ? slabs + (int64_t)ns * Bq * dim : nullptr;
  const InbatchHardArgs a = hard_args(InbatchArgs{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, n_split > 1 ? slabs : dQ, dim, part, row_lse, loss_sum, 0},
                                      thr_score, thr_pos);
  launch_hard<MODE_LSE_GRAD_R>(a, n_split, id_type, hard_emu(Bc, dim), s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxLseGradQHard");
  if (n_split > 1) {
    lse_grad_combine_kernel<<<(unsigned)ceil_div(Bq, (int64_t)4), 256, 0, s>>>(part, slabs, ns, Bq, dim, dim, C, Bc, diag_offset, row_lse, loss_sum, dQ);
    BR_CHECK_LAUNCH("brInBatchSoftmaxLseGradQHard(combine)");
  }
  return BR_OK;
}

// ---- log-Q correction (candidate_sampling_probability of tfrs.tasks.Retrieval; the reference's twoTower.py:47,82-83 builds the task and
// does not pass the option): x_ij = S_ij - cand_logq[j] in every sweep, before the mask and before the selection.  The sweeps are the
// HARD forms with the bias (softmax_logq.hip); without thresholds every query carries the key (-inf, none): nothing is cut. ----
#define BR_CHECK_LOGQ_COMMON(name)                                                                                                                  \
  BR_CHECK_HARD_COMMON(name);                                                                                                                       \
  BR_CHECK_ARG(cand_logq != nullptr, name ": cand_logq is required");                                                                              \
  BR_CHECK_ARG((thr_score == nullptr) == (thr_pos == nullptr), name ": thr_score and thr_pos both (hard negatives) or neither (plain)")

namespace {
InbatchLogqArgs logq_args(const InbatchArgs& b, const float* thr_s, const int32_t* thr_p, const float* bias) {
  InbatchLogqArgs h;
  static_cast<InbatchHardArgs&>(h) = hard_args(b, thr_s, thr_p);
  h.bias = bias;
  return h;
}

// one log-Q gradient sweep (grad_sweep_hard with the bias of the CANDIDATES, streamed or owned)
template <int MODE>
int grad_sweep_logq(const float* own, const float* str, int64_t n_own, int64_t n_str, int dim, const void* own_ids, const void* str_ids, int id_type, int64_t diag,
                    const float* lse, const float* thr_s, const int32_t* thr_p, const float* bias, bool emu, int64_t col0, float* out, void* ws, int64_t ws_bytes,
                    hipStream_t s) {
  const int n_split = choose_splits(n_own, n_str, ws ? ws_bytes / (int64_t)(n_own * dim * sizeof(float)) : 1);
  InbatchLogqArgs a = logq_args(InbatchArgs{own, str, n_own, n_str, dim, own_ids, str_ids, diag, lse, n_split > 1 ? (float*)ws : out, dim, nullptr, nullptr, nullptr, 0},
                                thr_s, thr_p, bias);
  a.col0 = col0;
  launch_logq<MODE>(a, n_split, id_type, emu, s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxGradLogQ");
  if (n_split > 1) {
    const int64_t tps = ceil_div(ceil_div(n_str, (int64_t)kTs), (int64_t)n_split) * kTs;
    const int64_t n = n_own * dim;
    slab_sum_kernel<<<(unsigned)ceil_div(ceil_div(n, (int64_t)4), (int64_t)256), 256, 0, s>>>((const float*)ws, (int)ceil_div(n_str, tps), n, out);
    BR_CHECK_LAUNCH("brInBatchSoftmaxGradLogQ(slab sum)");
  }
  return BR_OK;
}
}  // namespace

extern "C" int brInBatchSoftmaxHardThresholdLogQ(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                                 int64_t Bc, int dim, int64_t diag_offset, int M, float* thr_score, int32_t* thr_pos,
                                                 const float* cand_logq, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_HARD_COMMON("brInBatchSoftmaxHardThresholdLogQ");
  BR_CHECK_ARG(cand_logq != nullptr, "brInBatchSoftmaxHardThresholdLogQ: cand_logq is required");
  BR_CHECK_ARG(M >= 1 && M <= 64, "brInBatchSoftmaxHardThresholdLogQ: 1 <= M <= 64");
  BR_CHECK_ARG(thr_score && thr_pos, "brInBatchSoftmaxHardThresholdLogQ: thr_score and thr_pos are required");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / (Bq * M * (int64_t)sizeof(uint2)) : 1);
  const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
  const int ns = (int)ceil_div(Bc, tps);
  InbatchLogqArgs a = logq_args(InbatchArgs{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0}, nullptr, nullptr, cand_logq);
  a.M = M;
  if (n_split > 1) a.lists = (uint2*)ws; else { a.thr_s_out = thr_score; a.thr_p_out = thr_pos; }
  launch_logq<MODE_THR>(a, n_split, id_type, hard_emu(Bc, dim), s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxHardThresholdLogQ");
  if (n_split > 1) {
    thr_combine_kernel<<<(unsigned)Bq, 64, (size_t)ns * M * sizeof(uint2), s>>>((const uint2*)ws, ns * M, M, Bc, diag_offset, thr_score, thr_pos);
    BR_CHECK_LAUNCH("brInBatchSoftmaxHardThresholdLogQ(combine)");
  }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxLseLogQ(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                       int64_t Bc, int dim, int64_t diag_offset, float* row_lse, double* loss_sum, const float* thr_score,
                                       const int32_t* thr_pos, const float* cand_logq, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_LOGQ_COMMON("brInBatchSoftmaxLseLogQ");
  BR_CHECK_ARG(row_lse != nullptr, "brInBatchSoftmaxLseLogQ: row_lse is required");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / (int64_t)(3 * Bq * sizeof(float)) : 1);
  const InbatchLogqArgs a = logq_args(InbatchArgs{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, nullptr, 0, n_split > 1 ? (float*)ws : nullptr, row_lse, loss_sum, 0},
                                      thr_score, thr_pos, cand_logq);
  launch_logq<MODE_LSE>(a, n_split, id_type, hard_emu(Bc, dim), s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxLseLogQ");
  if (n_split > 1) {
    const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
    lse_combine_kernel<<<(unsigned)ceil_div(Bq, (int64_t)256), 256, 0, s>>>((const float*)ws, (int)ceil_div(Bc, tps), Bq, row_lse, loss_sum);
    BR_CHECK_LAUNCH("brInBatchSoftmaxLseLogQ(combine)");
  }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxGradLogQ(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                        int64_t Bc, int dim, int64_t diag_offset, const float* row_lse, float* dQ, float* dC, const float* thr_score,
                                        const int32_t* thr_pos, const float* cand_logq, int64_t c0, int64_t Bc_total, void* ws, int64_t ws_bytes,
                                        brStream stream) {
  BR_CHECK_LOGQ_COMMON("brInBatchSoftmaxGradLogQ");
  BR_CHECK_ARG(row_lse != nullptr, "brInBatchSoftmaxGradLogQ: row_lse is required");
  BR_CHECK_ARG(dQ || dC, "brInBatchSoftmaxGradLogQ: nothing to compute");
  BR_CHECK_ARG(c0 >= 0 && c0 + Bc <= Bc_total && Bc_total < ((int64_t)1 << 31), "brInBatchSoftmaxGradLogQ: the slice [c0, c0 + Bc) must lie in [0, Bc_total), Bc_total < 2^31");
  BR_CHECK_ARG(!dQ || (c0 == 0 && Bc_total == Bc), "brInBatchSoftmaxGradLogQ: dQ needs every candidate (a slice forms dC only)");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool emu = hard_emu(Bc_total, dim);
  if (dQ) { const int rc = grad_sweep_logq<MODE_GRAD_R>(Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, id_type, diag_offset, row_lse, thr_score, thr_pos, cand_logq, emu, 0, dQ, ws, ws_bytes, s); if (rc) return rc; }
  if (dC) { const int rc = grad_sweep_logq<MODE_GRAD_C>(C, Q, Bc, Bq, dim, cand_ids, q_pos_ids, id_type, -diag_offset, row_lse, thr_score, thr_pos, cand_logq, emu, c0, dC, ws, ws_bytes, s); if (rc) return rc; }
  return BR_OK;
}

extern "C" int brInBatchSoftmaxLseGradQLogQ(const float* Q, const float* C, const void* q_pos_ids, const void* cand_ids, int id_type, int64_t Bq,
                                            int64_t Bc, int dim, int64_t diag_offset, float* row_lse, double* loss_sum, float* dQ,
                                            const float* thr_score, const int32_t* thr_pos, const float* cand_logq, void* ws, int64_t ws_bytes,
                                            brStream stream) {
  BR_CHECK_LOGQ_COMMON("brInBatchSoftmaxLseGradQLogQ");
  BR_CHECK_ARG(row_lse && dQ, "brInBatchSoftmaxLseGradQLogQ: row_lse and dQ are required");
  if (Bq == 0) return BR_OK;
  hipStream_t s = (hipStream_t)stream;
  // as brInBatchSoftmaxLseGradQ: the fused sweep's registers only fit up to 64 features.  With 64-bit ids on the bf16x6 body at up to 32
  // features the log-Q form of the fused sweep does not fit the registers of its twin's three waves per SIMD without scratch
  // (profiles/softmax_logq/resources.txt): that combination takes the two sweeps as well.
  if (dim > 64 || (id_type == BR_IDS_I64 && dim <= 32 && hard_emu(Bc, dim))) {
    const int rc = brInBatchSoftmaxLseLogQ(Q, C, q_pos_ids, cand_ids, id_type, Bq, Bc, dim, diag_offset, row_lse, loss_sum, thr_score, thr_pos, cand_logq, ws, ws_bytes, stream);
    if (rc != BR_OK) return rc;
    return brInBatchSoftmaxGradLogQ(Q, C, q_pos_ids, cand_ids, id_type, Bq, Bc, dim, diag_offset, row_lse, dQ, nullptr, thr_score, thr_pos, cand_logq, 0, Bc, ws, ws_bytes, stream);
  }
  const int64_t per_split = (Bq * dim + 3 * Bq) * (int64_t)sizeof(float);
  const int n_split = choose_splits(Bq, Bc, ws ? ws_bytes / per_split : 1);
  const int64_t tps = ceil_div(ceil_div(Bc, (int64_t)kTs), (int64_t)n_split) * kTs;
  const int ns = (int)ceil_div(Bc, tps);
  float* slabs = (float*)ws;
  float* part = n_split > 1 ? slabs + (int64_t)ns * Bq * dim : nullptr;
  const InbatchLogqArgs a = logq_args(InbatchArgs{Q, C, Bq, Bc, dim, q_pos_ids, cand_ids, diag_offset, nullptr, n_split > 1 ? slabs : dQ, dim, part, row_lse, loss_sum, 0},
                                      thr_score, thr_pos, cand_logq);
  launch_logq<MODE_LSE_GRAD_R>(a, n_split, id_type, hard_emu(Bc, dim), s);
  BR_CHECK_LAUNCH("brInBatchSoftmaxLseGradQLogQ");
  if (n_split > 1) {
    lse_grad_combine_kernel<<<(unsigned)ceil_div(Bq, (int64_t)4), 256, 0, s>>>(part, slabs, ns, Bq, dim, dim, C, Bc, diag_offset, row_lse, loss_sum, dQ);
    BR_CHECK_LAUNCH("brInBatchSoftmaxLseGradQLogQ(combine)");
  }
  return BR_OK;
}

extern "C" int brScoreMatrix(const float* Q, const float* C, int64_t n_q, int64_t n_c, int dim, float* scores, int64_t ld_scores, brStream stream) {
  BR_CHECK_ARG(Q && C && scores && n_q >= 0 && n_c >= 1 && dim >= 1 && dim <= 128 && ld_scores >= n_c, "brScoreMatrix: bad args (dim <= 128)");
  if (n_q == 0) return BR_OK;
  // candidates own (lanes = consecutive candidates = coalesced score rows), queries stream; the splits write disjoint rows
  InbatchArgs a{C, Q, n_c, n_q, dim, nullptr, nullptr, 0, nullptr, scores, ld_scores, nullptr, nullptr, nullptr, 0};
  launch_inbatch<MODE_SCORES>(a, choose_splits(n_c, n_q, 64), BR_IDS_I32, (hipStream_t)stream);
  BR_CHECK_LAUNCH("brScoreMatrix");
  return BR_OK;
}

extern "C" int brTopKRows(const float* scores, int64_t n_users, int64_t n_items, int k, float* out_scores, int32_t* out_index, brStream stream) {
  BR_CHECK_ARG(scores && out_scores && out_index && n_users >= 0 && n_items >= 1 && k >= 1 && k <= n_items && n_items < ((int64_t)1 << 31),
               "brTopKRows: bad args (1 <= k <= n_items < 2^31)");
  if (n_users == 0) return BR_OK;
  topk_rows_kernel<<<(unsigned)n_users, 256, 0, (hipStream_t)stream>>>(scores, n_items, k, out_scores, out_index);
  BR_CHECK_LAUNCH("brTopKRows");
  return BR_OK;
}
