// L4: in-batch softmax of the TwoTower retrieval task (tfrs.tasks.Retrieval, twoTower.py:47,82-83)
// and E1 full-catalogue scoring - the only MFMA-bound pieces of the path (2*B^2*semb flop per GEMM).
//
//   S = Q C^T (Bq x Bc) is NEVER materialised for the loss.  One kernel, four modes; in each the workgroup OWNS 128 rows of one
//   operand (32 per wave, kept in registers as the stationary MFMA operand for the whole sweep) and STREAMS 64-row tiles of the
//   other operand through LDS:
//     MODE_LSE    owned = queries     streamed = candidates   online logsumexp per query, loss_sum += sum_i (lse_i - S_i,diag)
//     MODE_GRAD_R owned = queries     streamed = candidates   dQ_i = sum_j (exp(S_ij - lse_i) - [j = diag(i)]) C_j
//     MODE_GRAD_C owned = candidates  streamed = queries      dC_j = sum_i (exp(S_ij - lse_i) - [j = diag(i)]) Q_i
//     MODE_SCORES owned = candidates  streamed = queries      scores[q][c] (top-k scoring: topKmetrics.py:17-43, twoTower.py:64-69)
//     MODE_LSE_GRAD_R = MODE_LSE and MODE_GRAD_R in ONE sweep (the training step needs both): the accumulator of dQ is kept relative
//                 to the running row maximum and rescaled when it grows (online softmax); dQ_i = acc_i / l_i - C_diag(i) at the end.
//                 The score tiles are formed twice per step instead of three times (4 GEMMs instead of 5 for lse + dQ + dC)
//     MODE_THR    owned = queries     streamed = candidates   hard negatives: the key (score, column) of each query's M-th best negative;
//                 the HARD forms of the four softmax modes then run over the partner and those M columns only (InbatchHardArgs below)
//   MFMA: v_mfma_f32_32x32x2_f32.  The score tile is formed TRANSPOSED, D[m = streamed entity][n = owned row]: in the result
//   layout a lane then holds ONE owned row (n = lane % 32) and its 16 registers hold 16 streamed entities
//   (m = 8 (r / 4) + 4 (lane / 32) + r % 4), so
//     * everything that is per owned row (its lse, its id, the running max / sum, the diagonal column) is one register per lane,
//       and the softmax reductions run over a lane's own registers - no cross-lane traffic until the very end;
//     * P = exp(S - lse) - [diag] feeds the second GEMM straight from those registers as the B operand
//       (k = streamed entity = register index, n = owned row): out^T[f][owned] += sum_k T[k][f] P[k][owned]; the A operand
//       T[k][f] comes from a transposed copy of the streamed tile in LDS (one ds_read_b128 = 4 consecutive k).  P never goes
//       through LDS (the previous kernel wrote it out and read it back in the A layout).
//   Contraction order of the score product: k = KH * (lane / 32) + kk (each lane half walks its own half of the feature
//   axis), so both operands are read as whole 16-byte vectors.  Two 32-entity sub-tiles are interleaved so that consecutive
//   MFMAs never depend on each other.
//   Occupancy: 128 owned rows per workgroup would leave most of the chip idle at the batch sizes of the reference (8 192 rows =
//   64 workgroups), so the streamed axis is SPLIT over blockIdx.y: each split writes partial results (per-row (max, sum, diag) or
//   a dQ / dC slab) into the caller's workspace and a small second kernel combines them in a fixed order (deterministic; no
//   float atomics).  Without a workspace the split count is 1 and results are written directly.
// [TF-sem] accidental hits: S_ij += FLT_MIN_TFRS (= float32 min / 100) when cand_ids[j] equals the
// id of query i's own positive and j is not that positive's column; SUM reduction over rows.
//   Round 3 (EMU, "bf16x6": csrc/dense.h): both GEMMs as fp32 products on the bf16 matrix pipe - v_mfma_f32_32x32x16_bf16, six
//   per 16-deep block on three-piece operands, the same result layout as the fp32 32x32x2 (so everything above stays as it is).  Every
//   operand is split once: the owned rows at kernel start (registers), the streamed tile by the thread that stages it - into TP
//   [sub-tile][k-block][piece][lane half][entity][8 bf16] (A fragments of the score product, k = 16 kb + 8 hb + j) and TT
//   [sub-tile][16-entity group][feature tile][piece][lane half][feature][8 bf16] (A fragments of the second GEMM: slot j of lane half hb
//   <-> the streamed entity register 8 g2 + j of the score tile holds, m = 8 (r / 4) + 4 hb + r % 4) - and P by the lane that holds it
//   (consecutive registers = consecutive k slots).  BR_MLP_MATH=f32 keeps the fp32 MFMAs.
#pragma once
#include "common.h"
#include "dense.h"
#include <type_traits>

namespace br {

using f32x16 = __attribute__((ext_vector_type(16))) float;
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma32b(bf16x8 a, bf16x8 b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#else
  return c;
#endif
}
// x w as six bf16 products, smallest first (x = xh + xm + xl, w = wh + wm + wl)
__device__ __forceinline__ f32x16 mfma32x6(bf16x8 xh, bf16x8 xm, bf16x8 xl, bf16x8 wh, bf16x8 wm, bf16x8 wl, f32x16 c) {
  c = mfma32b(xl, wh, c); c = mfma32b(xh, wl, c); c = mfma32b(xm, wm, c);
  c = mfma32b(xm, wh, c); c = mfma32b(xh, wm, c); c = mfma32b(xh, wh, c);
  return c;
}
// the same six products with the operand roles swapped (the candidate-owned hard sweep: x = query, w = candidate): issued so that the
// piece pairs meet the accumulator in the order of mfma32x6 with x = candidate, w = query - the score bits of the query-owned sweeps
__device__ __forceinline__ f32x16 mfma32x6m(bf16x8 xh, bf16x8 xm, bf16x8 xl, bf16x8 wh, bf16x8 wm, bf16x8 wl, f32x16 c) {
  c = mfma32b(xh, wl, c); c = mfma32b(xl, wh, c); c = mfma32b(xm, wm, c);
  c = mfma32b(xh, wm, c); c = mfma32b(xm, wh, c); c = mfma32b(xh, wh, c);
  return c;
}
constexpr int kGs = 33;                      // 16-B slots per (..., lane half) group of the piece images: 32 + 1 (the staging's half-word stores of
                                             // the 8 groups a wave touches would otherwise hit the same banks)

enum { MODE_SCORES = 0, MODE_LSE = 1, MODE_GRAD_R = 2, MODE_GRAD_C = 3, MODE_LSE_GRAD_R = 4, MODE_THR = 5 };

// exp of a non-positive argument (score - running max, score - lse) on the hardware exp2: one evaluation per score made
// these kernels VALU-bound with the accurate expf (~30 instructions each).  |x| <= ~88; the relative
// error grows like |x| * 6e-8, i.e. it is largest on the terms that contribute least to the sums.
__device__ __forceinline__ float exp_hw(float x) { return __expf(x); }
constexpr int kOwn = 128;                    // owned rows per workgroup (32 per wave)
constexpr int kTs = 64;                      // streamed entities per step (two sub-tiles of 32)
constexpr int kLdT = kTs + 4;                // row pitch of the transposed tile
constexpr float kMinFloat = -3.4028234663852886e+36f;   // np.finfo(float32).min / 100

struct InbatchArgs {
  const float* R; const float* T;            // owned / streamed operand (n_r x dim, n_t x dim, row-major)
  int64_t n_r, n_t; int dim;
  const void* own_ids; const void* str_ids;  // id of each owned / streamed entity (both or neither)
  int64_t diag;                              // streamed index of owned row o's diagonal partner = o + diag
  const float* lse_in;                       // GRAD_R: per owned row; GRAD_C: per streamed row
  float* out; int64_t ldo;                   // GRAD: [split][n_r][ldo] (split 0 only when n_split == 1); SCORES: scores[streamed][owned]
  float* part;                               // LSE with splits: [3][n_split][n_r] (max, sum, diag score)
  float* lse_out; double* loss_sum;          // LSE without splits
  int64_t t_per_split;                       // streamed rows per blockIdx.y (multiple of kTs)
};

// Hard negatives (tfrs HardNegativeMining): per query the softmax runs over its partner column and its M best other
// columns by (masked score descending, column ascending).  MODE_THR finds the key (score, column) of the M-th of them in a sweep of
// its own, in the tile layout and arithmetic of the sweeps that use it; the HARD forms of the four sweeps keep a column iff it is
// the partner, or x > thr_s, or x == thr_s and column <= thr_p, and give every other column x = -inf.
struct InbatchHardArgs : InbatchArgs {
  const float* thr_s; const int32_t* thr_p;  // HARD: key of the last kept negative per query (owned rows; GRAD_C: streamed rows)
  float* thr_s_out; int32_t* thr_p_out;      // THR without splits
  uint2* lists; int M;                       // THR with splits: [n_r][n_split][M] keys (score bits, column), unordered
  int64_t col0;                              // HARD GRAD_C: the owned candidates are columns [col0, col0 + n_r) of those thr_p counts over
};
// Log-Q correction (tfrs candidate_sampling_probability): x_ij = S_ij - bias[j], before the accidental-hit mask and
// before the selection.  The LOGQ forms are MODE_THR and the HARD forms with one more pointer; thr_s == nullptr there means the key
// (-inf, kThrNone) for every query - nothing is cut, the plain softmax of the corrected scores.
struct InbatchLogqArgs : InbatchHardArgs {
  const float* bias;                         // log q of every CANDIDATE position (streamed rows; GRAD_C: owned rows)
};
constexpr int kThrNone = 0x7FFFFFFF;         // column of the key (-inf, kThrNone): nothing is cut
// what a HARD instantiation keeps per lane; the plain instantiations get the empty forms, so nothing of it exists in their code
template <bool ON> struct HardKey {};
template <> struct HardKey<true> { float ts = -INFINITY; int tp = kThrNone; int tl = 0; };      // a key, and tp as a tile-local column (minus jb)
template <bool ON> struct HardKeys4 {};
template <> struct HardKeys4<true> { float ts[4]; int tp[4]; };
// what a LOGQ instantiation keeps: the bias of the candidate a thread stages or a lane owns
template <bool ON> struct LogqBias {};
template <> struct LogqBias<true> { float b = 0.f; };
// waves per SIMD the register allocation of a LOGQ form is held to: those of its twin without the correction (profiles/softmax_logq/
// resources.txt).  The twins sit at the register limit of their occupancy (167 / 168 of 168, 128 of 128); with the few registers the
// bias costs and the kernel's own bound of 2 the compiler gives the limit up at once and takes a whole wave less.  Every other
// instantiation keeps 2.  (i64: ids are 64-bit.)
template <int MODE, int KQ, bool I64, bool EMU, bool LOGQ>
constexpr int inbatch_waves() {
  if (!LOGQ || KQ > 8) return 2;
  if (MODE == MODE_LSE_GRAD_R) return KQ == 4 && (EMU || !I64) ? 3 : 2;
  if (KQ == 4) return (!EMU && !I64 && (MODE == MODE_THR || MODE == MODE_GRAD_R)) ? 4 : 3;
  if (MODE == MODE_LSE) return EMU ? 2 : 3;
  if (MODE == MODE_THR) return I64 ? 2 : 3;
  return (!EMU && !I64) ? 3 : 2;             // GRAD_R, GRAD_C at 7 and 8 vectors
}
// key a is ranked after key b: lower score, or the same score at a higher column
__device__ __forceinline__ bool key_worse(float xa, int ja, float xb, int jb) { return xa < xb || (xa == xb && ja > jb); }

// KQ = 16-byte vectors per lane half of the feature axis: features are padded to Kp = 8 KQ
// ArgsT: InbatchHardArgs for MODE_THR and the HARD forms (InbatchLogqArgs for their LOGQ forms), else InbatchArgs - the plain
// instantiations take no new argument.  (A parameter
// of its own, not a type computed from MODE in the signature: the unnamed enum would enter the mangled name, differently on host and device.)
template <int MODE, int KQ, typename IdT, bool EMU, bool HARD = false, typename ArgsT = InbatchArgs>
__global__ __launch_bounds__(256, (inbatch_waves<MODE, KQ, sizeof(IdT) == 8, EMU, std::is_base_of<InbatchLogqArgs, ArgsT>::value>()))
void inbatch_kernel(const ArgsT a) {
  constexpr bool LOGQ = std::is_same<ArgsT, InbatchLogqArgs>::value;
  constexpr bool LOGQ_S = LOGQ && MODE != MODE_GRAD_C;   // the corrected candidates stream: their bias goes through LDS with their ids
  constexpr bool LOGQ_O = LOGQ && MODE == MODE_GRAD_C;   // ... are owned: one register per lane
  static_assert((std::is_same<ArgsT, InbatchHardArgs>::value || LOGQ) == (HARD || MODE == MODE_THR), "the hard arguments go with MODE_THR and the HARD forms");
  static_assert(!HARD || MODE == MODE_LSE || MODE == MODE_GRAD_R || MODE == MODE_GRAD_C || MODE == MODE_LSE_GRAD_R, "hard forms of the four softmax sweeps");
  constexpr int KH = 4 * KQ, Kp = 8 * KQ, ldt = Kp + 4;
  constexpr int FT = (Kp + 31) / 32;                     // 32-feature tiles of the second GEMM
  constexpr int KB = (Kp + 15) / 16;                     // EMU: 16-deep k-blocks of the score product
  constexpr bool GRAD = MODE == MODE_GRAD_R || MODE == MODE_GRAD_C || MODE == MODE_LSE_GRAD_R;
  constexpr bool FUSED = MODE == MODE_LSE_GRAD_R;
  constexpr int NPRE = (2 * KQ + 3) / 4;                 // 16-byte vectors each thread stages per step
  constexpr int kTpFloats = 2 * KB * 3 * 2 * kGs * 4, kTtFloats = GRAD ? 2 * 2 * FT * 3 * 2 * kGs * 4 : 0;      // EMU piece images
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ts = smem;                                      // [64][ldt]     streamed tile, row-major (A operand of the score product).  EMU: TP
  float* TsT = Ts + (EMU ? kTpFloats : kTs * ldt);       // [FT*32][68]   transposed (A operand of the second GEMM), GRAD only.  EMU: TT
  float* tlse = TsT + (EMU ? kTtFloats : (GRAD ? FT * 32 * kLdT : 0));       // [64]          GRAD_C: lse of the streamed queries
  float* tbias = tlse + kTs;                             // [64]          LOGQ, candidates stream: MINUS their bias
  IdT* tid = reinterpret_cast<IdT*>(tbias + (LOGQ_S ? kTs : 0));   // [64]          ids of the streamed entities
  float* tths = reinterpret_cast<float*>(tid + kTs);     // [64]          HARD GRAD_C: threshold score of the streamed queries
  int32_t* tthp = reinterpret_cast<int32_t*>(tths + kTs);   // [64]                      ... and column
  uint2* heap = reinterpret_cast<uint2*>(tid + kTs);     // [M][128]      THR: per owned row a min-heap of its M best keys, the worst at slot 0

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l32 = lane & 31, hb = lane >> 5;
  const int dim = a.dim;
  const int64_t own = (int64_t)blockIdx.x * kOwn + wave * 32 + l32;       // this lane's owned row
  const bool own_ok = own < a.n_r;
  const bool has_ids = a.own_ids != nullptr;
  const int64_t t_begin = (int64_t)blockIdx.y * a.t_per_split;
  const int64_t t_end = t_begin + a.t_per_split < a.n_t ? t_begin + a.t_per_split : a.n_t;

  // stationary operand: R[own][KH * hb + kk].  EMU: R[own][16 kb + 8 hb + j] as three bf16 pieces per k-block
  float rf[EMU ? 1 : KH];
  bf16x8 rh[EMU ? KB : 1], rm[EMU ? KB : 1], rl[EMU ? KB : 1];
  if constexpr (EMU) {
    const float* rp = a.R + (own_ok ? own : 0) * dim;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float e8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int k = 16 * kb + 8 * hb + j; e8[j] = (own_ok && k < dim) ? rp[k] : 0.f; }
      uint32_t ph[4], pm[4], pl[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) split3(e8[2 * q], e8[2 * q + 1], ph[q], pm[q], pl[q]);
      rh[kb] = frag8(ph); rm[kb] = frag8(pm); rl[kb] = frag8(pl);
    }
  } else {
    const float* rp = a.R + (own_ok ? own : 0) * dim;
    const bool v4 = (dim & 3) == 0 && (reinterpret_cast<uintptr_t>(a.R) & 15) == 0;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int k = KH * hb + 4 * q;
      if (v4) {
        const float4 t = (own_ok && k < dim) ? *reinterpret_cast<const float4*>(rp + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        rf[4 * q] = t.x; rf[4 * q + 1] = t.y; rf[4 * q + 2] = t.z; rf[4 * q + 3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) rf[4 * q + e] = (own_ok && k + e < dim) ? rp[k + e] : 0.f;
      }
    }
  }
  IdT own_id = (IdT)-1;
  float own_lse = 0.f;
  if (own_ok) {
    if (has_ids) own_id = reinterpret_cast<const IdT*>(a.own_ids)[own];
    if (MODE == MODE_GRAD_R) own_lse = a.lse_in[own];
  }
  LogqBias<LOGQ_O> ob;                                   // LOGQ, candidates own: MINUS the bias of this lane's candidate (k = 0: the lower lane half)
  if constexpr (LOGQ_O) { if (own_ok && hb == 0) ob.b = -a.bias[own]; }
  HardKey<HARD && MODE != MODE_GRAD_C> ok;               // HARD, queries own: the key of this row's last kept negative
  if constexpr (HARD && MODE != MODE_GRAD_C) {
    if (own_ok && (!LOGQ || a.thr_s)) { ok.ts = a.thr_s[own]; ok.tp = a.thr_p[own]; }
  }
  if constexpr (MODE == MODE_THR) {
    for (int idx = threadIdx.x; idx < a.M * kOwn; idx += 256) heap[idx] = make_uint2(__float_as_uint(-INFINITY), (uint32_t)kThrNone);
  }
  float run_m = -INFINITY, run_l = 0.f, diag_s = 0.f;    // LSE
  f32x16 gacc[GRAD ? FT : 1];
#pragma unroll
  for (int t = 0; t < (GRAD ? FT : 1); ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) gacc[t][r] = 0.f;
  if constexpr (EMU) {      // slots no step writes (features past Kp, the pad slot of every group) stay zero
    for (int idx = threadIdx.x; idx < kTpFloats + kTtFloats; idx += 256) Ts[idx] = 0.f;
  } else if (GRAD) {     // feature rows of the transposed tile that no step writes (Kp <= f < 32 FT) stay zero
    for (int idx = threadIdx.x; idx < (FT * 32 - Kp) * kLdT; idx += 256) TsT[Kp * kLdT + idx] = 0.f;
  }

  // staging: thread -> (streamed row sr = tid % 64, 16-byte feature chunks c4 = tid / 64 + 4 q): the transposed stores of a
  // wave hit 64 consecutive floats, the row-major ones 64 rows at a pitch of ldt floats (ldt % 64 in {36, 44, 60, 4}: conflict free)
  const int sr = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const bool tvec = (dim & 3) == 0 && (reinterpret_cast<uintptr_t>(a.T) & 15) == 0;
  float4 pre[NPRE];
  IdT pre_id = (IdT)-2;
  float pre_lse = 0.f;
  HardKey<HARD && MODE == MODE_GRAD_C> pk;               // HARD, candidates own: the key of the streamed query this thread stages
  LogqBias<LOGQ_S> pb;                                   // LOGQ, candidates stream: MINUS the bias of the candidate this thread stages
  auto fetch = [&](int64_t c0) {
    const int64_t gr = c0 + sr;
    const bool rin = gr < t_end;
    const float* tp = a.T + (rin ? gr : 0) * dim;
#pragma unroll
    for (int q = 0; q < NPRE; ++q) {
      const int c = 4 * (cg + 4 * q);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (tvec) {
        if (rin && c < dim) v = *reinterpret_cast<const float4*>(tp + c);
      } else if (rin) {
        v.x = c + 0 < dim ? tp[c + 0] : 0.f; v.y = c + 1 < dim ? tp[c + 1] : 0.f;
        v.z = c + 2 < dim ? tp[c + 2] : 0.f; v.w = c + 3 < dim ? tp[c + 3] : 0.f;
      }
      pre[q] = v;
    }
    if (cg == 0) {
      pre_id = (rin && has_ids) ? reinterpret_cast<const IdT*>(a.str_ids)[gr] : (IdT)-2;
      if (MODE == MODE_GRAD_C) pre_lse = rin ? a.lse_in[gr] : 0.f;
      if constexpr (HARD && MODE == MODE_GRAD_C) {
        const bool kin = rin && (!LOGQ || a.thr_s);
        pk.ts = kin ? a.thr_s[gr] : -INFINITY; pk.tp = kin ? a.thr_p[gr] : kThrNone;
      }
      if constexpr (LOGQ_S) pb.b = rin ? -a.bias[gr] : 0.f;
    }
  };
  if (t_begin < t_end) fetch(t_begin);

  // EMU: out^T[f][owned] += sum_k T[k][f] P[k][owned] for one 32-entity sub-tile whose P the lane holds in pv[0..15]: two 16-entity groups
  // (registers 8 g2 + j = k slot j), P split in registers, the A fragments (T^T pieces) from TT
  auto second_gemm_emu = [&](int sub, const float (&pv)[16]) {
    const float* tt = TsT + ((hb * kGs + l32) << 2);      // + ((((sub * 2 + g2) * FT + t) * 3 + p) * 2 * kGs) * 4
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2) {
      uint32_t ph[4], pm[4], pl[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) split3(pv[8 * g2 + 2 * q], pv[8 * g2 + 2 * q + 1], ph[q], pm[q], pl[q]);
      const bf16x8 wh = frag8(ph), wm = frag8(pm), wl = frag8(pl);
#pragma unroll
      for (int t = 0; t < (GRAD ? FT : 1); ++t) {
        bf16x8 x[3];
#pragma unroll
        for (int p3 = 0; p3 < 3; ++p3) x[p3] = frag8(*reinterpret_cast<const float4*>(tt + ((((((sub * 2 + g2) * FT + t) * 3 + p3) * 2) * kGs) << 2)));
        gacc[t] = mfma32x6(x[0], x[1], x[2], wh, wm, wl, gacc[t]);
      }
    }
  };
  // diagonal: streamed index of this lane's partner, as an offset into the current tile (compared against the tile-local index)
  const int64_t partner = own + a.diag;
  const int jb = 4 * hb;                                  // lane-half part of the tile-local streamed index
  for (int64_t c0 = t_begin; c0 < t_end; c0 += kTs) {
    __syncthreads();                                      // the previous step's readers of the tile are done
#pragma unroll
    for (int q = 0; q < NPRE; ++q) {
      const int c = 4 * (cg + 4 * q);
      if constexpr (EMU) {
        if (c < Kp) {
          uint32_t h0, m0, l0, h1, m1, l1;
          split3(pre[q].x, pre[q].y, h0, m0, l0);
          split3(pre[q].z, pre[q].w, h1, m1, l1);
          const int sub = sr >> 5, mm = sr & 31;
          {   // TP: features c..c+3 are slots j0..j0+3 of entity mm in k-block c / 16, lane half (c / 8) & 1
            const int slot = (((sub * KB + (c >> 4)) * 3) * 2 + ((c >> 3) & 1)) * kGs + mm;
            float* d = Ts + slot * 4 + ((c & 7) >> 1);
            *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(d + 2 * kGs * 4) = make_uint2(m0, m1);
            *reinterpret_cast<uint2*>(d + 4 * kGs * 4) = make_uint2(l0, l1);
          }
          if (GRAD) {   // TT: entity mm is slot j of lane half (mm / 4) & 1 in the 16-entity group mm / 16 - the register 8 g2 + j that holds it
            const int g2 = mm >> 4, hb2 = (mm >> 2) & 1, j = 4 * ((mm >> 3) & 1) + (mm & 3);
            uint16_t* tt = reinterpret_cast<uint16_t*>(TsT);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int f = c + e;
              const int slot = ((((sub * 2 + g2) * FT + (f >> 5)) * 3) * 2 + hb2) * kGs + (f & 31);
              uint16_t* d = tt + slot * 8 + j;
              const uint32_t vh = e < 2 ? h0 : h1, vm = e < 2 ? m0 : m1, vl = e < 2 ? l0 : l1;
              d[0] = (uint16_t)((e & 1) ? (vh >> 16) : (vh & 0xffffu));
              d[2 * kGs * 8] = (uint16_t)((e & 1) ? (vm >> 16) : (vm & 0xffffu));
              d[4 * kGs * 8] = (uint16_t)((e & 1) ? (vl >> 16) : (vl & 0xffffu));
            }
          }
        }
      } else
      if (c < Kp) {
        *reinterpret_cast<float4*>(Ts + sr * ldt + c) = pre[q];
        if (GRAD) {
          TsT[(c + 0) * kLdT + sr] = pre[q].x; TsT[(c + 1) * kLdT + sr] = pre[q].y;
          TsT[(c + 2) * kLdT + sr] = pre[q].z; TsT[(c + 3) * kLdT + sr] = pre[q].w;
        }
      }
    }
    if (cg == 0) {
      tid[sr] = pre_id;
      if (MODE == MODE_GRAD_C) tlse[sr] = pre_lse;
      if constexpr (HARD && MODE == MODE_GRAD_C) { tths[sr] = pk.ts; tthp[sr] = pk.tp; }
      if constexpr (LOGQ_S) tbias[sr] = pb.b;
    }
    __syncthreads();
    if (c0 + kTs < t_end) fetch(c0 + kTs);                // in flight during this step's MFMA work

    // ---- score tiles: D[m = streamed][n = owned], two sub-tiles interleaved ----
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
    if constexpr (EMU) {
      const float* tp = Ts + ((hb * kGs + l32) << 2);      // + (((sub * KB + kb) * 3 + p) * 2 * kGs) * 4
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        bf16x8 x0[3], x1[3];
#pragma unroll
        for (int p3 = 0; p3 < 3; ++p3) {
          x0[p3] = frag8(*reinterpret_cast<const float4*>(tp + ((((0 * KB + kb) * 3 + p3) * 2 * kGs) << 2)));
          x1[p3] = frag8(*reinterpret_cast<const float4*>(tp + ((((1 * KB + kb) * 3 + p3) * 2 * kGs) << 2)));
        }
        if constexpr (HARD && MODE == MODE_GRAD_C) {       // the streamed operand is the query here: the piece order of the query-owned sweeps
          s0 = mfma32x6m(x0[0], x0[1], x0[2], rh[kb], rm[kb], rl[kb], s0);
          s1 = mfma32x6m(x1[0], x1[1], x1[2], rh[kb], rm[kb], rl[kb], s1);
        } else {
          s0 = mfma32x6(x0[0], x0[1], x0[2], rh[kb], rm[kb], rl[kb], s0);
          s1 = mfma32x6(x1[0], x1[1], x1[2], rh[kb], rm[kb], rl[kb], s1);
        }
      }
    } else {
    const float* ap = Ts + l32 * ldt + KH * hb;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const float4 a0 = *reinterpret_cast<const float4*>(ap + 4 * q);
      const float4 a1 = *reinterpret_cast<const float4*>(ap + 32 * ldt + 4 * q);
      s0 = mfma32(a0.x, rf[4 * q + 0], s0); s1 = mfma32(a1.x, rf[4 * q + 0], s1);
      s0 = mfma32(a0.y, rf[4 * q + 1], s0); s1 = mfma32(a1.y, rf[4 * q + 1], s1);
      s0 = mfma32(a0.z, rf[4 * q + 2], s0); s1 = mfma32(a1.z, rf[4 * q + 2], s1);
      s0 = mfma32(a0.w, rf[4 * q + 3], s0); s1 = mfma32(a1.w, rf[4 * q + 3], s1);
    }
    }
    // LOGQ: x = s - b on the FINISHED dot products, one fp32 rounding per score, the same in every sweep and in both bodies: one more
    // fp32 MFMA per sub-tile after the products, with the operand pair (-b, 1) at k = 0 and (0, 1) at k = 1 - the products are exact, so
    // the accumulator takes fl(s - b).  -b of a streamed candidate is one LDS word per lane (A operand: m = streamed entity = l32), of an
    // owned one the lane's register (B operand: n = owned row = l32), both zero in the upper lane half (k = 1): nothing is added to the
    // registers of the score loops below, which read x where they read s without the correction.
    if constexpr (LOGQ_S) {
      const float nb0 = hb == 0 ? tbias[l32] : 0.f, nb1 = hb == 0 ? tbias[32 + l32] : 0.f;
      s0 = mfma32(nb0, 1.f, s0); s1 = mfma32(nb1, 1.f, s1);
    }
    if constexpr (LOGQ_O) { s0 = mfma32(1.f, ob.b, s0); s1 = mfma32(1.f, ob.b, s1); }
    if (MODE == MODE_SCORES) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t gs = c0 + 32 * sub + 8 * (r >> 2) + jb + (r & 3);
          if (gs < t_end && own_ok) a.out[gs * a.ldo + own] = sub ? s1[r] : s0[r];
        }
      continue;
    }
    const int dd = (int)((partner - c0 < -1) ? -1 : (partner - c0 > 4096 ? 4096 : partner - c0)) - jb;   // tile-local diag index minus jb
    // HARD, queries own: tile-local column of the threshold key minus jb (a column at the threshold score is kept up to it)
    if constexpr (HARD && MODE != MODE_GRAD_C) {
      const int64_t t = (int64_t)ok.tp - c0;
      ok.tl = (int)(t < -1 ? -1 : (t > 4096 ? 4096 : t)) - jb;
    }
    if constexpr (MODE == MODE_THR) {
      const int lim = (int)(t_end - c0) - jb;
      float v[32];                                        // the masked scores of this lane's 32 columns; NaN = not a negative (partner, past the end)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          IdT ids4[4];
          if (has_ids) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ids4[e] = tid[32 * sub + 8 * rq + jb + e];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int cj = 32 * sub + 8 * rq + e;
            float x = sub ? s1[4 * rq + e] : s0[4 * rq + e];
            const bool dg = cj == dd;
            if (has_ids) x += (!dg && ids4[e] == own_id) ? kMinFloat : 0.f;
            v[16 * sub + 4 * rq + e] = (cj < lim && !dg) ? x : __builtin_nanf("");
          }
        }
      // the two lane halves of a row share its heap: one half at a time (a wave runs in lockstep, so the halves' updates are
      // ordered); each half starts from the heap's current worst key and keeps it in registers, so a score that does not
      // beat it costs the compares alone
      const int hrow = wave * 32 + l32;
      const int cb = (int)c0 + jb;
#pragma unroll 1
      for (int ph = 0; ph < 2; ++ph) {
        if (hb == ph && own_ok) {
          uint2 root = heap[hrow];
          float ts = __uint_as_float(root.x);
          int tj = (int)root.y;
          // the scores that beat the key as it stands (a superset of those that will: it only rises), one bit each; then every lane
          // inserts ITS candidates in a loop of its own, so a tile costs the wave max-over-lanes sifts, not one per score slot
          // in which any lane inserts.  (The kept set does not depend on the order of insertion.)
          uint32_t todo = 0;
#pragma unroll
          for (int i = 0; i < 32; ++i) {
            const int col = cb + 32 * (i >> 4) + 8 * ((i & 15) >> 2) + (i & 3);
            todo |= (v[i] > ts || (v[i] == ts && col < tj)) ? (1u << i) : 0u;
          }
          while (todo) {
            const int i = __ffs(todo) - 1;
            todo &= todo - 1;
            float x = v[0];
#pragma unroll
            for (int k = 1; k < 32; ++k) x = (k == i) ? v[k] : x;
            const int col = cb + 32 * (i >> 4) + 8 * ((i & 15) >> 2) + (i & 3);
            if (x > ts || (x == ts && col < tj)) {        // beats the worst kept key: it leaves, the new key sifts down from the root
              int k = 0;
              for (;;) {
                int ch = 2 * k + 1;
                if (ch >= a.M) break;
                uint2 kc = heap[ch * kOwn + hrow];
                if (ch + 1 < a.M) {
                  const uint2 k2 = heap[(ch + 1) * kOwn + hrow];
                  if (key_worse(__uint_as_float(k2.x), (int)k2.y, __uint_as_float(kc.x), (int)kc.y)) { kc = k2; ch = ch + 1; }
                }
                if (!key_worse(__uint_as_float(kc.x), (int)kc.y, x, col)) break;
                heap[k * kOwn + hrow] = kc;
                k = ch;
              }
              heap[k * kOwn + hrow] = make_uint2(__float_as_uint(x), (uint32_t)col);
              root = heap[hrow];
              ts = __uint_as_float(root.x);
              tj = (int)root.y;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      continue;
    }
    if (MODE == MODE_LSE) {
      const int lim = (int)(t_end - c0) - jb;             // tile-local validity bound (only the last tile is partial)
      float v[32];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          IdT ids4[4];
          if (has_ids) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ids4[e] = tid[32 * sub + 8 * rq + jb + e];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int cj = 32 * sub + 8 * rq + e;         // tile-local streamed index minus jb
            float x = sub ? s1[4 * rq + e] : s0[4 * rq + e];
            const bool dg = cj == dd;
            if (has_ids) x += (!dg && ids4[e] == own_id) ? kMinFloat : 0.f;
            diag_s = dg ? x : diag_s;
            if constexpr (HARD && MODE != MODE_GRAD_C) x = (dg || x > ok.ts || (x == ok.ts && cj <= ok.tl)) ? x : -INFINITY;
            v[16 * sub + 4 * rq + e] = cj < lim ? x : -INFINITY;
          }
        }
      float m = v[0];
#pragma unroll
      for (int i = 1; i < 32; ++i) m = fmaxf(m, v[i]);
      const float nm = fmaxf(run_m, m);                   // > -inf: every tile has at least one valid entity
      if constexpr (HARD) {                               // ... but not necessarily a kept one: nothing kept so far leaves (-inf, 0)
        const float ne = nm > -INFINITY ? nm : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) sum += exp_hw(v[i] - ne);
        run_l = run_l * exp_hw(run_m - ne) + sum;
        run_m = nm;
        continue;
      }
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) sum += exp_hw(v[i] - nm);
      run_l = run_l * exp_hw(run_m - nm) + sum;
      run_m = nm;
      continue;
    }
    if (FUSED) {
      // ---- online softmax + dQ accumulator relative to the running maximum ----
      float v[32];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          IdT ids4[4];
          if (has_ids) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ids4[e] = tid[32 * sub + 8 * rq + jb + e];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int cj = 32 * sub + 8 * rq + e;
            float x = sub ? s1[4 * rq + e] : s0[4 * rq + e];
            const bool dg = cj == dd;
            if (has_ids) x += (!dg && ids4[e] == own_id) ? kMinFloat : 0.f;
            diag_s = dg ? x : diag_s;
            if constexpr (HARD && MODE != MODE_GRAD_C) x = (dg || x > ok.ts || (x == ok.ts && cj <= ok.tl)) ? x : -INFINITY;
            v[16 * sub + 4 * rq + e] = cj < (int)(t_end - c0) - jb ? x : -INFINITY;
          }
        }
      float m = v[0];
#pragma unroll
      for (int i = 1; i < 32; ++i) m = fmaxf(m, v[i]);
      m = fmaxf(m, __shfl_xor(m, 32, 64));               // both lane halves of an owned row feed the same accumulator: one maximum
      const float nm = fmaxf(run_m, m);                   // > -inf: every tile has at least one valid entity
      const float ne = (HARD && !(nm > -INFINITY)) ? 0.f : nm;   // HARD: ... but not necessarily a kept one (then every term below is 0)
      const float sc = exp_hw(run_m - ne);                // 0 on the first step (run_m = -inf)
      run_m = nm;
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) { v[i] = exp_hw(v[i] - ne); sum += v[i]; }
      run_l = run_l * sc + sum;
#pragma unroll
      for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) gacc[t][r] *= sc;
      if constexpr (EMU) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          float pv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) pv[r] = v[16 * sub + r];
          second_gemm_emu(sub, pv);
        }
        continue;
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int j0 = 32 * sub + 8 * rq + jb;
#pragma unroll
          for (int t = 0; t < FT; ++t) {
            const float4 a4 = *reinterpret_cast<const float4*>(TsT + (32 * t + l32) * kLdT + j0);
            gacc[t] = mfma32(a4.x, v[16 * sub + 4 * rq + 0], gacc[t]);
            gacc[t] = mfma32(a4.y, v[16 * sub + 4 * rq + 1], gacc[t]);
            gacc[t] = mfma32(a4.z, v[16 * sub + 4 * rq + 2], gacc[t]);
            gacc[t] = mfma32(a4.w, v[16 * sub + 4 * rq + 3], gacc[t]);
          }
        }
      continue;
    }
    // ---- GRAD: P in registers -> B operand of out^T[f][owned] += sum_k T[k][f] P[k][owned] ----
    // (streamed rows past the end and owned rows past the end need no mask: their T rows are zero / their results are not stored)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      float pv[16];
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int j0 = 32 * sub + 8 * rq + jb;
        IdT ids4[4];
        float l4[4];
        if (has_ids) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ids4[e] = tid[j0 + e];
        }
        if (MODE == MODE_GRAD_C) {
          const float4 t = *reinterpret_cast<const float4*>(tlse + j0);
          l4[0] = t.x; l4[1] = t.y; l4[2] = t.z; l4[3] = t.w;
        }
        HardKeys4<HARD && MODE == MODE_GRAD_C> k4;
        if constexpr (HARD && MODE == MODE_GRAD_C) {
          const float4 t = *reinterpret_cast<const float4*>(tths + j0);
          const int4 u = *reinterpret_cast<const int4*>(tthp + j0);
          k4.ts[0] = t.x; k4.ts[1] = t.y; k4.ts[2] = t.z; k4.ts[3] = t.w;
          k4.tp[0] = u.x; k4.tp[1] = u.y; k4.tp[2] = u.z; k4.tp[3] = u.w;
        }
        float p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int cj = 32 * sub + 8 * rq + e;
          float x = sub ? s1[4 * rq + e] : s0[4 * rq + e];
          const bool dg = cj == dd;
          if (has_ids) x += (!dg && ids4[e] == own_id) ? kMinFloat : 0.f;
          if constexpr (HARD && MODE == MODE_GRAD_C) x = (dg || x > k4.ts[e] || (x == k4.ts[e] && own + a.col0 <= (int64_t)k4.tp[e])) ? x : -INFINITY;   // this lane's candidate in the streamed query's kept set
          else if constexpr (HARD) x = (dg || x > ok.ts || (x == ok.ts && cj <= ok.tl)) ? x : -INFINITY;
          p[e] = exp_hw(x - (MODE == MODE_GRAD_R ? own_lse : l4[e])) - (dg ? 1.f : 0.f);
          pv[4 * rq + e] = p[e];
        }
        if constexpr (!EMU) {
#pragma unroll
          for (int t = 0; t < FT; ++t) {
            const float4 a4 = *reinterpret_cast<const float4*>(TsT + (32 * t + l32) * kLdT + j0);
            gacc[t] = mfma32(a4.x, p[0], gacc[t]);
            gacc[t] = mfma32(a4.y, p[1], gacc[t]);
            gacc[t] = mfma32(a4.z, p[2], gacc[t]);
            gacc[t] = mfma32(a4.w, p[3], gacc[t]);
          }
        }
      }
      if constexpr (EMU) second_gemm_emu(sub, pv);
    }
  }

  if constexpr (MODE == MODE_THR) {
    // a row with at most M negatives cuts nothing; otherwise slot 0 of its heap is the M-th best key of this split's columns
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (a.lists) {
      const int64_t ns = gridDim.y;
      for (int r = 0; r < 32; ++r) {
        const int64_t row = (int64_t)blockIdx.x * kOwn + wave * 32 + r;
        if (row >= a.n_r) break;
        for (int k = lane; k < a.M; k += 64) a.lists[(row * ns + blockIdx.y) * a.M + k] = heap[k * kOwn + wave * 32 + r];
      }
    } else if (hb == 0 && own_ok) {
      const int64_t n_neg = a.n_t - ((partner >= 0 && partner < a.n_t) ? 1 : 0);
      const uint2 root = heap[wave * 32 + l32];
      a.thr_s_out[own] = n_neg > a.M ? __uint_as_float(root.x) : -INFINITY;
      a.thr_p_out[own] = n_neg > a.M ? (int32_t)root.y : kThrNone;
    }
    return;
  }
  if (FUSED) {
    // run_m is already common to the two lane halves of a row; l and the diagonal score are per half
    const float l = run_l + __shfl_xor(run_l, 32, 64);
    const float d = diag_s + __shfl_xor(diag_s, 32, 64);
    const bool v4 = (a.ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0 && (dim & 3) == 0 && (reinterpret_cast<uintptr_t>(a.T) & 15) == 0;
    if (a.part) {                                         // split: unnormalised accumulator slab + (max, sum, diag) per row
      if (hb == 0 && own_ok) {
        const int64_t ns = gridDim.y;
        a.part[(0 * ns + blockIdx.y) * a.n_r + own] = run_m;
        a.part[(1 * ns + blockIdx.y) * a.n_r + own] = l;
        a.part[(2 * ns + blockIdx.y) * a.n_r + own] = d;
      }
    } else {
      const float lse = run_m + logf(l);
      double part = 0.0;
      if (hb == 0 && own_ok) { a.lse_out[own] = lse; part = (double)lse - (double)d; }
      part = wave_sum_d(part);
      __shared__ double red[4];
      if (lane == 0) red[wave] = part;
      __syncthreads();
      if (threadIdx.x == 0 && a.loss_sum) atomicAdd(a.loss_sum + (blockIdx.x & (BR_SUM_SLOTS - 1)), red[0] + red[1] + red[2] + red[3]);
    }
    const float inv_l = a.part ? 1.f : 1.f / l;           // direct: dQ = acc / l - C[diag]
    const int64_t partner_row = own + a.diag;
    const bool has_diag = !a.part && partner_row >= 0 && partner_row < a.n_t;
    float* op = a.out + ((int64_t)blockIdx.y * a.n_r + (own_ok ? own : 0)) * a.ldo;
    const float* cp = a.T + (has_diag ? partner_row : 0) * dim;
#pragma unroll
    for (int t = 0; t < FT; ++t)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int f = 32 * t + 8 * rq + jb;
        if (!own_ok || f >= dim) continue;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = gacc[t][4 * rq + e] * inv_l - ((has_diag && f + e < dim) ? cp[f + e] : 0.f);
        if (v4 && f + 3 < dim) {
          *reinterpret_cast<float4*>(op + f) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (f + e < dim) op[f + e] = o[e];
        }
      }
    return;
  }
  if (MODE == MODE_LSE) {
    // lanes l and l + 32 hold disjoint streamed entities of the same owned row
    const float om = __shfl_xor(run_m, 32, 64), ol = __shfl_xor(run_l, 32, 64), od = __shfl_xor(diag_s, 32, 64);
    const float nm = fmaxf(run_m, om);
    const float l = (run_m > -INFINITY ? run_l * exp_hw(run_m - nm) : 0.f) + (om > -INFINITY ? ol * exp_hw(om - nm) : 0.f);
    const float d = diag_s + od;                          // exactly one lane-step saw the diagonal (others hold 0)
    double part = 0.0;
    if (hb == 0 && own_ok) {
      if (a.part) {
        const int64_t ns = gridDim.y;
        a.part[(0 * ns + blockIdx.y) * a.n_r + own] = nm;
        a.part[(1 * ns + blockIdx.y) * a.n_r + own] = l;
        a.part[(2 * ns + blockIdx.y) * a.n_r + own] = d;
      } else {
        const float lse = nm + logf(l);
        a.lse_out[own] = lse;
        part = (double)lse - (double)d;
      }
    }
    if (!a.part) {
      part = wave_sum_d(part);
      __shared__ double red[4];
      if (lane == 0) red[wave] = part;
      __syncthreads();
      if (threadIdx.x == 0 && a.loss_sum) atomicAdd(a.loss_sum + (blockIdx.x & (BR_SUM_SLOTS - 1)), red[0] + red[1] + red[2] + red[3]);
    }
    return;
  }
  if (GRAD) {
    // gacc[t][r] = out[own][32 t + 8 (r / 4) + 4 hb + r % 4]: four consecutive features per register group
    float* op = a.out + ((int64_t)blockIdx.y * a.n_r + (own_ok ? own : 0)) * a.ldo;
    const bool v4 = (a.ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
#pragma unroll
    for (int t = 0; t < FT; ++t)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int f = 32 * t + 8 * rq + jb;
        if (!own_ok || f >= dim) continue;
        if (v4 && f + 3 < dim) {
          *reinterpret_cast<float4*>(op + f) = make_float4(gacc[t][4 * rq], gacc[t][4 * rq + 1], gacc[t][4 * rq + 2], gacc[t][4 * rq + 3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (f + e < dim) op[f + e] = gacc[t][4 * rq + e];
        }
      }
  }
}


// ---- launchers of MODE_THR and the HARD forms (ArgsT = InbatchHardArgs, or InbatchLogqArgs for their LOGQ forms) ----
template <int MODE, int KQ, typename IdT, bool EMU, bool HARD, typename ArgsT>
void launch_hard_e(const ArgsT& a, int n_split, hipStream_t s) {
  constexpr int Kp = 8 * KQ, FT = (Kp + 31) / 32, KB = (Kp + 15) / 16;
  constexpr bool GRAD = MODE == MODE_GRAD_R || MODE == MODE_GRAD_C || MODE == MODE_LSE_GRAD_R;
  constexpr bool LOGQ_S = std::is_same<ArgsT, InbatchLogqArgs>::value && MODE != MODE_GRAD_C;
  const size_t img = EMU ? (size_t)2 * KB * 3 * 2 * kGs * 4 + (GRAD ? (size_t)2 * 2 * FT * 3 * 2 * kGs * 4 : 0)
                         : (size_t)kTs * (Kp + 4) + (GRAD ? (size_t)FT * 32 * kLdT : 0);
  const size_t extra = MODE == MODE_THR ? (size_t)a.M * kOwn * sizeof(uint2) : (MODE == MODE_GRAD_C ? (size_t)kTs * 8 : 0);   // the heaps / the streamed thresholds
  const size_t shmem = (img + kTs + (LOGQ_S ? kTs : 0)) * sizeof(float) + kTs * sizeof(IdT) + extra;      // LOGQ_S: the streamed candidates' bias
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)inbatch_kernel<MODE, KQ, IdT, EMU, HARD, ArgsT>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr = true;
  }
  const dim3 grid((unsigned)ceil_div(a.n_r, (int64_t)kOwn), (unsigned)n_split);
  inbatch_kernel<MODE, KQ, IdT, EMU, HARD, ArgsT><<<grid, 256, shmem, s>>>(a);
}
template <int MODE, int KQ, typename IdT, bool HARD, typename ArgsT>
void launch_hard_k(const ArgsT& a, int n_split, bool emu, hipStream_t s) {
  if constexpr (KQ <= 8) {
    if (emu) { launch_hard_e<MODE, KQ, IdT, true, HARD>(a, n_split, s); return; }
  }
  launch_hard_e<MODE, KQ, IdT, false, HARD>(a, n_split, s);
}
template <int MODE, typename IdT, bool HARD, typename ArgsT>
void launch_hard_t(const ArgsT& a, int n_split, bool emu, hipStream_t s) {
  const int kq = (a.dim + 7) / 8;
  if (kq <= 4) launch_hard_k<MODE, 4, IdT, HARD>(a, n_split, emu, s);
  else if (kq <= 7) launch_hard_k<MODE, 7, IdT, HARD>(a, n_split, emu, s);
  else if (kq <= 8) launch_hard_k<MODE, 8, IdT, HARD>(a, n_split, emu, s);
  else if (kq <= 13) launch_hard_k<MODE, 13, IdT, HARD>(a, n_split, emu, s);
  else launch_hard_k<MODE, 16, IdT, HARD>(a, n_split, emu, s);
}
// emu: hard_emu of the CALL (not of this sweep's streamed length)
template <int MODE, typename ArgsT>
void launch_hard(ArgsT a, int n_split, int id_type, bool emu, hipStream_t s) {
  constexpr bool HARD = MODE != MODE_THR;
  const int64_t steps = ceil_div(a.n_t, (int64_t)kTs);
  a.t_per_split = ceil_div(steps, (int64_t)n_split) * kTs;
  n_split = (int)ceil_div(a.n_t, a.t_per_split);       // no empty split
  if (id_type == BR_IDS_I64) launch_hard_t<MODE, int64_t, HARD>(a, n_split, emu, s);
  else launch_hard_t<MODE, int32_t, HARD>(a, n_split, emu, s);
}
// the LOGQ forms are instantiated in softmax_logq.hip (a translation unit of their own: they are as much device code as the HARD forms)
template <int MODE>
void launch_logq(const InbatchLogqArgs& a, int n_split, int id_type, bool emu, hipStream_t s);
}  // namespace br
