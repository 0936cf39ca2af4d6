// Per-step negative sampling for the BPR fit (brBprSampleNegatives, include/binrec.h): one launch BESIDE the step that draws, for
// every triplet of the batch, M candidate negatives (uniform over the candidates or by Walker's alias table), rejects the customer's
// positives as bpr_triplets_kernel (sampling.hip) does and - M > 1, dynamic negative sampling - scores every candidate against the
// customer's row with the CURRENT model and keeps the hardest.  It stands in for src/models/BPRModel.py:94-98,111-119 like
// brBprSampleTriplets, but per step.
//
// "Current model" on deferred tables = the stored rows replayed over the steps (last[row], ss->step] in registers,
// exactly what the step's own lookup does next (gather_deferred_wave_row with step_add = 1, lookup_wave.h); nothing is written back.
// The composed form (ids, brGatherRowsDeferred into a B*M x dim buffer, dot, argmax) writes and re-reads that buffer for nothing.
//
// Shape: one wave per triplet, four per workgroup, wave-uniform control flow.  The launch is bound by its chains of dependent round
// trips (ids -> positives -> last[] -> rows), not by bytes, so everything is requested as early as it can be: the customer's row
// (last[], then theta, m, v) before the draw; lanes 0..M-1 then draw and reject their candidate in parallel (the one divergent part),
// each against the customer's positives fetched once, and fetch their candidate's last[] beside the rejection test; every id and
// last[] is then made wave-uniform by a readlane.  Candidates go in groups of R: the theta (and m, v) loads of R rows are all requested
// before the first replay (lookup_wave.h gather_deferred_wave_rows says why), the customer's replay runs behind the first group's.
// Rows of 64 * VEC floats (VEC = 1, 2, 4) are one vector per lane; every other dim is a loop of 64-float chunks per lane, where the
// lanes past the row's end carry zeros through the replay (the uniform helpers ballot and assume a converged wave) and the
// customer's chunk is replayed again for every group (the rare path: no per-dim register or LDS image of the row).
// The dot is a per-lane chain of fused multiply-adds in column order, then a fixed xor-shuffle tree: a (dim, inputs) pair always gives
// the same bits, whichever table form (deferred / swept) holds the rows.
#include "common.h"
#include "rows.h"
#include "adam_math.h"
#include "philox.h"
#include "sampling.h"

namespace br {

struct DrawArgs {
  const int64_t* pos_off; const void* pos_items; int64_t num_users;
  const void* cand; const uint32_t* thresh; const int32_t* alias; uint32_t n_cand;
  uint64_t seed; uint32_t step; uint32_t pos0; int max_tries;
};
struct SampleTable { const float* tab; const float* m; const float* v; const int32_t* last; int64_t rows; };
struct SampleArgs {
  DrawArgs d;
  const void* users; int64_t batch; int M;
  SampleTable user, item;
  const StepStateDev* ss; AdamHp h; int dim;
  void* out_neg; void* out_cands; float* out_scores; int* err;
};

// candidate j of position c0: attempt a takes Philox(c0, j * 256 + a, stream 5, draw step); the last attempt stands.  last != NULL: also
// -> seen = last[id] of the candidate that stands (0 and the RANGE flag for an id outside [0, rows)), requested BEFORE the rejection test
// of its attempt, which it does not depend on.
template <typename IdT>
__device__ __forceinline__ int64_t draw_candidate(const DrawArgs& a, int64_t user, uint32_t c0, uint32_t j, int* err, const int32_t* __restrict__ last = nullptr,
                                                  int64_t rows = 0, uint32_t* seen = nullptr) {
  Positives<IdT> pos;
  pos.load(a.pos_off, (const IdT*)a.pos_items, user);
  int64_t id = 0;
  for (int t = 0; t < a.max_tries; ++t) {
    const Philox4 d = philox4x32_10(c0, j * 256u + (uint32_t)t, 5u, a.step, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    id = candidate_of<IdT>(d, a.cand, a.thresh, a.alias, a.n_cand, err);
    if (last) *seen = (uint32_t)last[(uint64_t)id < (uint64_t)rows ? id : 0];
    if (!pos.has((IdT)id)) break;
  }
  return id;
}

// M == 1: no table is read - one thread per triplet
template <typename IdT>
__global__ __launch_bounds__(256) void bpr_sample_one_kernel(const DrawArgs a, const IdT* __restrict__ users, int64_t batch, IdT* __restrict__ out_neg,
                                                             IdT* __restrict__ out_cands, float* __restrict__ out_scores, int* err) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  int64_t u = (int64_t)users[b];
  if ((uint64_t)u >= (uint64_t)a.num_users) { if (err) atomicOr(err, BR_ERRFLAG_RANGE); u = 0; }
  const IdT id = (IdT)draw_candidate<IdT>(a, u, a.pos0 + (uint32_t)b, 0u, err);
  out_neg[b] = id;
  if (out_cands) out_cands[b] = id;
  if (out_scores) out_scores[b] = 0.f;
}

__device__ __forceinline__ float fma_chain(float acc, float4 a, float4 b) {
  return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, __builtin_fmaf(a.x, b.x, acc))));
}
__device__ __forceinline__ float fma_chain(float acc, float2 a, float2 b) { return __builtin_fmaf(a.y, b.y, __builtin_fmaf(a.x, b.x, acc)); }
__device__ __forceinline__ float fma_chain(float acc, float a, float b) { return __builtin_fmaf(a, b, acc); }

// M > 1.  CHUNKED = false: dim == 64 * VEC.  CHUNKED = true: VEC == 1, any dim, 64 floats per pass.
template <typename IdT, int VEC, int R, bool CHUNKED>
__global__ __launch_bounds__(256) void bpr_sample_hard_kernel(const SampleArgs a) {
  using V = typename VecT<VEC>::type;
  static_assert(!CHUNKED || VEC == 1, "chunk loop: one float per lane and pass");
  const int64_t b = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= a.batch) return;
  const int lane = (int)(threadIdx.x & 63);
  const int M = a.M, dim = a.dim;
  const StepStateDev* __restrict__ ss = a.ss;
  const bool deferred = a.user.m != nullptr;
  const uint32_t done = deferred ? ss->step : 0u;         // the last completed step: rows must include steps <= done

  int64_t u = load_id((const IdT*)a.users, b);
  const bool u_csr = (uint64_t)u < (uint64_t)a.d.num_users, u_tab = (uint64_t)u < (uint64_t)a.user.rows;
  if (!(u_csr && u_tab) && a.err && lane == 0) atomicOr(a.err, BR_ERRFLAG_RANGE);
  const int64_t u_draw = u_csr ? u : 0;
  if (!u_tab) u = 0;
  // the customer's row is requested BEFORE the draw: its round trips (last[], then theta, m, v) run beside those of the rejection test
  const uint32_t u_seen = deferred ? (uint32_t)a.user.last[u] : done;
  const bool u_lag = u_seen < done;
  const int passes = CHUNKED ? (dim + 63) >> 6 : 1;
  V ur = vzero<VEC>(), um = vzero<VEC>(), uv = vzero<VEC>();
  if constexpr (!CHUNKED) {
    const int64_t uo = u * dim + lane * VEC;
    ur = vload<VEC>(a.user.tab + uo);
    if (u_lag) { um = vload<VEC>(a.user.m + uo); uv = vload<VEC>(a.user.v + uo); }
  }
  // the one divergent part: lanes 0..M-1 draw and reject their candidate, and fetch its last[] (one load for all M candidates)
  int64_t mine = 0, drawn = 0;
  uint32_t mine_seen = done;
  if (lane < M) {
    mine = draw_candidate<IdT>(a.d, u_draw, a.d.pos0 + (uint32_t)b, (uint32_t)lane, a.err, deferred ? a.item.last : nullptr, a.item.rows, &mine_seen);
    drawn = mine;
    if (a.out_cands) ((IdT*)a.out_cands)[b * M + lane] = (IdT)mine;
    if ((uint64_t)mine >= (uint64_t)a.item.rows) { if (a.err) atomicOr(a.err, BR_ERRFLAG_RANGE); mine = -1; }      // scored as row 0 (mine < 0 below)
  }
  const int id_lo = (int)(uint32_t)mine, id_hi = (int)(uint32_t)((uint64_t)mine >> 32), id_seen = (int)mine_seen;

  float best = -__builtin_inff();
  int best_j = 0;
  for (int g = 0; g < M; g += R) {
    int64_t row[R];
    uint32_t seen[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {          // candidates past M repeat the last one (cached rows; their scores are dropped)
      const int j = g + q < M ? g + q : M - 1;
      row[q] = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(id_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(id_lo, j));
      if (row[q] < 0) row[q] = 0;          // an id outside the table (flagged by its lane)
      seen[q] = (uint32_t)__builtin_amdgcn_readlane(id_seen, j);
    }
    float acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.f;
    for (int p = 0; p < passes; ++p) {
      const int col = CHUNKED ? p * 64 + lane : lane * VEC;
      const bool in = !CHUNKED || col < dim;
      if constexpr (CHUNKED) {
        const int64_t uo = u * dim + col;
        ur = in ? vload<VEC>(a.user.tab + uo) : vzero<VEC>();
        um = vzero<VEC>(); uv = vzero<VEC>();
        if (u_lag && in) { um = vload<VEC>(a.user.m + uo); uv = vload<VEC>(a.user.v + uo); }
      }
      V th[R], m[R], v[R];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int64_t off = row[q] * dim + col;
        th[q] = in ? vload<VEC>(a.item.tab + off) : vzero<VEC>();
        m[q] = vzero<VEC>(); v[q] = vzero<VEC>();
        if (seen[q] < done && in) { m[q] = vload<VEC>(a.item.m + off); v[q] = vload<VEC>(a.item.v + off); }
      }
      // the customer's row (its chunk) is replayed behind the group's requests: they are in flight meanwhile
      if (u_lag && (CHUNKED || g == 0)) adam_catch_up_uniform_percall<false>(ur, um, uv, u_seen, done, ss, a.h);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (seen[q] < done) adam_catch_up_uniform_percall<false>(th[q], m[q], v[q], seen[q], done, ss, a.h);
        acc[q] = fma_chain(acc[q], ur, th[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float s = acc[q];
      s += __shfl_xor(s, 32, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 4, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 1, 64);
      const float sc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, s)));
      const int j = g + q;
      if (j < M) {
        if (a.out_scores && lane == 0) a.out_scores[b * M + j] = sc;
        if (sc > best) { best = sc; best_j = j; }          // the first strict maximum; a NaN never compares greater
      }
    }
  }
  if (lane == best_j) ((IdT*)a.out_neg)[b] = (IdT)drawn;      // the id as drawn (also where it lies outside the table)
}

}  // namespace br

using namespace br;

extern "C" int brBprSampleNegatives(const void* users, int id_type, int64_t batch, int64_t pos0, uint32_t draw_step, const int64_t* pos_off,
                                    const void* pos_items, int64_t num_users, const void* cand_items, int64_t n_cand, const uint32_t* alias_thresh,
                                    const int32_t* alias_slot, uint64_t seed, int n_candidates, int max_tries, const float* user_table,
                                    const float* user_m, const float* user_v, const int32_t* user_last, int64_t user_rows, const float* item_table,
                                    const float* item_m, const float* item_v, const int32_t* item_last, int64_t item_rows, int dim,
                                    const void* step_state, double beta1, double beta2, double eps, void* out_neg, void* out_cands,
                                    float* out_scores, int* err_flag, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brBprSampleNegatives: bad id_type");
  BR_CHECK_ARG(n_candidates >= 1 && n_candidates <= 32, "brBprSampleNegatives: n_candidates %d out of [1, 32]", n_candidates);
  BR_CHECK_ARG(max_tries >= 1 && max_tries <= 256, "brBprSampleNegatives: max_tries %d out of [1, 256]", max_tries);
  BR_CHECK_ARG(batch >= 0 && batch < ((int64_t)1 << 31) && pos0 >= 0 && num_users >= 1 && n_cand >= 1 && n_cand < ((int64_t)1 << 32),
               "brBprSampleNegatives: bad sizes");
  BR_CHECK_ARG((alias_thresh == nullptr) == (alias_slot == nullptr), "brBprSampleNegatives: alias_thresh and alias_slot: both or neither");
  const bool hard = n_candidates > 1;
  if (hard) {
    BR_CHECK_ARG(user_table && item_table && user_rows > 0 && item_rows > 0 && dim >= 1, "brBprSampleNegatives: n_candidates > 1 scores the candidates: tables required");
    const bool any = user_m || user_v || user_last || item_m || item_v || item_last;
    const bool all = user_m && user_v && user_last && item_m && item_v && item_last && step_state;
    BR_CHECK_ARG(!any || all, "brBprSampleNegatives: deferred tables need m, v, last of both tables and the step state; current tables none of them");
  }
  if (batch == 0) return BR_OK;
  BR_CHECK_ARG(users && pos_off && pos_items && out_neg, "brBprSampleNegatives: null pointer");
  const DrawArgs d{pos_off, pos_items, num_users, cand_items, alias_thresh, alias_slot, (uint32_t)n_cand, seed, draw_step, (uint32_t)pos0, max_tries};
  hipStream_t s = (hipStream_t)stream;
  if (!hard) {
    BR_DISPATCH_ID(id_type, (bpr_sample_one_kernel<IdT><<<(unsigned)ceil_div(batch, 256), 256, 0, s>>>(d, (const IdT*)users, batch, (IdT*)out_neg, (IdT*)out_cands, out_scores, err_flag)));
    BR_CHECK_LAUNCH("brBprSampleNegatives");
    return BR_OK;
  }
  SampleArgs a{};
  a.d = d; a.users = users; a.batch = batch; a.M = n_candidates;
  a.user = SampleTable{user_table, user_m, user_v, user_last, user_rows};
  a.item = SampleTable{item_table, item_m, item_v, item_last, item_rows};
  a.ss = (const StepStateDev*)step_state; a.h = make_hp(0.0, beta1, beta2, eps); a.dim = dim;
  a.out_neg = out_neg; a.out_cands = out_cands; a.out_scores = out_scores; a.err = err_flag;
  const unsigned grid = (unsigned)ceil_div(batch, 4);
  // R = 4 candidates whose loads are in flight together: 62 registers, 8 waves per SIMD at dim 64
  constexpr int R = 4;
  const int wvec = wave_row_vec(dim);
  const uintptr_t al = reinterpret_cast<uintptr_t>(user_table) | reinterpret_cast<uintptr_t>(item_table) | reinterpret_cast<uintptr_t>(user_m) |
                       reinterpret_cast<uintptr_t>(user_v) | reinterpret_cast<uintptr_t>(item_m) | reinterpret_cast<uintptr_t>(item_v);
  if (wvec && (al & (4 * wvec - 1)) == 0) {
    BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(wvec, (bpr_sample_hard_kernel<IdT, VEC, R, false><<<grid, 256, 0, s>>>(a))));
  } else {
    BR_DISPATCH_ID(id_type, (bpr_sample_hard_kernel<IdT, 1, R, true><<<grid, 256, 0, s>>>(a)));
  }
  BR_CHECK_LAUNCH("brBprSampleNegatives");
  return BR_OK;
}
