// S1 duplicate-id sums + O1 TF-form Adam + O2 Keras Adagrad on embedding rows.
//
// Design: no float atomics on the training path.  ids are radix-sorted once per id stream together with their batch position
// (row_index.hip; stable => equal ids stay in ascending position); every table that shares the stream reuses the index.  The kernels
// here walk each segment in that order, so the duplicate sum is exactly a sequential unsorted_segment_sum ([TF-sem]
// _deduplicate_indexed_slices): bitwise reproducible, and (sum g)^2 feeds Adam's v.  The per-pair row gradients are written ONCE with
// plain stores by the backward kernels and read back here through the inverted index (cdna_hip_programming.md App. B "Scatter / gather").
//
// Two concerns share this unit: the ordered segment sum (seg_walk / seg_acc, the partials, brSegmentSum*, brScatterAddRows) and the row
// optimizers that run the same walk inside their kernels (Adam rows with the keep-plane and finalize riders, flush, dense sweep, flat
// Adam, Adagrad).  A unit of their own for the segment-sum launches changes the code the compiler generates for segment_sum_kernel and
// segment_sum_to_slots_kernel (tools/asm_diff.py), so they stay beside the optimizers' instantiations of the walk.
#include "common.h"
#include "rows.h"
#include "adam_math.h"
#include "finalize.h"
#include "dense.h"
#include "step_state.h"

#include <algorithm>

namespace br {

// one row group per sorted position; only segment heads do work
template <typename IdT>
__device__ __forceinline__ bool segment_head(const IdT* sid, int64_t i) {
  return i == 0 || sid[i - 1] != sid[i];
}

// ---- long id segments (hot ids: a Zipf batch puts thousands of positions on one row) ------------------------------
// A segment head that adds its duplicates one by one is a chain of dependent loads as long as the segment (measured:
// 2.3 ms for the Adam-rows launch on a Zipf(1.05) batch of 65 536).  With a partial buffer the walk is two-level:
// segment_partials_kernel gives every kSegBlock-aligned block of the SORTED order that continues its predecessor's id
// the ordered sum of its own run (<= 64 adds, all blocks in parallel); the head then adds its own positions up to the
// next block boundary one by one and ONE partial row per later block.  Still a fixed order - (((g_i + ..) + P_b) + P_b+1)
// with P_b = ((g_64b + g_64b+1) + ..) - restated by the oracle (ordered_segment_sum); without a buffer: one by one.
constexpr int kSegBlock = 64;

// a row of per-pair gradients: g[pos], times sc[pos] when the source carries a per-position factor (the MF halves of a NeuMF
// step: the stashed partner row times ddot[pos] - the product the embed backward used to write out as its own launch)
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type grow(const float* __restrict__ g, int64_t ldg, const float* __restrict__ sc, int32_t pos) {
  const typename VecT<VEC>::type v = vload<VEC>(g + (int64_t)pos * ldg);
  return sc ? vmul(v, sc[pos]) : v;
}

// acc += rows of positions [j, end) while they belong to `row`, in that order - the additions are sequential (the fp32 order is part
// of the result), but the loads are not: eight ids / positions / gradient rows are requested together (one dependent round trip per eight
// positions instead of per position; a hot id walks thousands).  Rows past the run's end are loaded and dropped.  -> first position
// not added.
template <typename IdT, int VEC, int W>
__device__ __forceinline__ int64_t seg_walk(typename VecT<VEC>::type& acc, const IdT* __restrict__ sid, const int32_t* __restrict__ spos, int64_t j,
                                            int64_t end, IdT row, const float* __restrict__ g, int64_t ldg, const float* __restrict__ sc) {
  using V = typename VecT<VEC>::type;
  for (; j + W <= end; j += W) {
    IdT sv[W];
    int32_t pv[W];
    V v[W];
#pragma unroll
    for (int e = 0; e < W; ++e) sv[e] = sid[j + e];
    if (sv[0] != row) return j;
#pragma unroll
    for (int e = 0; e < W; ++e) pv[e] = spos[j + e];
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = grow<VEC>(g, ldg, sc, pv[e]);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      if (sv[e] != row) return j + e;
      acc = vadd(acc, v[e]);
    }
  }
  for (; j < end && sid[j] == row; ++j) acc = vadd(acc, grow<VEC>(g, ldg, sc, spos[j]));
  return j;
}

template <typename IdT, int VEC, int W = 1>
__device__ __forceinline__ void seg_acc_from(typename VecT<VEC>::type& acc, const IdT* __restrict__ sid, const int32_t* __restrict__ spos, int64_t n,
                                             int64_t i, int64_t j, IdT row, const float* __restrict__ g, int64_t ldg, const float* __restrict__ sc,
                                             const float* __restrict__ part, int pdim);

template <typename IdT, int VEC>
__device__ __forceinline__ typename VecT<VEC>::type seg_acc(const IdT* __restrict__ sid, const int32_t* __restrict__ spos, int64_t n, int64_t i,
                                                            IdT row, const float* __restrict__ g, int64_t ldg, const float* __restrict__ sc,
                                                            const float* __restrict__ part, int pdim) {
  using V = typename VecT<VEC>::type;
  V acc = grow<VEC>(g, ldg, sc, spos[i]);
  seg_acc_from<IdT, VEC>(acc, sid, spos, n, i, i + 1, row, g, ldg, sc, part, pdim);
  return acc;
}

// the rest of a head's sum from position j on (everything in [i, j) is already in acc, in order); W = positions requested together by the
// one-by-one part of the walk (same additions in the same order)
template <typename IdT, int VEC, int W>
__device__ __forceinline__ void seg_acc_from(typename VecT<VEC>::type& acc, const IdT* __restrict__ sid, const int32_t* __restrict__ spos, int64_t n,
                                             int64_t i, int64_t j, IdT row, const float* __restrict__ g, int64_t ldg, const float* __restrict__ sc,
                                             const float* __restrict__ part, int pdim) {
  using V = typename VecT<VEC>::type;
  const int64_t own_end = part ? ((i / kSegBlock + 1) * kSegBlock < n ? (i / kSegBlock + 1) * kSegBlock : n) : n;
  // (W = 1 in the row-group launches: they are bound by HBM latency at 8 waves / SIMD - the registers of a batched walk cost them more
  //  on ordinary batches than they save on hot ids; the long runs are cut to <= 63 positions by the partials.  The one-wave-per-row
  //  kernel walks eight at a time: its ids / positions are scalar loads, and a Zipf batch is full of runs of 5 - 60 positions whose
  //  heads otherwise pay three dependent round trips per position)
  j = seg_walk<IdT, VEC, W>(acc, sid, spos, j, own_end, row, g, ldg, sc);
  if (part && j == own_end) {
    // one partial per later block of the run, four at a time (same order of additions)
    for (; j + 3 * kSegBlock < n && sid[j + 3 * kSegBlock] == row; j += 4 * kSegBlock) {
      const V p0 = vload<VEC>(part + (j / kSegBlock) * pdim), p1 = vload<VEC>(part + (j / kSegBlock + 1) * pdim);
      const V p2 = vload<VEC>(part + (j / kSegBlock + 2) * pdim), p3 = vload<VEC>(part + (j / kSegBlock + 3) * pdim);
      acc = vadd(vadd(vadd(vadd(acc, p0), p1), p2), p3);
    }
    for (; j < n && sid[j] == row; j += kSegBlock) acc = vadd(acc, vload<VEC>(part + (j / kSegBlock) * pdim));
  }
}

struct SegJob {                // one table's gradient source for the partials
  const void* sid; const int32_t* spos;
  const float* g0; int64_t ldg0;
  const float* g1; int64_t ldg1;
  float* part;                 // [ceil(n / kSegBlock)][dim]
  const float* sc1 = nullptr;  // per-position factor of g1 rows, or null (last: positional initialisers of the other users stay valid)
  int64_t n = 0;               // this job's positions when the jobs of a launch differ in length (0: the launch's n)
};
struct SegJobs { SegJob j[2]; };

template <typename IdT, int VEC>
__global__ __launch_bounds__(256) void segment_partials_kernel(SegJobs jobs, int64_t n_launch, int dim, int chunks, int lpr_log2, int split, const StepAdvance adv) {
  using V = typename VecT<VEC>::type;
  if (adv.st && blockIdx.x == gridDim.x - 1) {      // (see segment_partials_wave_kernel)
    if (blockIdx.y == 0) step_state_advance_block(adv);
    return;
  }
  const SegJob& jb = jobs.j[blockIdx.y];
  const int64_t n = jb.n ? jb.n : n_launch;
  const IdT* __restrict__ sid = (const IdT*)jb.sid;
  const int32_t* __restrict__ spos = jb.spos;
  const int lpr = 1 << lpr_log2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t b = (tid >> lpr_log2) + 1;                 // block 0 starts at a head (or is walked by one)
  const int lir = (int)(tid & (lpr - 1));
  const int64_t i = b * kSegBlock;
  if (i >= n) return;
  const IdT row = sid[i];
  if (sid[i - 1] != row) return;                            // a head starts here: nobody reads this block's partial
  const int64_t end = i + kSegBlock < n ? i + kSegBlock : n;
  for (int c = lir; c < chunks; c += lpr) {
    const int col = c * VEC;
    const float* g = col < split ? jb.g0 + col : jb.g1 + (col - split);
    const int64_t ldg = col < split ? jb.ldg0 : jb.ldg1;
    const float* sc = col < split ? nullptr : jb.sc1;
    V acc = grow<VEC>(g, ldg, sc, spos[i]);
    (void)seg_walk<IdT, VEC, 8>(acc, sid, spos, i + 1, end, row, g, ldg, sc);
    vstore<VEC>(jb.part + b * dim + col, acc);
  }
}

// The same partials with one WAVE per 64-block, for rows of 64 * VEC floats: lane l holds the id and the position of sorted position
// 64 b + l (one coalesced round trip for the whole block instead of a dependent id -> position -> row chain per 8 positions), the run's
// length is a ballot, and the rows are requested eight at a time by position (readlane) and added in position order - the order
// seg_walk adds them in.  On a Zipf(1.05) batch ~70 % of the blocks continue a run: 40 us in the row-group form.
template <typename IdT, int VEC>
__global__ __launch_bounds__(256) void segment_partials_wave_kernel(SegJobs jobs, int64_t n_launch, int split, const StepAdvance adv) {
  using V = typename VecT<VEC>::type;
  // adv.st != NULL (a later step of a multi-step group, which has no chunk-rank launch): the grid has one extra column of workgroups,
  // whose y = 0 member advances the step state.  Nothing in this launch reads the state; the step's lookup in front computed its step
  // as ss->step + 1, the Adam-rows launch behind reads the advanced counter and alpha_t
  if (adv.st && blockIdx.x == gridDim.x - 1) {
    if (blockIdx.y == 0) step_state_advance_block(adv);
    return;
  }
  constexpr int dim = 64 * VEC;
  const SegJob& jb = jobs.j[blockIdx.y];
  const int64_t n = jb.n ? jb.n : n_launch;
  const IdT* __restrict__ sid = (const IdT*)jb.sid;
  const int32_t* __restrict__ spos = jb.spos;
  const int64_t b = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + 1;   // block 0 starts at a head
  const int64_t i = b * kSegBlock;
  if (i >= n) return;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t q = i + lane < n ? i + lane : n - 1;
  const IdT my_id = sid[q];
  const int32_t my_pos = spos[q];
  const IdT row = sid[i];
  if (sid[i - 1] != row) return;                            // a head starts here: nobody reads this block's partial
  // positions of the block that belong to the run: the leading lanes whose id is `row`
  const uint64_t same = __builtin_amdgcn_ballot_w64(i + lane < n && my_id == row);
  const int L = same == ~0ull ? 64 : __builtin_ctzll(~same);
  const int col = lane * VEC;
  const bool lo = col < split;
  const float* __restrict__ gp = lo ? jb.g0 + col : jb.g1 + (col - split);
  const int64_t ldg = lo ? jb.ldg0 : jb.ldg1;
  const float* __restrict__ sc = jb.sc1;
  V acc = vzero<VEC>();
  for (int j0 = 0; j0 < L; j0 += 8) {
    V v[8];
    float scl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t pos = (int64_t)__builtin_amdgcn_readlane(my_pos, (j0 + e) & 63);     // (past L: a row of the block, loaded and dropped)
      v[e] = vload<VEC>(gp + pos * ldg);
      scl[e] = (sc && !lo) ? sc[pos] : 1.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (j0 + e >= L) break;
      const V t = lo ? v[e] : vmul(v[e], scl[e]);            // grow(): the MF halves are scaled as they are read
      acc = (j0 + e == 0) ? t : vadd(acc, t);
    }
  }
  vstore<VEC>(jb.part + b * dim + col, acc);
}

template <typename IdT, int VEC>
__global__ __launch_bounds__(256) void segment_sum_kernel(const IdT* __restrict__ sid, const int32_t* __restrict__ spos,
                                                           int64_t n, const float* __restrict__ g, int64_t ldg, int dim,
                                                           int chunks, int lpr_log2, float* __restrict__ out,
                                                           int32_t* __restrict__ head_flag, const float* __restrict__ part) {
  using V = typename VecT<VEC>::type;
  const int lpr = 1 << lpr_log2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = tid >> lpr_log2;
  const int lir = (int)(tid & (lpr - 1));
  if (i >= n) return;
  const bool head = segment_head(sid, i);
  if (lir == 0 && head_flag) head_flag[i] = head ? 1 : 0;
  if (!head) return;
  const IdT row = sid[i];
  for (int c = lir; c < chunks; c += lpr) {
    const V acc = seg_acc<IdT, VEC>(sid, spos, n, i, row, g + c * VEC, ldg, nullptr, part ? part + c * VEC : nullptr, dim);
    vstore<VEC>(out + i * dim + c * VEC, acc);
  }
}

template <typename IdT>
__global__ __launch_bounds__(256) void scatter_add_kernel(float* __restrict__ gt, int64_t table_rows, const IdT* __restrict__ ids,
                                                           int64_t n, const float* __restrict__ rows, int dim, int* err) {
  // one lane per float: a wave covers 64 contiguous floats (256 B) of one row => the atomic
  // shape MI355X_MICROARCH.md "Global float atomics" measures at full rate for dim >= 64.
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * dim) return;
  const int64_t b = e / dim;
  const int d = (int)(e - b * dim);
  const int64_t id = load_id(ids, b);
  if ((uint64_t)id >= (uint64_t)table_rows) {
    flag_range(err, false, d == 0);
    return;
  }
  atomicAdd(gt + id * dim + d, rows[e]);
}

__global__ __launch_bounds__(256) void zero_bytes_kernel(uint8_t* __restrict__ p, int64_t n) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (i0 + q < n) p[i0 + q] = 0;
}

// Row gradients may come from two buffers: columns [0,split) from g0, [split,dim) from g1 (the fused
// NeuMF tables [mlp | mf] take their MLP half from dx0 and their MF half from the embed backward).
// One launch may serve two tables of the same geometry (the user and the item table of a NeuMF step, blockIdx.y):
// each alone leaves HBM half idle (random 512-B rows, a dependent chain per row), together they overlap.
struct AdamRowsJob {
  float* table; float* M; float* Vv;
  int64_t table_rows;
  const void* sid; const int32_t* spos;
  const float* g0; int64_t ldg0;
  const float* g1; int64_t ldg1;
  const float* sc1;           // per-position factor of g1 rows, or null
  const float* part;          // segment partials of this table's gradient source (NULL: one-by-one walk)
  uint8_t* mark; int32_t* last;
  // deferred mode, optional: the row as the step's lookup replayed it (theta at step t-1), per POSITION - columns [0,split) at
  // th0 + pos*ldt0, [split,dim) at th1 + pos*ldt1.  With it the optimizer replays only m and v (two multiplies per step) instead of
  // repeating the lookup's sqrt / rcp chain on theta: same bits (the lookup ran adam_replay on the same stored row).
  const float* th0 = nullptr; int64_t ldt0 = 0;
  const float* th1 = nullptr; int64_t ldt1 = 0;
  int64_t n = 0;              // this job's positions when the two jobs of a launch differ in length (wave kernel only; 0: the launch's n)
};
struct AdamRowsJobs { AdamRowsJob j[2]; };

template <typename IdT, int VEC>
__global__ __launch_bounds__(256) void adam_rows_sorted_kernel(AdamRowsJobs jobs, int dim, int chunks, int lpr_log2, int64_t n, int split,
                                                                AdamHp h, const StepStateDev* __restrict__ ss, const KeepFuse kf, int keep_x) {
  // keep_x columns of the grid fill the next step's dropout planes (ALU-bound Philox beside this HBM-bound kernel:
  // no fork / join around a launch of its own, which costs ~10 us each inside a hipGraph)
  // every P-th column of the grid (P = columns / keep_x) is a plane column, so the two kinds of work share the CUs from start to end
  int64_t bx = blockIdx.x;
  if (keep_x > 0) {
    const int P = (int)gridDim.x / keep_x;
    const int q = (int)blockIdx.x / P;
    if ((int)blockIdx.x - q * P == 0 && q < keep_x) {
      const int64_t wg = (int64_t)q * gridDim.y + blockIdx.y;
      if (wg < kf.total) keep_fuse_block(kf, wg);
      return;
    }
    const int before = ((int)blockIdx.x + P - 1) / P;          // plane columns left of this one
    bx -= before < keep_x ? before : keep_x;
  }
  const AdamRowsJob& jb = jobs.j[blockIdx.y];
  float* __restrict__ table = jb.table; float* __restrict__ M = jb.M; float* __restrict__ Vv = jb.Vv;
  const int64_t table_rows = jb.table_rows;
  const IdT* __restrict__ sid = (const IdT*)jb.sid;
  const int32_t* __restrict__ spos = jb.spos;
  const float* __restrict__ g0 = jb.g0; const float* __restrict__ g1 = jb.g1;
  const int64_t ldg0 = jb.ldg0, ldg1 = jb.ldg1;
  uint8_t* __restrict__ mark = jb.mark;
  int32_t* __restrict__ last = jb.last;
  using V = typename VecT<VEC>::type;
  __shared__ float ring[BR_ALPHA_RING];
  if (last) stage_alpha_ring(ring, ss);      // uniform branch: whole workgroup
  adam_resolve(h);
  const int lpr = 1 << lpr_log2;
  const int64_t tid = bx * blockDim.x + threadIdx.x;
  const int64_t i = tid >> lpr_log2;
  const int lir = (int)(tid & (lpr - 1));
  if (i >= n) return;
  if (!segment_head(sid, i)) return;
  const int64_t row = (int64_t)sid[i];
  if ((uint64_t)row >= (uint64_t)table_rows) return;  // out-of-range ids were flagged by the forward
  if (mark && lir == 0) mark[row] = 1;
  // deferred mode: this row includes the steps <= last[row]; replay the g = 0 steps up to t-1 first
  const uint32_t t = last ? ss->step : 0u;
  const uint32_t seen = last ? (uint32_t)last[row] : 0u;
  for (int c = lir; c < chunks; c += lpr) {
    const int col = c * VEC;
    const float* g = col < split ? g0 + col : g1 + (col - split);
    const int64_t ldg = col < split ? ldg0 : ldg1;
    const V acc = seg_acc<IdT, VEC>(sid, spos, n, i, sid[i], g, ldg, col < split ? nullptr : jb.sc1, jb.part ? jb.part + col : nullptr, dim);
    const int64_t off = row * dim + col;
    V th = vload<VEC>(table + off), m = vload<VEC>(M + off), v = vload<VEC>(Vv + off);
    if (last && seen + 1 < t) adam_catch_up<true>(th, m, v, seen, t - 1, ring, ss, h);
    adam_update(th, m, v, acc, h);
    vstore<VEC>(table + off, th);
    vstore<VEC>(M + off, m);
    vstore<VEC>(Vv + off, v);
  }
  if (last && lir == 0) last[row] = (int32_t)t;
}

__constant__ float kOneF = 1.f;
__constant__ int32_t kZeroI = 0;
// A kernel-argument pointer held in scalar registers from here on, typed as a GLOBAL pointer (behind the asm the compiler no longer
// knows where it came from and would fall back to flat loads, which also count on lgkmcnt: every scalar-load wait would drain them).
typedef __attribute__((address_space(1))) const float gcf;
typedef __attribute__((address_space(1))) float gwf;
typedef __attribute__((address_space(1))) const int32_t gci32;
typedef __attribute__((address_space(1))) int32_t gwi32;
__device__ __forceinline__ gcf* sgpr_g(const float* x) { gcf* y = (gcf*)x; BR_PIN_S(y); return y; }
__device__ __forceinline__ gwf* sgpr_g(float* x) { gwf* y = (gwf*)x; BR_PIN_S(y); return y; }
__device__ __forceinline__ gwi32* sgpr_g(int32_t* x) { gwi32* y = (gwi32*)x; BR_PIN_S(y); return y; }
__device__ __forceinline__ int64_t sgpr(int64_t x) { BR_PIN_S(x); return x; }
// (the HIP vector classes have no constructors from address-space-qualified objects: go through the native vector types)
template <int VEC> struct NatV { typedef float type __attribute__((ext_vector_type(VEC))); };
template <> struct NatV<1> { typedef float type; };
__device__ __forceinline__ float from_nat(float a) { return a; }
__device__ __forceinline__ float2 from_nat(NatV<2>::type a) { return make_float2(a.x, a.y); }
__device__ __forceinline__ float4 from_nat(NatV<4>::type a) { return make_float4(a.x, a.y, a.z, a.w); }
__device__ __forceinline__ float to_nat(float a) { return a; }
__device__ __forceinline__ NatV<2>::type to_nat(float2 a) { NatV<2>::type r = {a.x, a.y}; return r; }
__device__ __forceinline__ NatV<4>::type to_nat(float4 a) { NatV<4>::type r = {a.x, a.y, a.z, a.w}; return r; }
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type gvload(gcf* p) {
  typedef __attribute__((address_space(1))) const typename NatV<VEC>::type GV;
  const typename NatV<VEC>::type r = *(GV*)p;
  return from_nat(r);
}
template <int VEC>
__device__ __forceinline__ void gvstore(gwf* p, typename VecT<VEC>::type v) {
  typedef __attribute__((address_space(1))) typename NatV<VEC>::type GV;
  *(GV*)p = to_nat(v);
}


// The same update with one WAVE per row, for rows of 64 * VEC floats (the fused [mlp | mf] rows of embed_dim 32 / 64 / 128): a lane
// owns VEC consecutive columns, so everything that depends on the position - head test, id, duplicate walk, the row's lag in deferred
// mode - is wave-uniform (scalar loads and branches; the row-group form above runs two or four rows with different lags per wave and
// every lane waits for the longest).  A wave takes a STRIP of S consecutive sorted positions: one round trip for the strip's ids and
// positions, then every row load of the strip's heads (m, v, theta) and every gradient row a head of the strip can need are requested
// before the first is used - S rows of 3.5 KB in flight per wave instead of one, which is what an HBM-latency-bound gather / scatter
// of 512-B rows needs - and a head finds its duplicates inside the strip already in registers (added in position order, as seg_acc
// does; a run that leaves the strip continues through seg_acc_from).  Deferred mode takes theta as the lookup replayed it
// (AdamRowsJob::th0 / th1) and replays m and v only: no alpha ring, no sqrt / rcp per replayed step.
// Riders: the grid may carry two other pieces of the step as extra workgroups, spread evenly between the row workgroups
// (every P-th workgroup is a rider) - the NEXT step's dropout keep-bit planes (Philox: ALU work beside an HBM-bound kernel) and the
// dense finalize (slab reductions + BatchNorm gradients + Adam on the flat vector: only needs the backward).  As launches of their
// own they needed a fork / join around this kernel inside the step's hipGraph (~10 us each on the main branch, ROCm 7.2).
struct AdamRiders {
  KeepFuse kf;             // kf.total workgroups of keep-bit planes
  FinalArgs fin;           // n_final workgroups of the dense finalize
  int n_final, total;      // total = kf.total + n_final riders
  int rows_x;              // row workgroups per job
};

template <typename IdT, int VEC, int S>
__global__ __launch_bounds__(256) void adam_rows_wave_kernel(AdamRowsJobs jobs, int64_t n_launch, int split, AdamHp h, const StepStateDev* __restrict__ ss,
                                                              const AdamRiders rd) {
  using V = typename VecT<VEC>::type;
  constexpr int dim = 64 * VEC;
  static_assert(kSegBlock % S == 0, "a strip stays inside one partial block");
  __shared__ float fin_part[16][64];
  int64_t rb = blockIdx.x;                                    // row workgroup: job = rb / rows_x
  if (rd.total > 0) {
    const int P = (int)gridDim.x / rd.total;
    const int q = (int)blockIdx.x / P;
    if ((int)blockIdx.x - q * P == 0 && q < rd.total) {       // rider q
      if (q < rd.kf.total) { keep_fuse_block(rd.kf, q); return; }
      adam_resolve(h);
      finalize_block256(rd.fin, h, q - rd.kf.total, fin_part);
      return;
    }
    const int before = ((int)blockIdx.x + P - 1) / P;          // riders left of this workgroup
    rb -= before < rd.total ? before : rd.total;
  }
  const int job = (int)(rb / rd.rows_x);
  const AdamRowsJob& jb = jobs.j[job];
  const int64_t n = jb.n ? jb.n : n_launch;
  const int64_t base = ((rb - (int64_t)job * rd.rows_x) * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * S;
  if (base >= n) return;
  const IdT* __restrict__ sid = (const IdT*)jb.sid;
  const int32_t* __restrict__ spos = jb.spos;
  // round 1: the strip's ids / positions (+ the predecessor's id)
  IdT id[S];
  int64_t pos[S];
  const IdT prev = sid[base > 0 ? base - 1 : 0];
#pragma unroll
  for (int e = 0; e < S; ++e) {
    const int64_t q = base + e < n ? base + e : n - 1;
    id[e] = sid[q];
    pos[e] = (int64_t)spos[q];
  }
  bool head[S], live[S], need_g[S];
  bool any = false;
#pragma unroll
  for (int e = 0; e < S; ++e) {
    const bool in = base + e < n;
    head[e] = in && (e == 0 ? (base == 0 || prev != id[0]) : id[e] != id[e - 1]);
    live[e] = head[e] && (uint64_t)(int64_t)id[e] < (uint64_t)jb.table_rows;   // out-of-range ids were flagged by the forward
    any = any || head[e];
    need_g[e] = in && any;          // a position before the strip's first head belongs to an earlier strip's head
  }
  if (!any) return;
  adam_resolve(h);
  const int lane = (int)(threadIdx.x & 63);
  const int col = lane * VEC;
  const bool lo = col < split;
  // the job's fields as scalars first (a per-lane choice between two fields of the argument block would otherwise be compiled into a
  // per-lane LOAD of the chosen field: a dependent vector load in front of everything)
  gcf* g0 = sgpr_g(jb.g0); gcf* g1 = sgpr_g(jb.g1);
  const int64_t ldg0 = sgpr(jb.ldg0), ldg1 = sgpr(jb.ldg1);
  gcf* t0 = sgpr_g(jb.th0); gcf* t1 = sgpr_g(jb.th1);
  const int64_t ldt0 = sgpr(jb.ldt0), ldt1 = sgpr(jb.ldt1);
  gwf* const tab = sgpr_g(jb.table); gwf* const Mp = sgpr_g(jb.M); gwf* const Vp = sgpr_g(jb.Vv);
  gcf* sc = sgpr_g(jb.sc1);
  gwi32* const last = sgpr_g(jb.last);
  gcf* gp = lo ? g0 + col : g1 + (col - split);
  const int64_t ldg = lo ? ldg0 : ldg1;
  const bool stashed = t0 != nullptr;
  gcf* tp = lo ? t0 + col : t1 + (col - split);
  const int64_t ldt = lo ? ldt0 : ldt1;
  // round 2: everything the strip needs, requested together.  Branch-free on purpose: behind scalar branches the compiler sinks each
  // load to its first use and the wave is back to one row in flight.  A position that is no live head reads row 0 instead (the
  // same three lines for everybody: cache hits), a position before the strip's first head its own gradient row (dropped).
  V g[S], m[S], v[S], th[S];
  float scale[S];
  int32_t seen_v[S];               // last[row]: a vector load (the kernel writes the array, so no scalar cache) - uniform, read out below
#pragma unroll
  for (int e = 0; e < S; ++e) {
    const int64_t row = live[e] ? (int64_t)id[e] : 0;
    const int64_t off = row * dim + col;
    g[e] = gvload<VEC>(gp + pos[e] * ldg);
    scale[e] = *(sc ? sc + pos[e] : (gcf*)&kOneF);
    m[e] = gvload<VEC>(Mp + off);
    v[e] = gvload<VEC>(Vp + off);
    th[e] = gvload<VEC>(stashed && live[e] ? tp + pos[e] * ldt : (gcf*)(tab + off));
    seen_v[e] = *(last ? last + row : (gwi32*)&kZeroI);
  }
  const uint32_t t = last ? ss->step : 0u;
  const bool fast = last && ss->fast;                          // replay form of the deferred tables (adam_math.h)
  uint32_t seen[S];
#pragma unroll
  for (int e = 0; e < S; ++e) {                                               // one wait for the whole strip
    pin(g[e]), pin(m[e]), pin(v[e]), pin(th[e]);
    BR_PIN_V(seen_v[e]);
    seen[e] = (uint32_t)__builtin_amdgcn_readfirstlane(seen_v[e]);
  }
#pragma unroll
  for (int e = 0; e < S; ++e)
    if (!lo) g[e] = vmul(g[e], scale[e]);                      // the MF halves: stashed partner row times ddot[pos] (grow())
#pragma unroll
  for (int e = 0; e < S; ++e) {
    if (!live[e]) continue;
    const int64_t i = base + e;
    V acc = g[e];
    bool open = true;                                          // the run is still going at the strip's end
#pragma unroll
    for (int f = e + 1; f < S; ++f) {
      open = open && base + f < n && !head[f];
      if (open) acc = vadd(acc, g[f]);
    }
    if (open && base + S < n)
      seg_acc_from<IdT, VEC, 8>(acc, sid, spos, n, i, base + S, id[e], (const float*)gp, ldg, lo ? nullptr : (const float*)sc, jb.part ? jb.part + col : nullptr, dim);
    // deferred: the g = 0 steps (seen, t-1] of the moments (adam_decay's first two products; theta came replayed)
    V mm = m[e], vv = v[e], tt = th[e];
    if (last && seen[e] + 1 < t) {
      if (fast) fast_moments(mm, vv, t - 1 - seen[e], ss);
      else for (uint32_t j = seen[e] + 1; j < t; ++j) { mm = vmul(mm, h.b1); vv = vmul(vv, h.b2); }
    }
    adam_update(tt, mm, vv, acc, h);
    const int64_t off = (int64_t)id[e] * dim + col;
    gvstore<VEC>(tab + off, tt);
    gvstore<VEC>(Mp + off, mm);
    gvstore<VEC>(Vp + off, vv);
    if (lane == 0) {
      if (jb.mark) jb.mark[(int64_t)id[e]] = 1;
      if (last) last[(int64_t)id[e]] = (int32_t)t;
    }
  }
}

// Deferred mode, whole table: bring every row up to the current step (inclusive) — before the table is
// read by anything but the catch-up gather (inference, checkpoint), and at least once per BR_ALPHA_RING steps.
template <int VEC>
__global__ __launch_bounds__(256) void adam_flush_kernel(float* __restrict__ table, float* __restrict__ M, float* __restrict__ Vv,
                                                          int64_t n_vec, int chunks, AdamHp h, int32_t* __restrict__ last,
                                                          const StepStateDev* __restrict__ ss) {
  using V = typename VecT<VEC>::type;
  __shared__ float ring[BR_ALPHA_RING];
  stage_alpha_ring(ring, ss);
  const uint32_t t = ss->step;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_vec; e += stride) {
    const int64_t row = e / chunks;
    const uint32_t seen = (uint32_t)last[row];
    if (seen >= t) continue;
    V m = vload<VEC>(M + e * VEC), v = vload<VEC>(Vv + e * VEC);
    if (all_zero(m) && all_zero(v)) continue;
    V th = vload<VEC>(table + e * VEC);
    adam_catch_up<true>(th, m, v, seen, t, ring, ss, h);
    vstore<VEC>(table + e * VEC, th);
    vstore<VEC>(M + e * VEC, m);
    vstore<VEC>(Vv + e * VEC, v);
  }
}
__global__ __launch_bounds__(256) void fill_last_kernel(int32_t* __restrict__ last, int64_t rows, const StepStateDev* __restrict__ ss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) last[i] = (int32_t)ss->step;
}

// Dense sweep: all rows NOT marked get the zero-gradient update.  float4 streaming,
// 2 vectors per thread in flight, grid-stride.
template <int VEC>
__global__ __launch_bounds__(256) void adam_dense_sweep_kernel(float* __restrict__ table, float* __restrict__ M,
                                                                float* __restrict__ Vv, int64_t n_vec, int chunks,
                                                                AdamHp h, const uint8_t* __restrict__ mark) {
  using V = typename VecT<VEC>::type;
  adam_resolve(h);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_vec; e += stride) {
    const int64_t row = e / chunks;
    if (mark && mark[row]) continue;
    V th = vload<VEC>(table + e * VEC), m = vload<VEC>(M + e * VEC), v = vload<VEC>(Vv + e * VEC);
    adam_decay(th, m, v, h.alpha, h);
    vstore<VEC>(table + e * VEC, th);
    vstore<VEC>(M + e * VEC, m);
    vstore<VEC>(Vv + e * VEC, v);
  }
}

__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ th, float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ g, int64_t n, AdamHp h) {
  adam_resolve(h);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) adam_update1(th[i], m[i], v[i], g[i], h);
}

__device__ __forceinline__ void adagrad_update1(float& th, float& acc, float g, float lr, float eps) {
  acc = acc + g * g;
  th = th - lr * g / (sqrtf(acc) + eps);
}

__device__ __forceinline__ void adagrad_update(float4& th, float4& a, float4 g, float lr, float eps) {
  adagrad_update1(th.x, a.x, g.x, lr, eps); adagrad_update1(th.y, a.y, g.y, lr, eps);
  adagrad_update1(th.z, a.z, g.z, lr, eps); adagrad_update1(th.w, a.w, g.w, lr, eps);
}
__device__ __forceinline__ void adagrad_update(float2& th, float2& a, float2 g, float lr, float eps) {
  adagrad_update1(th.x, a.x, g.x, lr, eps); adagrad_update1(th.y, a.y, g.y, lr, eps);
}
__device__ __forceinline__ void adagrad_update(float& th, float& a, float g, float lr, float eps) { adagrad_update1(th, a, g, lr, eps); }

template <typename IdT, int VEC>
__global__ __launch_bounds__(256) void adagrad_rows_sorted_kernel(float* __restrict__ table, float* __restrict__ A,
                                                                   int64_t table_rows, int dim, int chunks, int lpr_log2,
                                                                   const IdT* __restrict__ sid, const int32_t* __restrict__ spos,
                                                                   int64_t n, const float* __restrict__ g, int64_t ldg,
                                                                   float lr, float eps, const float* __restrict__ part) {
  using V = typename VecT<VEC>::type;
  const int lpr = 1 << lpr_log2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = tid >> lpr_log2;
  const int lir = (int)(tid & (lpr - 1));
  if (i >= n) return;
  if (!segment_head(sid, i)) return;
  const int64_t row = (int64_t)sid[i];
  if ((uint64_t)row >= (uint64_t)table_rows) return;
  for (int c = lir; c < chunks; c += lpr) {
    const V acc = seg_acc<IdT, VEC>(sid, spos, n, i, sid[i], g + c * VEC, ldg, nullptr, part ? part + c * VEC : nullptr, dim);
    const int64_t off = row * dim + c * VEC;
    V th = vload<VEC>(table + off), a = vload<VEC>(A + off);
    adagrad_update(th, a, acc, lr, eps);
    vstore<VEC>(table + off, th);
    vstore<VEC>(A + off, a);
  }
}

__global__ __launch_bounds__(256) void adagrad_flat_kernel(float* __restrict__ th, float* __restrict__ acc,
                                                            const float* __restrict__ g, int64_t n, float lr, float eps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) adagrad_update1(th[i], acc[i], g[i], lr, eps);
}

}  // namespace br

using namespace br;

extern "C" int64_t brSegmentScratchFloats(int64_t n, int dim) { return ceil_div(n > 0 ? n : 1, kSegBlock) * (int64_t)dim; }

// partial rows of every kSegBlock-aligned block that continues a segment (see seg_acc); jobs share n / dim / split
// (adv: the step-state advance as one extra workgroup of the launch, which must then exist)
static int launch_partials(const SegJob* jobs, int n_jobs, int id_type, int64_t n, int dim, const RowGeom& g, int split, hipStream_t s,
                           const StepAdvance* adv = nullptr) {
  const int64_t blocks = ceil_div(n, kSegBlock) - 1;
  BR_CHECK_ARG(!adv || blocks > 0, "segment partials: no launch to carry the step-state advance");
  if (blocks <= 0) return BR_OK;
  const StepAdvance av = adv ? *adv : StepAdvance{};
  const unsigned extra = av.st ? 1u : 0u;
  SegJobs J;
  for (int q = 0; q < 2; ++q) J.j[q] = jobs[q < n_jobs ? q : 0];
  const int wvec = wave_row_vec(dim);
  if (wave_rows_enabled() && wvec && g.vec >= wvec) {     // (g.vec: the widest vector the sources' strides honour)
    const dim3 wgrid((unsigned)ceil_div(blocks, 4) + extra, (unsigned)n_jobs);
    BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(wvec, (segment_partials_wave_kernel<IdT, VEC><<<wgrid, 256, 0, s>>>(J, n, split, av))));
    BR_CHECK_LAUNCH("segment partials (wave)");
    return BR_OK;
  }
  const dim3 grid((unsigned)ceil_div(blocks, 256 >> g.lpr_log2) + extra, (unsigned)n_jobs);
  BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(g.vec, (segment_partials_kernel<IdT, VEC><<<grid, 256, 0, s>>>(J, n, dim, g.chunks, g.lpr_log2, split, av))));
  BR_CHECK_LAUNCH("segment partials");
  return BR_OK;
}

extern "C" int brSegmentSumRows(const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                                const float* row_grads, int64_t ldg, int dim, float* out_rows, int32_t* head_flag,
                                float* seg_ws, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brSegmentSumRows: bad id_type");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(sorted_ids && sorted_pos && row_grads && out_rows && dim >= 1 && ldg >= dim, "brSegmentSumRows: bad args");
  // widest vector that the source's stride and every base the kernels address by vector honour (rows of out / seg_ws are dim apart)
  const RowGeom g = row_geom_ld(dim, vec_width({ldg, dim}, {row_grads, out_rows, seg_ws}));
  const unsigned grid = (unsigned)ceil_div(n, 256 >> g.lpr_log2);
  hipStream_t s = (hipStream_t)stream;
  if (seg_ws) {
    const SegJob job{sorted_ids, sorted_pos, row_grads, ldg, row_grads, ldg, seg_ws};
    const int rc = launch_partials(&job, 1, id_type, n, dim, g, dim, s);
    if (rc != BR_OK) return rc;
  }
  BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(g.vec, (segment_sum_kernel<IdT, VEC><<<grid, 256, 0, s>>>((const IdT*)sorted_ids, sorted_pos, n, row_grads, ldg, dim, g.chunks,
                                                                                                 g.lpr_log2, out_rows, head_flag, seg_ws))));
  BR_CHECK_LAUNCH("brSegmentSumRows");
  return BR_OK;
}

// ---- requester side of the row-sharded exchange: per-unique-id gradient sums laid into the send slots -------------------------------
// One row group per sorted position of the (owner, id)-sorted index of brShardDedupPlanPair; a head sums its run (two-level order,
// as everywhere) straight from the step's gradient sources - columns [0, split) from g0 (the MLP half of dx0), [split, dim) from g1
// times sc1[position] (the partner's stashed MF row times ddot) - and stores the sum at row slot[position of the head] of the merged
// slot buffer.  Heads whose id found no slot (capacity overflow, id out of range: slot < 0) store nothing.
struct SlotSumJob {
  const void* sid; const int32_t* spos; const int32_t* slot;
  const float* g0; const float* g1; const float* part;
};
struct SlotSumJobs { SlotSumJob j[2]; };
template <typename IdT, int VEC>
__global__ __launch_bounds__(256) void segment_sum_to_slots_kernel(SlotSumJobs jobs, int64_t n, int64_t ldg0, int64_t ldg1, const float* __restrict__ sc1, int dim,
                                                                    int chunks, int lpr_log2, int split, float* __restrict__ out) {
  using V = typename VecT<VEC>::type;
  const SlotSumJob& jb = jobs.j[blockIdx.y];
  const IdT* __restrict__ sid = (const IdT*)jb.sid;
  const int32_t* __restrict__ spos = jb.spos;
  const int lpr = 1 << lpr_log2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = tid >> lpr_log2;
  const int lir = (int)(tid & (lpr - 1));
  if (i >= n) return;
  if (!segment_head(sid, i)) return;
  const int64_t sl = (int64_t)jb.slot[spos[i]];
  if (sl < 0) return;
  const IdT row = sid[i];
  for (int c = lir; c < chunks; c += lpr) {
    const int col = c * VEC;
    const bool lo = col < split;
    const float* g = lo ? jb.g0 + col : jb.g1 + (col - split);
    const V acc = seg_acc<IdT, VEC>(sid, spos, n, i, row, g, lo ? ldg0 : ldg1, lo ? nullptr : sc1, jb.part ? jb.part + col : nullptr, dim);
    vstore<VEC>(out + sl * dim + col, acc);
  }
}

extern "C" int brSegmentSumToSlotsPair(const void* sorted_ids_a, const int32_t* sorted_pos_a, const int32_t* slot_a, const float* g0_a, const float* g1_a,
                                       const void* sorted_ids_b, const int32_t* sorted_pos_b, const int32_t* slot_b, const float* g0_b, const float* g1_b,
                                       int64_t ldg0, int64_t ldg1, const float* hi_scale, int id_type, int64_t n, int dim, int split, float* out_slots,
                                       float* seg_ws_a, float* seg_ws_b, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brSegmentSumToSlotsPair: bad id_type");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(sorted_ids_a && sorted_pos_a && slot_a && g0_a && sorted_ids_b && sorted_pos_b && slot_b && g0_b && out_slots && dim >= 1, "brSegmentSumToSlotsPair: null pointer");
  if (!g1_a || !g1_b) { split = dim; g1_a = g0_a; g1_b = g0_b; ldg1 = ldg0; hi_scale = nullptr; }
  BR_CHECK_ARG(split >= 1 && split <= dim && ldg0 >= split && ldg1 >= dim - split, "brSegmentSumToSlotsPair: bad split / strides");
  BR_CHECK_ARG((seg_ws_a == nullptr) == (seg_ws_b == nullptr), "brSegmentSumToSlotsPair: seg_ws for both streams or neither");
  const RowGeom g = row_geom_ld(dim, vec_width({ldg0, ldg1, split, dim}, {g0_a, g1_a, g0_b, g1_b, out_slots}));
  hipStream_t s = (hipStream_t)stream;
  if (seg_ws_a) {
    const SegJob segs[2] = {SegJob{sorted_ids_a, sorted_pos_a, g0_a, ldg0, g1_a, ldg1, seg_ws_a, hi_scale}, SegJob{sorted_ids_b, sorted_pos_b, g0_b, ldg0, g1_b, ldg1, seg_ws_b, hi_scale}};
    const int rc = launch_partials(segs, 2, id_type, n, dim, g, split, s);
    if (rc != BR_OK) return rc;
  }
  SlotSumJobs J;
  J.j[0] = SlotSumJob{sorted_ids_a, sorted_pos_a, slot_a, g0_a, g1_a, seg_ws_a};
  J.j[1] = SlotSumJob{sorted_ids_b, sorted_pos_b, slot_b, g0_b, g1_b, seg_ws_b};
  const dim3 grid((unsigned)ceil_div(n, 256 >> g.lpr_log2), 2);
  BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(g.vec, (segment_sum_to_slots_kernel<IdT, VEC><<<grid, 256, 0, s>>>(J, n, ldg0, ldg1, hi_scale, dim, g.chunks, g.lpr_log2, split, out_slots))));
  BR_CHECK_LAUNCH("brSegmentSumToSlotsPair");
  return BR_OK;
}

extern "C" int brScatterAddRows(float* g_table, int64_t table_rows, const void* ids, int id_type, int64_t n,
                                const float* rows, int dim, int* err_flag, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brScatterAddRows: bad id_type");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(g_table && rows && dim >= 1 && table_rows > 0, "brScatterAddRows: bad args");
  const unsigned grid = (unsigned)ceil_div(n * dim, 256);
  hipStream_t s = (hipStream_t)stream;
  BR_DISPATCH_ID(id_type, (scatter_add_kernel<IdT><<<grid, 256, 0, s>>>(g_table, table_rows, (const IdT*)ids, n, rows, dim, err_flag)));
  BR_CHECK_LAUNCH("brScatterAddRows");
  return BR_OK;
}

struct AdamRowsArgs {      // one table's host-side arguments
  float *table, *m, *v;
  int64_t table_rows;
  const void* sorted_ids; const int32_t* sorted_pos;
  const float* row_grads; int64_t ldg;
  const float* row_grads_hi; int64_t ldg_hi;
  uint8_t* mark; int32_t* last;
  float* seg_ws;
  const float* hi_scale = nullptr;     // per-position factor of the row_grads_hi rows
  const float* th_lo = nullptr; const float* th_hi = nullptr; int64_t ld_th = 0;   // replayed theta by position (AdamRowsJob::th0 / th1)
  int64_t n = 0;              // positions of this table when the tables of a launch differ in length (wave kernel only)
};

static int adam_rows_launch(const AdamRowsArgs* a, int n_jobs, int dim, int id_type, int64_t n, int split, double alpha_t, double beta1,
                            double beta2, double eps, const StepStateDev* ss, brStream stream, const KeepArgs* keep = nullptr,
                            const FinalArgs* fin = nullptr, bool* fin_done = nullptr, const StepAdvance* adv = nullptr) {
  if (fin_done) *fin_done = false;
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brAdamRowsSorted: bad id_type");
  if (n == 0) return BR_OK;
  AdamRowsJobs jobs;
  SegJob segs[2];
  bool with_partials = true, all_stashed = true, per_job_n = false;
  int64_t ldmin = 4, th_min = 4, n_max = n;
  for (int q = 0; q < n_jobs; ++q) {
    AdamRowsArgs t = a[q];
    BR_CHECK_ARG(t.table && t.m && t.v && t.sorted_ids && t.sorted_pos && t.row_grads && dim >= 1 && t.table_rows > 0, "brAdamRowsSorted: bad args");
    if (!t.row_grads_hi) { if (n_jobs == 1) split = dim; t.ldg_hi = t.ldg; t.row_grads_hi = t.row_grads; }
    BR_CHECK_ARG(split >= 1 && split <= dim && t.ldg >= split && t.ldg_hi >= dim - split, "brAdamRowsSorted: bad split / strides");
    // widest vector (floats) that every row start of both sources and the split honour
    ldmin = std::min<int64_t>(ldmin, vec_width({t.ldg, t.ldg_hi, split}, {t.row_grads, t.row_grads_hi}));
    jobs.j[q] = AdamRowsJob{t.table, t.m, t.v, t.table_rows, t.sorted_ids, t.sorted_pos, t.row_grads, t.ldg, t.row_grads_hi, t.ldg_hi, t.hi_scale,
                            t.seg_ws, t.mark, t.last};
    if (t.th_lo && t.th_hi && t.last) {
      th_min = std::min<int64_t>(th_min, vec_width({t.ld_th}, {t.th_lo, t.th_hi}));
      jobs.j[q].th0 = t.th_lo; jobs.j[q].ldt0 = t.ld_th; jobs.j[q].th1 = t.th_hi; jobs.j[q].ldt1 = t.ld_th;
    } else if (t.last) {
      all_stashed = false;
    }
    segs[q] = SegJob{t.sorted_ids, t.sorted_pos, t.row_grads, t.ldg, t.row_grads_hi, t.ldg_hi, t.seg_ws, t.hi_scale, t.n};
    jobs.j[q].n = t.n;
    if (t.n > n_max) n_max = t.n;
    per_job_n = per_job_n || (t.n != 0 && t.n != n);
    with_partials = with_partials && t.seg_ws != nullptr;
  }
  if (n_jobs == 1) jobs.j[1] = jobs.j[0];
  if (!with_partials)
    for (int q = 0; q < 2; ++q) jobs.j[q].part = nullptr;     // all tables or none
  const RowGeom g = row_geom_ld(dim, ldmin);
  // rows of 64 / 128 / 256 floats: one wave per row (deferred tables only with the lookup's replayed theta at hand)
  const int wvec = wave_row_vec(dim);
  const bool wave_ok = wave_rows_enabled() && wvec && ldmin >= wvec && th_min >= wvec && all_stashed;
  BR_CHECK_ARG(!per_job_n || wave_ok, "brAdamRowsSorted: tables of different lengths in one launch need the one-wave-per-row shapes");
  BR_CHECK_ARG(!adv || with_partials, "brAdamRowsSorted: the step-state advance rides in the segment-partials launch (seg_ws missing)");
  if (with_partials) {
    const int rc = launch_partials(segs, n_jobs, id_type, n_max, dim, g, split, (hipStream_t)stream, adv);
    if (rc != BR_OK) return rc;
    probe_split(BR_TAG_SEG_PARTIALS, (hipStream_t)stream);
  }
  hipStream_t s = (hipStream_t)stream;
  AdamHp h = make_hp(alpha_t, beta1, beta2, eps);
  if (ss) h.alpha_ptr = &ss->alpha_t;
  probe_mark(s);
  // the keep-bit planes of the next step ride in either form of the launch: kf.blocks[i] workgroups for site i
  KeepFuse kf;
  kf.total = 0; kf.blocks[0] = kf.blocks[1] = kf.blocks[2] = 0; kf.a = KeepArgs{};
  if (keep && keep->batch > 0) {
    kf.a = *keep;
    for (int i = 0; i < keep->n_sites; ++i) { kf.blocks[i] = (int)ceil_div(keep->batch * keep->s[i].kw, (int64_t)256); kf.total += kf.blocks[i]; }
  }
  if (wave_ok) {
    static const int strip = [] { const char* e = getenv("BR_ADAM_STRIP"); return e ? atoi(e) : 4; }();      // knob: 2, 4 (default), 8 - measured at the bench config: 92 / 85 / 115 us with riders
    AdamRiders rd;
    rd.kf = kf;
    rd.n_final = 0;
    if (fin) { rd.fin = *fin; rd.n_final = (int)ceil_div(fin->n, 64); } else { rd.fin = FinalArgs{}; }
    rd.total = rd.kf.total + rd.n_final;
    const int S = (strip == 2 || strip == 8) && wvec <= 2 ? strip : 4;
    rd.rows_x = (int)ceil_div(n_max, 4 * S);
    const unsigned wgrid = (unsigned)((int64_t)rd.rows_x * n_jobs + rd.total);
#define BR_ADAM_WAVE(S_) BR_DISPATCH_VEC(wvec, (adam_rows_wave_kernel<IdT, VEC, S_><<<wgrid, 256, 0, s>>>(jobs, n, split, h, ss, rd)))
    BR_DISPATCH_ID(id_type, { if (S == 2) BR_ADAM_WAVE(2); else if (S == 8) BR_ADAM_WAVE(8); else BR_ADAM_WAVE(4); });
#undef BR_ADAM_WAVE
    BR_CHECK_LAUNCH("brAdamRowsSorted(wave)");
    if (fin_done) *fin_done = fin != nullptr;
    return BR_OK;
  }
  for (int q = 0; q < 2; ++q) { jobs.j[q].th0 = jobs.j[q].th1 = nullptr; }
  const int keep_x = (int)ceil_div((int64_t)kf.total, (int64_t)n_jobs);
  const dim3 grid((unsigned)(ceil_div(n, 256 >> g.lpr_log2) + keep_x), (unsigned)n_jobs);
  BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(g.vec, (adam_rows_sorted_kernel<IdT, VEC><<<grid, 256, 0, s>>>(jobs, dim, g.chunks, g.lpr_log2, n, split, h, ss, kf, keep_x))));
  BR_CHECK_LAUNCH("brAdamRowsSorted");
  return BR_OK;
}

extern "C" int brAdamRowsSorted(float* table, float* m, float* v, int64_t table_rows, int dim, const void* sorted_ids,
                                int id_type, const int32_t* sorted_pos, int64_t n, const float* row_grads, int64_t ldg,
                                const float* row_grads_hi, int64_t ldg_hi, int split, double alpha_t, double beta1,
                                double beta2, double eps, uint8_t* mark, float* seg_ws, brStream stream) {
  const AdamRowsArgs a{table, m, v, table_rows, sorted_ids, sorted_pos, row_grads, ldg, row_grads_hi, ldg_hi, mark, nullptr, seg_ws};
  return adam_rows_launch(&a, 1, dim, id_type, n, split, alpha_t, beta1, beta2, eps, nullptr, stream);
}

extern "C" int brAdamRowsSortedDeferred(float* table, float* m, float* v, int32_t* last, int64_t table_rows, int dim,
                                        const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                                        const float* row_grads, int64_t ldg, const float* row_grads_hi, int64_t ldg_hi, int split,
                                        const void* step_state, double beta1, double beta2, double eps, float* seg_ws, brStream stream) {
  BR_CHECK_ARG(last && step_state, "brAdamRowsSortedDeferred: last / step_state missing");
  const AdamRowsArgs a{table, m, v, table_rows, sorted_ids, sorted_pos, row_grads, ldg, row_grads_hi, ldg_hi, nullptr, last, seg_ws};
  return adam_rows_launch(&a, 1, dim, id_type, n, split, 0.0, beta1, beta2, eps, (const StepStateDev*)step_state, stream);
}

extern "C" int brAdamRowsSortedDeferredReplayed(float* table, float* m, float* v, int32_t* last, int64_t table_rows, int dim,
                                                const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                                                const float* row_grads, int64_t ldg, const float* row_grads_hi, int64_t ldg_hi, int split,
                                                const float* replayed_rows, int64_t ld_replayed, const void* step_state, double beta1,
                                                double beta2, double eps, float* seg_ws, brStream stream) {
  BR_CHECK_ARG(last && step_state, "brAdamRowsSortedDeferredReplayed: last / step_state missing");
  BR_CHECK_ARG(replayed_rows && ld_replayed >= dim, "brAdamRowsSortedDeferredReplayed: replayed rows missing or ld < dim");
  const int sp = row_grads_hi ? split : dim;
  AdamRowsArgs a{table, m, v, table_rows, sorted_ids, sorted_pos, row_grads, ldg, row_grads_hi, ldg_hi, nullptr, last, seg_ws};
  a.th_lo = replayed_rows; a.th_hi = replayed_rows + sp; a.ld_th = ld_replayed;
  return adam_rows_launch(&a, 1, dim, id_type, n, split, 0.0, beta1, beta2, eps, (const StepStateDev*)step_state, stream);
}

// both fused tables of a NeuMF step in one launch (same dim / n / split; `last` arrays: deferred mode, `marks`: sweep mode)
extern "C" int brAdamRowsSortedPair(float* table_a, float* m_a, float* v_a, int64_t rows_a, const void* sorted_ids_a, const int32_t* sorted_pos_a,
                                    const float* grads_a, int64_t ldg_a, const float* grads_hi_a, int64_t ldg_hi_a, uint8_t* mark_a, int32_t* last_a,
                                    float* table_b, float* m_b, float* v_b, int64_t rows_b, const void* sorted_ids_b, const int32_t* sorted_pos_b,
                                    const float* grads_b, int64_t ldg_b, const float* grads_hi_b, int64_t ldg_hi_b, uint8_t* mark_b, int32_t* last_b,
                                    int dim, int id_type, int64_t n, int split, const float* hi_scale, const void* step_state, double alpha_t,
                                    double beta1, double beta2, double eps, float* seg_ws_a, float* seg_ws_b, brStream stream) {
  const AdamPairCall c{table_a, m_a, v_a, rows_a, sorted_ids_a, sorted_pos_a, grads_a, ldg_a, grads_hi_a, ldg_hi_a, mark_a, last_a,
                       table_b, m_b, v_b, rows_b, sorted_ids_b, sorted_pos_b, grads_b, ldg_b, grads_hi_b, ldg_hi_b, mark_b, last_b,
                       dim, id_type, n, split, hi_scale, step_state, alpha_t, beta1, beta2, eps, seg_ws_a, seg_ws_b};
  return adam_rows_pair_keep(c, nullptr, stream);
}

extern "C" int brAdamRowsSortedPairReplayed(float* table_a, float* m_a, float* v_a, int64_t rows_a, const void* sorted_ids_a, const int32_t* sorted_pos_a,
                                            const float* grads_a, int64_t ldg_a, const float* grads_hi_a, int64_t ldg_hi_a, int32_t* last_a,
                                            const float* replayed_a,
                                            float* table_b, float* m_b, float* v_b, int64_t rows_b, const void* sorted_ids_b, const int32_t* sorted_pos_b,
                                            const float* grads_b, int64_t ldg_b, const float* grads_hi_b, int64_t ldg_hi_b, int32_t* last_b,
                                            const float* replayed_b, int64_t ld_replayed,
                                            int dim, int id_type, int64_t n, int64_t n_b, int split, const void* step_state,
                                            double beta1, double beta2, double eps, float* seg_ws_a, float* seg_ws_b, brStream stream) {
  BR_CHECK_ARG(last_a && last_b && step_state, "brAdamRowsSortedPairReplayed: last arrays / step_state missing");
  BR_CHECK_ARG((grads_hi_a == nullptr) == (grads_hi_b == nullptr), "brAdamRowsSortedPairReplayed: gradient halves for both tables or neither");
  if (!grads_hi_a) { split = dim; grads_hi_a = grads_a; grads_hi_b = grads_b; ldg_hi_a = ldg_a; ldg_hi_b = ldg_b; }     // one source: the whole row is the low part
  BR_CHECK_ARG(split >= 1 && split <= dim, "brAdamRowsSortedPairReplayed: split out of range");
  BR_CHECK_ARG(replayed_a && replayed_b && ld_replayed >= dim && n >= 0 && n_b >= 0, "brAdamRowsSortedPairReplayed: replayed rows missing, ld < dim or n < 0");
  if (n_b == 0) n_b = n;
  if (n == 0 && n_b == 0) return BR_OK;
  AdamRowsArgs a[2] = {{table_a, m_a, v_a, rows_a, sorted_ids_a, sorted_pos_a, grads_a, ldg_a, grads_hi_a, ldg_hi_a, nullptr, last_a, seg_ws_a},
                       {table_b, m_b, v_b, rows_b, sorted_ids_b, sorted_pos_b, grads_b, ldg_b, grads_hi_b, ldg_hi_b, nullptr, last_b, seg_ws_b}};
  a[0].th_lo = replayed_a; a[0].th_hi = replayed_a + (split < dim ? split : 0); a[0].ld_th = ld_replayed;
  a[1].th_lo = replayed_b; a[1].th_hi = replayed_b + (split < dim ? split : 0); a[1].ld_th = ld_replayed;
  if (n_b != n) { a[0].n = n; a[1].n = n_b; }
  return adam_rows_launch(a, 2, dim, id_type, n > n_b ? n : n_b, split, 0.0, beta1, beta2, eps, (const StepStateDev*)step_state, stream);
}

int br::adam_rows_pair_keep(const AdamPairCall& c, const KeepArgs* keep, brStream stream, const FinalArgs* fin, bool* fin_done) {
  BR_CHECK_ARG((c.last_a == nullptr) == (c.last_b == nullptr) && (c.last_a == nullptr || c.step_state), "brAdamRowsSortedPair: last arrays for both tables (with step_state) or neither");
  BR_CHECK_ARG(c.grads_hi_a && c.grads_hi_b, "brAdamRowsSortedPair: both gradient halves required");
  const AdamRowsArgs a[2] = {{c.table_a, c.m_a, c.v_a, c.rows_a, c.sorted_ids_a, c.sorted_pos_a, c.grads_a, c.ldg_a, c.grads_hi_a, c.ldg_hi_a, c.mark_a, c.last_a, c.seg_ws_a, c.hi_scale,
                              c.th_lo_a, c.th_hi_a, c.ld_th},
                             {c.table_b, c.m_b, c.v_b, c.rows_b, c.sorted_ids_b, c.sorted_pos_b, c.grads_b, c.ldg_b, c.grads_hi_b, c.ldg_hi_b, c.mark_b, c.last_b, c.seg_ws_b, c.hi_scale,
                              c.th_lo_b, c.th_hi_b, c.ld_th}};
  return adam_rows_launch(a, 2, c.dim, c.id_type, c.n, c.split, c.alpha_t, c.beta1, c.beta2, c.eps, c.last_a ? (const StepStateDev*)c.step_state : nullptr, stream, keep,
                          fin, fin_done, c.adv);
}

extern "C" int brAdamFlush(float* table, float* m, float* v, int32_t* last, int64_t table_rows, int dim, const void* step_state,
                           double beta1, double beta2, double eps, brStream stream) {
  BR_CHECK_ARG(table && m && v && last && step_state && dim >= 1 && table_rows > 0, "brAdamFlush: bad args");
  const RowGeom g = row_geom(dim);
  const int64_t n_vec = table_rows * g.chunks;
  const int64_t blocks = std::min<int64_t>(ceil_div(n_vec, 256), 256 * 16);
  const AdamHp h = make_hp(0.0, beta1, beta2, eps);
  const StepStateDev* ss = (const StepStateDev*)step_state;
  hipStream_t s = (hipStream_t)stream;
  BR_DISPATCH_VEC(g.vec, (adam_flush_kernel<VEC><<<(unsigned)blocks, 256, 0, s>>>(table, m, v, n_vec, g.chunks, h, last, ss)));
  BR_CHECK_LAUNCH("brAdamFlush");
  fill_last_kernel<<<(unsigned)ceil_div(table_rows, 256), 256, 0, s>>>(last, table_rows, ss);
  BR_CHECK_LAUNCH("brAdamFlush(last)");
  return BR_OK;
}

extern "C" int brAdamDenseSweep(float* table, float* m, float* v, int64_t table_rows, int dim, double alpha_t,
                                double beta1, double beta2, double eps, uint8_t* mark, brStream stream) {
  BR_CHECK_ARG(table && m && v && dim >= 1 && table_rows > 0, "brAdamDenseSweep: bad args");
  const RowGeom g = row_geom(dim);
  const int64_t n_vec = table_rows * g.chunks;
  int64_t blocks = ceil_div(n_vec, 256);
  const int64_t cap = 256 * 16;  // 16 workgroups per CU, grid-stride beyond
  if (blocks > cap) blocks = cap;
  const AdamHp h = make_hp(alpha_t, beta1, beta2, eps);
  hipStream_t s = (hipStream_t)stream;
  BR_DISPATCH_VEC(g.vec, (adam_dense_sweep_kernel<VEC><<<(unsigned)blocks, 256, 0, s>>>(table, m, v, n_vec, g.chunks, h, mark)));
  BR_CHECK_LAUNCH("brAdamDenseSweep");
  if (mark) {
    // not hipMemsetAsync: a memset NODE of this (odd) size inside a captured hipGraph left garbage in the marks
    // on ROCm 7.2 when the graph started with it (tests/test_gpu_neumf.py, split replay) - a kernel node is safe
    zero_bytes_kernel<<<(unsigned)ceil_div(table_rows, 1024), 256, 0, s>>>(mark, table_rows);
    BR_CHECK_LAUNCH("brAdamDenseSweep(marks)");
  }
  return BR_OK;
}

extern "C" int brAdamFlat(float* theta, float* m, float* v, const float* g, int64_t n, double alpha_t, double beta1,
                          double beta2, double eps, brStream stream) {
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(theta && m && v && g && n > 0, "brAdamFlat: bad args");
  adam_flat_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(theta, m, v, g, n, make_hp(alpha_t, beta1, beta2, eps));
  BR_CHECK_LAUNCH("brAdamFlat");
  return BR_OK;
}

extern "C" int brAdagradRowsSorted(float* table, float* acc, int64_t table_rows, int dim, const void* sorted_ids,
                                   int id_type, const int32_t* sorted_pos, int64_t n, const float* row_grads, int64_t ldg,
                                   double lr, double eps, float* seg_ws, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brAdagradRowsSorted: bad id_type");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(table && acc && sorted_ids && sorted_pos && row_grads && dim >= 1 && ldg >= dim && table_rows > 0,
               "brAdagradRowsSorted: bad args");
  const RowGeom g = row_geom_ld(dim, vec_width({ldg, dim}, {row_grads, table, acc, seg_ws}));
  const unsigned grid = (unsigned)ceil_div(n, 256 >> g.lpr_log2);
  hipStream_t s = (hipStream_t)stream;
  if (seg_ws) {
    const SegJob job{sorted_ids, sorted_pos, row_grads, ldg, row_grads, ldg, seg_ws};
    const int rc = launch_partials(&job, 1, id_type, n, dim, g, dim, s);
    if (rc != BR_OK) return rc;
  }
  BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(g.vec, (adagrad_rows_sorted_kernel<IdT, VEC><<<grid, 256, 0, s>>>(table, acc, table_rows, dim, g.chunks, g.lpr_log2, (const IdT*)sorted_ids,
                                                                                                         sorted_pos, n, row_grads, ldg, (float)lr, (float)eps, seg_ws))));
  BR_CHECK_LAUNCH("brAdagradRowsSorted");
  return BR_OK;
}

extern "C" int brAdagradFlat(float* theta, float* acc, const float* g, int64_t n, double lr, double eps, brStream stream) {
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(theta && acc && g && n > 0, "brAdagradFlat: bad args");
  adagrad_flat_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(theta, acc, g, n, (float)lr, (float)eps);
  BR_CHECK_LAUNCH("brAdagradFlat");
  return BR_OK;
}
