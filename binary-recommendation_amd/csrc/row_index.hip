// S1 dedup row index: ids are sorted once per id stream together with their batch position (stable), and every table that shares the
// stream reuses the index (sparse_opt.hip walks it).  hipcub radix sort for long streams, chunk sort + chunk rank for a step's batch, the
// merge of already sorted runs for the fixed-capacity exchange - and the two fused launches whose grids carry the chunk sorts beside
// the step's lookup / gather.
#include "common.h"
#include "rows.h"
#include "adam_math.h"
#include "lookup_wave.h"
#include "dense.h"
#include "step_state.h"

#include <hipcub/hipcub.hpp>

namespace br {

// positions 0..n-1 and the sort keys: ids outside [0, upper) become `upper` so that they sort behind every
// valid id instead of aliasing one in the low key bits (the optimizer kernels skip ids >= table rows)
template <typename IdT>
__global__ void sort_prep_kernel(const IdT* __restrict__ ids, int64_t upper, IdT* __restrict__ keys, int32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    p[i] = (int32_t)i;
    const int64_t id = (int64_t)ids[i];
    keys[i] = (upper > 0 && (uint64_t)id >= (uint64_t)upper) ? (IdT)upper : (IdT)id;
  }
}

static inline int bits_for(int64_t upper) {
  int bits = 1;
  while (bits < 63 && ((int64_t)1 << bits) < upper) ++bits;
  return bits;
}

template <typename IdT>
static int64_t sort_temp_bytes(int64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, bytes, (const IdT*)nullptr, (IdT*)nullptr, (const int32_t*)nullptr,
                                     (int32_t*)nullptr, (int)n, 0, (int)sizeof(IdT) * 8, (hipStream_t)0);
  return (int64_t)bytes;
}

}  // namespace br

using namespace br;

static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// ---- dedup index for small batches: 2 launches instead of hipcub's ~10 per id stream ------------------------
// hipcub::DeviceRadixSort on 65 536 pairs is a block sort + 6 merge passes (+ iota): ~10 launches of ~5 us each,
// and a hipGraph replay runs them on the critical path (rocprofv3 timeline, ROCm 7.2).  For n <= kRankMaxN:
//   K1 chunk_sort_kernel : every workgroup radix-sorts one chunk of (id, position) pairs in LDS (stable);
//   K2 chunk_rank_kernel : the final rank of an element = its index in its chunk + for every other chunk the
//                          number of keys that sort before it (binary search: "<=" in earlier chunks, "<" in
//                          later ones = stable), then one scatter.
// Chunk size: 2048 pairs (256 threads) up to 16 384 keys, 8192 pairs (1024 threads) above.  Round 1 used 2048 throughout:
// at n = 65 536 that is 31 other chunks x 11 probes = 341 dependent L2 probes per key, 25 us alone and 90 us beside the
// MLP kernels it overlaps (15 % of all GPU time in the rocprofv3 trace).  8 chunks of 8192 need 7 x 13 = 91 probes.
// Both id streams of a step share the two launches (blockIdx.y).  Out-of-range ids get the key `upper`
// (>= table rows: the optimizer kernels skip them), so only bits_for(upper + 2) key bits are sorted.
constexpr int kChunkS = 2048, kThreadsS = 256, kChunkL = 8192, kThreadsL = 1024, kRankMaxChunks = 64;
constexpr int64_t kChunkSwitchN = 16384;
constexpr int64_t kRankMaxN = (int64_t)kChunkL * kRankMaxChunks;
struct IdxJob {
  const void* ids;
  void* sorted_ids;
  int32_t* sorted_pos;
  uint32_t* ck;       // [n] chunk-sorted keys
  uint32_t* cp;       // [n] their positions
  uint32_t upper;     // ids are valid in [0, upper)
  int end_bit;
  // segmented id arrays (brRowIndexBuildPairSeg): logical position t sits at element seg_phys(t) of `ids`, and the index carries
  // that PHYSICAL position (the optimizer reads gradient rows by it); seg_len == 0: contiguous
  int64_t seg_len = 0, seg_stride = 0, seg_off = 0;
  int64_t n = 0;      // this stream's keys when the two streams of a launch differ in length (0: the launch's n)
  int n_chunks = 0;   // its chunk count then
};

// the id streams of a launch (blockIdx.y, or the sort workgroups' stream number): two of a step - or the two of every step of a
// multi-step group, whose head builds all of them (streams 2 k and 2 k + 1: step k).  Passed by value: 16 jobs are 1.4 KB of the 4 KB
constexpr int kIdxJobsMax = 2 * BR_GROUP_MAX;
struct IdxJobs { IdxJob j[kIdxJobsMax]; };

// chunk `chunk` of id stream `which` by the calling workgroup of kSortThreads threads
template <typename IdT, int kChunk, int kSortThreads>
__device__ __forceinline__ void chunk_sort_block(const IdxJobs& jobs, int64_t n, int chunk, int which) {
  constexpr int IPT = kChunk / kSortThreads;
  using Sort = hipcub::BlockRadixSort<uint32_t, kSortThreads, IPT, uint32_t>;
  __shared__ typename Sort::TempStorage tmp;
  const IdxJob& job = jobs.j[which];
  if (job.n) n = job.n;
  const IdT* ids = (const IdT*)job.ids;
  const int64_t base = (int64_t)chunk * kChunk + threadIdx.x * IPT;
  uint32_t k[IPT], p[IPT];
#pragma unroll
  for (int q = 0; q < IPT; ++q) {
    const int64_t e = base + q;
    const int64_t pe = seg_phys(e, job.seg_len, job.seg_stride, job.seg_off);
    const int64_t id = e < n ? (int64_t)ids[pe] : -1;
    k[q] = e < n ? (((uint64_t)id < (uint64_t)job.upper) ? (uint32_t)id : job.upper) : job.upper + 1u;   // padding sorts last
    p[q] = (uint32_t)pe;
  }
  Sort(tmp).Sort(k, p, 0, job.end_bit);
#pragma unroll
  for (int q = 0; q < IPT; ++q)
    if (base + q < n) { job.ck[base + q] = k[q]; job.cp[base + q] = p[q]; }
}
template <typename IdT, int kChunk, int kSortThreads>
__global__ __launch_bounds__(kSortThreads) void chunk_sort_kernel(IdxJobs jobs, int64_t n) {
  chunk_sort_block<IdT, kChunk, kSortThreads>(jobs, n, (int)blockIdx.x, (int)blockIdx.y);
}

// The deferred NeuMF lookup and the chunk sorts of the step's two id streams in ONE launch of 1024-thread workgroups: the first
// 2 * n_chunks workgroups each sort a chunk (they start first and run ~37 us on 16 CUs), the rest are lookup workgroups of 16 waves =
// 16 pairs that flow around them.  As a launch of their own on a side stream the sorts needed a fork and a join in the step's
// hipGraph (~10 us each on the main branch, ROCm 7.2) and stretched the lookup they ran beside; the chunk-rank launch follows on the
// same stream.  LDS: the sort's image is reserved by every workgroup (two per CU = 32 waves: the lookup's full occupancy anyway).
// n_streams: 2, or 2 S at the head of a group of S steps (all streams of n ids: the lookup workgroups serve the head's pairs only).
template <typename IdT, int VEC, int R>
__global__ __launch_bounds__(kThreadsL, 8) void lookup_sort_kernel(const LookupArgs a, IdxJobs jobs, int64_t n, int n_chunks, int n_streams) {
  const int n_sort = n_streams * n_chunks;
  if ((int)blockIdx.x < n_sort) {
    chunk_sort_block<IdT, kChunkL, kThreadsL>(jobs, n, (int)blockIdx.x % n_chunks, (int)blockIdx.x / n_chunks);
    return;
  }
  const int64_t b = (((int64_t)blockIdx.x - n_sort) * (kThreadsL / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * (R < 1 ? 1 : R);
  if (b >= a.batch) return;
  if constexpr (R == 0) {      // embed_dim 64: both rows of the pair side by side (lookup_half_pair); exact replay keeps the form above
    if (a.ss->fast) lookup_half_pair<IdT>(a, b, (int)(threadIdx.x & 63));
    else lookup_wave_pair<IdT, VEC>(a, b, (int)(threadIdx.x & 63));
  } else if constexpr (R == 1) lookup_wave_pair<IdT, VEC>(a, b, (int)(threadIdx.x & 63));
  else lookup_wave_pairs<IdT, VEC, R>(a, b, (int)(threadIdx.x & 63));
}
// form of the fused lookup at embed_dim 64: BR_LOOKUP_PAIRS = 1 (default: one pair per wave, lookup_wave_pair) | 2 (two pairs per wave) |
// 0 (lookup_half_pair: both rows of the pair side by side, 16 B per lane).  Measured at config 2, same bits in all three: 68-69 us | 70.5 us |
// 86-88 us - the half-wave form halves the load instructions but replays four elements per lane over max(lag_u, lag_i) steps with a
// per-lane alpha select.  (Taken while every form still fetched the step state per row and the alphas per group where they were used,
// lookup_wave.h LOOKUP WAITS: they rank the three forms, they do not show what bounds the launch.)
static int lookup_pairs_per_wave() {
  static const int r = [] { const char* e = getenv("BR_LOOKUP_PAIRS"); const int v = e ? atoi(e) : 1; return (v == 0 || v == 2) ? v : 1; }();
  return r;
}

// Two deferred gathers of one row width (rows of 64 * VEC floats, one wave per row) and the chunk sorts of their two id streams in ONE
// launch of 1024-thread workgroups - the BPR step's user gather (B rows) and [pos | neg] item gather (2 B rows): the first workgroups each
// sort a chunk, the rest gather 16 rows each and flow around them; the chunk-rank launch (+ the step-state advance) follows on the same
// stream.  As launches of their own on two side streams the sorts and ranks were 42 % of the step's kernel time and cost a fork / join
// inside the step's hipGraph.
// rows per wave of the fused gather: 1 KB of row per wave and table (dim 64: four rows)
template <int VEC> constexpr int kGatherRowsPerWave = VEC == 1 ? 4 : (VEC == 2 ? 2 : 1);
template <typename IdT, int VEC>
__global__ __launch_bounds__(kThreadsL) void gather_sort_kernel(const GatherDefJobs gj, const StepStateDev* __restrict__ ss, const AdamHp h, int64_t ld_out, int* err,
                                                                IdxJobs jobs, int n_sort_a, int n_sort_b, bool gather_group4_enabled) {
  const int n_sort = n_sort_a + n_sort_b;
  if ((int)blockIdx.x < n_sort) {
    const int which = (int)blockIdx.x < n_sort_a ? 0 : 1;
    chunk_sort_block<IdT, kChunkL, kThreadsL>(jobs, 0, which ? (int)blockIdx.x - n_sort_a : (int)blockIdx.x, which);
    return;
  }
  constexpr int R = kGatherRowsPerWave<VEC>;
  const int64_t b0 = (((int64_t)blockIdx.x - n_sort) * (kThreadsL / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * R;
  if (b0 >= gj.j[0].n + gj.j[1].n) return;
  if constexpr (VEC == 1) {      // 256-B rows: four rows side by side at 16 B per lane under the fast replay (gather_deferred_group4)
    if (ss->fast && (ld_out & 3) == 0 && gather_group4_enabled) { gather_deferred_group4<IdT>(gj, b0, (int)(threadIdx.x & 63), ss, h, ld_out, err); return; }
  }
  gather_deferred_wave_rows<IdT, VEC, R>(gj, b0, (int)(threadIdx.x & 63), ss, h, ld_out, err);
}

// adv.st != NULL: the grid has one extra column of workgroups, whose y = 0 member advances the step state (nothing in this launch reads it;
// the lookup in front computed its step as ss->step + 1, everything behind sees the advanced state) - one launch less per step.
// Head of a multi-step group (gridDim.y = all the group's streams): members 1 .. adv.n_more of that column clear the later steps' scratch
template <typename IdT, int kChunk>
__global__ __launch_bounds__(256) void chunk_rank_kernel(IdxJobs jobs, int64_t n, int n_chunks, const StepAdvance adv) {      // (n: the longer stream's keys)
  if (adv.st && blockIdx.x == gridDim.x - 1) {
    if (blockIdx.y == 0) step_state_advance_block(adv);
    else if ((int)blockIdx.y <= adv.n_more) step_state_zero_more(adv, (int)blockIdx.y - 1);
    return;
  }
  const IdxJob& job = jobs.j[blockIdx.y];
  if (job.n) { n = job.n; n_chunks = job.n_chunks; }
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e / kChunk);
  const uint32_t key = job.ck[e];
  uint32_t rank = (uint32_t)(e - (int64_t)c * kChunk);
  constexpr int G = 8;                                   // chunks searched together (independent probes in flight per step)
  for (int c0 = 0; c0 < n_chunks; c0 += G) {
    uint32_t lo[G], len[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int cc = c0 + u;
      const int64_t left = n - (int64_t)cc * kChunk;
      len[u] = (cc < n_chunks && cc != c) ? (uint32_t)(left < kChunk ? left : kChunk) : 0u;
      lo[u] = 0u;
    }
#pragma unroll
    for (int step = kChunk; step > 0; step >>= 1) {
      // the G probes of a step are issued first, then the G bounds move - as arithmetic, not predicated moves
      // (47 -> 38 us for the pair; more chunks per step, more lanes per element or an LDS splitter level were all slower)
      uint32_t v[G];
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const uint32_t idx = lo[u] + (uint32_t)step;
        const uint32_t at = idx <= len[u] ? idx - 1u : 0u;                          // clamped probe, branch-free
        v[u] = job.ck[(int64_t)(c0 + u < n_chunks ? c0 + u : 0) * kChunk + at];
      }
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const uint32_t idx = lo[u] + (uint32_t)step;
        const uint32_t lt = (c0 + u < c) ? (v[u] <= key ? 1u : 0u) : (v[u] < key ? 1u : 0u);   // earlier chunk: ties sort before
        lo[u] += (idx <= len[u] ? lt : 0u) * (uint32_t)step;
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) rank += lo[u];
  }
  ((IdT*)job.sorted_ids)[rank] = (IdT)key;
  job.sorted_pos[rank] = (int32_t)job.cp[e];
}

static bool rank_path_ok(int64_t n, int64_t upper) { return n <= kRankMaxN && upper > 0 && upper < ((int64_t)1 << 31) - 2; }

static int index_build_rank(IdxJobs& jobs, int n_jobs, int id_type, int64_t n, hipStream_t s) {
  const bool large = n > kChunkSwitchN;
  const int n_chunks = (int)ceil_div(n, large ? kChunkL : kChunkS);
  const dim3 g1((unsigned)n_chunks, (unsigned)n_jobs), g2((unsigned)ceil_div(n, 256), (unsigned)n_jobs);
  BR_DISPATCH_ID(id_type, {
    if (large) { chunk_sort_kernel<IdT, kChunkL, kThreadsL><<<g1, kThreadsL, 0, s>>>(jobs, n); probe_split(BR_TAG_INDEX_SORT, s); chunk_rank_kernel<IdT, kChunkL><<<g2, 256, 0, s>>>(jobs, n, n_chunks, StepAdvance{}); }
    else { chunk_sort_kernel<IdT, kChunkS, kThreadsS><<<g1, kThreadsS, 0, s>>>(jobs, n); probe_split(BR_TAG_INDEX_SORT, s); chunk_rank_kernel<IdT, kChunkS><<<g2, 256, 0, s>>>(jobs, n, n_chunks, StepAdvance{}); }
  });
  BR_CHECK_LAUNCH("brRowIndexBuild");
  return BR_OK;
}
static IdxJob make_job(const void* ids, void* sorted_ids, int32_t* sorted_pos, void* workspace, int64_t n, int64_t upper) {
  IdxJob j{};
  j.ids = ids; j.sorted_ids = sorted_ids; j.sorted_pos = sorted_pos;
  j.ck = (uint32_t*)workspace;
  j.cp = (uint32_t*)((char*)workspace + align256(n * 4));
  j.upper = (uint32_t)upper;
  j.end_bit = bits_for(upper + 2);
  return j;
}

extern "C" int64_t brRowIndexWorkspaceBytes(int64_t n, int id_type) {
  if (n <= 0) return 256;
  const int64_t iota = align256(n * 4);
  const int64_t tmp = id_type == BR_IDS_I64 ? sort_temp_bytes<int64_t>(n) : sort_temp_bytes<int32_t>(n);
  const int64_t rank = 2 * align256(n * 4);       // chunk-sorted keys + positions (small-batch path)
  const int64_t sort = iota + align256(n * 8) + align256(tmp);
  return (sort > rank ? sort : rank) + 256;
}

extern "C" int brRowIndexBuild(const void* ids, int id_type, int64_t n, int64_t id_upper_bound, void* sorted_ids,
                               int32_t* sorted_pos, void* workspace, int64_t workspace_bytes, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brRowIndexBuild: bad id_type");
  BR_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "brRowIndexBuild: n out of range");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(ids && sorted_ids && sorted_pos && workspace, "brRowIndexBuild: null pointer");
  const int64_t need = brRowIndexWorkspaceBytes(n, id_type);
  if (workspace_bytes < need) {
    set_error("brRowIndexBuild: workspace %lld < required %lld", (long long)workspace_bytes, (long long)need);
    return BR_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (rank_path_ok(n, id_upper_bound)) {
    IdxJobs jobs;
    jobs.j[0] = jobs.j[1] = make_job(ids, sorted_ids, sorted_pos, workspace, n, id_upper_bound);
    return index_build_rank(jobs, 1, id_type, n, s);
  }
  int32_t* iota = (int32_t*)workspace;
  void* keys = (char*)workspace + align256(n * 4);
  void* tmp = (char*)keys + align256(n * 8);
  size_t tmp_bytes = (size_t)(workspace_bytes - align256(n * 4) - align256(n * 8));
  const int end_bit_cap = (id_type == BR_IDS_I64 ? 64 : 32);
  int end_bit = id_upper_bound > 0 ? bits_for(id_upper_bound + 1) : end_bit_cap;
  if (end_bit > end_bit_cap) end_bit = end_bit_cap;
  hipError_t e;
  BR_DISPATCH_ID(id_type, {
    sort_prep_kernel<IdT><<<(unsigned)ceil_div(n, 256), 256, 0, s>>>((const IdT*)ids, id_upper_bound, (IdT*)keys, iota, n);
    e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const IdT*)keys, (IdT*)sorted_ids, (const int32_t*)iota, sorted_pos, (int)n, 0, end_bit, s);
  });
  if (e != hipSuccess) {
    set_error("brRowIndexBuild: radix sort failed: %s", hipGetErrorString(e));
    return BR_ERR_HIP;
  }
  BR_CHECK_LAUNCH("brRowIndexBuild");
  return BR_OK;
}

extern "C" int brRowIndexBuildPair(const void* ids_a, int64_t upper_a, void* sorted_ids_a, int32_t* sorted_pos_a, void* ws_a, int64_t ws_a_bytes,
                                   const void* ids_b, int64_t upper_b, void* sorted_ids_b, int32_t* sorted_pos_b, void* ws_b, int64_t ws_b_bytes,
                                   int id_type, int64_t n, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brRowIndexBuildPair: bad id_type");
  if (n == 0) return BR_OK;
  if (rank_path_ok(n, upper_a) && rank_path_ok(n, upper_b)) {
    BR_CHECK_ARG(ids_a && ids_b && sorted_ids_a && sorted_ids_b && sorted_pos_a && sorted_pos_b && ws_a && ws_b, "brRowIndexBuildPair: null pointer");
    const int64_t need = brRowIndexWorkspaceBytes(n, id_type);
    if (ws_a_bytes < need || ws_b_bytes < need) {
      set_error("brRowIndexBuildPair: workspace < required %lld", (long long)need);
      return BR_ERR_WORKSPACE;
    }
    IdxJobs jobs;
    jobs.j[0] = make_job(ids_a, sorted_ids_a, sorted_pos_a, ws_a, n, upper_a);
    jobs.j[1] = make_job(ids_b, sorted_ids_b, sorted_pos_b, ws_b, n, upper_b);
    return index_build_rank(jobs, 2, id_type, n, (hipStream_t)stream);
  }
  const int rc = brRowIndexBuild(ids_a, id_type, n, upper_a, sorted_ids_a, sorted_pos_a, ws_a, ws_a_bytes, stream);
  return rc != BR_OK ? rc : brRowIndexBuild(ids_b, id_type, n, upper_b, sorted_ids_b, sorted_pos_b, ws_b, ws_b_bytes, stream);
}

// The same pair of indexes over SEGMENTED id arrays: both streams of a row-sharded step arrive in ONE all-to-all buffer laid out
// [source rank][stream][cap] (parallel.py PaddedExchange), so stream k's logical position t = src * cap + j sits at element
// (src * 2 + k) * cap + j.  sorted_pos holds that physical element index: the owner's optimizer reads the received gradient rows (same
// layout, one buffer for both streams) by it.  Stable in logical = physical order.
extern "C" int brRowIndexBuildPairSeg(const void* ids_a, int64_t upper_a, void* sorted_ids_a, int32_t* sorted_pos_a, void* ws_a, int64_t ws_a_bytes,
                                      const void* ids_b, int64_t upper_b, void* sorted_ids_b, int32_t* sorted_pos_b, void* ws_b, int64_t ws_b_bytes,
                                      int id_type, int64_t n, int64_t seg_len, int64_t seg_stride, int64_t seg_off_a, int64_t seg_off_b, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brRowIndexBuildPairSeg: bad id_type");
  BR_CHECK_ARG(seg_len >= 1 && seg_stride >= seg_len && seg_off_a >= 0 && seg_off_b >= 0, "brRowIndexBuildPairSeg: bad segment geometry");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(ids_a && ids_b && sorted_ids_a && sorted_ids_b && sorted_pos_a && sorted_pos_b && ws_a && ws_b, "brRowIndexBuildPairSeg: null pointer");
  BR_CHECK_ARG(rank_path_ok(n, upper_a) && rank_path_ok(n, upper_b) && seg_phys(n - 1, seg_len, seg_stride, seg_off_a > seg_off_b ? seg_off_a : seg_off_b) < ((int64_t)1 << 31),
               "brRowIndexBuildPairSeg: n <= %lld positions and id bounds < 2^31 - 2", (long long)kRankMaxN);
  const int64_t need = brRowIndexWorkspaceBytes(n, id_type);
  if (ws_a_bytes < need || ws_b_bytes < need) { set_error("brRowIndexBuildPairSeg: workspace < required %lld", (long long)need); return BR_ERR_WORKSPACE; }
  IdxJobs jobs;
  jobs.j[0] = make_job(ids_a, sorted_ids_a, sorted_pos_a, ws_a, n, upper_a);
  jobs.j[1] = make_job(ids_b, sorted_ids_b, sorted_pos_b, ws_b, n, upper_b);
  jobs.j[0].seg_len = jobs.j[1].seg_len = seg_len; jobs.j[0].seg_stride = jobs.j[1].seg_stride = seg_stride;
  jobs.j[0].seg_off = seg_off_a; jobs.j[1].seg_off = seg_off_b;
  return index_build_rank(jobs, 2, id_type, n, (hipStream_t)stream);
}

// ---- the same index when every segment of the array is ALREADY sorted ascending (the fixed-capacity exchange: a requester sends each
// owner its distinct local rows in key order, pads = the spare row = the largest id, behind them): the W segments of a stream are W sorted
// runs, so the index is their merge - rank(e) = position in its own run + the number of smaller keys (earlier runs: smaller or equal) in
// every other run, one binary search each - and the 35 us chunk sort of brRowIndexBuildPairSeg is not needed.  Output identical to it
// (stable in logical order).  A run that is not sorted sets BR_ERRFLAG_RANGE in *err_flag (the index is then wrong).
template <typename IdT>
__global__ __launch_bounds__(256) void run_rank_kernel(IdxJobs jobs, int64_t n, int64_t run_len, int n_runs, int steps, int* err) {
  const IdxJob& job = jobs.j[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const IdT* __restrict__ ids = (const IdT*)job.ids;
  auto key_at = [&](int64_t t) -> uint32_t {
    const int64_t id = (int64_t)ids[seg_phys(t, job.seg_len, job.seg_stride, job.seg_off)];
    return ((uint64_t)id < (uint64_t)job.upper) ? (uint32_t)id : job.upper;
  };
  const int r = (int)(e / run_len);
  const int64_t i = e - (int64_t)r * run_len;
  const uint32_t key = key_at(e);
  if (i > 0 && key_at(e - 1) > key && err) atomicOr(err, BR_ERRFLAG_RANGE);
  uint32_t rank = (uint32_t)i;
  constexpr int G = 8;                                   // runs searched together (independent probes in flight per step)
  for (int r0 = 0; r0 < n_runs; r0 += G) {
    uint32_t lo[G], len[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int rr = r0 + u;
      const int64_t left = n - (int64_t)rr * run_len;
      len[u] = (rr < n_runs && rr != r) ? (uint32_t)(left < run_len ? left : run_len) : 0u;
      lo[u] = 0u;
    }
    for (int st = steps - 1; st >= 0; --st) {
      const uint32_t step = 1u << st;
      uint32_t v[G];
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const uint32_t idx = lo[u] + step;
        const uint32_t at = idx <= len[u] ? idx - 1u : 0u;                          // clamped probe, branch-free
        v[u] = key_at((int64_t)(r0 + u < n_runs ? r0 + u : 0) * run_len + at);
      }
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const uint32_t idx = lo[u] + step;
        const uint32_t lt = (r0 + u < r) ? (v[u] <= key ? 1u : 0u) : (v[u] < key ? 1u : 0u);   // earlier run: ties sort before
        lo[u] += (idx <= len[u] ? lt : 0u) * step;
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) rank += lo[u];
  }
  ((IdT*)job.sorted_ids)[rank] = (IdT)key;
  job.sorted_pos[rank] = (int32_t)seg_phys(e, job.seg_len, job.seg_stride, job.seg_off);
}

extern "C" int brRowIndexMergePairSeg(const void* ids_a, int64_t upper_a, void* sorted_ids_a, int32_t* sorted_pos_a, const void* ids_b, int64_t upper_b,
                                      void* sorted_ids_b, int32_t* sorted_pos_b, int id_type, int64_t n, int64_t seg_len, int64_t seg_stride, int64_t seg_off_a,
                                      int64_t seg_off_b, int* err_flag, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brRowIndexMergePairSeg: bad id_type");
  BR_CHECK_ARG(seg_len >= 1 && seg_stride >= seg_len && seg_off_a >= 0 && seg_off_b >= 0, "brRowIndexMergePairSeg: bad segment geometry");
  if (n == 0) return BR_OK;
  BR_CHECK_ARG(ids_a && ids_b && sorted_ids_a && sorted_ids_b && sorted_pos_a && sorted_pos_b, "brRowIndexMergePairSeg: null pointer");
  BR_CHECK_ARG(upper_a > 0 && upper_b > 0 && upper_a < ((int64_t)1 << 31) - 2 && upper_b < ((int64_t)1 << 31) - 2 && n < ((int64_t)1 << 31) &&
                   seg_phys(n - 1, seg_len, seg_stride, seg_off_a > seg_off_b ? seg_off_a : seg_off_b) < ((int64_t)1 << 31),
               "brRowIndexMergePairSeg: positions and id bounds < 2^31 - 2");
  IdxJobs jobs;
  jobs.j[0].ids = ids_a; jobs.j[0].sorted_ids = sorted_ids_a; jobs.j[0].sorted_pos = sorted_pos_a; jobs.j[0].upper = (uint32_t)upper_a;
  jobs.j[1].ids = ids_b; jobs.j[1].sorted_ids = sorted_ids_b; jobs.j[1].sorted_pos = sorted_pos_b; jobs.j[1].upper = (uint32_t)upper_b;
  jobs.j[0].ck = jobs.j[1].ck = nullptr; jobs.j[0].cp = jobs.j[1].cp = nullptr; jobs.j[0].end_bit = jobs.j[1].end_bit = 0;
  jobs.j[0].seg_len = jobs.j[1].seg_len = seg_len; jobs.j[0].seg_stride = jobs.j[1].seg_stride = seg_stride;
  jobs.j[0].seg_off = seg_off_a; jobs.j[1].seg_off = seg_off_b;
  const int n_runs = (int)ceil_div(n, seg_len);
  int steps = 0;
  while (((int64_t)1 << steps) <= seg_len) ++steps;       // 2^steps > seg_len: the search covers every length <= seg_len
  const dim3 grid((unsigned)ceil_div(n, 256), 2);
  hipStream_t s = (hipStream_t)stream;
  BR_DISPATCH_ID(id_type, (run_rank_kernel<IdT><<<grid, 256, 0, s>>>(jobs, n, seg_len, n_runs, steps, err_flag)));
  BR_CHECK_LAUNCH("brRowIndexMergePairSeg");
  return BR_OK;
}

// neumf_step.cpp: lookup + both dedup indexes on one stream (lookup_sort_kernel, then the chunk-rank launch).  supported(): the wave
// lookup's shapes, the large-chunk sort's range, BR_FUSED_SORT != 0.
bool br::lookup_with_index_supported(int dim, int64_t n, int64_t upper_a, int64_t upper_b, int64_t ld_stash, const void* x0, const void* stash_a,
                                     const void* stash_b) {
  // DELIBERATELY not cached in a static, unlike BR_LOOKUP_PAIRS, BR_LOOKUP_SPEC and BR_GATHER_GROUP4: it is read on every call (eager steps
  // and captures only: a replayed graph does not come here), so that one process can run the same engine both ways
  // (tests/test_gpu_lookup_chain.py, as tests/test_gpu_twotower_bpr.py does with the BPR step).  A change of the variable takes effect at
  // the next eager step or capture.
  const char* e = getenv("BR_FUSED_SORT");
  const bool on = !(e && e[0] == '0');
  const int wvec = wave_pair_vec(dim);      // (units of 32 floats: a lane owns the same columns of the user row and the item row)
  return on && wave_rows_enabled() && wvec && ld_stash % wvec == 0 &&
         ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(stash_a) | reinterpret_cast<uintptr_t>(stash_b)) & (4 * wvec - 1)) == 0 &&
         n > kChunkSwitchN && rank_path_ok(n, upper_a) && rank_path_ok(n, upper_b);
}
int br::lookup_index_chunks(int64_t n) { return (int)ceil_div(n, kChunkL); }
int br::lookup_with_index(const LookupArgs& la, int dim, int id_type, const IndexPairArgs& ix, brStream stream, const StepAdvance* adv,
                          const GroupIndexArgs* later) {
  const int64_t n = la.batch;
  const int n_later = later ? later->n : 0;
  BR_CHECK_ARG(n_later >= 0 && n_later < BR_GROUP_MAX, "lookup_with_index: at most %d steps per group", (int)BR_GROUP_MAX);
  const int64_t need = brRowIndexWorkspaceBytes(n, id_type);
  IdxJobs jobs;
  for (int k = 0; k <= n_later; ++k) {      // streams 2 k, 2 k + 1: step k of the group (0: this step)
    const IndexPairArgs& x = k ? later->ix[k - 1] : ix;
    const void* users = k ? later->users[k - 1] : la.users;
    const void* items = k ? later->items[k - 1] : la.items;
    BR_CHECK_ARG(x.sorted_ids_a && x.sorted_ids_b && x.sorted_pos_a && x.sorted_pos_b && x.ws_a && x.ws_b && (!k || (users && items)), "lookup_with_index: null pointer");
    if (x.ws_a_bytes < need || x.ws_b_bytes < need) { set_error("lookup_with_index: workspace < required %lld", (long long)need); return BR_ERR_WORKSPACE; }
    jobs.j[2 * k] = make_job(users, x.sorted_ids_a, x.sorted_pos_a, x.ws_a, n, la.user_rows);
    jobs.j[2 * k + 1] = make_job(items, x.sorted_ids_b, x.sorted_pos_b, x.ws_b, n, la.item_rows);
  }
  const int n_streams = 2 * (n_later + 1);
  const StepAdvance av = adv ? *adv : StepAdvance{};
  BR_CHECK_ARG(av.n_more >= 0 && av.n_more <= n_later && (av.n_more == 0 || av.st), "lookup_with_index: scratch buffers of later steps without their streams");
  const int n_chunks = (int)ceil_div(n, kChunkL);
  hipStream_t s = (hipStream_t)stream;
  const int wvec = wave_pair_vec(dim);      // (lookup_with_index_supported: 2 or 4)
  const int ppw = wvec == 2 ? lookup_pairs_per_wave() : 1;
  const unsigned grid = (unsigned)(n_streams * n_chunks + ceil_div(ceil_div(n, (int64_t)(ppw < 1 ? 1 : ppw)), (int64_t)(kThreadsL / 64)));
  BR_DISPATCH_ID(id_type, {
    if (wvec == 2 && ppw == 0) lookup_sort_kernel<IdT, 2, 0><<<grid, kThreadsL, 0, s>>>(la, jobs, n, n_chunks, n_streams);
    else if (wvec == 2 && ppw == 2) lookup_sort_kernel<IdT, 2, 2><<<grid, kThreadsL, 0, s>>>(la, jobs, n, n_chunks, n_streams);
    else if (wvec == 2) lookup_sort_kernel<IdT, 2, 1><<<grid, kThreadsL, 0, s>>>(la, jobs, n, n_chunks, n_streams);
    else lookup_sort_kernel<IdT, 4, 1><<<grid, kThreadsL, 0, s>>>(la, jobs, n, n_chunks, n_streams);
  });
  BR_CHECK_LAUNCH("lookup_with_index(lookup + sort)");
  probe_split(BR_TAG_EMBED_FWD, s);
  const dim3 g2((unsigned)(ceil_div(n, 256) + (av.st ? 1 : 0)), (unsigned)n_streams);
  BR_DISPATCH_ID(id_type, (chunk_rank_kernel<IdT, kChunkL><<<g2, 256, 0, s>>>(jobs, n, n_chunks, av)));
  BR_CHECK_LAUNCH("lookup_with_index(rank)");
  return BR_OK;
}

extern "C" int brGatherRowsDeferredPairWithIndex(const float* table_a, const float* m_a, const float* v_a, const int32_t* last_a, int64_t rows_a, const void* ids_a,
                                                 float* out_a, void* sorted_ids_a, int32_t* sorted_pos_a, void* ws_a, int64_t ws_a_bytes, const float* table_b,
                                                 const float* m_b, const float* v_b, const int32_t* last_b, int64_t rows_b, const void* ids_b, float* out_b,
                                                 void* sorted_ids_b, int32_t* sorted_pos_b, void* ws_b, int64_t ws_b_bytes, int dim, int id_type, int64_t n_a, int64_t n_b,
                                                 void* step_state, int advance, double lr, double beta1, double beta2, double eps, int64_t ld_out, int* err_flag,
                                                 brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brGatherRowsDeferredPairWithIndex: bad id_type");
  BR_CHECK_ARG(table_a && m_a && v_a && last_a && ids_a && out_a && sorted_ids_a && sorted_pos_a && ws_a && table_b && m_b && v_b && last_b && ids_b && out_b &&
                   sorted_ids_b && sorted_pos_b && ws_b && step_state && rows_a > 0 && rows_b > 0 && n_a > 0 && n_b > 0 && ld_out >= dim,
               "brGatherRowsDeferredPairWithIndex: bad args");
  const int wvec = wave_row_vec(dim);
  BR_CHECK_ARG(wvec && ld_out % wvec == 0 && ((reinterpret_cast<uintptr_t>(out_a) | reinterpret_cast<uintptr_t>(out_b)) & (4 * wvec - 1)) == 0,
               "brGatherRowsDeferredPairWithIndex: rows of 64 / 128 / 256 floats (one wave per row)");
  BR_CHECK_ARG(rank_path_ok(n_a, rows_a) && rank_path_ok(n_b, rows_b), "brGatherRowsDeferredPairWithIndex: at most %lld ids per stream, table rows < 2^31 - 2", (long long)kRankMaxN);
  if (ws_a_bytes < brRowIndexWorkspaceBytes(n_a, id_type) || ws_b_bytes < brRowIndexWorkspaceBytes(n_b, id_type)) {
    set_error("brGatherRowsDeferredPairWithIndex: index workspace too small");
    return BR_ERR_WORKSPACE;
  }
  GatherDefJobs G;
  G.j[0] = GatherDefJob{table_a, m_a, v_a, last_a, rows_a, ids_a, out_a, n_a};
  G.j[1] = GatherDefJob{table_b, m_b, v_b, last_b, rows_b, ids_b, out_b, n_b};
  G.step_add = advance ? 1u : 0u;
  IdxJobs jobs;
  jobs.j[0] = make_job(ids_a, sorted_ids_a, sorted_pos_a, ws_a, n_a, rows_a);
  jobs.j[1] = make_job(ids_b, sorted_ids_b, sorted_pos_b, ws_b, n_b, rows_b);
  const int ca = (int)ceil_div(n_a, kChunkL), cb = (int)ceil_div(n_b, kChunkL);
  jobs.j[0].n = n_a; jobs.j[0].n_chunks = ca; jobs.j[1].n = n_b; jobs.j[1].n_chunks = cb;
  const AdamHp h = make_hp(0.0, beta1, beta2, eps);
  StepStateDev* ss = (StepStateDev*)step_state;
  hipStream_t s = (hipStream_t)stream;
  const int rpw = wvec == 1 ? 4 : (wvec == 2 ? 2 : 1);      // kGatherRowsPerWave
  static const bool g4env = [] { const char* e = getenv("BR_GATHER_GROUP4"); return !(e && e[0] == '0'); }();
  const bool g4 = g4env && ((reinterpret_cast<uintptr_t>(table_a) | reinterpret_cast<uintptr_t>(table_b) | reinterpret_cast<uintptr_t>(m_a) | reinterpret_cast<uintptr_t>(m_b) |
                             reinterpret_cast<uintptr_t>(v_a) | reinterpret_cast<uintptr_t>(v_b) | reinterpret_cast<uintptr_t>(out_a) | reinterpret_cast<uintptr_t>(out_b)) & 15) == 0;
  const unsigned grid = (unsigned)(ca + cb + ceil_div(ceil_div(n_a + n_b, (int64_t)rpw), (int64_t)(kThreadsL / 64)));
  BR_DISPATCH_ID(id_type, BR_DISPATCH_VEC(wvec, (gather_sort_kernel<IdT, VEC><<<grid, kThreadsL, 0, s>>>(G, ss, h, ld_out, err_flag, jobs, ca, cb, g4))));
  BR_CHECK_LAUNCH("brGatherRowsDeferredPairWithIndex(gather + sort)");
  StepAdvance av;
  if (advance) { av.st = ss; av.lr = lr; av.b1 = beta1; av.b2 = beta2; }
  const int64_t nmax = n_a > n_b ? n_a : n_b;
  const dim3 g2((unsigned)(ceil_div(nmax, 256) + (advance ? 1 : 0)), 2);
  BR_DISPATCH_ID(id_type, (chunk_rank_kernel<IdT, kChunkL><<<g2, 256, 0, s>>>(jobs, nmax, ca > cb ? ca : cb, av)));
  BR_CHECK_LAUNCH("brGatherRowsDeferredPairWithIndex(rank)");
  return BR_OK;
}
