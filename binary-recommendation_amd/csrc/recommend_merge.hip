// Catalogue top-k scored where the item rows live (include/binrec.h "Catalogue top-k on row-sharded engines"): each of W owners runs
// the fused launch of recommend.hip / recommend_dot.hip over ITS candidates; the two entry points here turn the W shard-local answers
// into the answer of one launch over the whole candidate list.
//
//   brCsrSplitByOwner: the exclusion CSR of the global candidate list -> the CSR of one owner's candidates, in that owner's local
//     positions.  Three launches: entries kept per row (one wave per row), an exclusive prefix sum over the rows (one workgroup,
//     integer, in a fixed order), then the kept entries written behind their row's offset (one wave per row, ballot compaction: the
//     entries keep their order, and an ascending global -> local map keeps them ascending).  Integer arithmetic only: the output does
//     not depend on the launch shape.
//   brTopKListsMerge: one wave per user.  The user's W lists of k entries are offered 64 entries at a time to the WaveList of
//     topk_list.h - the list catalog_merge_kernel merges a launch's item splits with - after each local position has been mapped to
//     its global one, so the order is (score desc, GLOBAL position asc) under the one `beats` every catalogue kernel uses.  An
//     owner's list holds its k best candidates under that very order (its local -> global map is ascending), so the k best of the
//     union are the k best of the whole list: the result equals the single launch entry for entry.
#include <math.h>

#include "common.h"
#include "topk_list.h"

namespace br {
namespace {

constexpr int kSplitWaves = 4;            // rows (waves) per workgroup of the count / scatter kernels
constexpr int kScanThreads = 1024;        // the prefix sum's one workgroup
constexpr int kMergeMaxLists = 4096;      // W: far above any node (the kernel itself has no limit in W)

// local position of global position g under g2l, or -1: not this owner's (or outside the candidate list: never read)
__device__ __forceinline__ int32_t local_of(const int32_t* __restrict__ g2l, int64_t n_global, int32_t g) {
  return (g >= 0 && (int64_t)g < n_global) ? g2l[g] : -1;
}

// cnt[u] = entries of row u that this owner holds
__global__ __launch_bounds__(256) void csr_split_count_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int64_t n_rows,
                                                               const int32_t* __restrict__ g2l, int64_t n_global, int64_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * kSplitWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t u = w0; u < n_rows; u += (int64_t)gridDim.x * kSplitWaves) {
    const int64_t b = off[u], e = off[u + 1];
    int64_t n = 0;
    for (int64_t base = b; base < e; base += 64) {
      const int64_t q = base + lane;
      const bool keep = q < e && local_of(g2l, n_global, idx[q]) >= 0;
      n += __popcll(__ballot(keep));
    }
    if (lane == 0) cnt[u] = n;
  }
}

// out_off[0] = 0, out_off[u + 1] = cnt[0] + .. + cnt[u]: one workgroup walks the rows in tiles of kScanThreads
__global__ __launch_bounds__(kScanThreads) void csr_split_scan_kernel(const int64_t* __restrict__ cnt, int64_t n_rows, int64_t* __restrict__ out_off) {
  __shared__ int64_t wave_sum[kScanThreads / 64];
  __shared__ int64_t carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { carry_s = 0; out_off[0] = 0; }
  __syncthreads();
  for (int64_t base = 0; base < n_rows; base += kScanThreads) {
    const int64_t u = base + tid;
    int64_t v = u < n_rows ? cnt[u] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                      // inclusive scan inside the wave
      const int64_t o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    if (lane == 63) wave_sum[wave] = v;
    const int64_t carry = carry_s;
    __syncthreads();
    int64_t before = carry;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (u < n_rows) out_off[u + 1] = before + v;
    __syncthreads();
    if (tid == kScanThreads - 1) carry_s = before + v;
    __syncthreads();
  }
}

// out_idx[out_off[u] ..] = the local positions of row u's kept entries, in their order
__global__ __launch_bounds__(256) void csr_split_scatter_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int64_t n_rows,
                                                                 const int32_t* __restrict__ g2l, int64_t n_global,
                                                                 const int64_t* __restrict__ out_off, int32_t* __restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * kSplitWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t u = w0; u < n_rows; u += (int64_t)gridDim.x * kSplitWaves) {
    const int64_t b = off[u], e = off[u + 1];
    int64_t o = out_off[u];
    for (int64_t base = b; base < e; base += 64) {
      const int64_t q = base + lane;
      const int32_t l = q < e ? local_of(g2l, n_global, idx[q]) : -1;
      const uint64_t bal = __ballot(l >= 0);
      if (l >= 0) out_idx[o + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0))] = l;
      o += __popcll(bal);
    }
  }
}

// one wave per user: entry e of list w at [w * list_stride + u * user_stride + e] -> out[u * k + e]
__global__ __launch_bounds__(256) void topk_lists_merge_kernel(const float* __restrict__ in_s, const int32_t* __restrict__ in_p, int64_t list_stride,
                                                                int64_t user_stride, int n_lists, int64_t n_users, int k,
                                                                const int32_t* __restrict__ l2g, const int64_t* __restrict__ l2g_off,
                                                                float* __restrict__ out_s, int32_t* __restrict__ out_p) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * kRecWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (u >= n_users) return;
  WaveList list;
  list.init();
  for (int w = 0; w < n_lists; ++w) {
    const int64_t m0 = l2g_off[w], m1 = l2g_off[w + 1];
    const float* s = in_s + w * list_stride + u * user_stride;
    const int32_t* p = in_p + w * list_stride + u * user_stride;
    for (int base = 0; base < k; base += 64) {
      const int e = base + lane;
      float cs = -INFINITY;
      int32_t cp = kNoPos;
      bool ok = false;
      if (e < k) {
        const int32_t l = p[e];
        if (l >= 0 && (int64_t)l < m1 - m0) {              // (-1: the shard ran out of candidates; anything else outside the map: never read)
          cs = s[e];
          cp = l2g[m0 + l];
          ok = true;
        }
      }
      list.offer(cs, cp, ok, k, lane);
    }
  }
  list.store(out_s + u * k, out_p + u * k, k, lane, true);
}

int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brCsrSplitByOwnerWorkspaceBytes(int64_t n_rows) {
  if (n_rows < 0) return -1;
  return round256(n_rows * (int64_t)sizeof(int64_t));
}

extern "C" int brCsrSplitByOwner(const int64_t* off, const int32_t* idx, int64_t n_rows, const int32_t* g2l, int64_t n_global, int64_t* out_off,
                                 int32_t* out_idx, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(off && idx && g2l && out_off && out_idx, "brCsrSplitByOwner: null pointer");
  BR_CHECK_ARG(n_rows >= 0 && n_global >= 0 && n_global < ((int64_t)1 << 31), "brCsrSplitByOwner: n_rows = %lld, n_global = %lld outside [0, 2^31)",
               (long long)n_rows, (long long)n_global);
  BR_CHECK_ARG(out_off != off && out_idx != idx, "brCsrSplitByOwner: the output cannot alias the input");
  const int64_t need = brCsrSplitByOwnerWorkspaceBytes(n_rows);
  if (ws_bytes < need || (need > 0 && !ws)) {
    br::set_error("brCsrSplitByOwner: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)need);
    return BR_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int64_t* cnt = (int64_t*)ws;
  const unsigned grid = (unsigned)(n_rows ? (ceil_div(n_rows, kSplitWaves) < 8192 ? ceil_div(n_rows, kSplitWaves) : 8192) : 1);
  if (n_rows) {
    csr_split_count_kernel<<<grid, 256, 0, st>>>(off, idx, n_rows, g2l, n_global, cnt);
    BR_CHECK_LAUNCH("brCsrSplitByOwner count");
  }
  csr_split_scan_kernel<<<1, kScanThreads, 0, st>>>(cnt, n_rows, out_off);
  BR_CHECK_LAUNCH("brCsrSplitByOwner scan");
  if (n_rows) {
    csr_split_scatter_kernel<<<grid, 256, 0, st>>>(off, idx, n_rows, g2l, n_global, out_off, out_idx);
    BR_CHECK_LAUNCH("brCsrSplitByOwner scatter");
  }
  return BR_OK;
}

extern "C" int brTopKListsMerge(const float* scores, const int32_t* index, int64_t list_stride, int64_t user_stride, int n_lists, int64_t n_users,
                                int k, const int32_t* l2g, const int64_t* l2g_off, float* out_scores, int32_t* out_index, brStream stream) {
  BR_CHECK_ARG(scores && index && l2g && l2g_off && out_scores && out_index, "brTopKListsMerge: null pointer");
  BR_CHECK_ARG(k >= 1 && k <= kRecMaxK, "brTopKListsMerge: k = %d outside [1, %d]", k, kRecMaxK);
  BR_CHECK_ARG(n_lists >= 1 && n_lists <= kMergeMaxLists, "brTopKListsMerge: n_lists = %d outside [1, %d]", n_lists, kMergeMaxLists);
  BR_CHECK_ARG(n_users >= 0 && user_stride >= k && list_stride >= 0, "brTopKListsMerge: n_users = %lld, user_stride = %lld, list_stride = %lld",
               (long long)n_users, (long long)user_stride, (long long)list_stride);
  if (n_users == 0) return BR_OK;
  topk_lists_merge_kernel<<<(unsigned)ceil_div(n_users, kRecWaves), 256, 0, (hipStream_t)stream>>>(scores, index, list_stride, user_stride, n_lists,
                                                                                                   n_users, k, l2g, l2g_off, out_scores, out_index);
  BR_CHECK_LAUNCH("brTopKListsMerge");
  return BR_OK;
}
