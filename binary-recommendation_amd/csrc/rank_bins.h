// What the catalogue ranks of every model (ranks_dot.hip, ranks_neumf.hip) launch around their catalogue pass: the
// init, the excluded-positives kernel and the finalize over the bins.  Two CSRs in two roles, so that an item owner of a row-sharded
// engine runs them over its own entries against the users' full lists:
//   - the entry CSR (entry_off, entry_idx) indexes raw, above and tied: the truth entries ranked here, positions in the space of the
//     exclusion CSR beside it;
//   - the list CSR list_off indexes sorted, pcnt and the bins: user u's n = pcnt[u] sorted positives at sorted[list_off[u] ...], its
//     n + 1 bins and tie bins at [list_off[u] + u ...].  `cap`: the floats `sorted` holds (the bins hold cap + n_users); a list that
//     does not lie inside is left alone, its entries keep (-1, -1).
// The single-device entries pass the truth CSR in both roles.
#pragma once
#include "common.h"
#include "dot_tile.h"

namespace br {
namespace {

__global__ __launch_bounds__(256) void rank_init_kernel(int32_t* __restrict__ bins, int64_t n_bins, int32_t* __restrict__ above,
                                                         int32_t* __restrict__ tied, int64_t n_truth) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bins; i += stride) bins[i] = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_truth; i += stride) above[i] = tied[i] = -1;
}

// #{entries < s} and #{entries <= s} of the ascending v[0 .. n)
__device__ __forceinline__ void sorted_bounds(const float* v, int n, float s, int* lo_out, int* hi_out) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < s) lo = mid + 1; else hi = mid;
  }
  *lo_out = lo;
  hi = n;
  int l2 = lo;
  while (l2 < hi) {
    const int mid = (l2 + hi) >> 1;
    if (v[mid] <= s) l2 = mid + 1; else hi = mid;
  }
  *hi_out = l2;
}

__device__ __forceinline__ bool row_has(const int32_t* __restrict__ v, int64_t lo, int64_t hi, int32_t x) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo < end && v[lo] == x;
}

// one wave per user: a positive that is excluded too is no candidate of the user's positives (itself included): -1 where the list
// terms of rank_finalize_kernel count it
__global__ __launch_bounds__(256) void rank_excluded_kernel(const int64_t* __restrict__ eoff, const int32_t* __restrict__ eidx,
                                                             const int64_t* __restrict__ xoff, const int32_t* __restrict__ xidx,
                                                             const float* __restrict__ raw, const int64_t* __restrict__ loff,
                                                             const float* __restrict__ sorted, const int32_t* __restrict__ pcnt, int64_t cap,
                                                             int64_t n_users, int32_t* bins, int32_t* ties) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int n = pcnt[u];
  const int64_t l0 = loff[u];
  if (n <= 0 || l0 < 0 || l0 + n > cap) return;
  const int64_t o0 = eoff[u], o1 = eoff[u + 1], x0 = xoff[u], x1 = xoff[u + 1];
  if (x1 <= x0) return;
  for (int64_t e = o0 + lane; e < o1; e += 64) {
    const float s = raw[e];
    if (s != s || !row_has(xidx, x0, x1, eidx[e])) continue;
    int lo, hi;
    sorted_bounds(sorted + l0, n, s, &lo, &hi);
    atomicAdd(&bins[l0 + u + lo], -1);
    atomicAdd(&ties[l0 + u + lo], -1);
  }
}

// one wave per user: S[b] = sum of the bins b .. n in place, then the user's entries
__global__ __launch_bounds__(256) void rank_finalize_kernel(const int64_t* __restrict__ eoff, const int32_t* __restrict__ eidx,
                                                             const int64_t* __restrict__ xoff, const int32_t* __restrict__ xidx,
                                                             const float* __restrict__ raw, const int64_t* __restrict__ loff,
                                                             const float* __restrict__ sorted, const int32_t* __restrict__ pcnt, int64_t cap,
                                                             int64_t n_users, int32_t* bins, const int32_t* __restrict__ ties,
                                                             int32_t* __restrict__ above, int32_t* __restrict__ tied) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int n = pcnt[u];
  const int64_t l0 = loff[u];
  if (n <= 0 || l0 < 0 || l0 + n > cap) return;                       // no positive with a rank: the entries keep (-1, -1)
  const int64_t o0 = eoff[u], o1 = eoff[u + 1];
  int32_t* const B = bins + l0 + u;
  int carry = 0;
  for (int t = n; t >= 0; t -= 64) {                                  // lane l: bin t - l, the higher bins first
    const int b = t - lane;
    int x = b >= 0 ? B[b] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    x += carry;
    if (b >= 0) B[b] = x;
    carry = __shfl(x, 63, 64);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");             // this wave's stores before its loads below
  __builtin_amdgcn_wave_barrier();
  const int64_t x0 = xoff ? xoff[u] : 0, x1 = xoff ? xoff[u + 1] : 0;
  for (int64_t e = o0 + lane; e < o1; e += 64) {
    const float s = raw[e];
    if (s != s) continue;
    int lo, hi;
    sorted_bounds(sorted + l0, n, s, &lo, &hi);
    const bool excluded = x1 > x0 && row_has(xidx, x0, x1, eidx[e]);
    above[e] = B[hi] + (n - hi);
    tied[e] = ties[l0 + u + lo] + (hi - lo) - (excluded ? 0 : 1);
  }
}

// workspace of the single-device entries: P' int32 [n_users], the raw and the sorted positive scores float [n_truth + 1] each, the bins
// and the tie bins int32 [n_truth + n_users] each (user u: n + 1 bins from off[u] + u on)
struct RanksWs {
  int64_t pcnt, raw, sorted, bins, ties, total, n_bins;
};
RanksWs ranks_ws(int64_t n_users, int64_t n_truth) {
  RanksWs w;
  w.n_bins = n_truth + n_users;
  w.pcnt = 0;
  w.raw = w.pcnt + align256(4 * n_users);
  w.sorted = w.raw + align256(4 * (n_truth + 1));
  w.bins = w.sorted + align256(4 * (n_truth + 1));
  w.ties = w.bins + align256(4 * w.n_bins);
  w.total = w.ties + align256(4 * w.n_bins);
  return w;
}

// the bins, their padding and the tie bins zeroed in one run of int32, the outputs -1
void launch_rank_init(hipStream_t st, const RanksWs& w, void* ws, int32_t* above, int32_t* tied, int64_t n_truth) {
  const int64_t n_init = (w.ties - w.bins) / 4 + w.n_bins;
  const int64_t most = n_init > n_truth ? n_init : n_truth;
  rank_init_kernel<<<(unsigned)(ceil_div(most, 256) < 4096 ? ceil_div(most, 256) : 4096), 256, 0, st>>>((int32_t*)((char*)ws + w.bins), n_init,
                                                                                                    above, tied, n_truth);
}

}  // namespace
}  // namespace br
