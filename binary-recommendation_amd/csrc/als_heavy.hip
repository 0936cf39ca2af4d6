// ALS by conjugate gradients: the heavy rows.  A row with hundreds of thousands of entries is one wave's work in
// als_cg_kernel (als_wide.hip) and that wave walks the entries once per application of the operator.  Here the operator of such a row
// is formed once, by many workgroups, and the same recurrence then runs on the dense matrix:
//   H_u = sum_e c_e y_e y_e^T,   b_u = sum_e (1 + c_e) y_e,   A_u = G + reg I + H_u,   c_e = alpha * conf_e
//   brAlsNormalRows        first launch: grid = (slices of all listed rows, pairs (I, J <= I) of 128-column blocks), the scheme of
//                          gram_wide_partial_kernel.  A slice is `slice` consecutive entries of one row.  A workgroup gathers 64 entries'
//                          rows of Y of both column blocks into LDS through idx; wave w forms the 32 x 32 tiles (w, 0 .. 3) of
//                          (c . Ya)^T Yb on the fp32-input MFMA (the a operand is scaled by c_e as it leaves LDS), each chunk's sums
//                          from zero, joined to the slice's once.  The workgroups of the diagonal pairs also add the slice's share of
//                          b in double, in the order of the CSR.  Second launch: a row's slice partials are added in slice order in
//                          double, rounded once, H[i][j] and H[j][i] written from the one value.  No atomics on floats.
//   brAlsSolveRowsDenseCg  one workgroup per listed row, thread j owns feature j: x, r, p and every sum in double, q = (G + H) p read
//                          through the symmetric transpose (thread j reads column j: consecutive addresses), k = 0 .. dim - 1 in order.
#include <float.h>

#include "common.h"

namespace br {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kThreads = 256;
constexpr int kMaxDim = 512;
constexpr int kColBlock = 128;          // columns of a block
constexpr int kChunk = 64;              // entries staged per pass
constexpr int kPairFloats = 16 * 1024;  // a pair's partial: 16 tiles of 32 x 32
constexpr int kMaxSteps = 64;
constexpr size_t kPartialLds = 2 * kChunk * kColBlock * sizeof(float) + 3 * kChunk * (sizeof(double) + sizeof(float) + sizeof(int));

// C/D layout of the 32x32 MFMA: register r of lane l is element (row, col) of the tile
__device__ __forceinline__ int tile_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int tile_col(int lane) { return lane & 31; }
// pair p of the lower triangle, row by row: (0,0) (1,0) (1,1) (2,0) ...
__device__ __forceinline__ void block_pair(int p, int& bi, int& bj) {
  bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
  bj = p - bi * (bi + 1) / 2;
}

static int blocks_of(int dim) { return (dim + kColBlock - 1) / kColBlock; }
static int pairs_of(int dim) { const int nb = blocks_of(dim); return nb * (nb + 1) / 2; }
static bool rows_vec4(const float* p, int64_t ld, int dim) { return dim % 4 == 0 && ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }

struct NormalArgs {
  const float* Y; int64_t ld; int32_t n_y; int dim;
  const int64_t* off; const int32_t* idx; const float* conf; float alpha; int64_t n_rows;
  const int32_t* rows; const int64_t* slice_off; int n_heavy; int slice; int vec;
  float* ws; double* bws; int* err;
};

// the listed row that slice s belongs to: the last h with slice_off[h] <= s
__device__ __forceinline__ int row_of_slice(const int64_t* slice_off, int n_heavy, int64_t s) {
  int lo = 0, hi = n_heavy;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (slice_off[mid] <= s) lo = mid; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------------------------ H and b: partials
__global__ __launch_bounds__(kThreads, 2) void normal_partial_kernel(NormalArgs a) {
  constexpr int CB = kColBlock, CB4 = CB / 4, PRE = kChunk * CB / kThreads;     // floats of one block's chunk per thread
  extern __shared__ double smem[];             // kPartialLds bytes (above the 64 KB a launch gets unasked: brAlsNormalRows raises the limit)
  float* As = reinterpret_cast<float*>(smem);
  float* Bs = As + kChunk * CB;
  // ids (-1: absent), c_e and 1 + c_e of three chunks: the one being multiplied, the one being fetched, the one whose ids arrive
  double (*sb)[kChunk] = reinterpret_cast<double (*)[kChunk]>(Bs + kChunk * CB);
  float (*sc)[kChunk] = reinterpret_cast<float (*)[kChunk]>(sb + 3);
  int (*sid)[kChunk] = reinterpret_cast<int (*)[kChunk]>(sc + 3);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int bi, bj;
  block_pair(blockIdx.y, bi, bj);
  const bool diag = bi == bj;
  const int ca = bi * CB, cb = bj * CB;
  const int wa = a.dim - ca < CB ? a.dim - ca : CB, wb = a.dim - cb < CB ? a.dim - cb : CB;
  const float* Bsrc = diag ? As : Bs;

  const int64_t s = blockIdx.x;
  const int h = row_of_slice(a.slice_off, a.n_heavy, s);
  const int64_t u = a.rows[h];
  const bool row_ok = u >= 0 && u < a.n_rows;                       // (compared, never an address)
  if (!row_ok && a.err && tid == 0) atomicOr(a.err, BR_ERRFLAG_RANGE);
  const int64_t e_lo = row_ok ? a.off[u] : 0, e_hi = row_ok ? a.off[u + 1] : 0;
  const int64_t r0 = e_lo + (s - a.slice_off[h]) * a.slice;
  int64_t r1 = r0 + a.slice < e_hi ? r0 + a.slice : e_hi;
  if (r1 < r0) r1 = r0;

  // the tiles this wave forms: rows of tiles past dim are nobody's, and a diagonal pair needs its lower triangle only
  const bool wave_on = 32 * w < wa;
  unsigned tmask = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (wave_on && 32 * t < wb && !(diag && t > w)) tmask |= 1u << t;

  f32x16 tot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[t][r] = 0.f;
  double bacc = 0.0;

  auto load_ids = [&](int buf, int64_t c0) {
    if (tid < kChunk) {
      int id = -1;
      float c = 0.f;
      double b1 = 0.0;
      const int64_t e = c0 + tid;
      if (e < r1) {
        const int32_t v = a.idx[e];
        if (v >= 0 && v < a.n_y) {
          id = v;
          c = a.conf ? a.alpha * a.conf[e] : a.alpha;
          b1 = 1.0 + (a.conf ? (double)a.alpha * (double)a.conf[e] : (double)a.alpha);
        } else if (a.err) {
          atomicOr(a.err, BR_ERRFLAG_RANGE);     // never an address: the entry counts as absent
        }
      }
      sid[buf][tid] = id; sc[buf][tid] = c; sb[buf][tid] = b1;
    }
  };
  // Loads go to clamped addresses and the values are selected afterwards (als.hip): absent entries and columns past dim are zero, and
  // both load paths put the same values into the same places
  float pa[PRE], pb[PRE];
  auto fetch = [&](float* pre, int c0, int wd, int buf) {
    if (a.vec) {
#pragma unroll
      for (int q = 0; q < PRE / 4; ++q) {
        const int e = tid + q * kThreads, r = e / CB4, c4 = e - r * CB4;
        const int id = sid[buf][r];
        const bool in = id >= 0 && 4 * c4 < wd;
        const float4 v = *reinterpret_cast<const float4*>(a.Y + (int64_t)(in ? id : 0) * a.ld + c0 + 4 * (in ? c4 : 0));
        pre[4 * q] = in ? v.x : 0.f; pre[4 * q + 1] = in ? v.y : 0.f; pre[4 * q + 2] = in ? v.z : 0.f; pre[4 * q + 3] = in ? v.w : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < PRE; ++q) {
        const int e = tid + q * kThreads, r = e / CB, c = e - r * CB;
        const int id = sid[buf][r];
        const bool in = id >= 0 && c < wd;
        const float v = a.Y[(int64_t)(in ? id : 0) * a.ld + c0 + (in ? c : 0)];
        pre[q] = in ? v : 0.f;
      }
    }
  };
  auto stage = [&](float* dst, const float* pre) {
    if (a.vec) {
#pragma unroll
      for (int q = 0; q < PRE / 4; ++q) {
        const int e = tid + q * kThreads, r = e / CB4, c4 = e - r * CB4;
        *reinterpret_cast<float4*>(dst + r * CB + 4 * c4) = make_float4(pre[4 * q], pre[4 * q + 1], pre[4 * q + 2], pre[4 * q + 3]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < PRE; ++q) dst[tid + q * kThreads] = pre[q];
    }
  };

  if (r0 < r1) {
    load_ids(0, r0);
    __syncthreads();
    fetch(pa, ca, wa, 0);
    if (!diag) fetch(pb, cb, wb, 0);
    load_ids(1, r0 + kChunk);                 // (past the slice: all absent)
  }
  int cur = 0;
  for (int64_t c0 = r0; c0 < r1; c0 += kChunk) {
    const int n = (int)(r1 - c0 < kChunk ? r1 - c0 : kChunk);
    const int nxt = cur == 2 ? 0 : cur + 1, aft = nxt == 2 ? 0 : nxt + 1;
    __syncthreads();                          // the last chunk's products are done; the next chunk's ids are in place
    stage(As, pa);
    if (!diag) stage(Bs, pb);
    __syncthreads();
    if (c0 + kChunk < r1) {
      fetch(pa, ca, wa, nxt);
      if (!diag) fetch(pb, cb, wb, nxt);
      load_ids(aft, c0 + 2 * kChunk);         // (aft was last read before this iteration's first barrier)
    }
    if (tmask) {
      // the chunk's own sums start from zero and join the slice's once
      f32x16 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      const int ksteps = (n + 1) >> 1;         // entries past n are zero
      for (int kk = 0; kk < ksteps; ++kk) {
        const int row = 2 * kk + (lane >> 5);
        const float va = As[row * CB + 32 * w + (lane & 31)] * sc[cur][row];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (!((tmask >> t) & 1)) continue;   // (the same for every lane of the wave)
          const float vb = Bsrc[row * CB + 32 * t + (lane & 31)];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(va, vb, acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) tot[t] += acc[t];
    }
    // b of the block's own columns: in double, entry by entry in the order of the CSR
    if (diag && tid < wa) {
      for (int r = 0; r < n; ++r) bacc = fma(sb[cur][r], (double)As[r * CB + tid], bacc);
    }
    cur = nxt;
  }
  const int pairs = gridDim.y;
  float* out = a.ws + (s * pairs + blockIdx.y) * kPairFloats + (int64_t)w * 4 * 1024;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!((tmask >> t) & 1)) continue;         // (the reduce never reads a tile that nobody forms)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(t * 16 + r) * 64 + lane] = tot[t][r];
  }
  if (diag && tid < wa) a.bws[s * a.dim + ca + tid] = bacc;
}

// grid = (listed rows, 64 groups of 256 elements of a pair's partial + 1 for b, pairs): every element by one thread, the row's slices in
// their order, in double, rounded once.  A diagonal pair writes its lower triangle and mirrors it; the others write H[I][J] and H[J][I]
// from the one value
__global__ __launch_bounds__(kThreads) void normal_reduce_kernel(const float* __restrict__ ws, const double* __restrict__ bws,
                                                                  const int64_t* __restrict__ slice_off, int dim, float* __restrict__ H,
                                                                  double* __restrict__ b) {
  const int h = blockIdx.x, pairs = gridDim.z, pair = blockIdx.z;
  const int64_t s0 = slice_off[h], s1 = slice_off[h + 1];
  int bi, bj;
  block_pair(pair, bi, bj);
  if (blockIdx.y == kPairFloats / kThreads) {
    const int f = bi * kColBlock + threadIdx.x;
    if (bi != bj || threadIdx.x >= kColBlock || f >= dim) return;
    double sum = 0.0;
    for (int64_t s = s0; s < s1; ++s) sum += bws[s * dim + f];
    b[(int64_t)h * dim + f] = sum;
    return;
  }
  const int e = blockIdx.y * kThreads + threadIdx.x;      // (tile, register, lane) of the pair's partial
  const int tile = e >> 10, ti = tile >> 2, tj = tile & 3, el = e & 63;
  const int gi = bi * kColBlock + ti * 32 + tile_row((e >> 6) & 15, el), gj = bj * kColBlock + tj * 32 + tile_col(el);
  if (gi >= dim || gj >= dim || (bi == bj && gi < gj)) return;
  double sum = 0.0;
  for (int64_t s = s0; s < s1; ++s) sum += (double)ws[(s * pairs + pair) * kPairFloats + e];
  const float v = (float)sum;
  float* Hh = H + (int64_t)h * dim * dim;
  Hh[(int64_t)gi * dim + gj] = v;
  if (gi != gj) Hh[(int64_t)gj * dim + gi] = v;
}

// ------------------------------------------------------------------------------------------------------------------ dense CG
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);     // every lane ends with the same bits
  return v;
}

// blockDim.x = dim rounded up to 64: thread j owns feature j of the row's x, r and p
__global__ __launch_bounds__(kMaxDim) void dense_cg_kernel(const float* __restrict__ G, const float* __restrict__ H, const double* __restrict__ b,
                                                           int dim, double reg, const float* __restrict__ X0, int steps,
                                                           float* __restrict__ Xout, int64_t ld_out) {
  __shared__ double ps[kMaxDim];
  __shared__ double red[kMaxDim / 64];
  const int j = threadIdx.x, nw = blockDim.x >> 6;
  const int64_t h = blockIdx.x;
  const bool on = j < dim;
  const float* Gj = G + (on ? j : 0);
  const float* Hj = H + h * dim * dim + (on ? j : 0);

  // the waves' sums in wave order: every thread ends with the same bits
  auto block_sum = [&](double v) {
    v = wave_sum(v);
    __syncthreads();
    if ((j & 63) == 0) red[j >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
  };
  // (G + H) v for feature j, k = 0 .. dim - 1 in order; column j of the symmetric matrix is read as row k, element j
  auto apply = [&](double vj) {
    __syncthreads();
    ps[j] = on ? vj : 0.0;
    __syncthreads();
    double q = 0.0;
    if (on) {
#pragma unroll 8
      for (int k = 0; k < dim; ++k) q = fma((double)Gj[(int64_t)k * dim] + (double)Hj[(int64_t)k * dim], ps[k], q);
    }
    return q;
  };

  // (apply and block_sum hold barriers: every thread of the workgroup calls them, the threads past dim with zeros)
  double x = on ? (double)X0[h * dim + j] : 0.0;
  const double ax = apply(x);
  double r = on ? (b[h * dim + j] - ax) - reg * x : 0.0;
  double p = r;
  double rs = block_sum(r * r);
  for (int it = 0; it < steps; ++it) {
    if (!(rs >= 1e-20)) break;                                  // (every thread holds the same rs and d)
    const double ap = apply(p);
    const double q = on ? fma(reg, p, ap) : 0.0;
    const double d = block_sum(p * q);
    if (!(d > 0.0 && d <= DBL_MAX)) break;
    const double al = rs / d;
    x = fma(al, p, x);
    r = fma(-al, q, r);
    const double rn = block_sum(r * r);
    p = on ? fma(rn / rs, p, r) : 0.0;
    rs = rn;
  }
  if (on) Xout[h * ld_out + j] = (float)x;
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brAlsNormalRowsWorkspaceBytes(int64_t n_slices, int dim) {
  if (n_slices < 0 || n_slices >= ((int64_t)1 << 31) || dim < 1 || dim > kMaxDim) return -1;
  return n_slices * ((int64_t)pairs_of(dim) * kPairFloats * (int64_t)sizeof(float) + (int64_t)dim * (int64_t)sizeof(double));
}

extern "C" int brAlsNormalRows(const float* Y, int64_t ld_y, int64_t n_y, int dim, const int64_t* off, const int32_t* idx, const float* conf,
                               float alpha, int64_t n_rows, const int32_t* rows, const int64_t* slice_off, int64_t n_heavy,
                               int64_t n_slices, int slice, float* H, double* b, void* ws, int64_t ws_bytes, int* err_flag,
                               brStream stream) {
  BR_CHECK_ARG(dim >= 1 && dim <= kMaxDim, "brAlsNormalRows: dim = %d outside [1, %d]", dim, kMaxDim);
  BR_CHECK_ARG(ld_y >= dim, "brAlsNormalRows: ld_y = %lld below dim = %d", (long long)ld_y, dim);
  BR_CHECK_ARG(n_y >= 0 && n_y < ((int64_t)1 << 31), "brAlsNormalRows: n_y = %lld outside [0, 2^31)", (long long)n_y);
  BR_CHECK_ARG(alpha >= 0.f && alpha <= FLT_MAX, "brAlsNormalRows: alpha = %g must be >= 0 and finite", (double)alpha);
  BR_CHECK_ARG(slice >= kChunk && slice % kChunk == 0, "brAlsNormalRows: slice = %d must be a multiple of %d, at least %d", slice, kChunk, kChunk);
  BR_CHECK_ARG(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "brAlsNormalRows: n_rows = %lld outside [0, 2^31)", (long long)n_rows);
  BR_CHECK_ARG(n_heavy >= 0 && n_heavy < ((int64_t)1 << 31), "brAlsNormalRows: n_heavy = %lld outside [0, 2^31)", (long long)n_heavy);
  BR_CHECK_ARG(n_slices >= 0 && n_slices < ((int64_t)1 << 31), "brAlsNormalRows: n_slices = %lld outside [0, 2^31)", (long long)n_slices);
  if (n_heavy == 0) return BR_OK;
  BR_CHECK_ARG(n_y >= 1, "brAlsNormalRows: n_y = 0 with rows listed");
  BR_CHECK_ARG(Y && off && idx && rows && slice_off && H && b, "brAlsNormalRows: null pointer");
  const int64_t need = brAlsNormalRowsWorkspaceBytes(n_slices, dim);
  if (ws_bytes < need || (need > 0 && !ws)) {
    br::set_error("brAlsNormalRows: workspace %lld bytes < %lld", (long long)(ws ? ws_bytes : 0), (long long)need);
    return BR_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int pairs = pairs_of(dim);
  float* wsf = (float*)ws;
  double* bws = (double*)(wsf + n_slices * pairs * kPairFloats);
  if (n_slices > 0) {
    NormalArgs a{Y, ld_y, (int32_t)n_y, dim, off, idx, conf, alpha, n_rows, rows, slice_off, (int)n_heavy, slice,
                 rows_vec4(Y, ld_y, dim) ? 1 : 0, wsf, bws, err_flag};
    static bool attr = false;
    if (!attr) {
      const hipError_t e = hipFuncSetAttribute((const void*)normal_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPartialLds);
      if (e != hipSuccess) { br::set_error("brAlsNormalRows: cannot raise the dynamic LDS limit to %zu B: %s", kPartialLds, hipGetErrorString(e)); return BR_ERR_HIP; }
      attr = true;
    }
    normal_partial_kernel<<<dim3((unsigned)n_slices, (unsigned)pairs), kThreads, kPartialLds, st>>>(a);
    BR_CHECK_LAUNCH("brAlsNormalRows");
  }
  normal_reduce_kernel<<<dim3((unsigned)n_heavy, kPairFloats / kThreads + 1, (unsigned)pairs), kThreads, 0, st>>>(wsf, bws, slice_off, dim, H, b);
  BR_CHECK_LAUNCH("brAlsNormalRows reduce");
  return BR_OK;
}

extern "C" int brAlsSolveRowsDenseCg(const float* G, const float* H, const double* b, int dim, float reg, const float* X0, int64_t n_heavy,
                                     int steps, float* Xout, int64_t ld_out, brStream stream) {
  BR_CHECK_ARG(dim >= 1 && dim <= kMaxDim, "brAlsSolveRowsDenseCg: dim = %d outside [1, %d]", dim, kMaxDim);
  BR_CHECK_ARG(ld_out >= dim, "brAlsSolveRowsDenseCg: ld_out = %lld below dim = %d", (long long)ld_out, dim);
  BR_CHECK_ARG(reg > 0.f && reg <= FLT_MAX, "brAlsSolveRowsDenseCg: reg = %g must be positive and finite", (double)reg);
  BR_CHECK_ARG(steps >= 1 && steps <= kMaxSteps, "brAlsSolveRowsDenseCg: steps = %d outside [1, %d]", steps, kMaxSteps);
  BR_CHECK_ARG(n_heavy >= 0 && n_heavy < ((int64_t)1 << 31), "brAlsSolveRowsDenseCg: n_heavy = %lld outside [0, 2^31)", (long long)n_heavy);
  if (n_heavy == 0) return BR_OK;
  BR_CHECK_ARG(G && H && b && X0 && Xout, "brAlsSolveRowsDenseCg: null pointer");
  dense_cg_kernel<<<(unsigned)n_heavy, (unsigned)((dim + 63) / 64 * 64), 0, (hipStream_t)stream>>>(G, H, b, dim, (double)reg, X0, steps, Xout, ld_out);
  BR_CHECK_LAUNCH("brAlsSolveRowsDenseCg");
  return BR_OK;
}
