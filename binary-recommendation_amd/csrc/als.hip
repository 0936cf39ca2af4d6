// Implicit-feedback ALS (Hu, Koren, Volinsky 2008): the Gram matrix of a table and the fused per-row normal equations
//   A_u = G + reg I + sum_e c_e y_e y_e^T,  b_u = sum_e (1 + c_e) y_e,  x_u = A_u^-1 b_u        
// Both kernels run the products on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, exact f32), on 32 x 32 tiles
// of the dim x dim matrix padded to DP = 32 NT columns.  Only the tiles of the lower triangle (tj <= ti) are formed.
//   brGram          workgroup = a contiguous slice of rows, staged 64 at a time through LDS; wave w multiplies rows 16w .. 16w + 15 of
//                   the chunk into its own accumulators of every tile; the four waves' accumulators are added in the order 0 + 1 + 2 + 3
//                   and written to the workspace; a second launch adds the workgroups' partials in double, in index order, rounds once
//                   and writes both triangles from the one value.  No atomics: the bits are a function of (Y, rows, dim) alone.
//   brAlsSolveRows  workgroup = one row.  Accumulators start from G + reg I, the row's entries are gathered 32 at a time into LDS and
//                   added as (c . Y_t)^T Y_t; A goes to LDS (leading dimension DP + 1) with b as row `dim` below it, so the right-looking
//                   Cholesky performs the forward substitution on that row as it goes; wave 0 substitutes backwards.
#include <float.h>

#include "common.h"

namespace br {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kAlsThreads = 256;
constexpr int kAlsMaxDim = 128;
constexpr int kGramChunk = 64;          // rows staged per pass: 16 per wave
constexpr int kGramMinRows = 256;       // rows of a workgroup's slice, at least
constexpr int kGramCus = 256;           // workgroups: at most what the 256 CUs hold at once at the kernel's register count (gram_max_wg)
constexpr int kAlsTile = 32;            // gathered rows per tile (T)

// C/D layout of the 32x32 MFMA: register r of lane l is element (row, col) of the tile
__device__ __forceinline__ int mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int mfma_col(int lane) { return lane & 31; }
// tile t of the lower triangle, row by row: (0,0) (1,0) (1,1) (2,0) ...
__device__ __forceinline__ void tri_tile(int t, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

static int nt_of(int dim) { return (dim + 31) / 32; }
static int ntl_of(int dim) { const int nt = nt_of(dim); return nt * (nt + 1) / 2; }
static bool rows_vec4(const float* p, int64_t ld, int dim) { return dim % 4 == 0 && ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// rows >= 1 -> the workgroups of the partial launch and the rows each takes (a multiple of the chunk)
static int gram_max_wg(int nt) { return kGramCus * (nt <= 2 ? 4 : 1); }     // 124 registers and 24 KB at 64 columns, past 256 registers from 65 on
static void gram_plan(int64_t rows, int nt, int64_t* n_wg, int64_t* rows_per_wg) {
  int64_t per = ceil_div(rows, (int64_t)gram_max_wg(nt));
  if (per < kGramMinRows) per = kGramMinRows;
  per = ceil_div(per, (int64_t)kGramChunk) * kGramChunk;
  *rows_per_wg = per;
  *n_wg = ceil_div(rows, per);
}

constexpr int gram_lds_floats(int nt) {
  const int chunk = kGramChunk * nt * 32, exch = nt * (nt + 1) / 2 * 1024;
  return chunk > exch ? chunk : exch;
}

template <int NT>
__global__ __launch_bounds__(kAlsThreads) void gram_partial_kernel(const float* __restrict__ Y, int64_t ld, int64_t rows, int dim, int64_t rows_per_wg,
                                                                    int vec, float* __restrict__ ws) {
  constexpr int DP = NT * 32, NTL = NT * (NT + 1) / 2, DP4 = DP / 4;
  extern __shared__ float smem[];            // [kGramChunk][DP]; afterwards the exchange buffer of the waves' accumulators (gram_lds_floats)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
  f32x16 acc[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // (Loads are issued at clamped addresses and their values selected afterwards, here and in the solve: a load under a branch is
  // waited for before the next is issued - sixteen L2 round trips in a row for one accumulator tile of G.)
  // A chunk travels global -> registers -> LDS; the next chunk's loads are issued before this one is multiplied.  Both paths put the
  // same values into the same places: rows past the slice and columns past dim are zero
  constexpr int PRE = kGramChunk * DP / kAlsThreads;      // floats of a chunk per thread
  float pre[PRE];
  auto fetch = [&](int64_t c0) {
    const int n = (int)(r1 - c0 < kGramChunk ? r1 - c0 : kGramChunk);
    if (vec) {
      const int dim4 = dim >> 2;
#pragma unroll
      for (int q = 0; q < PRE / 4; ++q) {
        const int e = tid + q * kAlsThreads, r = e / DP4, c4 = e - r * DP4;
        const bool in = r < n && c4 < dim4;
        const float4 v = *reinterpret_cast<const float4*>(Y + (c0 + (in ? r : 0)) * ld + 4 * (in ? c4 : 0));
        pre[4 * q] = in ? v.x : 0.f; pre[4 * q + 1] = in ? v.y : 0.f; pre[4 * q + 2] = in ? v.z : 0.f; pre[4 * q + 3] = in ? v.w : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < PRE; ++q) {
        const int e = tid + q * kAlsThreads, r = e / DP, c = e - r * DP;
        const bool in = r < n && c < dim;
        const float v = Y[(c0 + (in ? r : 0)) * ld + (in ? c : 0)];
        pre[q] = in ? v : 0.f;
      }
    }
  };
  if (r0 < r1) fetch(r0);
  for (int64_t c0 = r0; c0 < r1; c0 += kGramChunk) {
    const int n = (int)(r1 - c0 < kGramChunk ? r1 - c0 : kGramChunk);
    __syncthreads();
    if (vec) {
#pragma unroll
      for (int q = 0; q < PRE / 4; ++q) {
        const int e = tid + q * kAlsThreads, r = e / DP4, c4 = e - r * DP4;
        *reinterpret_cast<float4*>(smem + r * DP + 4 * c4) = make_float4(pre[4 * q], pre[4 * q + 1], pre[4 * q + 2], pre[4 * q + 3]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < PRE; ++q) smem[tid + q * kAlsThreads] = pre[q];
    }
    __syncthreads();
    if (c0 + kGramChunk < r1) fetch(c0 + kGramChunk);
    const int kw = 16 * w;                   // this wave's rows of the chunk (all zero past n: skipped)
    if (kw < n) {
      const int steps = n - kw >= 16 ? 8 : (n - kw + 1) >> 1;
      for (int kk = 0; kk < steps; ++kk) {
        const float* row = smem + (kw + 2 * kk + (lane >> 5)) * DP + (lane & 31);
        float v[NT];
#pragma unroll
        for (int b = 0; b < NT; ++b) v[b] = row[32 * b];
        int t = 0;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
          for (int tj = 0; tj <= ti; ++tj, ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[ti], v[tj], acc[t], 0, 0, 0);
      }
    }
  }
  // wave 0 += wave 1, then 2, then 3 (a fixed order), through the chunk image
  for (int w2 = 1; w2 < 4; ++w2) {
    __syncthreads();
    if (w == w2) {
#pragma unroll
      for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) smem[(t * 16 + r) * 64 + lane] = acc[t][r];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] += smem[(t * 16 + r) * 64 + lane];
    }
  }
  if (w == 0) {
    float* out = ws + (int64_t)blockIdx.x * NTL * 1024;
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(t * 16 + r) * 64 + lane] = acc[t][r];
  }
}

// 64 elements per workgroup, each summed by 4 threads over a quarter of the partials in index order; the quarters are added (0 + 1) + (2 + 3)
__global__ __launch_bounds__(kAlsThreads) void gram_reduce_kernel(const float* __restrict__ ws, int64_t n_wg, int ntl, int dim, float* __restrict__ G) {
  __shared__ double part[kAlsThreads];
  const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;        // (tile, register, lane) of the partials' layout
  const int64_t p0 = n_wg * q / 4, p1 = n_wg * (q + 1) / 4;
  double s = 0.0;
  for (int64_t p = p0; p < p1; ++p) s += (double)ws[p * ntl * 1024 + e];
  part[threadIdx.x] = s;
  __syncthreads();
  if (q != 0) return;
  const float g = (float)((part[el] + part[64 + el]) + (part[128 + el] + part[192 + el]));
  int ti, tj;
  tri_tile(e >> 10, ti, tj);
  const int gi = ti * 32 + mfma_row((e >> 6) & 15, el), gj = tj * 32 + mfma_col(el);
  if (gi < dim && gj < dim) {
    G[(int64_t)gi * dim + gj] = g;
    if (ti != tj) G[(int64_t)gj * dim + gi] = g;
  }
}

struct SolveArgs {
  const float* Y; int64_t ld_y; int32_t n_y; int dim; const float* G;
  const int64_t* off; const int32_t* idx; const float* conf; float alpha, reg;
  float* X; int64_t ld_x; int* err; int vec;
};

// LDS of the solve: 1 / L[k][k], then ONE region that holds the tile (rows, weights, ids) while the entries are summed and A | b once
// they are (dim 128: 0.5 + 66.6 KB, two workgroups per CU; with the tile beside A it was 84 KB and one)
static size_t solve_lds_bytes(int nt) {
  const size_t dp = nt * 32, tile = kAlsTile * dp + 3 * kAlsTile, mat = (dp + 1) * (dp + 1);
  return sizeof(float) * (dp + (tile > mat ? tile : mat));
}

template <int NT>
__global__ __launch_bounds__(kAlsThreads) void als_solve_kernel(SolveArgs a) {
  constexpr int DP = NT * 32, NTL = NT * (NT + 1) / 2, SLOTS = (NTL + 3) / 4, DP4 = DP / 4, LD = DP + 1;
  extern __shared__ float smem[];
  float* dinv = smem;                         // [DP] 1 / L[k][k]
  float* Ts = dinv + DP;                      // [kAlsTile][DP] the gathered rows
  float* cw = Ts + kAlsTile * DP;             // [kAlsTile] c_e (0: padding or an id out of range)
  float* bw = cw + kAlsTile;                  // [kAlsTile] 1 + c_e (0 likewise)
  int* rid = reinterpret_cast<int*>(bw + kAlsTile);   // [kAlsTile] the row of Y, -1: none
  float* As = Ts;                             // [dim + 1][LD]: A, then b as row dim - over the tile, once the last one is consumed
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = a.dim;
  const int64_t u = blockIdx.x;
  const int64_t e0 = a.off[u], e1 = a.off[u + 1];
  float* xrow = a.X + u * a.ld_x;
  if (e1 <= e0) {                             // a row without entries: exact zeros, no factorisation
    if (tid < n) xrow[tid] = 0.f;
    return;
  }
  // the wave's tiles (t = w, w + 4, ...) start from G + reg I
  f32x16 acc[SLOTS];
  int ti[SLOTS], tj[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int t = w + 4 * s;
    ti[s] = tj[s] = 0;
    if (t < NTL) tri_tile(t, ti[s], tj[s]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gi = ti[s] * 32 + mfma_row(r, lane), gj = tj[s] * 32 + mfma_col(lane);
      const bool in = t < NTL && gi < n && gj < n;
      const float v = a.G[(in ? gi : 0) * n + (in ? gj : 0)];
      acc[s][r] = in ? (gi == gj ? v + a.reg : v) : 0.f;
    }
  }
  const int bd = tid - 128;                   // b on the VALU of waves 2 and 3 (they own the fewest tiles)
  float bacc = 0.f;

  for (int64_t t0 = e0; t0 < e1; t0 += kAlsTile) {
    const int cnt = (int)(e1 - t0 < kAlsTile ? e1 - t0 : kAlsTile);
    const int kmax = (cnt + 1) & ~1;          // the MFMA takes two entries at a time: an odd tail gets one zero row with c = 0
    __syncthreads();
    if (tid < kAlsTile) {
      int r = -1;
      float c = 0.f, b1 = 0.f;
      if (tid < cnt) {
        const int32_t id = a.idx[t0 + tid];
        if (id >= 0 && id < a.n_y) {
          r = id;
          c = a.conf ? a.alpha * a.conf[t0 + tid] : a.alpha;
          b1 = 1.f + c;
        } else if (a.err) {
          atomicOr(a.err, BR_ERRFLAG_RANGE);  // never an address: the entry counts as absent
        }
      }
      rid[tid] = r; cw[tid] = c; bw[tid] = b1;
    }
    __syncthreads();
    if (a.vec) {
      const int dim4 = n >> 2;
      for (int e = tid; e < kmax * DP4; e += kAlsThreads) {
        const int r = e / DP4, c4 = e - r * DP4;
        const int id = rid[r];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (id >= 0 && c4 < dim4) v = *reinterpret_cast<const float4*>(a.Y + (int64_t)id * a.ld_y + 4 * c4);
        *reinterpret_cast<float4*>(Ts + r * DP + 4 * c4) = v;
      }
    } else {
      for (int e = tid; e < kmax * DP; e += kAlsThreads) {
        const int r = e / DP, c = e - r * DP;
        const int id = rid[r];
        Ts[e] = (id >= 0 && c < n) ? a.Y[(int64_t)id * a.ld_y + c] : 0.f;
      }
    }
    __syncthreads();
    // the tile's own sums start from zero and are added to the row's once: the rounding error of a row with P entries grows with
    // 32 + P / 32 terms, not with P (a row of 300 entries summed in one chain was 4 x as far from float64 as a blocked float32 sum)
    if (bd >= 0 && bd < n) {
      float bt = 0.f;
      for (int r = 0; r < cnt; ++r) bt = fmaf(bw[r], Ts[r * DP + bd], bt);
      bacc += bt;
    }
    f32x16 tacc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) tacc[s][r] = 0.f;
    for (int kk = 0; kk < kmax / 2; ++kk) {
      const int k = 2 * kk + (lane >> 5);
      const float ck = cw[k];
      const float* row = Ts + k * DP + (lane & 31);
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (w + 4 * s < NTL) tacc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ck * row[32 * ti[s]], row[32 * tj[s]], tacc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) acc[s] += tacc[s];
  }
  // A (lower triangle) and b into LDS, over the tile: every wave is done reading it first
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (w + 4 * s >= NTL) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gi = ti[s] * 32 + mfma_row(r, lane), gj = tj[s] * 32 + mfma_col(lane);
      if (gi < n && gj < n) As[gi * LD + gj] = acc[s][r];
    }
  }
  if (bd >= 0 && bd < n) As[n * LD + bd] = bacc;
  __syncthreads();
  // Right-looking Cholesky, the trailing matrix in registers: thread (tx, ty) of a 16 x 16 grid owns the elements (ty + 16 a, tx + 16 b),
  // b <= a, and thread i also b_i.  Step k: the owners of column k store it (unscaled) to its place in LDS and thread k stores b_k beside
  // it as row n; one barrier; every thread reads A[k][k] and the 2 DP / 16 elements of the column that its own rows and columns need and
  // updates its registers.  1 / L[k][k] goes to dinv: L[i][k] = As[i][k] * dinv[k] wherever it is used later, and row n leaves as L^-1 b
  // scaled by the diagonal - the forward substitution, done on the way.  (The first form kept the matrix in LDS and issued ~ 2 000 wave
  // instructions per column at any size of the trailing matrix; at dim 64 that, not the MFMA or the loads, was the half-step.)
  constexpr int R = DP / 16;
  const int tx = tid & 15, ty = tid >> 4;
  float tr[R][R];
#pragma unroll
  for (int p = 0; p < R; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) tr[p][q] = As[(ty + 16 * p) * LD + tx + 16 * q];
  float bi = As[n * LD + (tid < n ? tid : n)];
  __syncthreads();                              // every element is in its register before a column is stored over its first value
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const int kb = k >> 4;
    if (tx == (k & 15)) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (q != kb) continue;
#pragma unroll
        for (int p = q; p < R; ++p) {
          const int i = ty + 16 * p;
          if (i >= k && i < n) As[i * LD + k] = tr[p][q];
        }
      }
    }
    if (tid == k) As[n * LD + k] = bi;
    __syncthreads();
    const float akk = As[k * LD + k];
    if (!(akk > 0.f && akk <= FLT_MAX)) bad = true;     // (the same value in every thread)
    const float rd = 1.0f / sqrtf(akk);
    float li[R], lj[R];                          // rows past n - 1 are clamped to row n: legal loads whose products nobody reads
#pragma unroll
    for (int p = 0; p < R; ++p) {
      const int i = ty + 16 * p, j = tx + 16 * p;
      li[p] = As[(i < n ? i : n) * LD + k] * rd;
      lj[p] = As[(j < n ? j : n) * LD + k] * rd;
    }
    const float zk = As[n * LD + k] * rd, lb = As[(tid < n ? tid : n) * LD + k] * rd;
#pragma unroll
    for (int p = 0; p < R; ++p) {
      if (16 * (p + 1) <= k) continue;           // the block row lies above the trailing matrix (the same for every thread)
#pragma unroll
      for (int q = 0; q <= p; ++q) tr[p][q] -= li[p] * lj[q];
    }
    if (tid > k && tid < n) bi -= lb * zk;
    if (tid == 0) dinv[k] = rd;
  }
  __syncthreads();
  if (w != 0) return;
  // L^T x = z backwards in wave 0: lane j holds elements j and j + 64
  const int j0 = lane, j1 = lane + 64;
  const float d0 = j0 < n ? dinv[j0] : 0.f, d1 = j1 < n ? dinv[j1] : 0.f;
  float z0 = j0 < n ? As[n * LD + j0] * d0 : 0.f, z1 = j1 < n ? As[n * LD + j1] * d1 : 0.f;
  float l0 = As[(n - 1) * LD + (j0 < n ? j0 : n)] * d0, l1 = As[(n - 1) * LD + (j1 < n ? j1 : n)] * d1;   // L[k][j], k = n - 1 (used for j < k only)
  for (int k = n - 1; k >= 0; --k) {
    const float c0 = l0, c1 = l1;
    const int kn = k > 0 ? k - 1 : 0;          // the next row's elements are on their way while this one is applied (used for j < k - 1 only)
    l0 = As[kn * LD + (j0 < n ? j0 : n)] * d0;
    l1 = As[kn * LD + (j1 < n ? j1 : n)] * d1;
    const float xk = __shfl(k < 64 ? z0 : z1, k & 63, 64) * __shfl(k < 64 ? d0 : d1, k & 63, 64);
    if (j0 < k) z0 = fmaf(-c0, xk, z0);
    if (j1 < k) z1 = fmaf(-c1, xk, z1);
    if (j0 == k) z0 = xk;
    if (j1 == k) z1 = xk;
  }
  if (bad) z0 = z1 = __builtin_nanf("");
  if (j0 < n) xrow[j0] = z0;
  if (j1 < n) xrow[j1] = z1;
}

template <int NT>
int launch_solve(const SolveArgs& a, int64_t n_rows, hipStream_t st) {
  const size_t lds = solve_lds_bytes(NT);
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)als_solve_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("brAlsSolveRows: cannot raise the dynamic LDS limit to %zu B: %s", lds, hipGetErrorString(e)); return BR_ERR_HIP; }
    attr = true;
  }
  als_solve_kernel<NT><<<(unsigned)n_rows, kAlsThreads, lds, st>>>(a);
  return BR_OK;
}

template <int NT>
void launch_gram(unsigned grid, hipStream_t st, const float* Y, int64_t ld, int64_t rows, int dim, int64_t per, int vec, float* ws) {
  gram_partial_kernel<NT><<<grid, kAlsThreads, sizeof(float) * gram_lds_floats(NT), st>>>(Y, ld, rows, dim, per, vec, ws);
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brGramWorkspaceBytes(int64_t rows, int dim) {
  if (rows < 0 || dim < 1 || dim > kAlsMaxDim) return -1;
  if (rows == 0) return 0;
  int64_t n_wg, per;
  gram_plan(rows, nt_of(dim), &n_wg, &per);
  return n_wg * ntl_of(dim) * 1024 * (int64_t)sizeof(float);
}

extern "C" int brGram(const float* Y, int64_t ld, int64_t rows, int dim, float* G, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(dim >= 1 && dim <= kAlsMaxDim, "brGram: dim = %d outside [1, %d]", dim, kAlsMaxDim);
  BR_CHECK_ARG(rows >= 0, "brGram: rows = %lld < 0", (long long)rows);
  BR_CHECK_ARG(ld >= dim, "brGram: ld = %lld < dim = %d", (long long)ld, dim);
  BR_CHECK_ARG(G && (Y || rows == 0), "brGram: null pointer");
  const int64_t need = brGramWorkspaceBytes(rows, dim);
  if (ws_bytes < need || (need > 0 && !ws)) {
    br::set_error("brGram: workspace %lld bytes < %lld", (long long)(ws ? ws_bytes : 0), (long long)need);
    return BR_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int64_t n_wg = 0, per = 0;
  if (rows > 0) {
    gram_plan(rows, nt_of(dim), &n_wg, &per);
    const int vec = rows_vec4(Y, ld, dim);
    switch (nt_of(dim)) {
      case 1: launch_gram<1>((unsigned)n_wg, st, Y, ld, rows, dim, per, vec, (float*)ws); break;
      case 2: launch_gram<2>((unsigned)n_wg, st, Y, ld, rows, dim, per, vec, (float*)ws); break;
      case 3: launch_gram<3>((unsigned)n_wg, st, Y, ld, rows, dim, per, vec, (float*)ws); break;
      default: launch_gram<4>((unsigned)n_wg, st, Y, ld, rows, dim, per, vec, (float*)ws); break;
    }
    BR_CHECK_LAUNCH("brGram");
  }
  const int ntl = ntl_of(dim);
  gram_reduce_kernel<<<(unsigned)(ntl * 1024 / 64), kAlsThreads, 0, st>>>((const float*)ws, n_wg, ntl, dim, G);
  BR_CHECK_LAUNCH("brGram reduce");
  return BR_OK;
}

extern "C" int brAlsSolveRows(const float* Y, int64_t ld_y, int64_t n_y, int dim, const float* G, const int64_t* off, const int32_t* idx,
                              const float* conf, float alpha, float reg, int64_t n_rows, float* X, int64_t ld_x, int* err_flag, brStream stream) {
  BR_CHECK_ARG(dim >= 1 && dim <= kAlsMaxDim, "brAlsSolveRows: dim = %d outside [1, %d]", dim, kAlsMaxDim);
  BR_CHECK_ARG(ld_y >= dim && ld_x >= dim, "brAlsSolveRows: ld_y = %lld, ld_x = %lld below dim = %d", (long long)ld_y, (long long)ld_x, dim);
  BR_CHECK_ARG(n_y >= 0 && n_y < ((int64_t)1 << 31), "brAlsSolveRows: n_y = %lld outside [0, 2^31)", (long long)n_y);
  BR_CHECK_ARG(reg > 0.f && reg <= FLT_MAX, "brAlsSolveRows: reg = %g must be positive and finite", (double)reg);
  BR_CHECK_ARG(alpha >= 0.f && alpha <= FLT_MAX, "brAlsSolveRows: alpha = %g must be >= 0 and finite", (double)alpha);
  BR_CHECK_ARG(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "brAlsSolveRows: n_rows = %lld outside [0, 2^31)", (long long)n_rows);
  if (n_rows == 0) return BR_OK;
  BR_CHECK_ARG(Y && G && off && X, "brAlsSolveRows: null pointer");
  SolveArgs a{Y, ld_y, (int32_t)n_y, dim, G, off, idx, conf, alpha, reg, X, ld_x, err_flag, rows_vec4(Y, ld_y, dim) ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (nt_of(dim)) {
    case 1: rc = launch_solve<1>(a, n_rows, st); break;
    case 2: rc = launch_solve<2>(a, n_rows, st); break;
    case 3: rc = launch_solve<3>(a, n_rows, st); break;
    default: rc = launch_solve<4>(a, n_rows, st); break;
  }
  if (rc != BR_OK) return rc;
  BR_CHECK_LAUNCH("brAlsSolveRows");
  return BR_OK;
}
