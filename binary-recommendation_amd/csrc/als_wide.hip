// Implicit-feedback ALS for rows up to 512 features: the Gram matrix in blocks of 128 columns, and the half-step by a
// few conjugate-gradient steps per row (Takacs, Pilaszy, Tikk 2011) instead of a factorisation.  The operator of a row is never formed:
//   A p = G p + reg p + sum_e c_e y_e (y_e . p),   b = sum_e (1 + c_e) y_e,   c_e = alpha * conf_e
//   brGramWide        grid = (row slices, pairs (I, J <= I) of 128-column blocks).  A workgroup stages 64 rows of both column blocks in LDS;
//                     wave w forms the four 32 x 32 tiles (w, 0 .. 3) of Ya^T Yb on the fp32-input MFMA over ALL rows of the chunk, adds
//                     the chunk's sums to its running ones and writes them to the workspace; a second launch adds the slices' partials
//                     in double in index order, rounds once and writes G[I][J] and G[J][I] from the one value.  No atomics.
//   brAlsSolveRowsCg  workgroup = 32 consecutive rows (16 above 256 features), wave w owns 8 (4) of them: x, r and p of a row live as
//                     doubles in the registers of its wave (lane l holds features l, l + 64, ...); LDS holds P rounded to float and
//                     Q = G P as [feature][row] (leading dimension 33).  One application of A: every wave multiplies its 32-row tiles
//                     of G into P on the fp32 MFMA (G is read once per batch, column r of the product depends on column r of P alone),
//                     then each wave adds, in double, the sparse term of its own rows: the row's entries 32 at a time, t_e = y_e . p
//                     by a butterfly over the wave, then q += c_e t_e y_e in the order of the CSR; reg p and the recurrence follow in
//                     double.  Rows never exchange a value: the bits of a row do not depend on the batch.
#include <float.h>

#include "common.h"

namespace br {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kThreads = 256;
constexpr int kWideMaxDim = 512;
constexpr int kColBlock = 128;          // columns of a block of the wide Gram
constexpr int kChunk = 64;              // rows staged per pass
constexpr int kMinRows = 256;           // rows of a workgroup's slice, at least
constexpr int kTargetWg = 1024;         // workgroups of the partial launch, about
constexpr int kPairFloats = 16 * 1024;  // a pair's partial: 16 tiles of 32 x 32

constexpr int kCgLd = 33;               // leading dimension of P and Q: feature-major reads and row-major reads both hit 32 banks
constexpr int kCgTile = 32;             // entries whose ids and weights one wave-load fetches
constexpr int kCgKBlock = 32;           // k-steps (2 features each) of G p summed from zero before they join the product
constexpr int kCgMaxSteps = 64;

// C/D layout of the 32x32 MFMA: register r of lane l is element (row, col) of the tile
__device__ __forceinline__ int mfma_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int mfma_col(int lane) { return lane & 31; }
// pair p of the lower triangle, row by row: (0,0) (1,0) (1,1) (2,0) ...
__device__ __forceinline__ void tri_pair(int p, int& bi, int& bj) {
  bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
  bj = p - bi * (bi + 1) / 2;
}

static int blocks_of(int dim) { return (dim + kColBlock - 1) / kColBlock; }
static int pairs_of(int dim) { const int nb = blocks_of(dim); return nb * (nb + 1) / 2; }
static bool rows_vec4(const float* p, int64_t ld, int dim) { return dim % 4 == 0 && ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// rows >= 1 -> the row slices of the partial launch and the rows each takes (a multiple of the chunk): a function of (rows, dim) alone
static void wide_plan(int64_t rows, int dim, int64_t* n_wg, int64_t* rows_per_wg) {
  int64_t max_wg = kTargetWg / pairs_of(dim);
  if (max_wg < 1) max_wg = 1;
  int64_t per = ceil_div(rows, max_wg);
  if (per < kMinRows) per = kMinRows;
  per = ceil_div(per, (int64_t)kChunk) * kChunk;
  *rows_per_wg = per;
  *n_wg = ceil_div(rows, per);
}

// ------------------------------------------------------------------------------------------------------------------ wide Gram
__global__ __launch_bounds__(kThreads, 2) void gram_wide_partial_kernel(const float* __restrict__ Y, int64_t ld, int64_t rows, int dim,
                                                                         int64_t rows_per_wg, int vec, float* __restrict__ ws) {
  constexpr int CB = kColBlock, CB4 = CB / 4, PRE = kChunk * CB / kThreads;     // floats of one block's chunk per thread
  __shared__ float As[kChunk * CB];
  __shared__ float Bs[kChunk * CB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int bi, bj;
  tri_pair(blockIdx.y, bi, bj);
  const bool diag = bi == bj;
  const int ca = bi * CB, cb = bj * CB;
  const int wa = dim - ca < CB ? dim - ca : CB, wb = dim - cb < CB ? dim - cb : CB;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
  const float* Bsrc = diag ? As : Bs;

  f32x16 tot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[t][r] = 0.f;

  // Loads go to clamped addresses and the values are selected afterwards (als.hip): rows past the slice and columns past dim are zero,
  // and both load paths put the same values into the same places
  float pa[PRE], pb[PRE];
  auto fetch = [&](float* pre, int c0, int wd, int64_t row0) {
    const int n = (int)(r1 - row0 < kChunk ? r1 - row0 : kChunk);
    if (vec) {
#pragma unroll
      for (int q = 0; q < PRE / 4; ++q) {
        const int e = tid + q * kThreads, r = e / CB4, c4 = e - r * CB4;
        const bool in = r < n && 4 * c4 < wd;
        const float4 v = *reinterpret_cast<const float4*>(Y + (row0 + (in ? r : 0)) * ld + c0 + 4 * (in ? c4 : 0));
        pre[4 * q] = in ? v.x : 0.f; pre[4 * q + 1] = in ? v.y : 0.f; pre[4 * q + 2] = in ? v.z : 0.f; pre[4 * q + 3] = in ? v.w : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < PRE; ++q) {
        const int e = tid + q * kThreads, r = e / CB, c = e - r * CB;
        const bool in = r < n && c < wd;
        const float v = Y[(row0 + (in ? r : 0)) * ld + c0 + (in ? c : 0)];
        pre[q] = in ? v : 0.f;
      }
    }
  };
  auto stage = [&](float* dst, const float* pre) {
    if (vec) {
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
    fetch(pa, ca, wa, r0);
    if (!diag) fetch(pb, cb, wb, r0);
  }
  for (int64_t c0 = r0; c0 < r1; c0 += kChunk) {
    const int n = (int)(r1 - c0 < kChunk ? r1 - c0 : kChunk);
    __syncthreads();
    stage(As, pa);
    if (!diag) stage(Bs, pb);
    __syncthreads();
    if (c0 + kChunk < r1) {
      fetch(pa, ca, wa, c0 + kChunk);
      if (!diag) fetch(pb, cb, wb, c0 + kChunk);
    }
    // the chunk's own sums start from zero and join the slice's once: a slice of 10 000 rows is 160 additions, not one chain of 10 000
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int ksteps = (n + 1) >> 1;           // rows past n are zero
    for (int kk = 0; kk < ksteps; ++kk) {
      const int row = 2 * kk + (lane >> 5);
      const float va = As[row * CB + 32 * w + (lane & 31)];
      float vb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) vb[t] = Bsrc[row * CB + 32 * t + (lane & 31)];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(va, vb[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) tot[t] += acc[t];
  }
  float* out = ws + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * kPairFloats + (int64_t)w * 4 * 1024;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(t * 16 + r) * 64 + lane] = tot[t][r];
}

// 64 elements of one pair per workgroup, each summed by 4 threads over a quarter of the slices in index order; the quarters are added
// (0 + 1) + (2 + 3).  A diagonal pair writes its lower triangle and mirrors it; the others write G[I][J] and G[J][I] from the one value
__global__ __launch_bounds__(kThreads) void gram_wide_reduce_kernel(const float* __restrict__ ws, int64_t n_wg, int dim, float* __restrict__ G) {
  __shared__ double part[kThreads];
  const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;        // (tile, register, lane) of the pair's partial
  const int64_t p0 = n_wg * q / 4, p1 = n_wg * (q + 1) / 4;
  double s = 0.0;
  for (int64_t p = p0; p < p1; ++p) s += (double)ws[(p * gridDim.y + blockIdx.y) * kPairFloats + e];
  part[threadIdx.x] = s;
  __syncthreads();
  if (q != 0) return;
  const float g = (float)((part[el] + part[64 + el]) + (part[128 + el] + part[192 + el]));
  int bi, bj;
  tri_pair(blockIdx.y, bi, bj);
  const int tile = e >> 10, ti = tile >> 2, tj = tile & 3;
  const int gi = bi * kColBlock + ti * 32 + mfma_row((e >> 6) & 15, el), gj = bj * kColBlock + tj * 32 + mfma_col(el);
  if (gi >= dim || gj >= dim || (bi == bj && gi < gj)) return;
  G[(int64_t)gi * dim + gj] = g;
  if (gi != gj) G[(int64_t)gj * dim + gi] = g;
}

// ------------------------------------------------------------------------------------------------------------------ CG half-step
struct CgArgs {
  const float* Y; int64_t ld_y; int32_t n_y; int dim; const float* G;
  const int64_t* off; const int32_t* idx; const float* conf; float alpha, reg;
  float* X; int64_t ld_x; int64_t n_rows; int* err; int steps;
};

static size_t cg_lds_bytes(int kf) { return sizeof(float) * 2 * (size_t)(kf * 64) * kCgLd; }
// dim -> features per lane of the row layout (the template argument): 1, 2, 4, 6, 8
static int cg_kf(int dim) { const int k = (dim + 63) / 64; return k <= 2 ? k : (k + 1) & ~1; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);     // every lane ends with the same bits
  return v;
}

// rows of a wave: 8, or 4 where a lane holds 6 or 8 features of a row (x, r and p of a row are doubles in registers)
constexpr int cg_rows_per_wave(int kf) { return kf >= 6 ? 4 : 8; }

template <int KF>
__global__ __launch_bounds__(kThreads) void als_cg_kernel(CgArgs a) {
  constexpr int FP = KF * 64, TPW = (2 * KF + 3) / 4, SUB = KF >= 8 ? 2 : (KF >= 4 ? 4 : 8), LD = kCgLd, RPW = cg_rows_per_wave(KF);
  extern __shared__ float smem[];
  float* Ps = smem;                           // [FP][LD] the search directions rounded to float (first: the start vectors), zero past dim
  float* Qs = smem + FP * LD;                 // [FP][LD] G P from the MFMA; then, with the row's column of Ps, the two halves of a double
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = a.dim, NT = (n + 31) >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * (4 * RPW) + w * RPW;     // this wave's first row
  const double reg = (double)a.reg;

  for (int i = tid; i < FP * LD; i += kThreads) Ps[i] = 0.f;          // the columns no wave owns (RPW = 4: 16 .. 31) stay zero
  __syncthreads();

  // ---- this wave's rows: x from X (the warm start); a row without entries is zeros and is never iterated.  The recurrence runs in
  // double: in float its roundings, not those of G p, decide an ill-conditioned row
  double x[RPW][KF], r[RPW][KF], p[RPW][KF], rs[RPW];
  unsigned live = 0, valid = 0;
#pragma unroll
  for (int m = 0; m < RPW; ++m) {
    const int64_t u = row0 + m;
    const bool in = u < a.n_rows;
    const bool has = in && a.off[u + 1] > a.off[u];
    valid |= (unsigned)in << m;
    live |= (unsigned)has << m;
    rs[m] = 0.0;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const int f = lane + 64 * k;
      float v = 0.f;
      if (has && f < n) v = a.X[u * a.ld_x + f];
      x[m][k] = (double)v;
      r[m][k] = p[m][k] = 0.0;
      Ps[f * LD + w * RPW + m] = v;
    }
  }

  // Q = G P on the MFMA: wave w forms the 32-feature tiles w, w + 4, ...; G is read through its transpose (G is symmetric: the lanes of
  // a load then read consecutive addresses).  Operand a: G[i][j], lane = (i, j parity); operand b: P[j][row]
  auto apply_g = [&]() {
    __syncthreads();
    f32x16 tot[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s)
#pragma unroll
      for (int q = 0; q < 16; ++q) tot[s][q] = 0.f;
    const int ksteps = (n + 1) >> 1;
    for (int kb = 0; kb < ksteps; kb += kCgKBlock) {
      f32x16 acc[TPW];
#pragma unroll
      for (int s = 0; s < TPW; ++s)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;
      const int kend = kb + kCgKBlock < ksteps ? kb + kCgKBlock : ksteps;
#pragma unroll 8
      for (int kk = kb; kk < kend; ++kk) {
        const int j = 2 * kk + (lane >> 5);
        const float bv = Ps[j * LD + (lane & 31)];
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
          const int t = w + 4 * s, i = t * 32 + (lane & 31);
          if (t >= NT) continue;              // (the same for every lane of the wave)
          const bool in = j < n && i < n;
          const float g = a.G[in ? (int64_t)j * n + i : 0];
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? g : 0.f, bv, acc[s], 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < TPW; ++s) tot[s] += acc[s];
    }
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
      const int t = w + 4 * s;
      if (t >= NT) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) Qs[(t * 32 + mfma_row(q, lane)) * LD + mfma_col(lane)] = tot[s][q];
    }
    __syncthreads();
  };

  // v = G p + sum_e c_e y_e (y_e . p) for this wave's live rows, in double from the float p of the row's column of P; first = true:
  // v = b - that.  v leaves as two floats, v ~ Q[:, row] + P[:, row] (the column of P is the row's own until the next apply_g and p
  // itself is in registers); reg p is added by the caller, which holds p as doubles.  Only LDS and the row's own entries are touched
  auto sparse = [&](bool first) {
#pragma unroll 1
    for (int m = 0; m < RPW; ++m) {
      if (!((live >> m) & 1)) continue;
      const int rho = w * RPW + m;
      const int64_t u = row0 + m;
      const int64_t e0 = a.off[u], e1 = a.off[u + 1];
      float p32[KF];
      double qrow[KF], brow[KF];
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        p32[k] = Ps[(lane + 64 * k) * LD + rho];
        qrow[k] = brow[k] = 0.0;
      }
      for (int64_t t0 = e0; t0 < e1; t0 += kCgTile) {
        const int cnt = (int)(e1 - t0 < kCgTile ? e1 - t0 : kCgTile);
        int id = -1;
        double c = 0.0, b1 = 0.0;
        if (lane < cnt) {
          const int32_t v = a.idx[t0 + lane];
          if (v >= 0 && v < a.n_y) {
            id = v;
            c = a.conf ? (double)a.alpha * (double)a.conf[t0 + lane] : (double)a.alpha;
            b1 = 1.0 + c;
          } else if (a.err) {
            atomicOr(a.err, BR_ERRFLAG_RANGE);   // never an address: the entry counts as absent
          }
        }
        for (int es = 0; es < cnt; es += SUB) {
          float y[SUB][KF];
#pragma unroll
          for (int s = 0; s < SUB; ++s) {
            const int ide = __shfl(id, es + s, 64);          // es + s < 40: lanes past cnt hold -1
#pragma unroll
            for (int k = 0; k < KF; ++k) {
              const int f = lane + 64 * k;
              float v = 0.f;
              if (ide >= 0 && f < n) v = a.Y[(int64_t)ide * a.ld_y + f];
              y[s][k] = v;
            }
          }
#pragma unroll
          for (int s = 0; s < SUB; ++s) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < KF; ++k) t = fma((double)y[s][k], (double)p32[k], t);
            t = wave_sum(t);
            const double ct = __shfl(c, es + s, 64) * t, b1e = __shfl(b1, es + s, 64);
#pragma unroll
            for (int k = 0; k < KF; ++k) {
              qrow[k] = fma(ct, (double)y[s][k], qrow[k]);
              brow[k] = fma(b1e, (double)y[s][k], brow[k]);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        const int f = lane + 64 * k;
        const double gp = f < n ? (double)Qs[f * LD + rho] : 0.0;     // (rows of Q past the last tile are never written)
        const double ap = gp + qrow[k];
        const double v = f < n ? (first ? brow[k] - ap : ap) : 0.0;
        const float hi = (float)v;
        Qs[f * LD + rho] = hi;
        Ps[f * LD + rho] = (float)(v - (double)hi);
      }
    }
  };

  // ---- r = b - A x, p = r, rs = r . r
  apply_g();
  sparse(true);
#pragma unroll
  for (int m = 0; m < RPW; ++m) {
    const int rho = w * RPW + m;
    const bool on = (live >> m) & 1;
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const int f = lane + 64 * k;
      const double v = on ? ((double)Qs[f * LD + rho] + (double)Ps[f * LD + rho]) - reg * x[m][k] : 0.0;
      r[m][k] = p[m][k] = v;
      Ps[f * LD + rho] = (float)v;
      t = fma(v, v, t);
    }
    rs[m] = wave_sum(t);
  }

  for (int it = 0; it < a.steps; ++it) {
    if (__syncthreads_or(live != 0) == 0) break;               // every row of the batch has stopped
    apply_g();
    sparse(false);
#pragma unroll
    for (int m = 0; m < RPW; ++m) {
      if (!((live >> m) & 1)) continue;
      const int rho = w * RPW + m;
      double q[KF], d = 0.0;
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        const int f = lane + 64 * k;
        q[k] = fma(reg, p[m][k], (double)Qs[f * LD + rho] + (double)Ps[f * LD + rho]);
        d = fma(p[m][k], q[k], d);
      }
      d = wave_sum(d);
      // (every lane holds the same rs and d: the row stops in all of them or in none)
      if (!(rs[m] >= 1e-20) || !(d > 0.0 && d <= DBL_MAX)) {
        live &= ~(1u << m);
#pragma unroll
        for (int k = 0; k < KF; ++k) Ps[(lane + 64 * k) * LD + rho] = 0.f;
        continue;
      }
      const double al = rs[m] / d;
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        x[m][k] = fma(al, p[m][k], x[m][k]);
        r[m][k] = fma(-al, q[k], r[m][k]);
        t = fma(r[m][k], r[m][k], t);
      }
      const double rn = wave_sum(t), beta = rn / rs[m];
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        p[m][k] = lane + 64 * k < n ? fma(beta, p[m][k], r[m][k]) : 0.0;
        Ps[(lane + 64 * k) * LD + rho] = (float)p[m][k];
      }
      rs[m] = rn;
    }
  }

#pragma unroll
  for (int m = 0; m < RPW; ++m) {
    if (!((valid >> m) & 1)) continue;
    float* xrow = a.X + (row0 + m) * a.ld_x;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const int f = lane + 64 * k;
      if (f < n) xrow[f] = (float)x[m][k];
    }
  }
}

template <int KF>
int launch_cg(const CgArgs& a, hipStream_t st) {
  const size_t lds = cg_lds_bytes(KF);
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)als_cg_kernel<KF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("brAlsSolveRowsCg: cannot raise the dynamic LDS limit to %zu B: %s", lds, hipGetErrorString(e)); return BR_ERR_HIP; }
    attr = true;
  }
  als_cg_kernel<KF><<<(unsigned)ceil_div(a.n_rows, (int64_t)(4 * cg_rows_per_wave(KF))), kThreads, lds, st>>>(a);
  return BR_OK;
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brGramWideWorkspaceBytes(int64_t rows, int dim) {
  if (rows < 0 || dim < 1 || dim > kWideMaxDim) return -1;
  if (rows == 0) return 0;
  int64_t n_wg, per;
  wide_plan(rows, dim, &n_wg, &per);
  return n_wg * pairs_of(dim) * kPairFloats * (int64_t)sizeof(float);
}

extern "C" int brGramWide(const float* Y, int64_t ld, int64_t rows, int dim, float* G, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(dim >= 1 && dim <= kWideMaxDim, "brGramWide: dim = %d outside [1, %d]", dim, kWideMaxDim);
  BR_CHECK_ARG(rows >= 0, "brGramWide: rows = %lld < 0", (long long)rows);
  BR_CHECK_ARG(ld >= dim, "brGramWide: ld = %lld < dim = %d", (long long)ld, dim);
  BR_CHECK_ARG(G && (Y || rows == 0), "brGramWide: null pointer");
  const int64_t need = brGramWideWorkspaceBytes(rows, dim);
  if (ws_bytes < need || (need > 0 && !ws)) {
    br::set_error("brGramWide: workspace %lld bytes < %lld", (long long)(ws ? ws_bytes : 0), (long long)need);
    return BR_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int pairs = pairs_of(dim);
  int64_t n_wg = 0, per = 0;
  if (rows > 0) {
    wide_plan(rows, dim, &n_wg, &per);
    gram_wide_partial_kernel<<<dim3((unsigned)n_wg, (unsigned)pairs), kThreads, 0, st>>>(Y, ld, rows, dim, per, rows_vec4(Y, ld, dim) ? 1 : 0, (float*)ws);
    BR_CHECK_LAUNCH("brGramWide");
  }
  gram_wide_reduce_kernel<<<dim3(kPairFloats / 64, (unsigned)pairs), kThreads, 0, st>>>((const float*)ws, n_wg, dim, G);
  BR_CHECK_LAUNCH("brGramWide reduce");
  return BR_OK;
}

extern "C" int brAlsSolveRowsCg(const float* Y, int64_t ld_y, int64_t n_y, int dim, const float* G, const int64_t* off, const int32_t* idx,
                                const float* conf, float alpha, float reg, int64_t n_rows, float* X, int64_t ld_x, int steps, int* err_flag,
                                brStream stream) {
  BR_CHECK_ARG(dim >= 1 && dim <= kWideMaxDim, "brAlsSolveRowsCg: dim = %d outside [1, %d]", dim, kWideMaxDim);
  BR_CHECK_ARG(ld_y >= dim && ld_x >= dim, "brAlsSolveRowsCg: ld_y = %lld, ld_x = %lld below dim = %d", (long long)ld_y, (long long)ld_x, dim);
  BR_CHECK_ARG(n_y >= 0 && n_y < ((int64_t)1 << 31), "brAlsSolveRowsCg: n_y = %lld outside [0, 2^31)", (long long)n_y);
  BR_CHECK_ARG(reg > 0.f && reg <= FLT_MAX, "brAlsSolveRowsCg: reg = %g must be positive and finite", (double)reg);
  BR_CHECK_ARG(alpha >= 0.f && alpha <= FLT_MAX, "brAlsSolveRowsCg: alpha = %g must be >= 0 and finite", (double)alpha);
  BR_CHECK_ARG(steps >= 1 && steps <= kCgMaxSteps, "brAlsSolveRowsCg: steps = %d outside [1, %d]", steps, kCgMaxSteps);
  BR_CHECK_ARG(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "brAlsSolveRowsCg: n_rows = %lld outside [0, 2^31)", (long long)n_rows);
  if (n_rows == 0) return BR_OK;
  BR_CHECK_ARG(Y && G && off && X, "brAlsSolveRowsCg: null pointer");
  CgArgs a{Y, ld_y, (int32_t)n_y, dim, G, off, idx, conf, alpha, reg, X, ld_x, n_rows, err_flag, steps};
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (cg_kf(dim)) {
    case 1: rc = launch_cg<1>(a, st); break;
    case 2: rc = launch_cg<2>(a, st); break;
    case 4: rc = launch_cg<4>(a, st); break;
    case 6: rc = launch_cg<6>(a, st); break;
    default: rc = launch_cg<8>(a, st); break;
  }
  if (rc != BR_OK) return rc;
  BR_CHECK_LAUNCH("brAlsSolveRowsCg");
  return BR_OK;
}
