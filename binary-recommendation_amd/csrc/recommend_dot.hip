// Catalogue recommendation for dot-product models (include/binrec.h "Catalogue top-k"): BPR tables or TwoTower tower outputs,
// score(u, i) = sum_j Q[u][j] C[i][j] in fp32, only the k best items per user written out, seen items excluded on the way; the
// U x I score matrix is never stored.
//
//   - scores come from v_mfma_f32_16x16x4_f32 with the features in natural order: bit for bit the k-ordered fmaf chain
//     acc = fma(q_j, c_j, acc) from acc = 0 (features padded with zeros to the instantiation's width), so a pair's score depends on
//     its two rows only, not on U, I, the split plan or where the pair falls in a tile;
//   - a workgroup is 4 waves; a wave owns 16 * RT users, whose A fragments (user rows) stay in registers for the whole launch;
//   - the workgroup streams its item split through LDS, NT = 16 * CT items per step (float4 loads when rows are 16-B aligned,
//     scalar loads otherwise), the next step's items in flight while the current step is scored;
//   - per step a wave computes RT x CT tiles of 16 x 16 scores; each lane compares its 4 * RT * CT scores with its users' k-th best
//     entries (one compare per pair); the rare pairs that pass are queued in LDS and then inserted into the user's list, which
//     lives in LDS (sorted by (score desc, position asc), inserted wave-cooperatively as WaveList does in registers);
//   - the exclusion CSR is walked with one cursor per user (lane u of the wave) as the item window advances: one 64-bit mask per
//     user and window, looked at only for the pairs that pass the threshold;
//   - the item axis is cut into splits so that a short user list still fills the device; catalog_merge_kernel (topk_list.h)
//     combines the splits' lists with the same order and pads with (-inf, -1).
#include <math.h>

#include "common.h"
#include "dot_tile.h"
#include "topk_list.h"

namespace br {
namespace {

constexpr int kDotQueue = 128;            // candidate queue entries per wave (flushed before it can overflow)

// list capacity, row tiles per wave and column tiles per step by k: the per-user lists of a workgroup live in LDS
// (4 waves x 16 RT users x KMAX entries x 8 B), so large k takes fewer users per workgroup
struct DotCfg {
  int kmax, rt, ct;
};
DotCfg dot_cfg(int k) {
  if (k <= 16) return {16, 2, 4};
  if (k <= 64) return {64, 2, 4};
  if (k <= 128) return {128, 1, 4};
  return {256, 1, 2};
}

void dot_plan(int64_t n_users, int64_t n_items, int k, int64_t* splits, int64_t* steps_per_split) {
  const DotCfg c = dot_cfg(k);
  split_plan(ceil_div(n_items, 16 * c.ct), n_users, 64 * c.rt, splits, steps_per_split);
}

template <int KB, int KMAX, int RT, int CT>
__global__ __launch_bounds__(256) void dot_topk_kernel(const float* __restrict__ Q, int64_t ld_q, int64_t n_users,
                                                        const float* __restrict__ C, int64_t ld_c, int64_t n_items, int dim, int vec,
                                                        const int64_t* __restrict__ ex_off, const int32_t* __restrict__ ex_idx, int k,
                                                        int64_t steps_per_split, int64_t n_splits, float* __restrict__ part_s,
                                                        int32_t* __restrict__ part_p, float* __restrict__ dump) {
  constexpr int UW = 16 * RT;              // users per wave
  constexpr int NT = 16 * CT;              // items per step (<= 64: one exclusion mask word)
  constexpr int LD = 4 * KB + 4;           // item tile row stride (floats): KB even -> the B-fragment reads hit 64 distinct banks
  constexpr int CHUNKS = NT * KB;          // float4 chunks per item tile
  constexpr int CPT = (CHUNKS + 255) / 256;
  constexpr int SLOTS = (KMAX + 63) / 64;
  static_assert(NT <= 64 && KB % 2 == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) float tile[NT * LD];
  __shared__ float lst_s[4 * UW * KMAX];
  __shared__ int32_t lst_p[4 * UW * KMAX];
  __shared__ float thr_s[4 * UW];
  __shared__ int32_t thr_p[4 * UW];
  __shared__ float q_s[4 * kDotQueue];
  __shared__ int32_t q_p[4 * kDotQueue];
  __shared__ int32_t q_r[4 * kDotQueue];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = ((int64_t)blockIdx.x * 4 + wave) * UW;         // first user of this wave
  const bool active = u0 < n_users;                                   // (inactive waves still take part in the barriers)
  const int64_t split = blockIdx.y;
  const int64_t p0 = split * steps_per_split * NT;
  const int64_t p1 = p0 + steps_per_split * NT < n_items ? p0 + steps_per_split * NT : n_items;
  float* const LS = lst_s + wave * UW * KMAX;
  int32_t* const LP = lst_p + wave * UW * KMAX;
  float* const TS = thr_s + wave * UW;
  int32_t* const TP = thr_p + wave * UW;
  float* const QS = q_s + wave * kDotQueue;
  int32_t* const QP = q_p + wave * kDotQueue;
  int32_t* const QR = q_r + wave * kDotQueue;

  // user rows as A fragments: lane l holds Q[u0 + 16 rt + (l & 15)][4 kb + (l >> 4)]
  float qa[RT][KB];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t u = u0 + 16 * rt + (lane & 15);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int f = 4 * kb + (lane >> 4);
      qa[rt][kb] = (u < n_users && f < dim) ? Q[u * ld_q + f] : 0.f;
    }
  }
  for (int i = lane; i < UW * KMAX; i += 64) { LS[i] = -INFINITY; LP[i] = kNoPos; }
  if (lane < UW) {                                                    // users past the end: a threshold nothing beats
    const bool ok = u0 + lane < n_users;
    TS[lane] = ok ? -INFINITY : INFINITY;
    TP[lane] = ok ? kNoPos : -1;
  }

  // exclusion cursor of user u0 + lane: the first entry of its list at or after p0, and that entry's position
  int64_t ex_cur = 0, ex_end = 0, ex_nxt = INT64_MAX;
  if (ex_off && lane < UW && u0 + lane < n_users) {
    int64_t lo = ex_off[u0 + lane], hi = ex_off[u0 + lane + 1];
    ex_end = hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)ex_idx[mid] < p0) lo = mid + 1; else hi = mid;
    }
    ex_cur = lo;
    if (ex_cur < ex_end) ex_nxt = ex_idx[ex_cur];
  }

  float4 pre[CPT];
  auto load_tile = [&](int64_t start) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int chunk = c * 256 + tid;
      const int it = chunk / KB, f = 4 * (chunk % KB);
      const int64_t p = start + it;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (chunk < CHUNKS && p < p1 && f < dim) {
        const float* row = C + p * ld_c + f;
        if (vec) {
          v = *reinterpret_cast<const float4*>(row);
        } else {
          v.x = row[0];
          if (f + 1 < dim) v.y = row[1];
          if (f + 2 < dim) v.z = row[2];
          if (f + 3 < dim) v.w = row[3];
        }
      }
      pre[c] = v;
    }
  };
  load_tile(p0);

  for (int64_t base = p0; base < p1; base += NT) {
    __syncthreads();                                                  // the previous step's tile reads are done
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int chunk = c * 256 + tid;
      if (chunk < CHUNKS) *reinterpret_cast<float4*>(tile + (chunk / KB) * LD + 4 * (chunk % KB)) = pre[c];
    }
    __syncthreads();
    if (base + NT < p1) load_tile(base + NT);                         // in flight while this step is scored
    if (!active) continue;

    // this window's exclusion mask of user u0 + lane (lanes < UW)
    uint64_t xm = 0;
    while (ex_nxt < base + NT) {
      if (ex_nxt >= base) xm |= 1ull << (ex_nxt - base);
      ++ex_cur;
      ex_nxt = ex_cur < ex_end ? (int64_t)ex_idx[ex_cur] : INT64_MAX;
    }
    const bool any_ex = __ballot(xm != 0) != 0;

    f32x4 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float b = tile[(16 * ct + (lane & 15)) * LD + 4 * kb + (lane >> 4)];   // B[k][j] = C[item j][feature 4 kb + k]
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[rt][kb], b, acc[rt][ct], 0, 0, 0);
      }
    }

    // D: lane l, register r = score(user u0 + 16 rt + 4 (l >> 4) + r, item base + 16 ct + (l & 15))
    float ts[RT][4];
    int32_t tp[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ts[rt][r] = TS[16 * rt + 4 * (lane >> 4) + r];
        tp[rt][r] = TP[16 * rt + 4 * (lane >> 4) + r];
      }
    int qn = 0;
    auto flush = [&]() {
      wave_lds_order();
      for (int i = 0; i < qn; ++i) {
        const int row = QR[i];
        const float cs = QS[i];
        const int32_t cp = QP[i];
        if (any_ex) {
          const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)xm, row, 64), hi = (uint32_t)__shfl((int)(uint32_t)(xm >> 32), row, 64);
          const uint64_t m = ((uint64_t)hi << 32) | lo;
          if ((m >> (cp - base)) & 1) continue;
        }
        float nts = TS[row];
        int32_t ntp = TP[row];
        if (!beats(cs, cp, nts, ntp)) continue;
        list_insert<SLOTS>(LS + row * KMAX, LP + row * KMAX, k, lane, cs, cp, nts, ntp);
        wave_lds_order();
        if (lane == 0) { TS[row] = nts; TP[row] = ntp; }
        wave_lds_order();
      }
      qn = 0;
    };
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int64_t p = base + 16 * ct + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[rt][ct][r];
          const int row = 16 * rt + 4 * (lane >> 4) + r;
          if (dump && p < p1 && u0 + row < n_users) dump[(u0 + row) * n_items + p] = s;
          const bool pass = p < p1 && beats(s, (int32_t)p, ts[rt][r], tp[rt][r]);
          const uint64_t bal = __ballot(pass);
          if (bal) {
            if (qn > kDotQueue - 64) flush();
            if (pass) {
              const int slot = qn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
              QS[slot] = s; QP[slot] = (int32_t)p; QR[slot] = row;
            }
            qn += __popcll(bal);
          }
        }
      }
    if (qn) flush();
  }

  __syncthreads();
  if (!active) return;
  for (int row = 0; row < UW; ++row) {
    const int64_t u = u0 + row;
    if (u >= n_users) break;
    const int64_t o = (u * n_splits + split) * k;
    for (int e = lane; e < k; e += 64) { part_s[o + e] = LS[row * KMAX + e]; part_p[o + e] = LP[row * KMAX + e]; }
  }
}

template <int KB>
void launch_dot_topk(int kmax, dim3 grid, hipStream_t st, const float* Q, int64_t ld_q, int64_t U, const float* C, int64_t ld_c, int64_t I,
                     int dim, int vec, const int64_t* ex_off, const int32_t* ex_idx, int k, int64_t sps, int64_t S, float* ps, int32_t* pp,
                     float* dump) {
#define BR_DOT_ARGS Q, ld_q, U, C, ld_c, I, dim, vec, ex_off, ex_idx, k, sps, S, ps, pp, dump
  switch (kmax) {
    case 16: dot_topk_kernel<KB, 16, 2, 4><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
    case 64: dot_topk_kernel<KB, 64, 2, 4><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
    case 128: dot_topk_kernel<KB, 128, 1, 4><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
    default: dot_topk_kernel<KB, 256, 1, 2><<<grid, 256, 0, st>>>(BR_DOT_ARGS); break;
  }
#undef BR_DOT_ARGS
}

}  // namespace
}  // namespace br

using namespace br;

extern "C" int64_t brDotCatalogTopKWorkspaceBytes(int64_t n_users, int64_t n_items, int k) {
  if (n_users < 0 || n_items < 1 || n_items >= ((int64_t)1 << 31) || k < 1 || k > kRecMaxK) return -1;
  int64_t S, sps;
  dot_plan(n_users, n_items, k, &S, &sps);
  return 2 * part_bytes(n_users, S, k);
}

extern "C" int brDotCatalogTopK(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                                const int64_t* excl_off, const int32_t* excl_idx, int k, float* out_scores, int32_t* out_index,
                                float* dump_scores, void* ws, int64_t ws_bytes, brStream stream) {
  BR_CHECK_ARG(Q && C && out_scores && out_index && ws, "brDotCatalogTopK: null pointer");
  BR_CHECK_ARG(k >= 1 && k <= kRecMaxK, "brDotCatalogTopK: k = %d outside [1, %d]", k, kRecMaxK);
  if (const int rc = dot_check_args("brDotCatalogTopK", ld_q, n_users, ld_c, n_items, dim)) return rc;
  BR_CHECK_ARG((excl_off == nullptr) == (excl_idx == nullptr), "brDotCatalogTopK: exclusion needs both excl_off and excl_idx");
  int64_t S, sps;
  dot_plan(n_users, n_items, k, &S, &sps);
  const int64_t pb = part_bytes(n_users, S, k);
  if (ws_bytes < 2 * pb) {
    br::set_error("brDotCatalogTopK: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)(2 * pb));
    return BR_ERR_WORKSPACE;
  }
  if (n_users == 0) return BR_OK;
  float* ps = (float*)ws;
  int32_t* pp = (int32_t*)((char*)ws + pb);
  const DotCfg c = dot_cfg(k);
  const dim3 grid((unsigned)ceil_div(n_users, 64 * c.rt), (unsigned)S);
  const int vec = rows_vec4(C, ld_c, dim);
  hipStream_t st = (hipStream_t)stream;
  dispatch_kb(dim, [&](auto kb) {
    launch_dot_topk<decltype(kb)::value>(c.kmax, grid, st, Q, ld_q, n_users, C, ld_c, n_items, dim, vec, excl_off, excl_idx, k, sps, S, ps, pp,
                                         dump_scores);
  });
  BR_CHECK_LAUNCH("brDotCatalogTopK");
  catalog_merge_kernel<<<(unsigned)ceil_div(n_users, kRecWaves), 256, 0, st>>>(ps, pp, n_users, S, k, out_scores, out_index);
  BR_CHECK_LAUNCH("brDotCatalogTopK merge");
  return BR_OK;
}
