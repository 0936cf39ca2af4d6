// Per-step batches for the NeuMF fit (brNeumfSampleBatch, include/binrec.h): one launch BESIDE the step forms rows [row0, row0 + B) of
// epoch e - positives with label 1 and, for every positive, r negatives with label 0 drawn again in every epoch and rejected while they
// are positives of the customer - straight into the (users, items, labels) buffers the step reads.  It stands in for
// src/models/NeuMFModel.py:102-123 (bootstrapDataset + the shuffled tf.data pipeline) like brBootstrapDataset, but per step: nothing of
// the epoch's n (1 + r) rows is ever materialised, and there is no host shuffle.
//
// A row is a pure function of (seed, epoch, global row g): src = feistel_perm(g, N, key of the epoch) names a positive (src < n) or
// negative j = src - n of positive j / r.  The draw keys on j, not on g: the negatives of a positive depend neither on the epoch's
// order nor on how it is cut into batches or ranks.
//
// Shape: one thread per output row, 256 per workgroup, no LDS.  The permutation and the Philox rounds are register arithmetic; the one
// chain of dependent round trips is src -> user -> CSR bounds -> the customer's positives -> (alias, candidate id) per attempt, so the
// launch is bound by latency and wants every wave the registers admit (DESIGN.md section 4o has the resource report).  The positives
// of a customer with up to 8 of them are fetched once by independent loads (Positives, sampling.h); the draw of an attempt is the
// text BPR's sampler uses (candidate_of).  Each lane stores the ids and the label it formed.
#include "common.h"
#include "rows.h"
#include "philox.h"
#include "sampling.h"

namespace br {

struct EpochArgs {
  const void* pos_users; const void* pos_items; uint32_t n, r, N;
  const int64_t* pos_off; const void* pos_sorted; int64_t num_users;
  const void* cand; const uint32_t* thresh; const int32_t* alias; uint32_t n_cand;
  uint64_t seed; uint32_t epoch; PermKey key; uint32_t row0; int max_tries;
};

template <typename IdT>
__global__ __launch_bounds__(256) void neumf_sample_batch_kernel(const EpochArgs a, int64_t batch, IdT* __restrict__ ou, IdT* __restrict__ oi,
                                                                 float* __restrict__ oy, int* err) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const uint32_t src = feistel_perm(a.row0 + (uint32_t)b, a.N, a.key);          // (row0 + batch <= N < 2^32: checked by the host)
  if (src < a.n) {
    ou[b] = ((const IdT*)a.pos_users)[src]; oi[b] = ((const IdT*)a.pos_items)[src]; oy[b] = 1.f;
    return;
  }
  const uint32_t j = src - a.n;
  const IdT user = ((const IdT*)a.pos_users)[j / a.r];
  int64_t u = (int64_t)user;
  if ((uint64_t)u >= (uint64_t)a.num_users) { if (err) atomicOr(err, BR_ERRFLAG_RANGE); u = 0; }
  Positives<IdT> pos;
  pos.load(a.pos_off, (const IdT*)a.pos_sorted, u);
  int64_t id = 0;
  for (int t = 0; t < a.max_tries; ++t) {
    const Philox4 d = philox4x32_10(j, (uint32_t)t, 6u, a.epoch, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    id = candidate_of<IdT>(d, a.cand, a.thresh, a.alias, a.n_cand, err);
    if (!pos.has((IdT)id)) break;          // the last attempt stands
  }
  ou[b] = user; oi[b] = (IdT)id; oy[b] = 0.f;
}

}  // namespace br

using namespace br;

extern "C" int brNeumfSampleBatch(const void* pos_users, const void* pos_items, int id_type, int64_t n, int neg_per_pos, const int64_t* pos_off,
                                  const void* pos_sorted_items, int64_t num_users, const void* cand_items, int64_t n_cand,
                                  const uint32_t* alias_thresh, const int32_t* alias_slot, uint64_t seed, uint32_t epoch, int64_t row0, int64_t batch,
                                  int max_tries, void* out_users, void* out_items, float* out_labels, int* err_flag, brStream stream) {
  BR_CHECK_ARG(id_type == BR_IDS_I32 || id_type == BR_IDS_I64, "brNeumfSampleBatch: bad id_type");
  BR_CHECK_ARG(neg_per_pos >= 0, "brNeumfSampleBatch: neg_per_pos %d < 0", neg_per_pos);
  BR_CHECK_ARG(max_tries >= 1 && max_tries <= 256, "brNeumfSampleBatch: max_tries %d out of [1, 256]", max_tries);
  BR_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 32) && n * ((int64_t)1 + neg_per_pos) < ((int64_t)1 << 32),
               "brNeumfSampleBatch: an epoch of n (1 + neg_per_pos) rows must have fewer than 2^32");
  const int64_t N = n * ((int64_t)1 + neg_per_pos);
  BR_CHECK_ARG(row0 >= 0 && batch >= 0 && batch < ((int64_t)1 << 31) && row0 + batch <= N, "brNeumfSampleBatch: rows [row0, row0 + batch) outside the epoch");
  BR_CHECK_ARG(num_users >= 1 && n_cand >= 1 && n_cand < ((int64_t)1 << 32), "brNeumfSampleBatch: bad sizes");
  BR_CHECK_ARG((alias_thresh == nullptr) == (alias_slot == nullptr), "brNeumfSampleBatch: alias_thresh and alias_slot: both or neither");
  if (batch == 0) return BR_OK;
  BR_CHECK_ARG(pos_users && pos_items && pos_off && pos_sorted_items && out_users && out_items && out_labels, "brNeumfSampleBatch: null pointer");
  // the epoch's own seed (stream 7) keys the order of its rows; the draws (stream 6) carry the epoch in their counter
  const Philox4 d = philox4x32_10(epoch, 0u, 7u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t seed_e = ((uint64_t)d.y << 32) | (uint64_t)d.x;
  const EpochArgs a{pos_users, pos_items, (uint32_t)n, (uint32_t)neg_per_pos, (uint32_t)N, pos_off, pos_sorted_items, num_users,
                    cand_items, alias_thresh, alias_slot, (uint32_t)n_cand, seed, epoch, perm_key(seed_e, 6u), (uint32_t)row0, max_tries};
  hipStream_t s = (hipStream_t)stream;
  BR_DISPATCH_ID(id_type, (neumf_sample_batch_kernel<IdT><<<(unsigned)ceil_div(batch, 256), 256, 0, s>>>(a, batch, (IdT*)out_users, (IdT*)out_items, out_labels, err_flag)));
  BR_CHECK_LAUNCH("brNeumfSampleBatch");
  return BR_OK;
}
