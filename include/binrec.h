/*
 * binrec.h — C-ABI of libbinrec_hip.so: the MI355X (gfx950) hot path of the
 * NeuMF / BPR / TwoTower trainers of leotimus/binary-recommendation.
 *
 * The reference has NO plugin / FFI / operator interface for this path: every op is a stock
 * Keras layer declared in Python.  Each entry point below therefore cites the
 * reference *call site* (path:line under /root/reference) whose arithmetic it replaces; the
 * Python host in binary-recommendation_amd/ re-exposes the reference's model surface
 * (compileModel / fit / train_step / predict ...) on top of these.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.  Every function returns int:
 *    BR_OK (0) or a negative BR_ERR_*; brGetLastError() gives the thread-local message.
 *  - Caller owns ALL memory (device buffers, e.g. torch tensors' data_ptr()); scratch needs are queried
 *    (br*WorkspaceBytes) and passed in.  The library allocates no device memory and does not synchronise on a step's
 *    path.  What it does keep, per process: the thread-local error string; four fork / join events for brNeumfStep.aux_stream
 *    (created on first use: ONE stepping thread per process, as everywhere in this build); the optional measurement probes
 *    (brProbe*, brProbeGraph*: HIP events created by brProbeEnable / brProbeGraphSelect, never in a launch path); and, during a
 *    brNeumfStepRun call, a pointer to that call's step state.  Two entry points synchronise their stream because they copy from
 *    pageable host memory: brStepStateSet and brStepStateInit (set-up / reload, never inside a step).
 *  - Every launch goes to the caller's stream (`brStream` = hipStream_t).
 *  - Tables are row-major fp32 [rows][dim].  ids are int32 or int64 (BR_IDS_*); ids == NULL
 *    means identity (row b of an already-gathered [batch][dim] buffer: the row-sharded
 *    multi-GPU path hands rows over that way).
 *  - Out-of-range ids never fault: the access is skipped (zeros are produced) and *err_flag
 *    (device int, may be NULL) is set to 1.  TF-CPU raises InvalidArgument there [TF-sem];
 *    the Python host turns the flag into an IndexError.
 *  - Dropout masks are a pure function (Philox4x32-10) of (seed, step, site, global row, col):
 *    see csrc/philox.h; restated bit-exactly in oracle/binrec_oracle.py.
 */
#ifndef BINREC_H
#define BINREC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* brStream; /* hipStream_t */

enum { BR_OK = 0, BR_ERR_ARG = -1, BR_ERR_HIP = -2, BR_ERR_UNSUPPORTED = -3, BR_ERR_WORKSPACE = -4 };
enum { BR_IDS_I32 = 0, BR_IDS_I64 = 1 };
enum { BR_ACT_LINEAR = 0, BR_ACT_SIGMOID = 1, BR_ACT_RELU = 2 };
enum { BR_LOSS_BCE = 0, BR_LOSS_MSE = 1 };
enum { BR_MAX_TABLES = 8, BR_SUM_SLOTS = 64, BR_STAT_REPLICAS = 8, BR_METRIC_SUMS = 8 };

const char* brGetLastError(void);
int brVersion(void);
/* cu_count / arch string of the current device (host-side query, no launch). */
int brDeviceInfo(int* cu_count, int* wave_size, char* arch, int arch_len);

/* ---- G1/G2: Embedding(...)(input) + Flatten ------------------------------------------------
 * NFC_plain.py:115-126, NeuMFModel.py:58-63, BPRModel.py:55-61, twoTower.py:34,36.
 * outs[t][b,:] = tables[t][ids[t][b],:] for t < n_tables, fused in one launch. Bit-exact. */
int brGatherRows(int n_tables, const float* const* tables, const int64_t* table_rows,
                 const void* const* ids, float* const* outs, int dim, int64_t batch,
                 int id_type, int* err_flag, brStream stream);

/* ---- M1: Dot(axes=1) — NFC_plain.py:148, NeuMFModel.py:79, twoTower.py:44,86 ----------------
 * out[b] = sum_d a[b,d]*b[b,d];  backward: da = dout*b, db = dout*a. */
int brRowDot(const float* a, const float* b, float* out, int dim, int64_t batch, brStream stream);
int brRowDotBackward(const float* a, const float* b, const float* dout, float* da, float* db,
                     int dim, int64_t batch, brStream stream);

/* ---- G1+M1+T1 fused for NeuMF: 4 lookups, GMF dot, MLP concat ------------------------------
 * NFC_plain.py:115-126,137,148 (item_first=1) / NeuMFModel.py:58-66,79 (item_first=0).
 * x0[b] = concat(first_mlp[b], second_mlp[b]) (B x 2*dim), dot[b] = user_mf[u]·item_mf[i].
 * ld_user / ld_item = row strides (floats) of the user / item tables: `dim` for four separate
 * tables, 2*dim when a stream's MLP and MF tables are stored interleaved as one [rows][mlp|mf]
 * allocation (then user_mf = user_mlp + dim): one 512-B row instead of two 256-B rows per id. */
int brNeumfEmbedForward(const float* user_mlp, const float* item_mlp, const float* user_mf,
                        const float* item_mf, int64_t ld_user, int64_t ld_item, int64_t user_rows,
                        int64_t item_rows, const void* users, const void* items, int id_type,
                        int dim, int64_t batch, int item_first, float* x0, float* dot,
                        int* err_flag, brStream stream);
/* The same, also leaving the two MF rows of every pair behind (stash_user[b] = user_mf[u_b], stash_item[b] = item_mf[i_b], stride ld_stash):
 * the backward of the GMF dot is then ddot[b] * the partner's stash, formed where it is consumed (brSegmentSumToSlotsPair,
 * brAdamRowsSortedPair hi_scale) instead of by a launch that writes it out per pair. */
int brNeumfEmbedForwardStash(const float* user_mlp, const float* item_mlp, const float* user_mf,
                             const float* item_mf, int64_t ld_user, int64_t ld_item, int64_t user_rows,
                             int64_t item_rows, const void* users, const void* items, int id_type, int dim,
                             int64_t batch, int item_first, float* x0, float* dot, float* stash_user, float* stash_item, int64_t ld_stash,
                             int* err_flag, brStream stream);
/* B1 for the same block: per-pair row gradients (IndexedSlices values, [TF-sem]).
 * dx0: (B x 2*dim) gradient w.r.t. the concat; ddot: (B).
 * g_user_mf[b] = ddot[b]*item_mf[i_b], g_item_mf[b] = ddot[b]*user_mf[u_b];
 * g_*_mlp (optional, both or neither) = the two halves of dx0 in concat order.
 * All outputs have row stride ldg (dim, or 2*dim for fused [mlp|mf] gradient buffers). */
int brNeumfEmbedBackward(const float* user_mf, const float* item_mf, int64_t ld_user,
                         int64_t ld_item, int64_t user_rows, int64_t item_rows, const void* users,
                         const void* items, int id_type, int dim, int64_t batch, int item_first,
                         const float* dx0, const float* ddot, float* g_user_mlp, float* g_item_mlp,
                         float* g_user_mf, float* g_item_mf, int64_t ldg, int out_rows_by_id,
                         brStream stream);   /* out_rows_by_id: pair b's gradients go to rows users[b] / items[b] of the outputs
                                                (row-sharded host: ids = slots of the padded exchange buffers) instead of row b */

/* ---- L3: BPR triplet step — BPRModel.py:49-74,124-144; bpr.py:141-157 -----------------------
 * x = u·p - u·n ; l = 1 - sigmoid(x) ; loss = mean(l).  One fused launch: 3 gathers, 2 dots,
 * loss partials, 3 row gradients.  g_item is (2B x dim): rows [0,B) = d/d pos, [B,2B) = d/d neg
 * (the shared item table's two IndexedSlices concatenated).  loss_sum: device
 * double[BR_SUM_SLOTS], slot (workgroup & 63) += sum l (same-address atomics serialise at
 * ~12 ns each on MI355X; the caller adds the slots).  per_triplet (B) may be NULL.
 * inv_batch = 1/global batch. */
int brBprForwardBackward(const float* user_table, const float* item_table, int64_t user_rows,
                         int64_t item_rows, const void* users, const void* pos, const void* neg,
                         int id_type, int dim, int64_t batch, float inv_batch, float* per_triplet,
                         double* loss_sum, float* g_user, float* g_item, int* err_flag,
                         brStream stream);

/* ---- S1: duplicate-id handling ([TF-sem] _deduplicate_indexed_slices) ----------------------
 * brRowIndexBuild: stable radix sort of (id, batch position) -> sorted_ids, sorted_pos (int32).
 * Equal ids stay in ascending batch position, so every later segment sum runs in exactly the
 * order of a sequential unsorted_segment_sum: bitwise reproducible, no float atomics. */
int64_t brRowIndexWorkspaceBytes(int64_t n, int id_type);
int brRowIndexBuild(const void* ids, int id_type, int64_t n, int64_t id_upper_bound,
                    void* sorted_ids, int32_t* sorted_pos, void* workspace,
                    int64_t workspace_bytes, brStream stream);
/* Both id streams of a step (same n) in shared launches: for n <= 524 288 (64 chunks of 8192) and id bounds < 2^31 the index is
 * built in TWO launches for the pair (chunk sort in LDS + rank-by-binary-search scatter) instead of one device
 * radix sort (~10 launches) per stream.  Same outputs as two brRowIndexBuild calls. */
int brRowIndexBuildPair(const void* ids_a, int64_t upper_a, void* sorted_ids_a, int32_t* sorted_pos_a, void* ws_a, int64_t ws_a_bytes,
                        const void* ids_b, int64_t upper_b, void* sorted_ids_b, int32_t* sorted_pos_b, void* ws_b, int64_t ws_b_bytes,
                        int id_type, int64_t n, brStream stream);
/* Row-sharded exchange planning for one or two equally long id streams (ids_b NULL: one): owner(id) = id mod world.
 * order[j] = batch position of bucket slot j (buckets = positions stably sorted by owner), inv[b] = bucket slot of position b,
 * send_local[j] = id div world in bucket order, counts[d] = rows for owner d (int64[world]).  dest / sorted_dest: scratch of n
 * ids each; ws: brRowIndexWorkspaceBytes(n) bytes each. */
int brShardPlanPair(const void* ids_a, const void* ids_b, int id_type, int64_t n, int world, void* dest_a, void* dest_b,
                    void* sorted_dest_a, void* sorted_dest_b, int32_t* order_a, int32_t* order_b, void* ws_a, void* ws_b,
                    int64_t ws_bytes, int32_t* inv_a, int32_t* inv_b, void* send_local_a, void* send_local_b,
                    int64_t* counts_a, int64_t* counts_b, brStream stream);
/* Fixed-capacity form of that plan: every owner gets exactly `cap` slots per stream (slot d*cap + k = the k-th row for owner d in
 * bucket order), so the three all-to-alls of a step have equal, static splits and no row count crosses to the host.
 * send_pad[world*cap]: local row ids, pad slots hold the owner's SPARE row (local index = the owner's row count; a padded engine
 * allocates one row more per table, its gradient is always 0); slot[n]: batch position -> slot; bpos[world*cap]: slot -> batch
 * position or -1.  More than `cap` rows for one owner sets bit BR_ERRFLAG_CAPACITY in *err_flag (the surplus rows collide in the
 * owner's last slot: the step's result is then wrong and the host must raise). */
enum { BR_ERRFLAG_RANGE = 1, BR_ERRFLAG_CAPACITY = 2 };
int brShardPadPair(const void* sorted_dest_a, const void* sorted_dest_b, const int32_t* order_a, const int32_t* order_b,
                   const void* send_local_a, const void* send_local_b, const int64_t* counts_a, const int64_t* counts_b, int id_type,
                   int64_t n, int world, int64_t cap, int64_t total_rows_a, int64_t total_rows_b, void* send_pad_a, void* send_pad_b,
                   int32_t* slot_a, int32_t* slot_b, int32_t* bpos_a, int32_t* bpos_b, float* zero_a, float* zero_b, int zero_dim,
                   int* err_flag, brStream stream);   /* zero_*: optional [world*cap][zero_dim] buffers whose pad rows are cleared
                                                         (the gradient send slots, written in place by brNeumfEmbedBackward out_rows_by_id) */
/* ---- The same exchange with duplicate ids MERGED and both id streams in ONE all-to-all buffer per phase (parallel.py PaddedExchange) ----
 * Replaces the reference's mirrored variables + all-reduced IndexedSlices (src/models/RModel.py:119, NeuMFModel.py:92-98) for one
 * NeuMF step: owner(id) = id mod world serves each DISTINCT id of the batch once.
 * Requester side, brShardDedupPlanPair: key = owner * R + id div world (R = rows per owner, rounded up, + 1), (key, position) sorted;
 * the k-th distinct key of owner d gets physical slot (d * 2 + stream) * cap + k of the merged buffers [owner][user | item][cap]
 * (ids out: send_ids; rows back and gradients out: the same slot numbering, `dim` floats per slot); slot[b] = the slot of batch
 * position b's id or -1; sorted_keys / sorted_pos stay behind as the dedup index of the backward (brSegmentSumToSlotsPair).  Pad slots
 * name the owner's spare row (index = its row count) and their rows of grad_slots (optional, zero_dim floats each) are cleared.
 * More than cap DISTINCT ids for one owner and stream: the surplus ids get slot -1 (the step reads zeros for them and sends no
 * gradient - no slot is ever written twice, no table row sees another row's gradient) and BR_ERRFLAG_CAPACITY is set; ids outside
 * [0, total_rows): slot -1, BR_ERRFLAG_RANGE.  Scratch: keys / urank [n] each, first [world + 1] int32 each, ws brRowIndexWorkspaceBytes(n). */
int brShardDedupPlanPair(const void* ids_a, const void* ids_b, int id_type, int64_t n, int world, int64_t cap, int64_t total_rows_a,
                         int64_t total_rows_b, void* keys_a, void* keys_b, void* sorted_keys_a, void* sorted_keys_b, int32_t* sorted_pos_a,
                         int32_t* sorted_pos_b, void* ws_a, void* ws_b, int64_t ws_bytes, int32_t* urank_a, int32_t* urank_b, int32_t* first_a,
                         int32_t* first_b, void* send_ids, int32_t* slot_a, int32_t* slot_b, float* grad_slots, int zero_dim, int* err_flag,
                         brStream stream);
/* Backward of that plan: out_slots[slot[p]] = ordered (two-level, see below) sum over the positions p' of p's id of the per-pair row
 * gradient [g0[p'] (split floats, stride ldg0) | hi_scale[p'] * g1[p'] (dim - split floats, stride ldg1)] - for a NeuMF step g0 = the
 * MLP half of dx0, g1 = the PARTNER stream's stashed MF rows, hi_scale = ddot (brNeumfEmbedBackward's products without writing them
 * out per pair).  g1_* NULL: one source (split = dim).  seg_ws_*: brSegmentScratchFloats(n, dim) each, or both NULL. */
int brSegmentSumToSlotsPair(const void* sorted_ids_a, const int32_t* sorted_pos_a, const int32_t* slot_a, const float* g0_a, const float* g1_a,
                            const void* sorted_ids_b, const int32_t* sorted_pos_b, const int32_t* slot_b, const float* g0_b, const float* g1_b,
                            int64_t ldg0, int64_t ldg1, const float* hi_scale, int id_type, int64_t n, int dim, int split, float* out_slots,
                            float* seg_ws_a, float* seg_ws_b, brStream stream);
/* Owner side: the ids arrive as ONE array [source rank][stream][cap]; stream k's logical position t = src * cap + j sits at element
 * (src * 2 + k) * cap + j (seg_len = cap, seg_stride = 2 * cap, seg_off = k * cap).  brRowIndexBuildPairSeg = brRowIndexBuildPair over
 * such arrays, sorted_pos = the PHYSICAL element index (so the optimizer kernels read received gradient rows / served rows of the same
 * layout unchanged); brGatherRows[Deferred]PairSeg: out[p] = row ids[p] of the stream's table at every physical position p of both
 * streams, one launch. */
int brRowIndexBuildPairSeg(const void* ids_a, int64_t upper_a, void* sorted_ids_a, int32_t* sorted_pos_a, void* ws_a, int64_t ws_a_bytes,
                           const void* ids_b, int64_t upper_b, void* sorted_ids_b, int32_t* sorted_pos_b, void* ws_b, int64_t ws_b_bytes,
                           int id_type, int64_t n, int64_t seg_len, int64_t seg_stride, int64_t seg_off_a, int64_t seg_off_b, brStream stream);
/* The same index when every segment is ALREADY sorted ascending - what the fixed-capacity exchange delivers: each requester sends an owner
 * its distinct local rows in key order with the pads (the spare row = the largest id) behind them, so the W segments of a stream are W
 * sorted runs and the index is their merge (one binary search per other run and key, no sort, no workspace).  Output identical to
 * brRowIndexBuildPairSeg.  A segment that is not sorted sets BR_ERRFLAG_RANGE in *err_flag (may be NULL); the index is then wrong.
 * Replaces on the owners of parallel.py what RModel.py:119's MultiWorkerMirroredStrategy does with an all-reduce of IndexedSlices. */
int brRowIndexMergePairSeg(const void* ids_a, int64_t upper_a, void* sorted_ids_a, int32_t* sorted_pos_a, const void* ids_b, int64_t upper_b,
                           void* sorted_ids_b, int32_t* sorted_pos_b, int id_type, int64_t n, int64_t seg_len, int64_t seg_stride, int64_t seg_off_a,
                           int64_t seg_off_b, int* err_flag, brStream stream);
int brGatherRowsDeferredPairSeg(const float* table_a, const float* m_a, const float* v_a, const int32_t* last_a, int64_t rows_a, const float* table_b,
                                const float* m_b, const float* v_b, const int32_t* last_b, int64_t rows_b, const void* ids, float* out, int dim,
                                int id_type, int64_t n, int64_t seg_len, int64_t seg_stride, int64_t seg_off_a, int64_t seg_off_b,
                                const void* step_state, double beta1, double beta2, double eps, int64_t ld_out, int* err_flag, brStream stream);
int brGatherRowsPairSeg(const float* table_a, int64_t rows_a, const float* table_b, int64_t rows_b, const void* ids, float* out, int dim, int id_type,
                        int64_t n, int64_t seg_len, int64_t seg_stride, int64_t seg_off_a, int64_t seg_off_b, int64_t ld_out, int* err_flag,
                        brStream stream);
/* dst[t] = bpos[t] >= 0 ? src[bpos[t]] : 0 (n_slots rows of dim floats; src rows at stride ld): per-pair rows -> padded send slots,
 * for one or two sets of equal shape (set b NULL: one). */
int brRowsToSlotsPair(const float* src_a, const float* src_b, int64_t ld, const int32_t* bpos_a, const int32_t* bpos_b, float* dst_a,
                      float* dst_b, int64_t n_slots, int dim, brStream stream);
/* The ordered duplicate sum and its scratch.  Every kernel that sums a segment (brSegmentSumRows, brAdamRowsSorted*,
 * brAdagradRowsSorted) takes an optional `seg_ws` of brSegmentScratchFloats(n, dim) floats (16-byte aligned):
 *   seg_ws == NULL: the segment head adds its duplicates one by one in ascending batch position = a sequential fp32
 *     unsorted_segment_sum ([TF-sem] _deduplicate_indexed_slices).  The chain is as long as the segment: fine for
 *     near-uniform ids, 2.3 ms for ONE launch on a Zipf(1.05) batch of 65 536 (one id holds thousands of positions).
 *   seg_ws != NULL: two levels, still a fixed order: every 64-aligned block of the SORTED order that continues its
 *     predecessor's id gets the one-by-one sum of its own run (one extra small launch, all blocks in parallel); the head
 *     adds its own positions up to the next block boundary one by one, then one partial per later block:
 *     ((((g_i + g_i+1) + ..) + P_b) + P_b+1) + .., P_b = ((g_64b + g_64b+1) + ..).  Segments that do not cross a
 *     64-aligned boundary are summed exactly as with NULL.  oracle/binrec_oracle.py::ordered_segment_sum restates it. */
int64_t brSegmentScratchFloats(int64_t n, int dim);
/* Materialised dedup: for each segment head h (sorted position), out_rows[h] = ordered sum of
 * row_grads[sorted_pos[j]] over the segment, head_flag[h]=1; non-head rows untouched, flag 0. */
int brSegmentSumRows(const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                     const float* row_grads, int64_t ldg, int dim, float* out_rows,
                     int32_t* head_flag, float* seg_ws, brStream stream);
/* Fast form (order-nondeterministic float atomics): g_table[ids[b],:] += rows[b,:]. */
int brScatterAddRows(float* g_table, int64_t table_rows, const void* ids, int id_type,
                     int64_t n, const float* rows, int dim, int* err_flag, brStream stream);

/* ---- O1: Keras/TF-form Adam — NFC_plain.py:153, NeuMFModel.py:89, BPRModel.py:70 ------------
 * alpha_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed by the caller in double; the launcher rounds
 * alpha_t, b1, 1-b1, b2, 1-b2, eps to fp32 once.  row_grads rows have stride ldg floats (so the
 * two halves of a (B x 2*dim) dx0 buffer serve as the MLP tables' row gradients in place).
 * m = b1*m+(1-b1)*g ; v = b2*v+(1-b2)*g^2 ; theta -= alpha_t*m/(sqrt(v)+eps)   (eps outside).
 * brAdamRowsSorted: touched rows only; g = ordered segment sum (dedup BEFORE the square).
 *   row_grads_hi non-NULL: columns [split, dim) of a row's gradient come from row_grads_hi
 *   (stride ldg_hi), columns [0, split) from row_grads: a fused [mlp|mf] table takes its MLP half
 *   straight from the (B x 2*dim) input gradient and its MF half from the embed backward.
 *   mark (uint8[table_rows]) non-NULL: set mark[row]=1 for touched rows (for the sweep).
 * brAdamDenseSweep: every row NOT marked gets the g=0 update (m,v decay + theta step): with
 *   brAdamRowsSorted before it this is exactly Keras' non-lazy sparse Adam; it clears marks. */
int brAdamRowsSorted(float* table, float* m, float* v, int64_t table_rows, int dim,
                     const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                     const float* row_grads, int64_t ldg, const float* row_grads_hi,
                     int64_t ldg_hi, int split, double alpha_t, double beta1, double beta2,
                     double eps, uint8_t* mark, float* seg_ws, brStream stream);
int brAdamDenseSweep(float* table, float* m, float* v, int64_t table_rows, int dim,
                     double alpha_t, double beta1, double beta2, double eps, uint8_t* mark,
                     brStream stream);
/* Flat dense parameters (MLP weights, biases, BN gamma/beta): plain TF-form Adam. */
int brAdamFlat(float* theta, float* m, float* v, const float* g, int64_t n, double alpha_t,
               double beta1, double beta2, double eps, brStream stream);

/* ---- O2: Keras Adagrad — twoTower.py:209,278-279 ([TF-sem] acc0 = 0.1, eps 1e-7) -------------
 * acc += g^2 ; theta -= lr*g/(sqrt(acc)+eps); sparse apply touches only deduplicated rows. */
int brAdagradRowsSorted(float* table, float* acc, int64_t table_rows, int dim,
                        const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                        const float* row_grads, int64_t ldg, double lr, double eps,
                        float* seg_ws, brStream stream);
int brAdagradFlat(float* theta, float* acc, const float* g, int64_t n, double lr, double eps,
                  brStream stream);

/* ---- T4: Dropout keep-bit planes — NFC_plain.py:138,141,144; NeuMFModel.py:67,71,75 ----------
 * The masks are a pure function (Philox4x32-10, csrc/philox.h) of (seed, step, site, global row, col).  They are
 * materialised once per (step, site) as bit planes and read by the forward and the backward of the layer behind the
 * site: keep[r][w] (uint32, row stride ceil(K/32) words), bit b of word w = element (row0 + r, 32w + b) is KEPT.
 * brDropoutKeepWords(batch, K) = words of one plane.  Up to three sites (widths[i] columns, dropout site id sites[i],
 * plane out[i]) in one launch.  Inside brNeumfStepRun `step` comes from the device step state when there is one. */
int64_t brDropoutKeepWords(int64_t batch, int K);
int brDropoutKeepBits(float drop_p, uint64_t seed, uint32_t step, int64_t row0, int64_t batch, int n_sites,
                      const uint32_t* sites, const int* widths, uint32_t* const* out, brStream stream);

/* BatchNorm finalize folded into the consumer of the normalised activations (brDenseForward / brNeumfTailFused): the
 * consumer's workgroups each turn the producer's column sums into scale / shift in their prologue (a few hundred flops),
 * workgroup 0 also writes scale / shift / mean / rstd (N each, kept for the backward) and updates the moving statistics -
 * the same arithmetic as brBnFinalize without its launch. */
typedef struct brBnFold {
  const double* stats;        /* [BR_STAT_REPLICAS][2N] column sums of y, y^2 */
  double batch_total;         /* rows behind the sums */
  const float* gamma; const float* beta;
  float eps; float momentum;
  float* moving_mean; float* moving_var;            /* may be NULL (both) */
  float* scale; float* shift; float* mean; float* rstd;   /* outputs */
} brBnFold;

/* ---- T1-T4: MLP tower layer, fp32 MFMA (v_mfma_f32_16x16x4_f32) ----------------------------
 * Dense/BatchNormalization/Dropout: NFC_plain.py:138-147, NeuMFModel.py:67-78, twoTower.py:40-41.
 * y = act( T(x)·W + bias ),  T(x)[r,k] = (x[r,k]*in_scale[k] + in_shift[k]) * keep(r,k)/(1-p)
 *   in_scale/in_shift (K) NULL => identity (they carry the previous layer's BatchNorm); in_bn != NULL (then in_scale and
 *   in_shift must be NULL): the BatchNorm is finalized from its column sums in this launch (brBnFold);
 *   drop_p == 0 (keep NULL) => no dropout; else keep = the site's bit plane (brDropoutKeepBits).
 * stats (double[BR_STAT_REPLICAS][2N], may be NULL): += column sums of y and y^2 (BatchNorm batch
 *   statistics), spread over 8 replicas (workgroup % 8) so same-address atomics do not serialise;
 *   consumers (brBnFinalize, brDenseBackward, brBnParamGrads) add the replicas.  The same layout
 *   holds for every BN-sum buffer below (bn_sums, in_bn_sums).
 * x: (B x K) row stride ldx; W: (K x N) row-major; y: (B x N) row stride ldy. */
int brDenseForward(const float* x, int64_t ldx, const float* W, const float* bias, float* y,
                   int64_t ldy, int64_t batch, int K, int N, int act, const float* in_scale,
                   const float* in_shift, const brBnFold* in_bn, float drop_p, const uint32_t* keep,
                   double* stats, brStream stream);
/* BatchNorm bookkeeping from the column sums (tiny): mean, biased var, scale = gamma*rstd,
 * shift = beta - mean*scale, moving stats <- momentum*moving + (1-momentum)*batch [TF-sem].
 * bstats (mean[N], rstd[N]) kept for the backward. */
int brBnFinalize(const double* stats, double batch_total, const float* gamma, const float* beta,
                 float eps, float momentum, float* moving_mean, float* moving_var, float* scale,
                 float* shift, float* mean, float* rstd, int N, brStream stream);
/* Inference-mode affine from the moving statistics. */
int brBnInference(const float* gamma, const float* beta, const float* moving_mean,
                  const float* moving_var, float eps, float* scale, float* shift, int N,
                  brStream stream);
/* Backward of one tower layer.
 *  gy: (B x N) gradient w.r.t. this layer's BatchNorm output h = BN(y) (dropout already
 *      transposed by the consumer's backward), or w.r.t. y itself when no BN follows (out_* NULL).
 *  out BN (after this layer): out_mean/out_rstd/out_gamma (N) and bn_sums (double[2N]:
 *      sum_r gy, sum_r gy*xhat — accumulated by the consumer's backward, see in_bn_sums).
 *      da = gamma*rstd*(gy - mean(gy) - xhat*mean(gy*xhat)); dz = da*act'(y).
 *  in transform (before this layer) as in brDenseForward, plus in_mean/in_rstd (K) when the
 *      input carries a BN: then in_bn_sums (double[2K]) += (sum gx, sum gx*xhat_in).
 *  Outputs: gx (B x K) = (dz·W^T) * keep(r,k)/(1-p): gradient w.r.t. the producer's BN output
 *      (w.r.t. x itself when the input has no BN) — may be NULL for the first layer of a tower
 *      whose input needs no gradient;  dW_slabs: (n_slabs x (K*N + N)) per-workgroup partials
 *      of [dW | db], reduced by brReduceSlabs in a fixed order (bitwise reproducible; no float
 *      atomics).  n_slabs = brDenseBackwardSlabs(). */
int brDenseBackwardSlabs(int64_t batch, int K, int N);
/* One launch (dz, dx and dW together, dz never leaves the CU: csrc/dense_bwd.hip) when K % 4 == N % 4 == 0 and every row is
 * 16-B aligned; other shapes run a dx and a dW kernel with dz handed over through dz_ws: caller scratch of
 * brDenseBackwardWorkspaceFloats() floats (16-B aligned).  keep: the bit plane of the layer's input dropout (brDropoutKeepBits),
 * required exactly when in_drop_p > 0. */
int64_t brDenseBackwardWorkspaceFloats(int64_t batch, int K, int N);
int brDenseBackward(const float* gy, int64_t ldgy, const float* y, int64_t ldy, const float* x,
                    int64_t ldx, const float* W, int64_t batch, int K, int N, int act,
                    const float* out_mean, const float* out_rstd, const float* out_gamma,
                    const double* bn_sums, double batch_total, const float* in_scale,
                    const float* in_shift, const float* in_mean, const float* in_rstd,
                    float in_drop_p, const uint32_t* keep, float* gx, int64_t ldgx, float* dz_ws,
                    float* dW_slabs, int n_slabs, double* in_bn_sums, brStream stream);
/* dgamma = sum gy*xhat, dbeta = sum gy: the BN-backward column sums as fp32 parameter grads. */
int brBnParamGrads(const double* bn_sums, float* dgamma, float* dbeta, int N, brStream stream);
int brBnParamGradsPair(const double* sums_a, float* dgamma_a, float* dbeta_a, int Na, const double* sums_b, float* dgamma_b,
                       float* dbeta_b, int Nb, brStream stream);
int brReduceSlabs(const float* slabs, int n_slabs, int64_t slab_elems, float* out, brStream stream);

/* End of the dense backward in one launch (single-process path): fixed-order reduction of three slab regions into their
 * ranges of the flat gradient (region r: n_slabs[r] slabs of slab_elems[r] floats -> grad[grad_off[r] ...)), the two BatchNorm
 * blocks' dgamma/dbeta from their backward column sums (as brBnParamGrads), then Adam on theta/m/v (as brAdamFlat).
 * The regions and BatchNorm blocks must tile [0, n) exactly. */
/* theta == NULL (then m, v unused): gradients only */
int brDenseFinalize(const float* const* slabs, const int* n_slabs, const int64_t* slab_elems, const int64_t* grad_off,
                    const double* const* bn_sums, const int* bn_n, const int64_t* dgamma_off, const int64_t* dbeta_off,
                    float* theta, float* m, float* v, float* grad, int64_t n, double alpha_t, double beta1, double beta2,
                    double eps, brStream stream);

/* ---- fused tail of the training step: T(a2) -> Dense(n3) -> concat [dot | a3] -> Dense(1) -> sigmoid -> loss and the
 * backward of all of it, one launch (trainers/NFC_plain.py:143-155, src/models/NeuMFModel.py:75-93) ----
 * Same results as brDenseForward(layer 3) + brNeumfHead + brDenseBackward(layer 3) (fp32 sums in a different
 * order).  a2: (B x n2) raw output of layer 2; scale2/shift2/mean2/rstd2 from brBnFinalize, or all NULL with bn2 given
 * (BatchNorm 2 finalized inside this launch, brBnFold); keep: the bit plane of the dropout in front of layer 3
 * (brDropoutKeepBits; NULL with drop_p == 0).
 * Two forms.  n2 <= 64, n3 <= 16, lda2 % 4 == ldgh2 % 4 == 0 and 16-B aligned a2 / gh2 run on MFMA (csrc/tail_mfma.hip).  That form
 * loads a2 in 16-B pieces, so it reads the columns n2 .. lda2-1 of every row and multiplies them by a zero scale: they must hold
 * FINITE values (Inf or NaN there would turn z3 into NaN); it also stores zeros into the same columns of gh2.  Every other shape
 * runs on VALU through LDS tiles (csrc/tail.hip), for every n2 <= 128 and n3 <= 32 (BR_ERR_ARG beyond).  With N3P = n3 rounded up to
 * a multiple of 4, a workgroup's 128 rows are one tile where 4*(2*128*(n2|1) + n2*N3P + 2*128*(N3P+1) + 4*n2 + 2*N3P) bytes of dynamic
 * LDS stay within 150 KiB (n2 = 128 up to n3 = 8, n3 = 32 up to n2 = 101, n3 <= 16 up to n2 = 123); wider towers run the same rows as
 * two 64-row tiles.  A size the LDS could not hold is BR_ERR_UNSUPPORTED before any launch.
 * Outputs: a3 (B x n3, may be NULL), logit/prob/ddot (B), gh2 (B x n2) = gradient w.r.t. BN2's output,
 * bn_sums (double[BR_STAT_REPLICAS][2*n2]) += (sum gh2, sum gh2*xhat2), sums as brNeumfHead, and one slab per
 * workgroup [dW3 (n2*n3) | db3 (n3) | dW4 (n3+1, concat order) | db4]: n_slabs = brNeumfTailSlabs(batch),
 * brNeumfTailSlabElems(n2, n3) floats each, reduced by ONE brReduceSlabs into the adjacent W3|b3|W4|b4 grads. */
int brNeumfTailSlabs(int64_t batch);
int64_t brNeumfTailSlabElems(int n2, int n3);
int brNeumfTailFused(const float* a2, int64_t lda2, const float* W3, const float* b3, const float* w4, const float* b4,
                     const float* dot, const float* labels, const float* scale2, const float* shift2, const float* mean2,
                     const float* rstd2, const brBnFold* bn2, float drop_p, const uint32_t* keep,
                     int64_t batch, int n2, int n3, int act, int mf_first, int loss, float inv_batch, float* a3,
                     float* logit, float* prob, double* sums, float* ddot, float* gh2, int64_t ldgh2, double* bn_sums,
                     float* slabs, int n_slabs, brStream stream);

/* ---- head: concat [GMF dot | MLP out] -> Dense(1) -> sigmoid -> loss, and its backward --------
 * NFC_plain.py:149-155 (mf_first=1, BCE) / NeuMFModel.py:80-91 (mf_first=0, MSE).
 * a3: (B x N3); dot: (B); w4: (N3+1) in concat order; b4: (1).  Outputs: logit, prob (B);
 * sums (double[BR_SUM_SLOTS][BR_METRIC_SUMS], slot = workgroup & 63) += [loss, sum (p-y)^2, sum |p-y|, #correct@0.5,
 * sum BCE(logit, y), TP, FP, FN at threshold 0.5] - the sums behind the compiled metrics of trainers/NFC_plain.py:155
 * (BinaryCrossentropy, mse, mae, FalseNegatives, FalsePositives, TrueNegatives = n - TP - FP - FN, TruePositives,
 * BinaryAccuracy); the caller adds the slots; when labels && training:
 * da3 (B x N3), ddot (B), head_slabs (n_slabs x (N3+2)) partials of [dW4 | db4].
 * inv_batch = 1/global batch. */
int brHeadSlabs(int64_t batch);
int brNeumfHead(const float* a3, int64_t lda3, const float* dot, const float* labels,
                const float* w4, const float* b4, int64_t batch, int N3, int mf_first, int loss,
                float inv_batch, float* logit, float* prob, double* sums, float* da3,
                int64_t ldda3, float* ddot, float* head_slabs, int n_slabs, brStream stream);

/* ---- L1 stand-alone: sigmoid + BCE-from-logits (twoTower.py:85-87 rdZero path) ---------------
 * sums[0] += sum_b max(z,0) - z*y + log1p(exp(-|z|)); dz = (sigmoid(z)-y)*inv_batch. */
int brBceLogits(const float* z, const float* y, int64_t batch, float inv_batch, float* prob,
                float* dz, double* sums, brStream stream);

/* ---- L4: in-batch softmax (tfrs.tasks.Retrieval, twoTower.py:47,82-83) [TF-sem] --------------
 * S = Q C^T (Bq x Bc), accidental hits (cand_ids[j]==q_pos_ids[i], j != diag) masked, loss =
 * SUM_i [logsumexp_j S_ij - S_i,diag(i)].  Streaming (the Bq x Bc matrix is never stored).
 * Pass 1 (brInBatchSoftmaxLse): row_lse (Bq), loss_sum (double[BR_SUM_SLOTS], slot = workgroup & 63) +=.
 * Pass 2 (brInBatchSoftmaxGrad): dQ = (P - I) C, dC = (P - I)^T Q (each optional).
 * diag_offset: column of C holding query i's positive = i + diag_offset (data-parallel ranks
 * all-gather C; rank r's queries sit at offset r*Bq).
 * ws / ws_bytes: optional scratch (brInBatchSoftmaxWorkspaceBytes; 16-byte aligned).  A workgroup owns 128 rows, so at the
 * reference's batch sizes the row blocks alone do not fill 256 CUs: with a workspace the other axis is split over more
 * workgroups and the partial results (per-row max / sum / diagonal score, dQ / dC slabs) are combined by a second launch in a
 * fixed order (bit-reproducible).  ws = NULL: one workgroup per 128 rows, results written directly. */
int64_t brInBatchSoftmaxWorkspaceBytes(int64_t Bq, int64_t Bc, int dim);
int brInBatchSoftmaxLse(const float* Q, const float* C, const void* q_pos_ids,
                        const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                        int64_t diag_offset, float* row_lse, double* loss_sum, void* ws,
                        int64_t ws_bytes, brStream stream);
/* Pass 1 and the dQ half of pass 2 in ONE sweep (what a training step needs: twoTower.py:99-102): the dQ accumulator is kept relative
 * to the running row maximum (online softmax) and normalised at the end, so the score tiles are formed twice per step instead of
 * three times.  Same outputs as brInBatchSoftmaxLse + brInBatchSoftmaxGrad(dQ) to rounding. */
int brInBatchSoftmaxLseGradQ(const float* Q, const float* C, const void* q_pos_ids,
                             const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                             int64_t diag_offset, float* row_lse, double* loss_sum, float* dQ,
                             void* ws, int64_t ws_bytes, brStream stream);
int brInBatchSoftmaxGrad(const float* Q, const float* C, const void* q_pos_ids,
                         const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                         int64_t diag_offset, const float* row_lse, float* dQ, float* dC,
                         void* ws, int64_t ws_bytes, brStream stream);

/* ---- L4 with hard negatives (tfrs.tasks.Retrieval num_hard_negatives = M) [TF-sem] -------------
 * Per query i the softmax runs over its partner column p_i = i + diag_offset and the set H_i: the first min(M, #negatives)
 * of the columns j != p_i ordered by (masked score x_ij descending, j ascending) - a tie at the cut goes to the lower
 * column, as tf.nn.top_k does.  x_ij is the score of the plain entries, accidental-hit mask included.  1 <= M <= 64.
 * Scratch for every entry below (>= brInBatchSoftmaxWorkspaceBytes; the per-split key lists of the threshold sweep). */
int64_t brInBatchSoftmaxHardWorkspaceBytes(int64_t Bq, int64_t Bc, int dim, int M);
/* The key of the LAST member of H_i: thr_score[i] (float32) and thr_pos[i] (its column, int32).  A query with at most M
 * negatives gets (-inf, INT32_MAX): nothing is cut.  One sweep in the tile layout of brInBatchSoftmaxLse (queries own,
 * candidates stream) with the M best keys of every owned query in LDS; with a workspace the candidate axis is split and a
 * second launch takes the M-th key of the union of a query's lists in a fixed order (bit-reproducible, no atomics).
 * Bc < 2^31. */
int brInBatchSoftmaxHardThreshold(const float* Q, const float* C, const void* q_pos_ids,
                                  const void* cand_ids, int id_type, int64_t Bq, int64_t Bc,
                                  int dim, int64_t diag_offset, int M, float* thr_score,
                                  int32_t* thr_pos, void* ws, int64_t ws_bytes, brStream stream);
/* The three entries above over the kept columns only: column j of query i takes part iff j == p_i, or x_ij > thr_score[i],
 * or x_ij == thr_score[i] and j <= thr_pos[i] (thr_score / thr_pos per QUERY, of brInBatchSoftmaxHardThreshold on the same
 * Q, C, ids, Bq, Bc, dim and diag_offset; both required).  Every sweep of these entries and the threshold sweep forms
 * its scores with one arithmetic, chosen from (Bc, dim) alone, so that all of them agree on H_i bit for bit. */
int brInBatchSoftmaxLseHard(const float* Q, const float* C, const void* q_pos_ids,
                            const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                            int64_t diag_offset, float* row_lse, double* loss_sum,
                            const float* thr_score, const int32_t* thr_pos, void* ws,
                            int64_t ws_bytes, brStream stream);
/* brInBatchSoftmaxLseGradQ over the kept columns (above 64 features: brInBatchSoftmaxLseHard + brInBatchSoftmaxGradHard(dQ)). */
int brInBatchSoftmaxLseGradQHard(const float* Q, const float* C, const void* q_pos_ids,
                                 const void* cand_ids, int id_type, int64_t Bq, int64_t Bc,
                                 int dim, int64_t diag_offset, float* row_lse, double* loss_sum,
                                 float* dQ, const float* thr_score, const int32_t* thr_pos,
                                 void* ws, int64_t ws_bytes, brStream stream);
/* brInBatchSoftmaxGrad over the kept columns; the dC sweep streams the queries with their thresholds.  C must be the
 * candidates the thresholds were taken over, all of them: thr_pos counts their columns and the arithmetic follows their count. */
int brInBatchSoftmaxGradHard(const float* Q, const float* C, const void* q_pos_ids,
                             const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                             int64_t diag_offset, const float* row_lse, float* dQ, float* dC,
                             const float* thr_score, const int32_t* thr_pos, void* ws,
                             int64_t ws_bytes, brStream stream);
/* dC of a SLICE of those candidates (the data-parallel step: a rank owns B of the world * B gathered candidates, all Bq
 * gathered queries stream past them with their thresholds): C and cand_ids hold rows [c0, c0 + Bc) of the Bc_total
 * candidates of the threshold sweep, diag_offset is relative to the slice (query i's positive is row i + diag_offset of
 * C), thr_pos stays as the threshold sweep wrote it.  The arithmetic is chosen from (Bc_total, dim) - that of the sweep that
 * formed the keys - not from the slice's Bc, so every rank keeps exactly the columns the whole-batch call would keep. */
int brInBatchSoftmaxGradHardSlice(const float* Q, const float* C, const void* q_pos_ids,
                                  const void* cand_ids, int id_type, int64_t Bq, int64_t Bc,
                                  int dim, int64_t diag_offset, const float* row_lse, float* dC,
                                  const float* thr_score, const int32_t* thr_pos, int64_t c0,
                                  int64_t Bc_total, void* ws, int64_t ws_bytes, brStream stream);

/* Log-Q correction: Retrieval's candidate_sampling_probability (tfrs.tasks.Retrieval; twoTower.py:47,82-83 builds the task
 * and does not pass the option) [TF-sem], after Yi et al. 2019.  The score of every entry below is
 * x_ij = Q_i . C_j - cand_logq[j], the partner's column included; then the accidental-hit mask, then the hard negatives
 * (selected on the corrected, masked scores).  cand_logq: Bc floats, one per row of the C that is passed (as cand_ids),
 * log of the clipped sampling probability; required, finite (device data is not checked).  Each entry is its Hard twin
 * plus cand_logq; thr_score / thr_pos both NULL selects the plain softmax over every column (one without the other is
 * refused).  One arithmetic per call, chosen from (Bc or Bc_total, dim) as the Hard entries choose it, with or without
 * thresholds; the subtraction is one fp32 rounding of the finished dot product, fl(s - b), the same in every sweep.  Scratch:
 * brInBatchSoftmaxHardWorkspaceBytes for M >= 1, brInBatchSoftmaxWorkspaceBytes otherwise. */
/* brInBatchSoftmaxHardThreshold on the corrected scores (thr_score / thr_pos are its outputs: required). */
int brInBatchSoftmaxHardThresholdLogQ(const float* Q, const float* C, const void* q_pos_ids,
                                      const void* cand_ids, int id_type, int64_t Bq, int64_t Bc,
                                      int dim, int64_t diag_offset, int M, float* thr_score,
                                      int32_t* thr_pos, const float* cand_logq, void* ws,
                                      int64_t ws_bytes, brStream stream);
/* brInBatchSoftmaxLse / brInBatchSoftmaxLseHard on the corrected scores; the loss term of a row is lse_i - x_i,p_i. */
int brInBatchSoftmaxLseLogQ(const float* Q, const float* C, const void* q_pos_ids,
                            const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                            int64_t diag_offset, float* row_lse, double* loss_sum,
                            const float* thr_score, const int32_t* thr_pos,
                            const float* cand_logq, void* ws, int64_t ws_bytes, brStream stream);
/* brInBatchSoftmaxLseGradQ / ...Hard on the corrected scores (above 64 features: ...LseLogQ + ...GradLogQ(dQ)). */
int brInBatchSoftmaxLseGradQLogQ(const float* Q, const float* C, const void* q_pos_ids,
                                 const void* cand_ids, int id_type, int64_t Bq, int64_t Bc,
                                 int dim, int64_t diag_offset, float* row_lse, double* loss_sum,
                                 float* dQ, const float* thr_score, const int32_t* thr_pos,
                                 const float* cand_logq, void* ws, int64_t ws_bytes,
                                 brStream stream);
/* brInBatchSoftmaxGrad / ...GradHard / ...GradHardSlice on the corrected scores: dQ and / or dC.  c0, Bc_total as in
 * brInBatchSoftmaxGradHardSlice (C, cand_ids and cand_logq hold rows [c0, c0 + Bc) of the Bc_total candidates; a proper
 * slice forms dC only); c0 = 0, Bc_total = Bc: the whole batch. */
int brInBatchSoftmaxGradLogQ(const float* Q, const float* C, const void* q_pos_ids,
                             const void* cand_ids, int id_type, int64_t Bq, int64_t Bc, int dim,
                             int64_t diag_offset, const float* row_lse, float* dQ, float* dC,
                             const float* thr_score, const int32_t* thr_pos,
                             const float* cand_logq, int64_t c0, int64_t Bc_total, void* ws,
                             int64_t ws_bytes, brStream stream);

/* scores[q][c] = Q[q]·C[c] (n_q x n_c, row stride ld_scores): candidate scoring for top-k
 * (TwoTower BruteForce, twoTower.py:64-69,229-230; bpr_predict, src/models/bpr.py:122-133). */
int brScoreMatrix(const float* Q, const float* C, int64_t n_q, int64_t n_c, int dim, float* scores,
                  int64_t ld_scores, brStream stream);

/* ---- E1: full-catalogue scoring + stable top-k — topKmetrics.py:17-72, twoTower.py:64-69 -----
 * scores (U x I) row-major -> top-k per user, descending, ties keep the LOWER item position
 * (strict '>' in __topk, topKmetrics.py:59,68).  out_scores/out_index: (U x k). */
int brTopKRows(const float* scores, int64_t n_users, int64_t n_items, int k, float* out_scores,
               int32_t* out_index, brStream stream);
/* brTopKRows with the seen items masked (src/models/bpr.py / twoTower.py candidate scoring, "unseen only"): excl_off (n_users + 1)
 * int64 / excl_idx int32 = per user the ascending COLUMN indices that must not be returned (the CSR of brFullAuc; both NULL: none).
 * Where fewer than k columns remain, the trailing slots are (-inf, -1).  k >= 1 (may exceed n_items). */
int brTopKRowsExclude(const float* scores, int64_t n_users, int64_t n_items, int k, const int64_t* excl_off,
                      const int32_t* excl_idx, float* out_scores, int32_t* out_index, brStream stream);

/* ---- Catalogue top-k for NeuMF: csrc/recommend.hip ------------------------------------------------------------------------------
 * Stands in for trainers/topKmetrics.py:17-43 (topKRatings / __topk: every (user, item) pair through model.predict, then a
 * python insertion sort per user) and src/models/NeuMFModel.py:133-150 (predictForUser: one user against the product list), with
 * the user's seen items optionally excluded.  Inference mode: BatchNorm on the moving statistics, no dropout.
 * The first layer is separable, z1 = Pu[user] + Pi[item] (b1 on the user side), and each BatchNorm folds into the next layer:
 * brNeumfCatalogFold: theta + moving -> the folded tower (brNeumfCatalogTowerFloats(n1, n2, n3) floats, layout private to the
 *   library): W2' = diag(g1 rstd1) W2, b2' = b2 + (be1 - g1 mm1 rstd1) W2, the same for layer 3, and the head weights in the
 *   order of mf_first (concat [dot, tower] when 1, [tower, dot] when 0).  rstd = 1 / sqrt(moving_var + bn_eps).
 * brNeumfCatalogProject: out[n] = table[ids[n], 0:dim] . W1[half] (+ b1 when b1 != NULL), then (copy_mf) the row's mf half
 *   table[ids[n], dim:2*dim] in columns n1 .. n1 + dim.  table = a fused [mlp | mf] table, row stride ld.  half = the user or the
 *   item rows of W1 (2*dim x n1) for the concat order item_first (A: [item, user], B: [user, item]).  col_major = 0: out[n][c]
 *   (row stride ld_out); 1: out[c][n] (column stride ld_out; the item side of brNeumfCatalogTopK).  ids outside [0, rows) set
 *   BR_ERRFLAG_RANGE in *err_flag and produce zeros.
 * brNeumfCatalogTopK: pu [n_users][ld_u] = projected users with their mf rows (row-major, copy_mf), pit [n1 + dim][ld_i] = projected
 *   items with their mf rows (col_major, copy_mf); per user the k best candidate positions by the head's sigmoid output (the value
 *   predict returns) -> out_scores / out_index (n_users x k, int32 positions into the item list), descending, ties keep the LOWER
 *   position (brTopKRows).  excl_off / excl_idx (optional, the CSR of brTopKRowsExclude): positions never returned; where fewer than k
 *   remain the trailing slots are (-inf, -1).  dump_logits / dump_probs (optional, n_users x n_items): every pair's head logit /
 *   probability (tests).  act = BR_ACT_*.  Limits: 2*dim <= 256, n1, n2 <= 128, n3 <= 32, 1 <= k <= 256, n_items < 2^31; anything
 *   else is BR_ERR_ARG before any launch.  ws: brNeumfCatalogTopKWorkspaceBytes(n_users, n_items, k) bytes (the per-split lists). */
int64_t brNeumfCatalogTowerFloats(int n1, int n2, int n3);
int brNeumfCatalogFold(const float* W2, const float* b2, const float* g1, const float* be1, const float* mm1, const float* mv1,
                       const float* W3, const float* b3, const float* g2, const float* be2, const float* mm2, const float* mv2,
                       const float* W4, const float* b4, int n1, int n2, int n3, int mf_first, float bn_eps, float* tower,
                       brStream stream);
int brNeumfCatalogProject(const float* table, int64_t ld, int64_t rows, const void* ids, int id_type, int64_t n, int dim,
                          const float* W1, int n1, int item_first, int user_side, const float* b1, int copy_mf, float* out,
                          int64_t ld_out, int col_major, int* err_flag, brStream stream);
int64_t brNeumfCatalogTopKWorkspaceBytes(int64_t n_users, int64_t n_items, int k);
int brNeumfCatalogTopK(const float* pu, int64_t ld_u, const float* pit, int64_t ld_i, int64_t n_users, int64_t n_items, int dim,
                       int n1, int n2, int n3, int act, const float* tower, const int64_t* excl_off, const int32_t* excl_idx, int k,
                       float* out_scores, int32_t* out_index, float* dump_logits, float* dump_probs, void* ws, int64_t ws_bytes,
                       brStream stream);

/* ---- Catalogue top-k for dot-product models (BPR, TwoTower): csrc/recommend_dot.hip ------------------------------------------------
 * Stands in for score_matrix + brTopKRows over the whole U x I matrix (bpr.py predict_scores, mean_average_precision_k, TwoTower
 * topk) without storing it.
 * brDotCatalogTopK: Q [n_users][ld_q] (row-major user rows), C [n_items][ld_c] (row-major item rows: a BPR table as it is); per user the
 *   k best item positions by score(u, i) = sum_j Q[u][j] C[i][j] in fp32 (features in natural order, one fmaf chain from 0: a pair's
 *   score depends on its two rows only) -> out_scores / out_index (n_users x k, int32 positions into C), descending, ties keep the
 *   LOWER position (brTopKRows).  excl_off / excl_idx (optional, the CSR of brTopKRowsExclude): positions never returned; where fewer
 *   than k remain the trailing slots are (-inf, -1).  dump_scores (optional, n_users x n_items): every pair's score (tests).
 *   Limits: 1 <= dim <= 128, 1 <= k <= 256, n_items < 2^31, ld_q, ld_c >= dim (16-B aligned item rows take the float4 path, any other
 *   stride a scalar one with the same scores); anything else is BR_ERR_ARG before any launch.
 *   ws: brDotCatalogTopKWorkspaceBytes(n_users, n_items, k) bytes (the per-split lists); -1 for sizes outside the limits. */
int64_t brDotCatalogTopKWorkspaceBytes(int64_t n_users, int64_t n_items, int k);
int brDotCatalogTopK(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                     const int64_t* excl_off, const int32_t* excl_idx, int k, float* out_scores, int32_t* out_index,
                     float* dump_scores, void* ws, int64_t ws_bytes, brStream stream);

/* ---- Catalogue AUC for dot-product models (BPR, TwoTower): csrc/auc_dot.hip ---------------------------------------------------------
 * Stands in for score_matrix + brFullAuc (full_auc, src/models/bpr.py:230-254) without storing the U x I score matrix.
 * brDotCatalogAuc: Q [n_users][ld_q], C [n_items][ld_c] and the scores of brDotCatalogTopK (features in natural order, one fmaf chain
 *   from 0); truth_off (n_users + 1) / truth_idx: per user the ascending, unique positions into C of its positives (ops.truth_csr,
 *   the CSR of brFullAuc).  out_auc[u] = W / (P N) with P = the user's truth entries, N = n_items - P and W = sum over positives p
 *   and the other items i of [s_i < s_p] + [s_i == s_p] / 2, summed exactly and divided once in double: bit for bit brFullAuc on
 *   the same scores (while P N < 2^53).  NaN for P == 0 or N == 0.  A NaN score gets no credit on either side.  dump_scores
 *   (optional, n_users x n_items): every pair's score (tests).
 *   Limits: those of brDotCatalogTopK (1 <= dim <= 128, 1 <= n_items < 2^31, ld_q, ld_c >= dim); BR_ERR_ARG / BR_ERR_WORKSPACE
 *   before any launch.  ws: brDotCatalogAucWorkspaceBytes(n_users, n_items, truth_off[n_users]) bytes (per-split partials and the
 *   sorted positive scores); -1 for sizes outside the limits.  The truth entries the workspace cannot hold (and any past 2^31 - 1)
 *   are never written: their users get NaN.  The user's positives are sorted by counting rank, O(P^2) compares per user. */
int64_t brDotCatalogAucWorkspaceBytes(int64_t n_users, int64_t n_items, int64_t n_truth);
int brDotCatalogAuc(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                    const int64_t* truth_off, const int32_t* truth_idx, float* out_auc, float* dump_scores, void* ws, int64_t ws_bytes,
                    brStream stream);

/* ---- Catalogue top-k and AUC for wide rows (BPR at the reference's latent_dim = 350): csrc/recommend_dot_wide.hip, auc_dot_wide.hip -----
 * brDotCatalogTopK / brDotCatalogAuc for 1 <= dim <= 512: the same stand-ins (bpr_predict, src/models/bpr.py:122-133, with
 * full_auc and mean_average_precision_k, bpr.py:230-289, over the whole U x I matrix, which is never stored), the same arguments and
 * the same contract: score(u, i) = sum_j Q[u][j] C[i][j] in fp32, features in natural order, one fmaf chain from 0 over the
 * instantiated width (zero padded), so a pair's score depends on its two rows only.
 * brDotCatalogTopKWide: bpr.py:122-133, :257-289.  dim <= 128 without BR_DOT_FORCE_WIDE: the launches of brDotCatalogTopK (same kernels,
 *   same plan, same bits).  dim > 128, or BR_DOT_FORCE_WIDE in flags: the block kernels - the item rows stream through LDS 128 features
 *   at a time and the accumulators are carried from block to block (no per-block partial sums), so the scores are those the whole-row
 *   kernel would give: at dim <= 128 both paths return the same bits.  Selection, exclusion, dump_scores and the (-inf, -1) tails as
 *   in brDotCatalogTopK.  Limits: 1 <= dim <= 512, otherwise those of brDotCatalogTopK; flags other than BR_DOT_FORCE_WIDE are
 *   BR_ERR_ARG.  ws: brDotCatalogTopKWideWorkspaceBytes(n_users, n_items, dim, k) bytes (enough for either path at that dim); -1 for
 *   sizes outside the limits.
 * brDotCatalogAucWide: bpr.py:122-133, :230-254.  The same switch for brDotCatalogAuc: the positives are scored over the same padded width
 *   and chain as the catalogue pass, the Mann-Whitney count is summed in integers and divided once in double, so out_auc equals
 *   brFullAuc on the same scores bit for bit.  ws: brDotCatalogAucWideWorkspaceBytes(n_users, n_items, dim, truth_off[n_users]) bytes.
 *   BR_ERR_ARG / BR_ERR_WORKSPACE before any launch, as the narrow entries. */
enum { BR_DOT_FORCE_WIDE = 1 };
int64_t brDotCatalogTopKWideWorkspaceBytes(int64_t n_users, int64_t n_items, int dim, int k);
int brDotCatalogTopKWide(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                         const int64_t* excl_off, const int32_t* excl_idx, int k, float* out_scores, int32_t* out_index,
                         float* dump_scores, int flags, void* ws, int64_t ws_bytes, brStream stream);
int64_t brDotCatalogAucWideWorkspaceBytes(int64_t n_users, int64_t n_items, int dim, int64_t n_truth);
int brDotCatalogAucWide(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                        const int64_t* truth_off, const int32_t* truth_idx, float* out_auc, float* dump_scores, int flags, void* ws,
                        int64_t ws_bytes, brStream stream);

/* ---- Catalogue ranks for dot-product models (BPR, TwoTower): NDCG@k, MRR, recall@k, hit@k over the whole catalogue: csrc/ranks_dot.hip ----
 * The reference evaluates with full_auc and mean_average_precision_k (src/models/bpr.py:230-289) and HR@k (trainers/topKmetrics.py:74-99);
 * these two entries add the ranking measures it lacks over the same scores (bpr_predict, bpr.py:122-133), without the U x I matrix.
 * brDotCatalogRanks: Q, C, dim, the score contract and BR_DOT_FORCE_WIDE of brDotCatalogAucWide (1 <= dim <= 512; whole-row kernel up to
 *   128 features unless forced, block kernel above): a pair's score is bit for bit the one brDotCatalogAuc[Wide] / brDotCatalogTopK[Wide]
 *   form and dump.  truth_off (n_users + 1) / truth_idx: the CSR of brDotCatalogAuc, n_truth = truth_off[n_users] entries; excl_off /
 *   excl_idx (optional, both or neither): per user the ascending, unique positions into C never offered as candidates (the exclusion CSR
 *   of brDotCatalogTopK).  Per truth entry e = (u, p), in truth-CSR order, over the candidates i != p that are not excluded for u:
 *     out_above[e] = #{i: score(u, i) > score(u, p)},  out_tied[e] = #{i: score(u, i) == score(u, p)}.
 *   The user's other positives are candidates like any other item.  Exclusion never removes a truth entry: a position in both CSRs is
 *   ranked against the non-excluded others (and is no candidate for them).  A positive whose score is NaN (or whose position lies
 *   outside [0, n_items)) gets (-1, -1); a candidate whose score is NaN is never above and never tied; +-inf compare as floats do.  All
 *   counting is in integers (integer atomics only): the result does not depend on the plan, the user order or the order of arrival.
 *   dump_scores (optional, n_users x n_items): every pair's score (tests).  Limits: those of brDotCatalogAucWide and
 *   n_truth + n_users < 2^31; BR_ERR_ARG / BR_ERR_WORKSPACE before any launch; n_users == 0 is BR_OK.
 *   ws: brDotCatalogRanksWorkspaceBytes(n_users, n_items, dim, n_truth) bytes (the positives' raw and sorted scores and two int32 bins per
 *   truth entry and user); -1 for sizes outside the limits.  The user's positives are sorted by counting rank, O(P^2) compares per user.
 * brRankMetrics: above / tied / truth_off of brDotCatalogRanks, ks: n_ks cutoffs on the HOST (1 <= n_ks <= 8, every k >= 1).  The rank of
 *   a positive is r = 1 + above + tied - pessimistic: a tied candidate is taken to outrank the positive, so a model that scores everything
 *   equal earns nothing.  A positive with above < 0 has no rank: a miss that still counts in P = the user's truth entries.  Per user, in
 *   double, stored float32, NaN for P == 0:
 *     out_mrr[u] = 1 / min r (0 if no positive has a rank);  for cutoff j, at [j * n_users + u]:
 *     out_ndcg = sum over r <= k of 1 / log2(1 + r)  /  sum over i = 1 .. min(P, k) of 1 / log2(1 + i);
 *     out_recall = #{r <= k} / P;  out_hit = [min r <= k]. */
int64_t brDotCatalogRanksWorkspaceBytes(int64_t n_users, int64_t n_items, int dim, int64_t n_truth);
int brDotCatalogRanks(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                      const int64_t* truth_off, const int32_t* truth_idx, int64_t n_truth, const int64_t* excl_off,
                      const int32_t* excl_idx, int32_t* out_above, int32_t* out_tied, float* dump_scores, int flags, void* ws,
                      int64_t ws_bytes, brStream stream);
int brRankMetrics(const int32_t* above, const int32_t* tied, const int64_t* truth_off, int64_t n_users, const int32_t* ks, int n_ks,
                  float* out_mrr, float* out_ndcg, float* out_recall, float* out_hit, brStream stream);

/* ---- Catalogue top-k on row-sharded engines, scored where the item rows live: csrc/recommend_merge.hip ----------------------------
 * W owners each run brNeumfCatalogTopK / brDotCatalogTopK over the candidates whose rows they hold (parallel.py recommend_at_owners);
 * these two turn the W shard-local answers into the answer of ONE launch over the whole candidate list, entry for entry.  The reference
 * has no counterpart: MultiWorkerMirroredStrategy (src/models/RModel.py:119) mirrors every table on every worker, so its predictForUser
 * (src/models/NeuMFModel.py:133-150) and topKRatings (trainers/topKmetrics.py:17-43) score the whole catalogue on each worker.
 * brCsrSplitByOwner: stands in for re-deriving every owner's seen-item lists on the host.  (off (n_rows + 1) int64, idx int32): the
 *   exclusion CSR of brTopKRowsExclude over the GLOBAL candidate list (ascending positions per row); g2l (n_global) int32: global
 *   position -> this owner's local position, or -1 where another owner holds the candidate.  -> (out_off (n_rows + 1), out_idx): the
 *   rows restricted to this owner's candidates, in local positions, in their input order (so ascending when g2l is ascending over the
 *   positions it keeps).  out_idx needs room for off[n_rows] entries (the kept ones are not known to the host).  Positions outside
 *   [0, n_global) are dropped.  Integer arithmetic in a fixed order (count per row, prefix sum over the rows, scatter): no float
 *   atomics, and the output does not depend on the launch shape.  ws: brCsrSplitByOwnerWorkspaceBytes(n_rows) bytes (the per-row counts).
 *   Limits: n_global < 2^31; BR_ERR_ARG / BR_ERR_WORKSPACE before any launch.
 * brTopKListsMerge: stands in for the final merge of brNeumfCatalogTopK / brDotCatalogTopK (their item splits -> one list) one level up:
 *   per user n_lists lists of k entries (score, LOCAL position), entry e of list w of user u at [w * list_stride + u * user_stride + e]
 *   of scores / index (so the concatenated outputs of n_lists launches, or the receive buffer of one all-to-all, are read in place);
 *   list w's local position l is global position l2g[l2g_off[w] + l] (l2g_off: n_lists + 1 int64, device), every map ascending, so a
 *   list's order is the global order.  -> out_scores / out_index (n_users x k): the k best (score, GLOBAL position) of the union,
 *   descending, ties to the LOWER global position, strict '>' - the one compare of brTopKRows and of the catalogue kernels, NaN scores
 *   treated as that compare treats them (they never enter a list).  Entries with position -1 (a shard with fewer than k candidates
 *   left) or outside their map never win and are never used as an index; where fewer than k entries exist over all lists the tail is
 *   (-inf, -1).  One wave per user, no workspace.  Limits: 1 <= k <= 256, 1 <= n_lists <= 4096, user_stride >= k; BR_ERR_ARG before any
 *   launch. */
int64_t brCsrSplitByOwnerWorkspaceBytes(int64_t n_rows);
int brCsrSplitByOwner(const int64_t* off, const int32_t* idx, int64_t n_rows, const int32_t* g2l, int64_t n_global, int64_t* out_off,
                      int32_t* out_idx, void* ws, int64_t ws_bytes, brStream stream);
int brTopKListsMerge(const float* scores, const int32_t* index, int64_t list_stride, int64_t user_stride, int n_lists, int64_t n_users,
                     int k, const int32_t* l2g, const int64_t* l2g_off, float* out_scores, int32_t* out_index, brStream stream);

/* ---- Catalogue AUC on row-sharded engines, counted where the item rows live: csrc/auc_owner.hip -----------------------------------------
 * brDotCatalogAuc[Wide] (full_auc, src/models/bpr.py:230-254, over bpr_predict, bpr.py:122-133) cut into four phases, so that W owners,
 * each over the candidates whose rows it holds (parallel.py auc_at_owners), return out_auc of ONE launch over the whole candidate list
 * bit for bit: a pair's score depends on its two rows only, the Mann-Whitney count is a sum over the other items, and it is summed in
 * integers.  The reference has no counterpart of the split: MultiWorkerMirroredStrategy (src/models/RModel.py:119) mirrors every table.
 * flags: BR_DOT_FORCE_WIDE as in brDotCatalogAucWide; the positives and the count must get the same flags.  BR_ERR_ARG /
 * BR_ERR_WORKSPACE before any launch; n_users == 0 is BR_OK; no allocation and no sync inside.
 * brDotAucOwnerPositives: bpr.py:122-133 for the pairs (user, positive) alone, the scoring half of brDotCatalogAuc's prepass.  C: this
 *   owner's candidate rows; (pos_off (n_users + 1), pos_idx): per user its positives among them, LOCAL positions (brCsrSplitByOwner).
 *   raw[pos_off[u] + j] = score(u, the user's j-th entry) on v_mfma_f32_16x16x4_f32, one chain from 0 over the padded width the count
 *   instantiates at this dim and flags: the catalogue pass's score bit for bit.  An entry outside [0, n_items) scores NaN.  raw holds
 *   pos_off[n_users] floats.  Limits: 1 <= dim <= 512, 1 <= n_items < 2^31, ld_q, ld_c >= dim.
 * brAucSortPieces: the sorting half of that prepass (the ranking roc_auc_score does inside, bpr.py:252) over the pieces of all owners.
 *   piece_off: n_pieces rows of (n_users + 1) int64: piece w of user u is raw[piece_off[w][u] ... piece_off[w][u + 1]) (so the receive
 *   buffer of an all-gather is read in place; n_raw: raw's floats).  -> sorted[list_off[u] ...]: the user's entries ascending, NaN
 *   dropped, their number P' in pcnt[u]: the multiset the single-device prepass produces, whatever the order of the pieces.
 *   pcnt[u] = -1 (NaN from the finalize) for a user whose list lies past cap (the floats `sorted` holds), whose pieces outnumber
 *   list_off[u + 1] - list_off[u] or lie outside raw; nothing of such a user is read or written.  O(P^2) compares per user.
 *   Limits: 1 <= n_pieces <= 4096.  ws: brAucSortPiecesWorkspaceBytes(n_pieces, cap) bytes; -1 outside the limits.
 * brDotAucOwnerCount: brDotCatalogAuc[Wide]'s catalogue pass (bpr.py:252 without the U x I matrix) over this owner's candidates C with
 *   two CSRs in two roles: (skip_off, skip_idx) the owner's positives, ascending LOCAL positions, skipped; list_off / sorted / pcnt of
 *   brAucSortPieces the user's FULL list every other score is counted against (2P' below its minimum, 0 above its maximum, 2 #{> s} +
 *   #{== s} inside; a NaN score adds 0).  out_w2[u]: the user's 2W over these candidates, uint64, the item splits already summed in
 *   integers.  dump_scores (optional, n_users x n_items): every pair's score (tests).  Limits: 1 <= dim <= 512 (whole-row kernels up to
 *   128 unless BR_DOT_FORCE_WIDE, block kernels above), otherwise those of brDotCatalogAuc.
 *   ws: brDotAucOwnerCountWorkspaceBytes(n_users, n_items, dim) bytes (the per-split partials); -1 outside the limits.
 * brAucFinalizeLists: the division of roc_auc_score (bpr.py:252) and the skip of a user without positives (bpr.py:251).  n_lists partial
 *   2W per user, list w of user u at part[w * list_stride + u] (the receive buffer of an all-to-all read in place); truth_off
 *   (n_users + 1): the GLOBAL truth offsets (P = the user's entries, N = n_items - P over the global n_items); pcnt of brAucSortPieces.
 *   out_auc[u] = (float)((double)W / ((double)P (double)N)), NaN for P <= 0, N <= 0 or pcnt[u] < 0.
 *   Limits: 1 <= n_lists <= 4096, list_stride >= n_users, 1 <= n_items < 2^31. */
int brDotAucOwnerPositives(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                           const int64_t* pos_off, const int32_t* pos_idx, float* raw, int flags, brStream stream);
int64_t brAucSortPiecesWorkspaceBytes(int n_pieces, int64_t cap);
int brAucSortPieces(const float* raw, int64_t n_raw, const int64_t* piece_off, int n_pieces, int64_t n_users, const int64_t* list_off,
                    float* sorted, int64_t cap, int32_t* pcnt, void* ws, int64_t ws_bytes, brStream stream);
int64_t brDotAucOwnerCountWorkspaceBytes(int64_t n_users, int64_t n_items, int dim);
int brDotAucOwnerCount(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                       const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off, const float* sorted, const int32_t* pcnt,
                       int64_t cap, uint64_t* out_w2, float* dump_scores, int flags, void* ws, int64_t ws_bytes, brStream stream);
int brAucFinalizeLists(const uint64_t* part, int64_t list_stride, int n_lists, const int64_t* truth_off, const int32_t* pcnt,
                       int64_t n_users, int64_t n_items, float* out_auc, brStream stream);

/* ---- Catalogue AUC for NeuMF, single-device and at the item owners: csrc/auc_neumf.hip -------------------------------------------------
 * Stands in for full_auc (src/models/bpr.py:230-254) over the NeuMF graph: every (user, item) pair through model.predict as
 * predictForUser does for one user (src/models/NeuMFModel.py:133-150), then roc_auc_score per user - without the U x I matrix.
 * Operands as brNeumfCatalogTopK: pu [n_users][ld_u] (brNeumfCatalogProject, row-major, copy_mf), pit [n1 + dim][ld_i] (col_major,
 * copy_mf), tower of brNeumfCatalogFold, act = BR_ACT_*.  The score of a pair is the head's sigmoid output in inference mode, formed by
 * brNeumfCatalogTopK's operation sequence: it equals that entry's dump_probs bit for bit and depends on the user row, the item column and
 * the tower only.  Limits: those of brNeumfCatalogTopK (2*dim <= 256, n1, n2 <= 128, n3 <= 32, 1 <= n_items < 2^31, ld_u >= n1 + dim,
 * ld_i >= n_items); BR_ERR_ARG / BR_ERR_WORKSPACE before any launch; n_users == 0 is BR_OK; no allocation and no sync inside.
 * brNeumfAucPositives: bpr.py:230-254, NeuMFModel.py:133-150 for the pairs (user, positive) alone.  (pos_off (n_users + 1), pos_idx):
 *   per user its positives among these candidates, positions into pit (LOCAL ones on a row-sharded engine: brCsrSplitByOwner).
 *   raw[pos_off[u] + j] = score(u, the user's j-th entry); an entry outside [0, n_items) scores NaN.  raw holds pos_off[n_users] floats.
 * brNeumfAucCount: bpr.py:230-254, NeuMFModel.py:133-150: the catalogue pass over these candidates with two CSRs in two roles, as
 *   brDotAucOwnerCount: (skip_off, skip_idx) the positives among THESE candidates, ascending positions, skipped; list_off / sorted /
 *   pcnt / cap of brAucSortPieces: the user's FULL list every other score is counted against (2P' below its minimum, 0 above its
 *   maximum, 2 #{> s} + #{== s} inside; a NaN score adds 0).  out_w2[u]: the user's 2W over these candidates, uint64, the item splits
 *   already summed in integers; no float atomics.  dump_probs (optional, n_users x n_items): every pair's score (tests).
 *   ws: brNeumfAucCountWorkspaceBytes(n_users, n_items) bytes (the per-split partials); -1 outside the limits.
 * brNeumfCatalogAuc: bpr.py:230-254, NeuMFModel.py:133-150: the single-device call, four phases chained inside the library:
 *   brNeumfAucPositives, brAucSortPieces with one piece, brNeumfAucCount, brAucFinalizeLists with one list.  truth_off (n_users + 1) /
 *   truth_idx: per user the ascending, unique positions into the item list of its positives (ops.truth_csr, the CSR of brFullAuc).
 *   out_auc[u] = (float)((double)W / ((double)P (double)N)) with P = the user's truth entries and N = n_items - P: bit for bit brFullAuc
 *   on the same scores (while P N < 2^53).  NaN for P == 0 or N == 0.  A NaN score gets no credit on either side.  dump_probs as above.
 *   ws: brNeumfCatalogAucWorkspaceBytes(n_users, n_items, truth_off[n_users]) bytes (per-split partials, the raw and the sorted positive
 *   scores and the sort's scratch); -1 for sizes outside the limits.  The truth entries the workspace cannot hold (and any past
 *   2^31 - 1) are never written: their users get NaN.  The user's positives are sorted by counting rank, O(P^2) compares per user. */
int brNeumfAucPositives(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1,
                        int n2, int n3, int act, const float* tower, const int64_t* pos_off, const int32_t* pos_idx, float* raw,
                        brStream stream);
int64_t brNeumfAucCountWorkspaceBytes(int64_t n_users, int64_t n_items);
int brNeumfAucCount(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1, int n2,
                    int n3, int act, const float* tower, const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off,
                    const float* sorted, const int32_t* pcnt, int64_t cap, uint64_t* out_w2, float* dump_probs, void* ws, int64_t ws_bytes,
                    brStream stream);
int64_t brNeumfCatalogAucWorkspaceBytes(int64_t n_users, int64_t n_items, int64_t n_truth);
int brNeumfCatalogAuc(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1,
                      int n2, int n3, int act, const float* tower, const int64_t* truth_off, const int32_t* truth_idx, float* out_auc,
                      float* dump_probs, void* ws, int64_t ws_bytes, brStream stream);

/* ---- Catalogue ranks for NeuMF: NDCG@k, MRR, recall@k, hit@k over the whole catalogue, single-device and at the item owners: csrc/ranks_neumf.hip ----
 * The reference ranks NeuMF with HR@k over 1 + 100 sampled items (trainers/topKmetrics.py:74-99) and lists at most the top of
 * predictForUser (src/models/NeuMFModel.py:133-150); these entries give the exact rank of every positive among ALL candidates over the
 * same probabilities, without the U x I matrix.  Operands, score and limits as brNeumfCatalogAuc (pu, pit, tower, act; 2*dim <= 256,
 * n1, n2 <= 128, n3 <= 32, 1 <= n_items < 2^31, ld_u >= n1 + dim, ld_i >= n_items): a pair's probability is bit for bit the one
 * brNeumfCatalogAuc / brNeumfCatalogTopK dump.  BR_ERR_ARG / BR_ERR_WORKSPACE before any launch; n_users == 0 is BR_OK; no allocation
 * and no sync inside.
 * brNeumfCatalogRanks: NeuMFModel.py:133-150 over every pair, then the counts of brDotCatalogRanks, whose contract this is: truth_off
 *   (n_users + 1) / truth_idx: the CSR of brNeumfCatalogAuc, n_truth = truth_off[n_users] entries; excl_off / excl_idx (optional, both
 *   or neither): the exclusion CSR of brNeumfCatalogTopK.  Per truth entry e = (u, p), in truth-CSR order, over the candidates i != p
 *   that are not excluded for u:
 *     out_above[e] = #{i: prob(u, i) > prob(u, p)},  out_tied[e] = #{i: prob(u, i) == prob(u, p)}.
 *   The user's other positives are candidates; a position in both CSRs is ranked against the non-excluded others (and is no candidate
 *   for them); a NaN positive, or a position outside [0, n_items), gets (-1, -1); a NaN candidate is never above and never tied.  All
 *   counting is in integers (integer atomics only): the result does not depend on the split plan, the user order or the order of
 *   arrival.  dump_probs (optional, n_users x n_items): every pair's probability (tests).  Limits: those of brNeumfCatalogAuc and
 *   n_truth + n_users < 2^31.  ws: brNeumfCatalogRanksWorkspaceBytes(n_users, n_items, n_truth) bytes (the positives' raw and sorted
 *   scores, two int32 bins per truth entry and user, the sort's scratch); -1 for sizes outside the limits.  brRankMetrics turns the
 *   integers into MRR, NDCG@k, recall@k and hit@k.
 * brNeumfRankCount: the catalogue pass of brNeumfCatalogRanks alone, over the candidates one owner holds (parallel.py ranks_at_owners):
 *   (skip_off, skip_idx): per user the owner's truth and excluded positions in ONE ascending list of LOCAL positions, skipped; list_off /
 *   sorted / pcnt / cap of brAucSortPieces: the user's FULL list of n = pcnt[u] positives.  Every other valid score s adds 1 to the
 *   user's bin #{v < s} when v_0 <= s <= v_{n-1} (and to the tie bin of the same index when v_lo == s), to bin n when s > v_{n-1}, and
 *   nothing below v_0 or when NaN.  bins / ties: int32 [cap + n_users] each, user u's n + 1 bins from list_off[u] + u on; the call ADDS
 *   into them and does not zero them.  Limits: cap + n_users < 2^31.  dump_probs (optional, n_users x n_items).  No workspace.
 * brRankBinsExcluded / brRankBinsFinalize: the two model-independent kernels around the pass, with two CSRs in two roles: the entry CSR
 *   (entry_off (n_users + 1), entry_idx) indexes raw, above and tied: the truth entries ranked by this call, positions in the space of
 *   the exclusion CSR (excl_off, excl_idx) beside it (LOCAL ones at an owner: brCsrSplitByOwner of both); the list CSR list_off indexes
 *   sorted, pcnt and the bins as in brNeumfRankCount.  raw[e]: the score of entry e (brNeumfAucPositives, brDotAucOwnerPositives).
 *   brRankBinsExcluded: an entry that is also excluded is no candidate of the user's positives: -1 in its bin and its tie bin (an
 *   exclusion CSR is required).  brRankBinsFinalize: per user the suffix sums S over the bins IN PLACE (so once per copy of the bins),
 *   then with lo = #{v < raw[e]}, hi = #{v <= raw[e]}: above[e] = S[hi] + (n - hi), tied[e] = T[lo] + (hi - lo) - 1, without the - 1 for
 *   an entry that is itself excluded (excl_off / excl_idx optional, both or neither).  A NaN entry, and every entry of a user whose
 *   list is empty or lies outside cap, is left as it is (the caller presets -1). */
int64_t brNeumfCatalogRanksWorkspaceBytes(int64_t n_users, int64_t n_items, int64_t n_truth);
int brNeumfCatalogRanks(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1,
                        int n2, int n3, int act, const float* tower, const int64_t* truth_off, const int32_t* truth_idx, int64_t n_truth,
                        const int64_t* excl_off, const int32_t* excl_idx, int32_t* out_above, int32_t* out_tied, float* dump_probs, void* ws,
                        int64_t ws_bytes, brStream stream);
int brNeumfRankCount(const float* pu, int64_t ld_u, int64_t n_users, const float* pit, int64_t ld_i, int64_t n_items, int dim, int n1, int n2,
                     int n3, int act, const float* tower, const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off,
                     const float* sorted, const int32_t* pcnt, int64_t cap, int32_t* bins, int32_t* ties, float* dump_probs, brStream stream);
int brRankBinsExcluded(const int64_t* entry_off, const int32_t* entry_idx, const int64_t* excl_off, const int32_t* excl_idx, const float* raw,
                       const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap, int64_t n_users, int32_t* bins,
                       int32_t* ties, brStream stream);
int brRankBinsFinalize(const int64_t* entry_off, const int32_t* entry_idx, const int64_t* excl_off, const int32_t* excl_idx, const float* raw,
                       const int64_t* list_off, const float* sorted, const int32_t* pcnt, int64_t cap, int64_t n_users, int32_t* bins,
                       const int32_t* ties, int32_t* above, int32_t* tied, brStream stream);

/* ---- Catalogue ranks at the item owners for dot-product models (BPR, TwoTower on row-sharded engines): csrc/ranks_owner.hip ------------
 * brDotCatalogRanks (the ranking measures over bpr_predict, src/models/bpr.py:122-133) cut into phases, so that W owners, each holding
 * a share of the candidates, together compute what one launch over all candidates computes, integer for integer (parallel.py
 * ranks_at_owners): brDotAucOwnerPositives and brAucSortPieces, this count, brRankBinsExcluded and brRankBinsFinalize.
 * brDotRankCount: the catalogue pass of brDotCatalogRanks alone (bpr.py:122-133 without the U x I matrix), over the candidates C one
 *   owner holds: the dot-product counterpart of brNeumfRankCount.  Q, C, dim and BR_DOT_FORCE_WIDE as brDotCatalogRanks: a pair's score
 *   is bit for bit the one brDotCatalogRanks and brDotAucOwnerPositives form (v_mfma_f32_16x16x4_f32, the same padded width, one
 *   chain from 0).  Two CSRs in two roles: (skip_off (n_users + 1), skip_idx): per user the owner's truth and excluded positions in ONE
 *   ascending list of LOCAL positions into C, never counted; list_off / sorted / pcnt / cap of brAucSortPieces: the user's FULL list of
 *   n = pcnt[u] positives v_0 <= ... <= v_{n-1} at sorted[list_off[u] ...] (`sorted` holds cap + 1 floats).  The counting rule is
 *   brNeumfRankCount's: every other score s adds 1 to the user's bin #{v < s} when v_0 <= s <= v_{n-1} (and to the tie bin of the same
 *   index when v_lo == s), to bin n when s > v_{n-1}, and nothing below v_0 or when NaN.  bins / ties: int32 [cap + n_users] each, user
 *   u's n + 1 bins from list_off[u] + u on; the call ADDS into them and does not zero them (integer atomics only: the sums do not depend
 *   on the split plan or the order of arrival).  A list with list_off[u] < 0 or ending past cap is left alone (pcnt[u] = -1 of
 *   brAucSortPieces: n = 0).  dump_scores (optional, n_users x n_items): every pair's score (tests).  Limits: those of
 *   brDotCatalogRanks (1 <= dim <= 512, 1 <= n_items < 2^31, ld_q, ld_c >= dim) and cap + n_users < 2^31; BR_ERR_ARG before any launch;
 *   n_users == 0 is BR_OK.  No workspace, no allocation and no sync inside. */
int brDotRankCount(const float* Q, int64_t ld_q, int64_t n_users, const float* C, int64_t ld_c, int64_t n_items, int dim,
                   const int64_t* skip_off, const int32_t* skip_idx, const int64_t* list_off, const float* sorted, const int32_t* pcnt,
                   int64_t cap, int32_t* bins, int32_t* ties, float* dump_scores, int flags, brStream stream);

/* ---- evaluation of the BPR notebook model and hit counting -------------------
 * Ground truth per user = CSR list of COLUMN indices into the scored item list, ascending: truth_off (n_users + 1), truth_idx.
 * brFullAuc: full_auc (src/models/bpr.py:230-254) = per user sklearn.roc_auc_score(ground truth, scores over all items): the
 *   Mann-Whitney statistic with ties counted one half.  auc[u] = NaN for a user without positives (skipped by the reference,
 *   bpr.py:251) or without negatives; the caller averages the others.
 * brMapAtK: mean_average_precision_k (bpr.py:257-289) on the top-k lists of brTopKRows: ap[u] = sum over hits of
 *   (hits so far / rank) / min(len(actual), k) (0 for a user without positives); hits[u] = hits of the list = the per-user true
 *   positives of topKMetrics (trainers/topKmetrics.py:85-93).  ap or hits may be NULL. */
int brFullAuc(const float* scores, int64_t ld_scores, const int64_t* truth_off, const int32_t* truth_idx, int64_t n_users,
              int64_t n_items, float* auc, brStream stream);
int brMapAtK(const int32_t* topk_index, int64_t n_users, int k, const int64_t* truth_off, const int32_t* truth_idx, float* ap,
             int32_t* hits, brStream stream);

/* ---- batch construction on the device: csrc/sampling.hip ---------------------
 * Pure functions of (seed, output position): Philox4x32-10 draws + 4-round Feistel permutations with cycle walking, restated
 * bit for bit in oracle/binrec_oracle.py.  [pandas-sem] the reference's samplers are unseeded pandas calls: the distributions
 * are restated, not the streams.
 * brBootstrapDataset: NeuMFModel.bootstrapDataset (src/models/NeuMFModel.py:102-109): n positives (label 1) + n_neg rows sampled
 *   with replacement whose item column is permuted (label 0, no collision check), all shuffled.  Outputs have n + n_neg entries.
 * brBprSampleTriplets: for every positive (user, item) row neg_per_pos triplets (user, item, negative): the negative is drawn
 *   uniformly from cand_items (n_cand ids; NULL = 0..n_cand-1) and re-drawn while it is a positive of the user (at most max_tries
 *   draws) - the sampled replacement of the O(U*I) enumeration of src/models/BPRModel.py:111-119.  pos_off (num_users + 1) /
 *   pos_items: the users' positives as CSR with ascending items.
 * brNcfNegativeCandidates + brSortUniqueKeys64 + brGatherPermutedPairs: generateNegativeFeedback (Data handling/synthetic.py:
 *   208-223,237-256): candidates = customer column and product column shuffled independently, round after round (candidate j:
 *   round j / n); keys[j] = user * num_items + item, or ~0 for a positive pair.  Sorted and de-duplicated they are the pool of
 *   distinct negatives (n_unique counts a trailing ~0 if any candidate was invalid); brGatherPermutedPairs takes n_out of the
 *   first n_keys of them in a shuffled order (the reference's head(size)).
 * brBprSampleNegatives (csrc/sampling_step.hip): the negatives of ONE batch, drawn per step - the per-step form of the site
 *   brBprSampleTriplets stands in for (src/models/BPRModel.py:94-98,111-119), with the two standard strategies: popularity-weighted
 *   draws and dynamic negative sampling (n_candidates = M > 1: draw M, score them with the current model, keep the hardest).
 *   out_neg[b] is a pure function of (seed, draw_step, pos0 + b) and - M > 1 - of the tables:
 *     candidate j < M, attempt a < max_tries: d = Philox4x32-10(counter (pos0 + b, j * 256 + a, 5, draw_step), key seed) (stream 5;
 *       1-4 are taken above); slot = (d.x * n_cand) >> 32; with an alias table (alias_thresh uint32 / alias_slot int32, n_cand
 *       entries each, Walker's method; both NULL = uniform): if d.y >= alias_thresh[slot] then slot = alias_slot[slot];
 *       id = cand_items ? cand_items[slot] : slot; re-drawn while id is a positive of users[b] and a + 1 < max_tries (the last attempt
 *       stands: the rule of brBprSampleTriplets).  pos_off (num_users + 1) / pos_items: the positives' CSR, items ascending.
 *     M > 1: score_j = <user row, candidate j's row> in fp32 (per-lane fused multiply-adds in column order, then a fixed shuffle
 *       tree: the same bits for the same inputs); out_neg[b] = the first candidate whose score is strictly greater than every earlier
 *       one (a NaN never wins).  The rows are those of the last completed step: deferred tables (m, v, last of both tables and the
 *       step state given) are replayed over (last[row], step_state->step] in registers as brGatherRowsDeferred does, nothing is
 *       written back; current tables (sweep / lazy Adam) pass m = v = last = NULL and are read as stored.
 *     M == 1 reads no table: the table pointers may be NULL.
 *   out_neg (batch) and the optional out_cands (batch x M ids) have the id type of `users`; out_scores (batch x M floats, optional;
 *   0 for M == 1).  Ids outside their table or CSR set BR_ERRFLAG_RANGE in *err_flag and use row 0.
 *   Limits: 1 <= M <= 32, 1 <= max_tries <= 256, batch < 2^31, n_cand < 2^32; M > 1 needs both tables; BR_ERR_ARG before any launch.
 * brNeumfSampleBatch (csrc/sampling_epoch.hip): rows [row0, row0 + batch) of epoch `epoch` of the NeuMF fit, formed per step - the
 *   per-step form of the site brBootstrapDataset stands in for (src/models/NeuMFModel.py:102-123): every positive once with label 1
 *   and, per positive, r = neg_per_pos negatives with label 0, drawn again in every epoch and rejected while they are positives of
 *   the customer.  An epoch has N = n (1 + r) rows; a row is a pure function of (seed, epoch, global row g):
 *     d = Philox4x32-10(counter (epoch, 0, 7, 0), key seed); seed_e = d.y << 32 | d.x; src = feistel_perm(g, N, perm_key(seed_e, 6)).
 *     src < n: the row is (pos_users[src], pos_items[src], 1.0f).  Otherwise j = src - n, p = j / r: the user is pos_users[p], the
 *     label 0.0f and the item the draw of brBprSampleNegatives keyed on j: attempt a < max_tries takes
 *     d = Philox4x32-10(counter (j, a, 6, epoch), key seed) (streams 6 and 7; 1-5 are taken above); slot = (d.x * n_cand) >> 32; with an
 *     alias table: if d.y >= alias_thresh[slot] then slot = alias_slot[slot]; id = cand_items ? cand_items[slot] : slot; re-drawn
 *     while id is a positive of the user and a + 1 < max_tries (the last attempt stands).
 *   So every positive gets exactly r negatives per epoch, and they depend neither on the epoch's order nor on the batch size or the
 *   number of ranks (a rank asks for its own slice of the global batch).  pos_users / pos_items (n) and the outputs (batch each) have
 *   one id type; pos_off (num_users + 1) / pos_sorted_items: the positives' CSR, items ascending.  A user outside the CSR sets
 *   BR_ERRFLAG_RANGE in *err_flag and is treated as user 0 for the rejection test.  Limits: neg_per_pos >= 0, N < 2^32,
 *   1 <= max_tries <= 256, n_cand < 2^32, 0 <= row0, row0 + batch <= N; BR_ERR_ARG before any launch; batch == 0 is BR_OK. */
int brBootstrapDataset(const void* users, const void* items, int id_type, int64_t n, int64_t n_neg, uint64_t seed, void* out_users,
                       void* out_items, float* out_labels, brStream stream);
int brBprSampleTriplets(const void* users, const void* items, int id_type, int64_t n, int neg_per_pos, const int64_t* pos_off,
                        const void* pos_items, const void* cand_items, int64_t n_cand, uint64_t seed, int max_tries, void* out_users,
                        void* out_pos, void* out_neg, brStream stream);
int brBprSampleNegatives(const void* users, int id_type, int64_t batch, int64_t pos0, uint32_t draw_step, const int64_t* pos_off,
                         const void* pos_items, int64_t num_users, const void* cand_items, int64_t n_cand, const uint32_t* alias_thresh,
                         const int32_t* alias_slot, uint64_t seed, int n_candidates, int max_tries, const float* user_table,
                         const float* user_m, const float* user_v, const int32_t* user_last, int64_t user_rows, const float* item_table,
                         const float* item_m, const float* item_v, const int32_t* item_last, int64_t item_rows, int dim,
                         const void* step_state, double beta1, double beta2, double eps, void* out_neg, void* out_cands,
                         float* out_scores, int* err_flag, brStream stream);
int brNeumfSampleBatch(const void* pos_users, const void* pos_items, int id_type, int64_t n, int neg_per_pos, const int64_t* pos_off,
                       const void* pos_sorted_items, int64_t num_users, const void* cand_items, int64_t n_cand, const uint32_t* alias_thresh,
                       const int32_t* alias_slot, uint64_t seed, uint32_t epoch, int64_t row0, int64_t batch, int max_tries, void* out_users,
                       void* out_items, float* out_labels, int* err_flag, brStream stream);
int brNcfNegativeCandidates(const void* users, const void* items, int id_type, int64_t n, int64_t n_cand, const int64_t* pos_off,
                            const void* pos_items, int64_t num_items, uint64_t seed, uint64_t* keys, brStream stream);
int64_t brSortUniqueWorkspaceBytes(int64_t n);
int brSortUniqueKeys64(const uint64_t* keys, int64_t n, uint64_t* out_keys, int64_t* n_unique, void* workspace, int64_t workspace_bytes,
                       brStream stream);
int brGatherPermutedPairs(const uint64_t* keys, int64_t n_keys, int64_t n_out, int64_t num_items, uint64_t seed, int id_type, void* out_users,
                          void* out_items, brStream stream);

/* ---- fused step driver: the whole NeuMF training / inference step from ONE host call ----------
 * trainers/NFC_plain.py:165 `model.fit` step, src/models/RModel.py:130.  Pure launch sequencing
 * over the entry points above (no new arithmetic): removes ~35 Python->C transitions per step so
 * the host stays ahead of the GPU.  The caller fills the struct once, then per step updates
 * users/items/labels/batch/step/alpha_t.  `phases` selects segments so a data-parallel host can
 * interleave its collectives (BatchNorm sums, dense-gradient all-reduce, row exchange):
 *   FWD1 zero scratch, [EMBED] embed forward, dense L1 (+ BN1 sums)
 *   FWD2 BN1 finalize, dense L2 (+ BN2 sums)
 *   FWD3 BN2 finalize, dense L3, head (+ loss/metric sums, head grads), backward L3 (+ BN2-bwd sums)
 *   BWD2 backward L2 (+ BN1-bwd sums)        BWD1 backward L1
 *   BNG  gamma/beta grads from the BN-backward sums
 *   OPT_TABLES [EMBED] embed backward   INDEX the dedup indexes   ROWS_USER / SWEEP_USER / ROWS_ITEM / SWEEP_ITEM the table
 *   optimizer launches (separate bits so a host can keep one of them outside a captured hipGraph)
 *   OPT_DENSE Adam on theta
 * EMBED: include the table-side embed forward/backward (single GPU); cleared by the row-sharded
 * host, which runs its own exchange and calls brNeumfEmbedForward/Backward on the received rows.
 * Dense parameter layout (theta/grad/adam_m/adam_v, floats):
 *   [W1 2*dim x n1 | b1 n1 | g1 n1 | be1 n1 | W2 n1 x n2 | b2 n2 | g2 n2 | be2 n2 | W3 n2 x n3 | b3 n3 | W4 n3+1 | b4 1] */
enum {
  BR_PH_FWD1 = 1, BR_PH_FWD2 = 2, BR_PH_FWD3 = 4, BR_PH_BWD2 = 8, BR_PH_BWD1 = 16, BR_PH_BNG = 32,
  BR_PH_OPT_TABLES = 64,      /* [EMBED] embed backward */
  BR_PH_OPT_DENSE = 128, BR_PH_EMBED = 256,
  BR_PH_ROWS_USER = 512, BR_PH_SWEEP_USER = 1024, BR_PH_ROWS_ITEM = 2048, BR_PH_SWEEP_ITEM = 4096,
  BR_PH_INDEX = 8192,         /* build the two dedup indexes in this call: on aux_stream beside the forward when the
                                 call also holds FWD1 (joined before ROWS_* or at the end of the call), else inline */
  BR_PH_ALL = 16383
};
/* One step of a multi-step group (brNeumfStep.group_sets): what that step's own brNeumfStepRun call carries in `users`, `items`,
 * the u_ / i_ index fields (workspaces of u_ws_bytes / i_ws_bytes, as the call's own) and `dstat`.  The head call of the group
 * builds the index of every step from these; the later calls only read theirs. */
enum { BR_GROUP_MAX = 8 };
typedef struct brNeumfGroupSet {
  const void* users; const void* items;
  void* u_sorted_ids; int32_t* u_sorted_pos; void* u_ws;
  void* i_sorted_ids; int32_t* i_sorted_pos; void* i_ws;
  double* dstat;
} brNeumfGroupSet;
typedef struct brNeumfStep {
  int64_t batch, batch_total, row0, user_rows, item_rows;
  int32_t dim, n1, n2, n3, act, loss, item_first, mf_first, id_type, adam_dense, training, step;
  int32_t bn_local;   /* 1: BatchNorm statistics over THIS process' batch (per-replica BN, what MirroredStrategy does with a
                         plain BatchNormalization [TF-sem]) while the loss is still scaled by 1/batch_total; 0: the column
                         sums are all-reduced by the host and cover batch_total rows */
  int32_t fused_final;   /* 1 (single process): the slab reductions, the BatchNorm parameter gradients and the dense Adam run
                            as ONE launch at BR_PH_OPT_DENSE (brDenseFinalize) instead of inside their phases; `slabs` then
                            holds three regions [tail | layer 2 | layer 1] (brNeumfStepSlabFloats).
                            2 (data-parallel host): the reductions and the BatchNorm parameter gradients as ONE launch at BR_PH_BNG
                            (brDenseFinalize without parameters); the host all-reduces `grad` and runs BR_PH_OPT_DENSE (brAdamFlat) */
  float dropout, bn_eps, bn_momentum, pad0;
  uint64_t seed;
  double alpha_t, beta1, beta2, adam_eps;
  const void* users;
  const void* items;
  const float* labels;                     /* may be NULL in inference */
  float* user_tab; float* user_m; float* user_v;   /* fused [rows][mlp|mf] (row = 2*dim floats) */
  float* item_tab; float* item_m; float* item_v;
  uint8_t* user_mark; uint8_t* item_mark;          /* [rows], adam_dense only */
  float* theta; float* grad; float* adam_m; float* adam_v;
  float* moving;                           /* [mm1 n1 | mv1 n1 | mm2 n2 | mv2 n2] */
  float* x0; float* dot; float* a1; float* a2; float* a3; float* logit; float* prob;    /* a1 / gh1 and a2 / gh2: row stride n rounded up to 4 floats */
  float* da3; float* ddot; float* gh2; float* gh1; float* dx0; float* g_user; float* g_item;
  float* bn;                               /* [scale1|shift1|mean1|rstd1] n1 each, then the same for layer 2 */
  double* dstat;                           /* [stats1 | stats2 | bsum1 | bsum2], each [BR_STAT_REPLICAS][2n]; zeroed in FWD1 */
  double* msums;                           /* [BR_SUM_SLOTS][BR_METRIC_SUMS] accumulated (brNeumfHead) */
  float* slabs; float* hslabs;
  float* dz_ws;                            /* brDenseBackwardWorkspaceFloats(max layer) floats */
  uint32_t* keep_bits;                     /* the three dropout planes of a step back to back: brDropoutKeepWords(batch, 2*dim) +
                                              (batch, n1) + (batch, n2) words (training with dropout > 0) */
  int* err_flag;
  float* u_seg_ws; float* i_seg_ws;        /* brSegmentScratchFloats(max batch, 2*dim) each, or NULL (one-by-one duplicate sums) */
  void* u_sorted_ids; int32_t* u_sorted_pos; void* u_ws; int64_t u_ws_bytes;
  void* i_sorted_ids; int32_t* i_sorted_pos; void* i_ws; int64_t i_ws_bytes;
  double lr;          /* learning rate (only used with step_state) */
  void* step_state;   /* optional device step state (brStepStateBytes()): when non-NULL (and the call holds
                         BR_PH_FWD1|BR_PH_EMBED; a host that runs the lookup itself advances it itself, before the lookup) the step advances it in
                         FWD1 (step += 1, alpha_t = lr*sqrt(1-b2^step)/(1-b1^step)) and every kernel reads the
                         dropout step / Adam alpha from there instead of `step` / `alpha_t` above, so the whole
                         call can be captured once in a hipGraph and replayed */
  int32_t* user_last; int32_t* item_last;   /* [rows], adam_dense == 2 only (deferred dense Adam, see brAdamFlush) */
  void* aux_stream;   /* optional second hipStream_t: the two dedup sorts depend only on the ids, so a call that
                         holds BR_PH_INDEX together with BR_PH_FWD1 runs them here beside the forward/backward and
                         joins them (event) before the Adam-rows kernels; NULL = same stream */
  int64_t keep_rows;  /* rows the three planes of keep_bits are laid out for (plane offsets = brDropoutKeepWords(keep_rows, K));
                         0 = the batch of the call */
  int32_t keep_ready; /* 1: keep_bits already holds THIS step's masks (a previous call prefetched them): FWD1 does not generate them */
  int32_t keep_prefetch;  /* 1 or 2 (training, dropout, single process): the call that holds BR_PH_ROWS_USER also fills keep_bits with the
                         NEXT step's masks (step + 1, same seed / row0, keep_rows rows) beside the Adam-rows kernel (Philox is ALU-bound,
                         the optimizer HBM-bound): 1 = as a launch on aux_stream (needed), joined before the call returns; 2 = as extra
                         workgroups of the paired Adam-rows launch when the call holds BR_PH_ROWS_ITEM too (no fork / join - 4 us less
                         per step inside a hipGraph - but that launch then takes 101 instead of 94 us).  The host sets keep_ready on
                         the next call if that call's step / row0 are the ones prefetched */
  int32_t group_size; /* 0: a step on its own.  2 .. BR_GROUP_MAX: this call is step group_pos of a group of group_size consecutive
                         training steps issued back to back on one stream (NeuMFEngine.enable_graph_multi), all of whose ids are on the
                         device before the first call: the row index of EVERY step is built by the head call (group_pos == 0: the chunk
                         sorts of all 2 * group_size id streams ride in its lookup launch, one chunk-rank launch ranks them, advances
                         the step state for the head and clears the `dstat` of every step).  A later call (group_pos >= 1) launches
                         the plain one-wave-per-pair lookup, no sort and no rank, and advances the step state by one extra workgroup
                         of its segment-partials launch - behind its lookup, in front of its Adam-rows launch.  Only where
                         brNeumfGroupIndexPlan() > 0 for the struct, with phases == BR_PH_ALL; anything else is BR_ERR_ARG */
  int32_t group_pos;
  const brNeumfGroupSet* group_sets;   /* HOST array of group_size entries, read during the call (entry k: step k; the head's own
                                          entry 0 is not read, its fields above count); every step its own index buffers and dstat */
} brNeumfStep;
/* step_state: device {uint32 step; float alpha_t; double b1^step, b2^step; float alpha_hist[BR_ALPHA_RING + BR_RING_MIRROR]; replay form},
 * brStepStateBytes() bytes, zero-initialised (or step / alpha_t set by the host after a reload).
 * Advance: step += 1, alpha_t = alpha_hist[step % BR_ALPHA_RING] = lr*sqrt(1-b2^step)/(1-b1^step) (b^step kept as a
 * running double product), and `zero[0..n_zero)` (the step's double scratch) cleared in the same launch. */
enum { BR_ALPHA_RING = 1024, BR_RING_MIRROR = 8 };
int64_t brStepStateBytes(void);
/* How the deferred kernels replay a row's pending g = 0 steps (see "Deferred dense Adam" below).  Written into the step state once,
 * before the first step (host -> device copy, synchronises the stream); a zero-initialised state replays exactly.
 *   BR_REPLAY_EXACT: step by step with the sweep's own fp32 operations (m *= b1; v *= b2; theta -= alpha_j m / (sqrt(v) + eps)):
 *                    tables bit-equal to brAdamDenseSweep.
 *   BR_REPLAY_FAST : the same recurrence in a cheaper form - d_j = sqrt(v_j) + eps advanced as d_j = sqrt(b2) d_{j-1} + eps (1 - sqrt(b2))
 *                    (one v_sqrt per row visit, none per step), 1 / d_j by one Newton step from 1 / d_{j-1} (relative error
 *                    (1 - sqrt(b2))^2 = 2.5e-7: what the hardware v_rcp_f32 of the exact form is allowed), theta replayed over at most
 *                    `trunc` steps of a lag (the steps behind that move it by less than one ulp of the first: m has decayed by b1^trunc),
 *                    and the moments of a lag of L steps as ONE product each: m b1^L, v b2^L.  Agrees with the exact form to ~1e-6 of
 *                    a row's movement (tests/test_gpu_neumf.py); no longer bit-equal to the sweep. */
enum { BR_REPLAY_EXACT = 0, BR_REPLAY_FAST = 1 };
int brStepStateInit(void* step_state, double beta1, double beta2, double eps, int replay_mode, brStream stream);
int brStepStateAdvance(void* step_state, double lr, double beta1, double beta2, double* zero, int64_t n_zero, brStream stream);
/* host -> device: step, alpha_t and the running beta powers for that step (after a reload); synchronises the stream */
int brStepStateSet(void* step_state, uint32_t step, double lr, double beta1, double beta2, brStream stream);
/* one launch that copies a batch (ids, ids, labels) into the static input buffers a captured hipGraph reads */
int brStageBatch(void* dst_users, void* dst_items, float* dst_labels, const void* users, const void* items,
                 const float* labels, int id_type, int64_t n, brStream stream);

/* ---- Deferred dense Adam (brNeumfStep.adam_dense == 2) --------------------------------------------------
 * Keras' Adam applies the g = 0 update to every row of an embedding table on every step ([TF-sem], the
 * reference's trainers/NFC_plain.py:155 optimizer on Embedding variables): a 6-floats-per-element sweep of the
 * table per step.  The deferred form produces the SAME values without the sweep: last[row] = last step the
 * stored (theta, m, v) of that row include; the lookup replays the missing g = 0 steps in registers
 * (brNeumfEmbedForwardDeferred, nothing written), the optimizer replays them and applies this step's
 * gradient for the rows of the batch (brAdamRowsSortedDeferred, last[row] = step), and brAdamFlush brings the
 * whole table to the current step — required before anything else reads the table, and at least every
 * BR_ALPHA_RING - 1 steps (the replay takes each step's alpha_t from the ring in step_state).
 * Same fp32 operations in the same order as brAdamDenseSweep => bit-equal tables after a flush. */
int brNeumfEmbedForwardDeferred(const float* user_tab, const float* user_m, const float* user_v, const int32_t* user_last,
                                const float* item_tab, const float* item_m, const float* item_v, const int32_t* item_last,
                                int64_t user_rows, int64_t item_rows, const void* users, const void* items, int id_type,
                                int dim, int64_t batch, int item_first, const void* step_state, double beta1, double beta2,
                                double eps, float* x0, float* dot, float* stash_user, float* stash_item, int64_t ld_stash,
                                int* err_flag, brStream stream);
/* G1 on one deferred table: out[b] = row ids[b] as of step-1 (replayed in registers, nothing written back). */
int brGatherRowsDeferred(const float* table, const float* m, const float* v, const int32_t* last, int64_t table_rows, int dim,
                         const void* ids, int id_type, int64_t n, const void* step_state, double beta1, double beta2,
                         double eps, float* out, int64_t ld_out, int* err_flag, brStream stream);
/* the same for two tables of one geometry (dim, ld_out) in ONE launch: a row-sharded owner serves its user and its item shard
 * (n_b != 0: ids_b has n_b entries instead of n) */
int brGatherRowsDeferredPair(const float* table_a, const float* m_a, const float* v_a, const int32_t* last_a, int64_t rows_a, const void* ids_a,
                             float* out_a, const float* table_b, const float* m_b, const float* v_b, const int32_t* last_b, int64_t rows_b,
                             const void* ids_b, float* out_b, int dim, int id_type, int64_t n, int64_t n_b, const void* step_state, double beta1,
                             double beta2, double eps, int64_t ld_out, int* err_flag, brStream stream);
/* brGatherRowsDeferredPair AND both dedup indexes of the step (brRowIndexBuild of ids_a over n_a, of ids_b over n_b) in two launches on
 * one stream: the chunk sorts of the two id streams run as workgroups of the gather's own launch, the chunk-rank launch follows.
 * advance != 0: the step state is advanced (brStepStateAdvance with lr) by that second launch - the gather then computes the step as
 * step + 1 - so a BPR step (src/models/BPRModel.py:49-74: user gather of B rows, [pos | neg] gather of 2 B rows of the shared item
 * table) needs no launch of its own for it and no side stream for its sorts.  Rows of 64 / 128 / 256 floats, n <= 524 288 per stream. */
int brGatherRowsDeferredPairWithIndex(const float* table_a, const float* m_a, const float* v_a, const int32_t* last_a, int64_t rows_a, const void* ids_a,
                                      float* out_a, void* sorted_ids_a, int32_t* sorted_pos_a, void* ws_a, int64_t ws_a_bytes, const float* table_b,
                                      const float* m_b, const float* v_b, const int32_t* last_b, int64_t rows_b, const void* ids_b, float* out_b,
                                      void* sorted_ids_b, int32_t* sorted_pos_b, void* ws_b, int64_t ws_b_bytes, int dim, int id_type, int64_t n_a, int64_t n_b,
                                      void* step_state, int advance, double lr, double beta1, double beta2, double eps, int64_t ld_out, int* err_flag,
                                      brStream stream);
/* B1 of the GMF dot on the MF rows the deferred forward stashed, in place: (u_b, i_b) -> (ddot_b i_b, ddot_b u_b). */
int brMfGradInplace(float* stash_user, float* stash_item, int64_t ld, const float* ddot, int64_t batch, int dim, brStream stream);
int brAdamRowsSortedDeferred(float* table, float* m, float* v, int32_t* last, int64_t table_rows, int dim,
                             const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                             const float* row_grads, int64_t ldg, const float* row_grads_hi, int64_t ldg_hi, int split,
                             const void* step_state, double beta1, double beta2, double eps, float* seg_ws, brStream stream);
/* Same, handed the rows as the step's lookup replayed them: replayed_rows + pos * ld_replayed = row sorted_ids[.] of position pos as
 * brGatherRowsDeferred wrote it this step (bpr.py: the gathered rows; a row-sharded owner: the rows it served).  The optimizer then
 * replays only the moments (two multiplies per lagging step instead of the lookup's sqrt / rcp chain on theta): same bits, since the
 * lookup ran the same replay on the same stored row.  Replaces Keras' sparse apply of an Embedding variable (NFC_plain.py:155,
 * BPRModel.py:52) on the touched rows. */
int brAdamRowsSortedDeferredReplayed(float* table, float* m, float* v, int32_t* last, int64_t table_rows, int dim,
                                     const void* sorted_ids, int id_type, const int32_t* sorted_pos, int64_t n,
                                     const float* row_grads, int64_t ldg, const float* row_grads_hi, int64_t ldg_hi, int split,
                                     const float* replayed_rows, int64_t ld_replayed, const void* step_state, double beta1,
                                     double beta2, double eps, float* seg_ws, brStream stream);
/* The user and the item table of one NeuMF step in ONE launch (same dim, n, split; each alone leaves HBM half idle).
 * last_* non-NULL (both): deferred mode (step_state required, alpha_t ignored); else brAdamRowsSorted semantics with marks.
 * hi_scale (n floats, may be NULL): the grads_hi rows of BOTH tables are multiplied by hi_scale[position] as they are read.  The
 * deferred step passes the stashed partner MF rows as grads_hi (user table: the item rows, item table: the user rows) and
 * ddot here: g_user_mf[b] = ddot[b]*item_mf[i_b] (brNeumfEmbedBackward) without the launch that used to write it out. */
int brAdamRowsSortedPair(float* table_a, float* m_a, float* v_a, int64_t rows_a, const void* sorted_ids_a, const int32_t* sorted_pos_a,
                         const float* grads_a, int64_t ldg_a, const float* grads_hi_a, int64_t ldg_hi_a, uint8_t* mark_a, int32_t* last_a,
                         float* table_b, float* m_b, float* v_b, int64_t rows_b, const void* sorted_ids_b, const int32_t* sorted_pos_b,
                         const float* grads_b, int64_t ldg_b, const float* grads_hi_b, int64_t ldg_hi_b, uint8_t* mark_b, int32_t* last_b,
                         int dim, int id_type, int64_t n, int split, const float* hi_scale, const void* step_state, double alpha_t,
                         double beta1, double beta2, double eps, float* seg_ws_a, float* seg_ws_b, brStream stream);
/* brAdamRowsSortedPair on deferred tables, handed the rows as the step's gathers replayed them (see brAdamRowsSortedDeferredReplayed):
 * replayed_x + pos * ld_replayed = the full row (dim floats) of position pos of table x.  A row-sharded owner updates its user and its
 * item shard with this one launch (both streams have the same number of slots under the fixed-capacity exchange).  n_b != 0: table b has
 * n_b positions instead of n (bpr.py: B user positions, 2B [pos | neg] item positions); grads_hi_* both NULL: one gradient source per table. */
int brAdamRowsSortedPairReplayed(float* table_a, float* m_a, float* v_a, int64_t rows_a, const void* sorted_ids_a, const int32_t* sorted_pos_a,
                                 const float* grads_a, int64_t ldg_a, const float* grads_hi_a, int64_t ldg_hi_a, int32_t* last_a,
                                 const float* replayed_a,
                                 float* table_b, float* m_b, float* v_b, int64_t rows_b, const void* sorted_ids_b, const int32_t* sorted_pos_b,
                                 const float* grads_b, int64_t ldg_b, const float* grads_hi_b, int64_t ldg_hi_b, int32_t* last_b,
                                 const float* replayed_b, int64_t ld_replayed,
                                 int dim, int id_type, int64_t n, int64_t n_b, int split, const void* step_state,
                                 double beta1, double beta2, double eps, float* seg_ws_a, float* seg_ws_b, brStream stream);
int brAdamFlush(float* table, float* m, float* v, int32_t* last, int64_t table_rows, int dim, const void* step_state,
                double beta1, double beta2, double eps, brStream stream);
int64_t brNeumfStepSizeof(void);
/* floats of brNeumfStep.slabs for batches up to `batch`: the three slab regions [tail | layer 2 | layer 1] back to back */
int64_t brNeumfStepSlabFloats(int64_t batch, int dim, int n1, int n2, int n3);
int brNeumfStepRun(const brNeumfStep* s, uint32_t phases, brStream stream);
int64_t brNeumfGroupSetSizeof(void);
/* Host only: may `s` (filled as for a training call of the group; group_size / group_pos / group_sets are not read) run as a step of a
 * group of `steps` steps whose index is built at the head (brNeumfStep.group_size)?  -> the sort workgroups of the head's lookup
 * launch, 2 * chunks * steps, or 0: the step's own fused lookup + index path would not be taken (single GPU, deferred tables,
 * batch > 16 384, embed_dim 64 / 128, BR_FUSED_SORT != 0), the dropout planes are not prefetched (dropout > 0 without keep_ready),
 * steps is outside 2 .. BR_GROUP_MAX, the segment scratch is missing, or BR_GROUP_INDEX=0 (read on every call: A/B runs). */
int brNeumfGroupIndexPlan(const brNeumfStep* s, int steps);

/* Implicit-feedback ALS (Hu, Koren, Volinsky 2008; csrc/als.hip).  Single device.
 * brGram: G = Y^T Y of the rows x dim table Y (row stride ld), dim x dim row-major, both triangles, exactly symmetric.  Workgroups
 *   multiply contiguous slices of rows on the fp32-input MFMA into partials in ws (brGramWorkspaceBytes(rows, dim); -1 outside the
 *   limits); a second launch adds the partials in index order in double and rounds once.  No atomics: two calls on one input give the
 *   same bits.  rows == 0 gives G = 0.
 * brAlsSolveRows: one half-step.  For every row u of the CSR (off int64 [n_rows + 1] non-decreasing, idx int32 positions into Y,
 *   conf float32 >= 0 per entry or NULL = 1) with c_e = alpha * conf[e]:
 *       A_u = G + reg I + sum_e c_e y_e y_e^T,   b_u = sum_e (1 + c_e) y_e,   X[u] = A_u^-1 b_u
 *   by an in-LDS Cholesky factorisation, one workgroup per row.  X[u] is a function of (G, reg, alpha, the row's entries in their
 *   order and the rows of Y they name) alone; columns of X past dim are not written.  A row without entries gets exact zeros.  An
 *   idx outside [0, n_y) is never dereferenced: it sets BR_ERRFLAG_RANGE in *err_flag (may be NULL) and counts as absent.  A pivot
 *   that is not a positive finite number makes the row NaN.
 * Limits: 1 <= dim <= 128 (any value), ld >= dim, n_y < 2^31, n_rows < 2^31, reg > 0 and alpha >= 0 finite; BR_ERR_ARG /
 * BR_ERR_WORKSPACE before any launch; n_rows == 0 is BR_OK; no allocation and no sync inside. */
int64_t brGramWorkspaceBytes(int64_t rows, int dim);
int brGram(const float* Y, int64_t ld, int64_t rows, int dim, float* G, void* ws, int64_t ws_bytes, brStream stream);
int brAlsSolveRows(const float* Y, int64_t ld_y, int64_t n_y, int dim, const float* G, const int64_t* off, const int32_t* idx,
                   const float* conf, float alpha, float reg, int64_t n_rows, float* X, int64_t ld_x, int* err_flag, brStream stream);

/* ALS for rows up to 512 features (csrc/als_wide.hip).  Single device.
 * brGramWide: brGram's contract for 1 <= dim <= 512: both triangles, G bit-equal to its transpose, the bits a function of (Y, rows, dim)
 *   alone (two calls, and the 16-byte and the scalar load paths, give the same bits), any ld >= dim, rows == 0 gives G = 0.  G is formed
 *   in blocks of 128 columns: a workgroup multiplies a slice of rows of one pair of column blocks on the fp32-input MFMA into a partial
 *   in ws (brGramWideWorkspaceBytes(rows, dim); -1 outside the limits); a second launch adds the slices' partials in index order in
 *   double, rounds once and writes G[I][J] and G[J][I] from the one value.  No atomics.  (Not the bits of brGram at dim <= 128.)
 * brAlsSolveRowsCg: one half-step by `steps` conjugate-gradient steps per row from the row's current vector (Takacs, Pilaszy, Tikk
 *   2011), X in and out.  With A_u and b_u as for brAlsSolveRows, applied as A p = G p + reg p + sum_e c_e y_e (y_e . p), never formed:
 *       x = X[u]; r = b - A x; p = r; rs = r.r
 *       `steps` times: stop unless rs >= 1e-20; q = A p; d = p.q; stop unless d is positive and finite;
 *                      a = rs / d; x += a p; r -= a q; rn = r.r; p = r + (rn / rs) p; rs = rn
 *       X[u] = x
 *   "stop" ends that row alone.  G must be symmetric (brGram / brGramWide: it is read through its transpose).  G p runs on the
 *   fp32 MFMA; the sparse term, the dot products and x, r, p are carried in double and x is rounded to float once, at the end.  A
 *   workgroup takes 32 consecutive rows (16 above 256 features) and reads G once per application of A; X[u] is a function of (G, reg, alpha, the row's entries in their order,
 *   the rows of Y they name, X[u] on entry, steps) alone - not of the rows beside it, n_rows or the grid; two calls give the same
 *   bits; no atomics on floats.  Columns of X past dim are not written.  A row without entries gets exact zeros.  An idx outside
 *   [0, n_y) is never dereferenced: it sets BR_ERRFLAG_RANGE in *err_flag (may be NULL) and counts as absent.
 * Limits: 1 <= dim <= 512 (any value), ld >= dim, 1 <= steps <= 64, n_y < 2^31, n_rows < 2^31, reg > 0 and alpha >= 0 finite;
 * BR_ERR_ARG / BR_ERR_WORKSPACE before any launch; n_rows == 0 is BR_OK; no allocation and no sync inside. */
int64_t brGramWideWorkspaceBytes(int64_t rows, int dim);
int brGramWide(const float* Y, int64_t ld, int64_t rows, int dim, float* G, void* ws, int64_t ws_bytes, brStream stream);
int brAlsSolveRowsCg(const float* Y, int64_t ld_y, int64_t n_y, int dim, const float* G, const int64_t* off, const int32_t* idx,
                     const float* conf, float alpha, float reg, int64_t n_rows, float* X, int64_t ld_x, int steps, int* err_flag,
                     brStream stream);

/* ALS by conjugate gradients, the heavy rows (csrc/als_heavy.hip).  Single device.  A row with very many entries leaves
 * brAlsSolveRowsCg (one wave walks all of them, once per application of A): its operator is formed once, by many workgroups, and the
 * same recurrence runs on the dense matrix.
 * brAlsNormalRows: for every listed row rows[h] (int32, ascending, unique, h < n_heavy) of the CSR (off, idx, conf or NULL = 1, as for
 *   brAlsSolveRows; n_rows = rows of the CSR) with c_e = alpha * conf[e]:
 *       H[h] = sum_e c_e y_e y_e^T   (float32 [n_heavy][dim][dim], both triangles, bit-equal to its transpose)
 *       b[h] = sum_e (1 + c_e) y_e    (double  [n_heavy][dim])
 *   A row's entries are cut into slices of `slice` entries (a multiple of 64, at least 64); slice_off (int64 [n_heavy + 1], device,
 *   slice_off[0] = 0, slice_off[h + 1] - slice_off[h] = ceil(len(rows[h]) / slice), slice_off[n_heavy] = n_slices) is planned by the
 *   caller once per CSR.  First launch: grid = (n_slices, pairs (I, J <= I) of 128-column blocks); a workgroup gathers 64 entries' rows
 *   of Y through idx, scales one operand by c_e and multiplies on the fp32-input MFMA, each 64-entry chunk's sums from zero, joined to
 *   the slice's once; partials go to ws (brAlsNormalRowsWorkspaceBytes(n_slices, dim); -1 outside the limits).  Second launch: a row's
 *   slice partials are added in slice order in double and rounded once, H[i][j] and H[j][i] written from the one value; b is summed in
 *   double, in the order of the CSR within a slice and in slice order across slices.  H[h] and b[h] are a function of (the row's
 *   entries in their order, the rows of Y they name, conf, alpha, dim, slice) alone - not of the other listed rows or the grid; two
 *   calls, and the 16-byte and the scalar load paths, give the same bits; no atomics on floats.  An idx outside [0, n_y), or a listed
 *   row outside [0, n_rows), is compared, never used as an address: it sets BR_ERRFLAG_RANGE in *err_flag (may be NULL) and counts as
 *   absent.  A slice_off that promises a row more slices than it has gives zeros for them; fewer, and the row's tail is left out.
 * brAlsSolveRowsDenseCg: the recurrence of brAlsSolveRowsCg, word for word, on A_h = G + reg I + H[h] and b[h], one workgroup per
 *   listed row: x = X0[h] (float32, compact rows of dim), `steps` steps with the same stop rules, Xout[h] (row stride ld_out) = x
 *   rounded to float once.  q = G p + H[h] p + reg p is summed in double in feature order k = 0 .. dim - 1 (thread j owns feature j
 *   and reads column j through the symmetric transpose); x, r, p and the dot products are doubles.  It takes no ids.  Xout[h] is a
 *   function of (G, H[h], b[h], reg, X0[h], steps) alone; two calls give the same bits.
 * Limits: 1 <= dim <= 512, ld >= dim, 1 <= n_y < 2^31 where rows are listed, n_rows, n_heavy, n_slices < 2^31, alpha >= 0 and finite,
 * reg > 0 and finite, 1 <= steps <= 64; BR_ERR_ARG / BR_ERR_WORKSPACE before any launch; n_heavy == 0 is BR_OK; no allocation and no
 * sync inside. */
int64_t brAlsNormalRowsWorkspaceBytes(int64_t n_slices, int dim);
int brAlsNormalRows(const float* Y, int64_t ld_y, int64_t n_y, int dim, const int64_t* off, const int32_t* idx, const float* conf,
                    float alpha, int64_t n_rows, const int32_t* rows, const int64_t* slice_off, int64_t n_heavy, int64_t n_slices,
                    int slice, float* H, double* b, void* ws, int64_t ws_bytes, int* err_flag, brStream stream);
int brAlsSolveRowsDenseCg(const float* G, const float* H, const double* b, int dim, float reg, const float* X0, int64_t n_heavy, int steps,
                          float* Xout, int64_t ld_out, brStream stream);

/* Optional launch probe for measurement (bench.py roofline leg): HIP events on the launch stream
 * around every inner launch of brNeumfStepRun, tagged BR_TAG_*.  brProbeEnable(capacity) creates
 * the events (capacity 0 disables and frees them); after synchronising the stream the host reads
 * record i with brProbeRead (elapsed ms of that launch).  Process-global, not thread-safe. */
enum {
  BR_TAG_EMBED_FWD = 1, BR_TAG_FWD_L1 = 2, BR_TAG_FWD_L2 = 3, BR_TAG_FWD_L3 = 4, BR_TAG_HEAD = 5,
  BR_TAG_BWD_L3 = 6, BR_TAG_BWD_L2 = 7, BR_TAG_BWD_L1 = 8, BR_TAG_EMBED_BWD = 9,
  BR_TAG_INDEX_USER = 10, BR_TAG_INDEX_ITEM = 11, BR_TAG_ADAM_ROWS_USER = 12, BR_TAG_SWEEP_USER = 13,
  BR_TAG_ADAM_ROWS_ITEM = 14, BR_TAG_SWEEP_ITEM = 15, BR_TAG_ADAM_FLAT = 16, BR_TAG_REDUCE = 17,
  BR_TAG_SMALL = 18, BR_TAG_KEEP_BITS = 19, BR_TAG_STEP_STATE = 20,
  BR_TAG_SEG_PARTIALS = 21,   /* first kernel of an ADAM_ROWS_* call */
  BR_TAG_INDEX_SORT = 22      /* first kernel of an INDEX_* call (chunk sort); the rank / merge kernel keeps INDEX_* */
};
int brProbeEnable(int capacity);
int brProbeCount(void);
int brProbeRead(int i, int* tag, float* ms);
/* The same measurement INSIDE a replayed hipGraph, for one tag.  A timed event recorded into a stream capture cannot be read
 * (hipEventElapsedTime: invalid resource handle, ROCm 7.2), an event-record NODE can: while brNeumfStepRun is being captured
 * (hipStreamBeginCapture / torch.cuda.graph), the launch tagged `tag` gets such a node in front and behind
 * (hipStreamGetCaptureInfo_v2 + hipGraphAddEventRecordNode + hipStreamUpdateCaptureDependencies).
 *   brProbeGraphSelect(tag)        before the capture (tag >= 0 forgets earlier nodes; tag < 0: later captures carry none)
 *   brProbeGraphNodes()            after it: record nodes placed (0: that launch was not in the capture)
 *   brProbeGraphEnable(capacity)   event pairs for `capacity` replays (0 frees them)
 *   brProbeGraphArm(exec, slot)    before a replay of the instantiated graph `exec` (hipGraphExec_t): its nodes record into pair `slot`
 *   brProbeGraphRead(slot, &ms)    after synchronising: elapsed ms of the launch in that replay
 * tools/diag/graph_events.cpp is the stand-alone check of the mechanism.  Process-global, not thread-safe. */
int brProbeGraphSelect(int tag);
int brProbeGraphNodes(void);
int brProbeGraphEnable(int capacity);
int brProbeGraphArm(void* graph_exec, int slot);
int brProbeGraphRead(int slot, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* BINREC_H */
