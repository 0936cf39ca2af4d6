"""Thin torch-tensor wrappers over the C-ABI (include/binrec.h).

PyTorch is plumbing here: device memory (`tensor.data_ptr()`), the current HIP stream and,
for the multi-GPU path, `torch.distributed` (RCCL).  All arithmetic happens in
libbinrec_hip.so; nothing in this module computes on the CPU or with torch ops.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check

I32, I64 = 0, 1
ACT = {"linear": 0, "sigmoid": 1, "relu": 2}
LOSS = {"bce": 0, "mse": 1}
STAT_REPLICAS = 8   # BR_STAT_REPLICAS: every BatchNorm column-sum buffer is double[8][2N]


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_DEV_INDEX = None


def _stream() -> int:
    """hipStream_t of torch's current stream on this process' device (one process per GPU).  The raw getter costs ~1 us;
    building a torch.cuda.Stream object per launch was 0.1 ms of a 0.75 ms row-sharded step."""
    global _DEV_INDEX
    if _RAW_STREAM is None:
        return torch.cuda.current_stream().cuda_stream
    if _DEV_INDEX is None:
        _DEV_INDEX = torch.cuda.current_device()
    return _RAW_STREAM(_DEV_INDEX)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _f32(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous float32 device tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")
    return t


def _ids(t, name: str):
    if t is None:
        return None, I32
    if not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: expected contiguous int32/int64 device ids, got {t.dtype} {t.device}")
    return t, (I64 if t.dtype == torch.int64 else I32)


def _same_id_type(*types):
    ts = {t for t in types}
    if len(ts) != 1:
        raise TypeError("all id tensors of one call must share a dtype (int32 or int64)")
    return ts.pop()


def new_err_flag(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def raise_if_flag(flag: torch.Tensor, what="embedding id"):
    """Host sync. Turns the device flag into the IndexError TF-CPU would raise [TF-sem]."""
    v = int(flag.item())
    if v != 0:
        flag.zero_()
        if v & 2:      # BR_ERRFLAG_CAPACITY (brShardDedupPlanPair)
            raise RuntimeError("row-sharded exchange: more DISTINCT ids for one owner than the fixed per-peer capacity in a step (the surplus ids "
                               "were dropped from that step: zeros in the forward, no gradient); raise exchange_capacity or use exchange='exact'")
        raise IndexError(f"{what} out of range")


# ------------------------------------------------------------------------------ G1 / M1
def gather_rows(tables, ids, outs=None, err_flag=None):
    """outs[t] = tables[t][ids[t]] for all t in ONE launch (Embedding lookups)."""
    n = len(tables)
    dim = tables[0].shape[1]
    idt = [_ids(i, "ids") for i in ids]
    id_type = _same_id_type(*[t for _, t in idt])
    batch = ids[0].shape[0] if ids[0] is not None else outs[0].shape[0]
    if outs is None:
        outs = [torch.empty((batch, dim), dtype=torch.float32, device=tables[0].device) for _ in range(n)]
    for t in tables:
        _f32(t, "table")
        if t.shape[1] != dim:
            raise ValueError("gather_rows: all tables must share dim")
    TP = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tables])
    IP = (ctypes.c_void_p * n)(*[_p(i) for i, _ in idt])
    OP = (ctypes.c_void_p * n)(*[_f32(o, "out").data_ptr() for o in outs])
    RW = (ctypes.c_int64 * n)(*[t.shape[0] for t in tables])
    check(_lib.load().brGatherRows(n, TP, RW, IP, OP, dim, batch, id_type, _p(err_flag), _stream()), "brGatherRows")
    return outs


def gather_rows_deferred(table, m, v, last, ids, step_state, beta1=0.9, beta2=0.999, eps=1e-7, out=None, err_flag=None):
    """Lookup on a deferred-Adam table (include/binrec.h "Deferred dense Adam"): rows as of the previous step."""
    t, ty = _ids(ids, "ids")
    n, dim = t.shape[0], table.shape[1]
    if out is None:
        out = torch.empty((n, dim), dtype=torch.float32, device=table.device)
    check(_lib.load().brGatherRowsDeferred(_f32(table, "table").data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), table.shape[0], dim,
                                           t.data_ptr(), ty, n, step_state.data_ptr(), beta1, beta2, eps, out.data_ptr(), out.stride(0),
                                           _p(err_flag), _stream()), "brGatherRowsDeferred")
    return out


def gather_rows_deferred_pair(tab_a, m_a, v_a, last_a, ids_a, out_a, tab_b, m_b, v_b, last_b, ids_b, out_b, step_state, beta1=0.9, beta2=0.999, eps=1e-7,
                              err_flag=None):
    """gather_rows_deferred on two tables of one geometry in one launch (brGatherRowsDeferredPair)."""
    ta, ty = _ids(ids_a, "ids_a"); tb, tyb = _ids(ids_b, "ids_b")
    n, nb, dim = ta.shape[0], tb.shape[0], tab_a.shape[1]
    if ty != tyb or tab_b.shape[1] != dim or out_a.stride(0) != out_b.stride(0) or out_a.shape[0] < n or out_b.shape[0] < nb:
        raise ValueError("gather_rows_deferred_pair: the two gathers must share id type, dim and output stride")
    check(_lib.load().brGatherRowsDeferredPair(_f32(tab_a, "table_a").data_ptr(), m_a.data_ptr(), v_a.data_ptr(), last_a.data_ptr(), tab_a.shape[0], ta.data_ptr(),
                                               _f32(out_a, "out_a").data_ptr(), _f32(tab_b, "table_b").data_ptr(), m_b.data_ptr(), v_b.data_ptr(), last_b.data_ptr(),
                                               tab_b.shape[0], tb.data_ptr(), _f32(out_b, "out_b").data_ptr(), dim, ty, n, nb, step_state.data_ptr(), beta1, beta2, eps,
                                               out_a.stride(0), _p(err_flag), _stream()), "brGatherRowsDeferredPair")
    return out_a, out_b


def gather_rows_deferred_pair_with_index(tab_a, m_a, v_a, last_a, ids_a, out_a, idx_a: "RowIndex", tab_b, m_b, v_b, last_b, ids_b, out_b, idx_b: "RowIndex",
                                         step_state, lr, beta1=0.9, beta2=0.999, eps=1e-7, advance=True, err_flag=None):
    """gather_rows_deferred_pair + both dedup indexes (+ the step-state advance) in two launches on one stream
    (brGatherRowsDeferredPairWithIndex): the chunk sorts ride in the gather's launch."""
    ta, ty = _ids(ids_a, "ids_a"); tb, tyb = _ids(ids_b, "ids_b")
    na, nb, dim = ta.shape[0], tb.shape[0], tab_a.shape[1]
    if ty != tyb or ty != idx_a.id_type or ty != idx_b.id_type or tab_b.shape[1] != dim or out_a.stride(0) != out_b.stride(0) or na > idx_a.capacity or nb > idx_b.capacity:
        raise ValueError("gather_rows_deferred_pair_with_index: id type / dim / stride / capacity mismatch")
    idx_a.n, idx_b.n = na, nb
    check(_lib.load().brGatherRowsDeferredPairWithIndex(
        _f32(tab_a, "table_a").data_ptr(), m_a.data_ptr(), v_a.data_ptr(), last_a.data_ptr(), tab_a.shape[0], ta.data_ptr(), _f32(out_a, "out_a").data_ptr(),
        idx_a.sorted_ids.data_ptr(), idx_a.sorted_pos.data_ptr(), idx_a.ws.data_ptr(), idx_a.ws_bytes,
        _f32(tab_b, "table_b").data_ptr(), m_b.data_ptr(), v_b.data_ptr(), last_b.data_ptr(), tab_b.shape[0], tb.data_ptr(), _f32(out_b, "out_b").data_ptr(),
        idx_b.sorted_ids.data_ptr(), idx_b.sorted_pos.data_ptr(), idx_b.ws.data_ptr(), idx_b.ws_bytes,
        dim, ty, na, nb, step_state.data_ptr(), 1 if advance else 0, float(lr), beta1, beta2, eps, out_a.stride(0), _p(err_flag), _stream()),
        "brGatherRowsDeferredPairWithIndex")
    return out_a, out_b


def adam_rows_sorted_deferred(table, m, v, last, index, row_grads, ldg, step_state, beta1=0.9, beta2=0.999, eps=1e-7,
                              row_grads_hi=None, ldg_hi=0, split=0, replayed=None):
    """replayed: (n, >= dim) rows as this step's gather_rows_deferred wrote them, aligned with the positions the index was built
    on - the optimizer then replays the moments only (brAdamRowsSortedDeferredReplayed)."""
    if replayed is not None:
        check(_lib.load().brAdamRowsSortedDeferredReplayed(table.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), table.shape[0], table.shape[1],
                                                           index.sorted_ids.data_ptr(), index.id_type, index.sorted_pos.data_ptr(), index.n,
                                                           row_grads.data_ptr(), ldg, _p(row_grads_hi), ldg_hi, split, _f32(replayed, "replayed").data_ptr(),
                                                           replayed.stride(0), step_state.data_ptr(), beta1, beta2, eps,
                                                           index.seg_ws(table.shape[1]).data_ptr(), _stream()), "brAdamRowsSortedDeferredReplayed")
        return
    check(_lib.load().brAdamRowsSortedDeferred(table.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(), table.shape[0], table.shape[1],
                                               index.sorted_ids.data_ptr(), index.id_type, index.sorted_pos.data_ptr(), index.n,
                                               row_grads.data_ptr(), ldg, _p(row_grads_hi), ldg_hi, split, step_state.data_ptr(),
                                               beta1, beta2, eps, index.seg_ws(table.shape[1]).data_ptr(), _stream()), "brAdamRowsSortedDeferred")


def adam_rows_sorted_deferred_pair_replayed(tab_a, m_a, v_a, last_a, idx_a, g_a, rep_a, tab_b, m_b, v_b, last_b, idx_b, g_b, rep_b, split, step_state,
                                            beta1=0.9, beta2=0.999, eps=1e-7):
    """two deferred tables of one row width in ONE launch (brAdamRowsSortedPairReplayed): g_x = (n_x, dim) row gradients by position
    (split > 0: [0, split) | [split, dim) read as two halves of the same rows; split = 0: one source), rep_x = the rows as this step's
    deferred gather wrote them, same positions.  The two indexes may differ in length (one wave per row shapes: dim 64 / 128 / 256)."""
    dim = tab_a.shape[1]
    if tab_b.shape[1] != dim or g_a.stride(0) != g_b.stride(0) or rep_a.stride(0) != rep_b.stride(0) or idx_a.id_type != idx_b.id_type:
        raise ValueError("adam_rows_sorted_deferred_pair_replayed: the two tables must share dim, id type and strides")
    ld, ldr = g_a.stride(0), rep_a.stride(0)
    hi_a = g_a.data_ptr() + 4 * split if split else None
    hi_b = g_b.data_ptr() + 4 * split if split else None
    check(_lib.load().brAdamRowsSortedPairReplayed(
        tab_a.data_ptr(), m_a.data_ptr(), v_a.data_ptr(), tab_a.shape[0], idx_a.sorted_ids.data_ptr(), idx_a.sorted_pos.data_ptr(),
        g_a.data_ptr(), ld, hi_a, ld, last_a.data_ptr(), _f32(rep_a, "rep_a").data_ptr(),
        tab_b.data_ptr(), m_b.data_ptr(), v_b.data_ptr(), tab_b.shape[0], idx_b.sorted_ids.data_ptr(), idx_b.sorted_pos.data_ptr(),
        g_b.data_ptr(), ld, hi_b, ld, last_b.data_ptr(), _f32(rep_b, "rep_b").data_ptr(), ldr,
        dim, idx_a.id_type, idx_a.n, idx_b.n if idx_b.n != idx_a.n else 0, split if split else dim, step_state.data_ptr(), beta1, beta2, eps,
        idx_a.seg_ws(dim).data_ptr(), idx_b.seg_ws(dim).data_ptr(), _stream()), "brAdamRowsSortedPairReplayed")


def row_dot(a, b, out=None):
    _f32(a, "a"); _f32(b, "b")
    if out is None:
        out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    check(_lib.load().brRowDot(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[1], a.shape[0], _stream()), "brRowDot")
    return out


def row_dot_backward(a, b, dout, da=None, db=None):
    da = torch.empty_like(a) if da is None else da
    db = torch.empty_like(b) if db is None else db
    check(_lib.load().brRowDotBackward(_f32(a, "a").data_ptr(), _f32(b, "b").data_ptr(), _f32(dout, "dout").data_ptr(),
                                       da.data_ptr(), db.data_ptr(), a.shape[1], a.shape[0], _stream()), "brRowDotBackward")
    return da, db


def neumf_embed_forward(user_mlp, item_mlp, user_mf, item_mf, users, items, item_first, x0, dot, err_flag=None, stash=None):
    """Tables may be separate (row stride = dim) or column views of fused [rows][mlp|mf] allocations.
    stash = (stash_user, stash_item): (B, dim) views of one row stride that receive the two MF rows of every pair (brNeumfEmbedForwardStash)."""
    u, ut = _ids(users, "users"); i, it = _ids(items, "items")
    id_type = _same_id_type(ut, it)
    dim = user_mlp.shape[1]
    batch = x0.shape[0]
    if user_mlp.stride(0) != user_mf.stride(0) or item_mlp.stride(0) != item_mf.stride(0):
        raise ValueError("mlp/mf tables of one stream must share a row stride")
    su, si = stash if stash is not None else (None, None)
    if su is not None and (su.stride(0) != si.stride(0) or su.shape[0] < batch or si.shape[0] < batch):
        raise ValueError("stashes must share a row stride and hold the batch")
    check(_lib.load().brNeumfEmbedForwardStash(user_mlp.data_ptr(), item_mlp.data_ptr(), user_mf.data_ptr(), item_mf.data_ptr(),
                                               user_mlp.stride(0), item_mlp.stride(0), user_mlp.shape[0], item_mlp.shape[0],
                                               _p(u), _p(i), id_type, dim, batch, int(item_first), _f32(x0, "x0").data_ptr(),
                                               _f32(dot, "dot").data_ptr(), _p(su), _p(si), su.stride(0) if su is not None else 0, _p(err_flag), _stream()),
          "brNeumfEmbedForwardStash")


def neumf_embed_backward(user_mf, item_mf, users, items, item_first, dx0, ddot, g_user_mf, g_item_mf,
                         g_user_mlp=None, g_item_mlp=None, out_rows_by_id=False):
    """g_* may be (B, dim) buffers or column views of fused (B, 2*dim) buffers (shared row stride)."""
    u, ut = _ids(users, "users"); i, it = _ids(items, "items")
    id_type = _same_id_type(ut, it)
    dim = user_mf.shape[1]
    batch = ddot.shape[0]
    ldg = g_user_mf.stride(0)
    for t in (g_item_mf, g_user_mlp, g_item_mlp):
        if t is not None and t.stride(0) != ldg:
            raise ValueError("row-gradient outputs must share a row stride")
    check(_lib.load().brNeumfEmbedBackward(user_mf.data_ptr(), item_mf.data_ptr(), user_mf.stride(0), item_mf.stride(0),
                                           user_mf.shape[0], item_mf.shape[0], _p(u), _p(i), id_type, dim, batch,
                                           int(item_first), _p(dx0), _f32(ddot, "ddot").data_ptr(), _p(g_user_mlp),
                                           _p(g_item_mlp), g_user_mf.data_ptr(), g_item_mf.data_ptr(), ldg, 1 if out_rows_by_id else 0, _stream()),
          "brNeumfEmbedBackward")


def mf_grad_inplace(stash_user, stash_item, ddot):
    """(u, i) -> (ddot * i, ddot * u) in place on the MF rows the forward stashed: (B, dim) views of one row stride (brMfGradInplace)."""
    if stash_user.shape != stash_item.shape or stash_user.stride(0) != stash_item.stride(0) or stash_user.shape[0] < ddot.shape[0]:
        raise ValueError("stashes must share a shape and a row stride and hold the batch")
    check(_lib.load().brMfGradInplace(_p(stash_user), _p(stash_item), stash_user.stride(0), _f32(ddot, "ddot").data_ptr(), ddot.shape[0],
                                      stash_user.shape[1], _stream()), "brMfGradInplace")


# ------------------------------------------------------------------------------ L3 BPR
def bpr_forward_backward(user_table, item_table, users, pos, neg, inv_batch, loss_sum, g_user, g_item,
                         per_triplet=None, err_flag=None):
    u, ut = _ids(users, "users"); p, pt = _ids(pos, "pos"); n, nt = _ids(neg, "neg")
    id_type = _same_id_type(ut, pt, nt)
    check(_lib.load().brBprForwardBackward(_f32(user_table, "user_table").data_ptr(), _f32(item_table, "item_table").data_ptr(),
                                           user_table.shape[0], item_table.shape[0], u.data_ptr(), p.data_ptr(), n.data_ptr(),
                                           id_type, user_table.shape[1], u.shape[0], float(inv_batch), _p(per_triplet),
                                           loss_sum.data_ptr(), _f32(g_user, "g_user").data_ptr(),
                                           _f32(g_item, "g_item").data_ptr(), _p(err_flag), _stream()), "brBprForwardBackward")


# ------------------------------------------------------------------------------ S1 index
class RowIndex:
    """Sorted (id, batch position) index of one id stream, reusable by every table fed by it."""

    def __init__(self, capacity: int, id_dtype: torch.dtype, device):
        self.capacity = capacity
        self.id_dtype = id_dtype
        self.id_type = I64 if id_dtype == torch.int64 else I32
        self.sorted_ids = torch.empty(capacity, dtype=id_dtype, device=device)
        self.sorted_pos = torch.empty(capacity, dtype=torch.int32, device=device)
        self.ws_bytes = int(_lib.load().brRowIndexWorkspaceBytes(capacity, self.id_type))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.n = 0
        self._seg = {}

    def seg_ws(self, dim: int):
        """scratch for the two-level ordered duplicate sum (brSegmentScratchFloats): hot ids cost a chain of
        capacity/64 + 64 dependent adds instead of one as long as the segment"""
        t = self._seg.get(dim)
        if t is None:
            t = self._seg[dim] = torch.empty(int(_lib.load().brSegmentScratchFloats(self.capacity, dim)), dtype=torch.float32,
                                             device=self.sorted_ids.device)
        return t

    def build(self, ids: torch.Tensor, id_upper_bound: int = 0):
        t, ty = _ids(ids, "ids")
        if ty != self.id_type or t.shape[0] > self.capacity:
            raise ValueError("RowIndex.build: dtype/capacity mismatch")
        self.n = t.shape[0]
        check(_lib.load().brRowIndexBuild(t.data_ptr(), ty, self.n, int(id_upper_bound), self.sorted_ids.data_ptr(),
                                          self.sorted_pos.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()),
              "brRowIndexBuild")
        return self


class SideIndexes:
    """Dedup indexes built on side streams of their own beside a step's other launches: start() forks them off `main` behind what is
    already on it (the previous step's readers of the indexes), join() makes `main` wait for them.  Streams made once, on first use."""

    def __init__(self, device):
        self.device, self.streams = device, None

    def start(self, main, jobs):
        """jobs: (RowIndex, ids, id upper bound) per side stream"""
        if self.streams is None:
            self.streams = tuple(torch.cuda.Stream(device=self.device) for _ in jobs)
            self.forked, self.built = torch.cuda.Event(), tuple(torch.cuda.Event() for _ in jobs)
        self.forked.record(main)
        for s, built, (idx, ids, upper) in zip(self.streams, self.built, jobs):
            s.wait_event(self.forked)
            with torch.cuda.stream(s):
                idx.build(ids, upper)
                built.record(s)

    def join(self, main):
        for built in self.built:
            main.wait_event(built)


def row_index_build_pair(idx_a: RowIndex, ids_a, upper_a: int, idx_b: RowIndex, ids_b, upper_b: int):
    """both dedup indexes of a step in shared launches (brRowIndexBuildPair); ids of equal length and type."""
    ta, ty = _ids(ids_a, "ids_a"); tb, tyb = _ids(ids_b, "ids_b")
    n = ta.shape[0]
    if ty != tyb or tb.shape[0] != n or ty != idx_a.id_type or ty != idx_b.id_type or n > min(idx_a.capacity, idx_b.capacity):
        raise ValueError("row_index_build_pair: dtype / length / capacity mismatch")
    idx_a.n = idx_b.n = n
    check(_lib.load().brRowIndexBuildPair(ta.data_ptr(), int(upper_a), idx_a.sorted_ids.data_ptr(), idx_a.sorted_pos.data_ptr(), idx_a.ws.data_ptr(), idx_a.ws_bytes,
                                          tb.data_ptr(), int(upper_b), idx_b.sorted_ids.data_ptr(), idx_b.sorted_pos.data_ptr(), idx_b.ws.data_ptr(), idx_b.ws_bytes,
                                          ty, n, _stream()), "brRowIndexBuildPair")


def row_index_build_pair_seg(idx_a: RowIndex, upper_a: int, idx_b: RowIndex, upper_b: int, ids, n: int, seg):
    """both owner-side dedup indexes over the merged id array of the row-sharded exchange ([source][stream][cap]; seg = (seg_len,
    seg_stride, offset a, offset b)): n logical positions per stream, sorted_pos = physical element index (brRowIndexBuildPairSeg)."""
    t, ty = _ids(ids, "ids")
    if ty != idx_a.id_type or ty != idx_b.id_type or n > min(idx_a.capacity, idx_b.capacity):
        raise ValueError("row_index_build_pair_seg: dtype / capacity mismatch")
    idx_a.n = idx_b.n = n
    check(_lib.load().brRowIndexBuildPairSeg(t.data_ptr(), int(upper_a), idx_a.sorted_ids.data_ptr(), idx_a.sorted_pos.data_ptr(), idx_a.ws.data_ptr(), idx_a.ws_bytes,
                                             t.data_ptr(), int(upper_b), idx_b.sorted_ids.data_ptr(), idx_b.sorted_pos.data_ptr(), idx_b.ws.data_ptr(), idx_b.ws_bytes,
                                             ty, n, *[int(v) for v in seg], _stream()), "brRowIndexBuildPairSeg")


def row_index_merge_pair_seg(idx_a: RowIndex, upper_a: int, idx_b: RowIndex, upper_b: int, ids, n: int, seg, err_flag=None):
    """the same two indexes when every segment of `ids` is already sorted ascending (the fixed-capacity exchange delivers each requester's
    distinct rows in key order, pads last): a merge of the per-source runs, no sort (brRowIndexMergePairSeg).  An unsorted segment sets
    BR_ERRFLAG_RANGE in err_flag."""
    t, ty = _ids(ids, "ids")
    if ty != idx_a.id_type or ty != idx_b.id_type or n > min(idx_a.capacity, idx_b.capacity):
        raise ValueError("row_index_merge_pair_seg: dtype / capacity mismatch")
    idx_a.n = idx_b.n = n
    check(_lib.load().brRowIndexMergePairSeg(t.data_ptr(), int(upper_a), idx_a.sorted_ids.data_ptr(), idx_a.sorted_pos.data_ptr(),
                                             t.data_ptr(), int(upper_b), idx_b.sorted_ids.data_ptr(), idx_b.sorted_pos.data_ptr(),
                                             ty, n, *[int(v) for v in seg], _p(err_flag), _stream()), "brRowIndexMergePairSeg")


def gather_rows_deferred_pair_seg(tab_a, m_a, v_a, last_a, tab_b, m_b, v_b, last_b, ids, out, n, seg, step_state, beta1=0.9, beta2=0.999, eps=1e-7, err_flag=None):
    """owner-side lookup of both streams of the merged exchange buffer on deferred tables, one launch: out[p] = row ids[p] of the stream's
    table (as of step - 1) at every physical slot p."""
    t, ty = _ids(ids, "ids")
    dim = tab_a.shape[1]
    check(_lib.load().brGatherRowsDeferredPairSeg(_f32(tab_a, "table_a").data_ptr(), m_a.data_ptr(), v_a.data_ptr(), last_a.data_ptr(), tab_a.shape[0],
                                                  _f32(tab_b, "table_b").data_ptr(), m_b.data_ptr(), v_b.data_ptr(), last_b.data_ptr(), tab_b.shape[0], t.data_ptr(),
                                                  _f32(out, "out").data_ptr(), dim, ty, n, *[int(v) for v in seg], step_state.data_ptr(), beta1, beta2, eps,
                                                  out.stride(0), _p(err_flag), _stream()), "brGatherRowsDeferredPairSeg")
    return out


def gather_rows_pair_seg(tab_a, tab_b, ids, out, n, seg, err_flag=None):
    """the same on plain tables (brGatherRowsPairSeg)."""
    t, ty = _ids(ids, "ids")
    check(_lib.load().brGatherRowsPairSeg(_f32(tab_a, "table_a").data_ptr(), tab_a.shape[0], _f32(tab_b, "table_b").data_ptr(), tab_b.shape[0], t.data_ptr(),
                                          _f32(out, "out").data_ptr(), tab_a.shape[1], ty, n, *[int(v) for v in seg], out.stride(0), _p(err_flag), _stream()),
          "brGatherRowsPairSeg")
    return out


def segment_sum_rows(index: RowIndex, row_grads, dim=None, ldg=None, out=None, head_flag=None, two_level=True):
    dim = row_grads.shape[1] if dim is None else dim
    ldg = row_grads.stride(0) if ldg is None else ldg
    if out is None:
        out = torch.zeros((index.n, dim), dtype=torch.float32, device=row_grads.device)
    if head_flag is None:
        head_flag = torch.empty(index.n, dtype=torch.int32, device=row_grads.device)
    check(_lib.load().brSegmentSumRows(index.sorted_ids.data_ptr(), index.id_type, index.sorted_pos.data_ptr(), index.n,
                                       row_grads.data_ptr(), ldg, dim, out.data_ptr(), head_flag.data_ptr(),
                                       index.seg_ws(dim).data_ptr() if two_level else None, _stream()),
          "brSegmentSumRows")
    return out, head_flag


def scatter_add_rows(g_table, ids, rows, err_flag=None):
    t, ty = _ids(ids, "ids")
    check(_lib.load().brScatterAddRows(_f32(g_table, "g_table").data_ptr(), g_table.shape[0], t.data_ptr(), ty, t.shape[0],
                                       _f32(rows, "rows").data_ptr(), g_table.shape[1], _p(err_flag), _stream()),
          "brScatterAddRows")


# ------------------------------------------------------------------------------ O1 / O2
def adam_rows_sorted(table, m, v, index: RowIndex, row_grads, ldg, alpha_t, beta1=0.9, beta2=0.999, eps=1e-7, mark=None,
                     row_grads_hi=None, ldg_hi=0, split=0):
    check(_lib.load().brAdamRowsSorted(_f32(table, "table").data_ptr(), _f32(m, "m").data_ptr(), _f32(v, "v").data_ptr(),
                                       table.shape[0], table.shape[1], index.sorted_ids.data_ptr(), index.id_type,
                                       index.sorted_pos.data_ptr(), index.n, row_grads.data_ptr(), int(ldg), _p(row_grads_hi),
                                       int(ldg_hi), int(split), float(alpha_t), float(beta1), float(beta2), float(eps),
                                       _p(mark), index.seg_ws(table.shape[1]).data_ptr(), _stream()), "brAdamRowsSorted")


def adam_rows_sorted_pair(tab_a, m_a, v_a, idx_a: RowIndex, g_a, ldg_a, hi_a, ldg_hi_a, tab_b, m_b, v_b, idx_b: RowIndex, g_b, ldg_b, hi_b, ldg_hi_b,
                          split, alpha_t, beta1=0.9, beta2=0.999, eps=1e-7, hi_scale=None, mark_a=None, mark_b=None):
    """two swept tables of one row width in ONE launch (brAdamRowsSortedPair): columns [0, split) of table x take their gradients from g_x,
    [split, dim) from hi_x times hi_scale[position] (n floats, or None: as stored); both indexes hold the same number of positions."""
    dim = tab_a.shape[1]
    if tab_b.shape[1] != dim or idx_a.id_type != idx_b.id_type or idx_a.n != idx_b.n:
        raise ValueError("adam_rows_sorted_pair: the two tables must share dim, id type and the number of positions")
    check(_lib.load().brAdamRowsSortedPair(
        _f32(tab_a, "tab_a").data_ptr(), _f32(m_a, "m_a").data_ptr(), _f32(v_a, "v_a").data_ptr(), tab_a.shape[0], idx_a.sorted_ids.data_ptr(),
        idx_a.sorted_pos.data_ptr(), g_a.data_ptr(), int(ldg_a), hi_a.data_ptr(), int(ldg_hi_a), _p(mark_a), None,
        _f32(tab_b, "tab_b").data_ptr(), _f32(m_b, "m_b").data_ptr(), _f32(v_b, "v_b").data_ptr(), tab_b.shape[0], idx_b.sorted_ids.data_ptr(),
        idx_b.sorted_pos.data_ptr(), g_b.data_ptr(), int(ldg_b), hi_b.data_ptr(), int(ldg_hi_b), _p(mark_b), None,
        dim, idx_a.id_type, idx_a.n, int(split), _p(hi_scale), None, float(alpha_t), float(beta1), float(beta2), float(eps),
        idx_a.seg_ws(dim).data_ptr(), idx_b.seg_ws(dim).data_ptr(), _stream()), "brAdamRowsSortedPair")


def adam_dense_sweep(table, m, v, alpha_t, beta1=0.9, beta2=0.999, eps=1e-7, mark=None):
    check(_lib.load().brAdamDenseSweep(_f32(table, "table").data_ptr(), _f32(m, "m").data_ptr(), _f32(v, "v").data_ptr(),
                                       table.shape[0], table.shape[1], float(alpha_t), float(beta1), float(beta2), float(eps),
                                       _p(mark), _stream()), "brAdamDenseSweep")


def adam_flat(theta, m, v, g, alpha_t, beta1=0.9, beta2=0.999, eps=1e-7):
    check(_lib.load().brAdamFlat(_f32(theta, "theta").data_ptr(), _f32(m, "m").data_ptr(), _f32(v, "v").data_ptr(),
                                 _f32(g, "g").data_ptr(), theta.numel(), float(alpha_t), float(beta1), float(beta2), float(eps),
                                 _stream()), "brAdamFlat")


def adagrad_rows_sorted(table, acc, index: RowIndex, row_grads, ldg, lr, eps=1e-7):
    check(_lib.load().brAdagradRowsSorted(_f32(table, "table").data_ptr(), _f32(acc, "acc").data_ptr(), table.shape[0],
                                          table.shape[1], index.sorted_ids.data_ptr(), index.id_type,
                                          index.sorted_pos.data_ptr(), index.n, row_grads.data_ptr(), int(ldg), float(lr),
                                          float(eps), index.seg_ws(table.shape[1]).data_ptr(), _stream()), "brAdagradRowsSorted")


def adagrad_flat(theta, acc, g, lr, eps=1e-7):
    check(_lib.load().brAdagradFlat(_f32(theta, "theta").data_ptr(), _f32(acc, "acc").data_ptr(), _f32(g, "g").data_ptr(),
                                    theta.numel(), float(lr), float(eps), _stream()), "brAdagradFlat")


REPLAY = {"exact": 0, "fast": 1}     # BR_REPLAY_EXACT / BR_REPLAY_FAST


def new_step_state(device, beta1=0.9, beta2=0.999, eps=1e-7, replay="fast") -> torch.Tensor:
    """The device step state of a deferred-Adam engine (brStepStateBytes): zeroed, with the replay form written into it
    (brStepStateInit: "fast" = the cheaper recurrence, "exact" = the sweep's own operations, bit-equal tables)."""
    st = torch.zeros(int(_lib.load().brStepStateBytes()) // 4, dtype=torch.int32, device=device)
    check(_lib.load().brStepStateInit(st.data_ptr(), float(beta1), float(beta2), float(eps), REPLAY[replay], _stream()), "brStepStateInit")
    return st


def adam_alpha(lr: float, t: int, beta1=0.9, beta2=0.999) -> float:
    """[TF-sem] alpha_t = lr*sqrt(1-b2^t)/(1-b1^t) in double on the host."""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


# ------------------------------------------------------------------------------ T1-T4 MLP tower
def dropout_keep_words(batch, K) -> int:
    return int(_lib.load().brDropoutKeepWords(batch, K))


def dropout_keep_bits(drop_p, seed, step, row0, batch, sites, widths, outs=None):
    """T4: the Philox keep-bit planes of up to three dropout sites in one launch (uint32 [batch][ceil(K/32)] each)."""
    n = len(sites)
    if outs is None:
        dev = torch.device("cuda", torch.cuda.current_device())
        outs = [torch.empty(dropout_keep_words(batch, k), dtype=torch.int32, device=dev) for k in widths]
    S = (ctypes.c_uint32 * n)(*[int(s) for s in sites])
    Wd = (ctypes.c_int * n)(*[int(k) for k in widths])
    OP = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    check(_lib.load().brDropoutKeepBits(float(drop_p), int(seed), int(step), int(row0), int(batch), n, S, Wd, OP, _stream()), "brDropoutKeepBits")
    return outs


def dense_forward(x, W, bias, y, act, in_scale=None, in_shift=None, drop_p=0.0, seed=0, step=0, site=0, row0=0,
                  stats=None, batch=None, keep=None):
    """keep: the site's bit plane (dropout_keep_bits); built here from (seed, step, site, row0) when drop_p > 0 and it is None."""
    B = x.shape[0] if batch is None else batch
    K, N = W.shape
    if drop_p > 0 and keep is None and B > 0:
        keep = dropout_keep_bits(drop_p, seed, step, row0, B, [site], [K])[0]
    check(_lib.load().brDenseForward(x.data_ptr(), x.stride(0), _f32(W, "W").data_ptr(), _p(bias), y.data_ptr(), y.stride(0),
                                     B, K, N, ACT[act], _p(in_scale), _p(in_shift), None, float(drop_p), _p(keep) if drop_p > 0 else 0,
                                     _p(stats), _stream()), "brDenseForward")


def bn_finalize(stats, batch_total, gamma, beta, eps, momentum, moving_mean, moving_var, scale, shift, mean, rstd):
    check(_lib.load().brBnFinalize(stats.data_ptr(), float(batch_total), gamma.data_ptr(), beta.data_ptr(), float(eps),
                                   float(momentum), _p(moving_mean), _p(moving_var), scale.data_ptr(), shift.data_ptr(),
                                   mean.data_ptr(), rstd.data_ptr(), gamma.numel(), _stream()), "brBnFinalize")


def bn_inference(gamma, beta, moving_mean, moving_var, eps, scale, shift):
    check(_lib.load().brBnInference(gamma.data_ptr(), beta.data_ptr(), moving_mean.data_ptr(), moving_var.data_ptr(),
                                    float(eps), scale.data_ptr(), shift.data_ptr(), gamma.numel(), _stream()), "brBnInference")


def dense_backward_slabs(batch, K, N) -> int:
    return int(_lib.load().brDenseBackwardSlabs(batch, K, N))


def dense_backward_ws_floats(batch, K, N) -> int:
    return int(_lib.load().brDenseBackwardWorkspaceFloats(batch, K, N))


def dense_backward(gy, y, x, W, act, slabs, n_slabs, gx=None, out_bn=None, bn_sums=None, batch_total=None,
                   in_scale=None, in_shift=None, in_bn=None, in_drop_p=0.0, in_site=0, seed=0, step=0, row0=0,
                   in_bn_sums=None, batch=None, dz_ws=None, keep=None):
    """out_bn = (mean, rstd, gamma) of the BN after this layer; in_bn = (mean, rstd) of the BN before it.
    keep: bit plane of the input dropout; built from (seed, step, in_site, row0) when in_drop_p > 0 and it is None."""
    B = gy.shape[0] if batch is None else batch
    K, N = W.shape
    om, ors, og = out_bn if out_bn is not None else (None, None, None)
    im, irs = in_bn if in_bn is not None else (None, None)
    if dz_ws is None:
        dz_ws = torch.empty(dense_backward_ws_floats(B, K, N), dtype=torch.float32, device=gy.device)
    if in_drop_p > 0 and keep is None and B > 0:
        keep = dropout_keep_bits(in_drop_p, seed, step, row0, B, [in_site], [K])[0]
    check(_lib.load().brDenseBackward(gy.data_ptr(), gy.stride(0), y.data_ptr(), y.stride(0), x.data_ptr(), x.stride(0),
                                      W.data_ptr(), B, K, N, ACT[act], _p(om), _p(ors), _p(og), _p(bn_sums),
                                      float(batch_total if batch_total is not None else B), _p(in_scale), _p(in_shift),
                                      _p(im), _p(irs), float(in_drop_p), _p(keep) if in_drop_p > 0 else 0,
                                      _p(gx), gx.stride(0) if gx is not None else 0, dz_ws.data_ptr(), slabs.data_ptr(), int(n_slabs),
                                      _p(in_bn_sums), _stream()), "brDenseBackward")


def reduce_slabs(slabs, n_slabs, slab_elems, out):
    check(_lib.load().brReduceSlabs(slabs.data_ptr(), int(n_slabs), int(slab_elems), out.data_ptr(), _stream()), "brReduceSlabs")


def bn_param_grads(bn_sums, dgamma, dbeta):
    check(_lib.load().brBnParamGrads(bn_sums.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), dgamma.numel(), _stream()),
          "brBnParamGrads")


def bn_param_grads_pair(bn_sums_a, dgamma_a, dbeta_a, bn_sums_b, dgamma_b, dbeta_b):
    """bn_param_grads of two BatchNorms (the two of a tower) in one launch."""
    check(_lib.load().brBnParamGradsPair(bn_sums_a.data_ptr(), dgamma_a.data_ptr(), dbeta_a.data_ptr(), dgamma_a.numel(),
                                         bn_sums_b.data_ptr(), dgamma_b.data_ptr(), dbeta_b.data_ptr(), dgamma_b.numel(), _stream()),
          "brBnParamGradsPair")


def dense_finalize(regions, bn_blocks, grad, theta=None, m=None, v=None, alpha_t=0.0, beta1=0.9, beta2=0.999, eps=1e-7):
    """End of the dense backward in one launch (brDenseFinalize): reduce_slabs of three regions, bn_param_grads of two BatchNorms and
    adam_flat on the flat vector.  regions: three (slabs, n_slabs, elems, grad_off); bn_blocks: two (bn_sums, N, dgamma_off, dbeta_off),
    bn_sums = double [STAT_REPLICAS][2N]; together they cover grad[0:n] exactly once.  theta, m, v: all three (Adam with the new
    gradient) or none (gradients only: the data-parallel host all-reduces `grad` before its optimizer)."""
    if len(regions) != 3 or len(bn_blocks) != 2:
        raise ValueError("dense_finalize: three slab regions and two BatchNorm blocks")
    if len({theta is None, m is None, v is None}) != 1:
        raise ValueError("dense_finalize: theta, m and v go together (all three or none)")
    n = _f32(grad, "grad").numel()
    for name, t in (("theta", theta), ("m", m), ("v", v)):
        if t is not None and _f32(t, name).numel() != n:
            raise ValueError(f"dense_finalize: {name} has {t.numel()} elements, grad {n}")
    for s, ns, el, _ in regions:
        if _f32(s, "slabs").numel() < int(ns) * int(el):
            raise ValueError("dense_finalize: a slab buffer is shorter than n_slabs x elems")
    for s, N, _, _ in bn_blocks:
        if s.dtype != torch.float64 or not s.is_cuda or not s.is_contiguous() or s.numel() < STAT_REPLICAS * 2 * int(N):
            raise TypeError("dense_finalize: bn_sums is a contiguous float64 device tensor [STAT_REPLICAS][2N]")
    SP = (ctypes.c_void_p * 3)(*[r[0].data_ptr() for r in regions])
    NS = (ctypes.c_int * 3)(*[int(r[1]) for r in regions])
    EL = (ctypes.c_int64 * 3)(*[int(r[2]) for r in regions])
    GO = (ctypes.c_int64 * 3)(*[int(r[3]) for r in regions])
    BS = (ctypes.c_void_p * 2)(*[b[0].data_ptr() for b in bn_blocks])
    BN = (ctypes.c_int * 2)(*[int(b[1]) for b in bn_blocks])
    DG = (ctypes.c_int64 * 2)(*[int(b[2]) for b in bn_blocks])
    DB = (ctypes.c_int64 * 2)(*[int(b[3]) for b in bn_blocks])
    check(_lib.load().brDenseFinalize(SP, NS, EL, GO, BS, BN, DG, DB, _p(theta), _p(m), _p(v), grad.data_ptr(), n, float(alpha_t), float(beta1),
                                      float(beta2), float(eps), _stream()), "brDenseFinalize")


def head_slabs(batch) -> int:
    return int(_lib.load().brHeadSlabs(batch))


def neumf_head(a3, dot, labels, w4, b4, mf_first, loss, inv_batch, logit=None, prob=None, sums=None, da3=None, ddot=None,
               slabs=None, n_slabs=0, batch=None):
    B = dot.shape[0] if batch is None else batch
    check(_lib.load().brNeumfHead(a3.data_ptr(), a3.stride(0), dot.data_ptr(), _p(labels), w4.data_ptr(), b4.data_ptr(), B,
                                  a3.shape[1], int(mf_first), LOSS[loss], float(inv_batch), _p(logit), _p(prob), _p(sums),
                                  _p(da3), da3.stride(0) if da3 is not None else 0, _p(ddot), _p(slabs), int(n_slabs),
                                  _stream()), "brNeumfHead")


def neumf_tail_slabs(batch) -> int:
    return int(_lib.load().brNeumfTailSlabs(batch))


def neumf_tail_slab_elems(n2, n3) -> int:
    return int(_lib.load().brNeumfTailSlabElems(n2, n3))


_BN_FOLD = None


def _bn_fold(stats, batch_total, gamma, beta, eps, momentum, moving_mean, moving_var, scale, shift, mean, rstd):
    """brBnFold (include/binrec.h) from tensors, field order as in the header."""
    global _BN_FOLD
    if _BN_FOLD is None:
        _BN_FOLD = type("brBnFold", (ctypes.Structure,), {"_fields_": _lib.parse_struct("brBnFold")})
    return _BN_FOLD(stats.data_ptr(), float(batch_total), gamma.data_ptr(), beta.data_ptr(), float(eps), float(momentum), _p(moving_mean) or None,
                    _p(moving_var) or None, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr())


def neumf_tail_fused(a2, W3, b3, w4, b4, dot, labels, act, mf_first, loss, inv_batch, logit, prob, ddot, gh2, scale2=None, shift2=None,
                     mean2=None, rstd2=None, bn2=None, drop_p=0.0, keep=None, a3=None, sums=None, bn_sums=None, slabs=None, batch=None):
    """brNeumfTailFused.  a2 / gh2: (B, n2) views whose row strides go in as lda2 / ldgh2.  BatchNorm 2 either as the four vectors
    scale2/shift2/mean2/rstd2 or as bn2 = (stats, batch_total, gamma, beta, eps, momentum, moving_mean, moving_var, scale, shift, mean,
    rstd) (the fields of brBnFold; the moving statistics may both be None).  keep: the bit plane of dropout site 2 (dropout_keep_bits),
    exactly when drop_p > 0.  slabs=None allocates brNeumfTailSlabs(B) x brNeumfTailSlabElems(n2, n3) floats.
    -> (slabs, n_slabs), to be reduced by reduce_slabs into [dW3 | db3 | dW4 | db4]."""
    B = dot.shape[0] if batch is None else batch
    n2, n3 = W3.shape
    n_slabs = neumf_tail_slabs(B)
    if slabs is None:
        slabs = torch.empty(n_slabs * neumf_tail_slab_elems(n2, n3), dtype=torch.float32, device=dot.device)
    fold = _bn_fold(*bn2) if bn2 is not None else None
    check(_lib.load().brNeumfTailFused(a2.data_ptr(), a2.stride(0), _f32(W3, "W3").data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(),
                                       dot.data_ptr(), labels.data_ptr(), _p(scale2), _p(shift2), _p(mean2), _p(rstd2),
                                       ctypes.byref(fold) if fold is not None else None, float(drop_p), _p(keep) if drop_p > 0 else 0, B, n2, n3,
                                       ACT[act], int(mf_first), LOSS[loss], float(inv_batch), _p(a3), logit.data_ptr(), prob.data_ptr(), _p(sums),
                                       ddot.data_ptr(), gh2.data_ptr(), gh2.stride(0), _p(bn_sums), slabs.data_ptr(), n_slabs, _stream()),
          "brNeumfTailFused")
    return slabs, n_slabs


def bce_logits(z, y, inv_batch, prob=None, dz=None, sums=None):
    check(_lib.load().brBceLogits(z.data_ptr(), y.data_ptr(), z.shape[0], float(inv_batch), _p(prob), _p(dz), _p(sums),
                                  _stream()), "brBceLogits")


# ------------------------------------------------------------------------------ L4 in-batch softmax / E1 scoring + top-k
SUM_SLOTS = 64   # BR_SUM_SLOTS
METRIC_SUMS = 8  # BR_METRIC_SUMS: [loss, se, ae, correct, bce, tp, fp, fn]


_softmax_ws = {}


def _softmax_workspace(Q, C, hard_m=None):
    """scratch of the split in-batch softmax sweeps, one grow-only buffer per (device, stream).  hard_m: the threshold sweep of M hard
    negatives (its per-split key lists; never less than the plain count)."""
    if hard_m is None:
        need = int(_lib.load().brInBatchSoftmaxWorkspaceBytes(Q.shape[0], C.shape[0], Q.shape[1]))
    else:
        need = int(_lib.load().brInBatchSoftmaxHardWorkspaceBytes(Q.shape[0], C.shape[0], Q.shape[1], int(hard_m)))
    key = (Q.device, _stream())
    buf = _softmax_ws.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, 16), dtype=torch.uint8, device=Q.device)
        _softmax_ws[key] = buf
    return buf


MAX_HARD_NEGATIVES = 64


def _thr(thr, Bq):
    """thr = (thr_score float32 (Bq), thr_pos int32 (Bq)) of inbatch_softmax_hard_threshold -> the two pointers"""
    ts, tp = thr
    if ts.dtype != torch.float32 or tp.dtype != torch.int32 or not ts.is_contiguous() or not tp.is_contiguous() or ts.shape[0] != Bq or tp.shape[0] != Bq:
        raise ValueError("thr = (thr_score float32, thr_pos int32), contiguous, one entry per query")
    return ts.data_ptr(), tp.data_ptr()


def _logq(logq, Bc):
    """logq = log of the clipped sampling probability of every candidate ROW of the C that is passed (float32, Bc) -> its pointer"""
    if logq.dtype != torch.float32 or not logq.is_contiguous() or logq.numel() != Bc:
        raise ValueError("logq: float32, contiguous, one entry per candidate row")
    return logq.data_ptr()


def _thr_or_null(thr, Bq):
    return (None, None) if thr is None else _thr(thr, Bq)


def inbatch_softmax_hard_threshold(Q, C, q_pos_ids, cand_ids, diag_offset, num_hard_negatives, thr_score, thr_pos, logq=None):
    """Per query the key (masked score, column) of the last of its num_hard_negatives (1..64) best negatives by (score descending,
    column ascending) -> thr_score float32 (Bq), thr_pos int32 (Bq); (-inf, INT32_MAX) where nothing is cut.  The pair is the
    thr= argument of the three wrappers below, which then run over the partner and those negatives only.
    logq= (here and below): the log-Q correction, scores Q.C - logq[column] before the mask and the selection; every
    sweep of one step takes the same logq."""
    qi, qt = _ids(q_pos_ids, "q_pos_ids"); ci, ct = _ids(cand_ids, "cand_ids")
    id_type = _same_id_type(qt, ct) if qi is not None else I32
    ws = _softmax_workspace(Q, C, hard_m=num_hard_negatives)
    tsp, tpp = _thr((thr_score, thr_pos), Q.shape[0])
    if logq is not None:
        check(_lib.load().brInBatchSoftmaxHardThresholdLogQ(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                            Q.shape[1], int(diag_offset), int(num_hard_negatives), tsp, tpp, _logq(logq, C.shape[0]),
                                                            ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxHardThresholdLogQ")
        return
    check(_lib.load().brInBatchSoftmaxHardThreshold(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                    Q.shape[1], int(diag_offset), int(num_hard_negatives), tsp, tpp, ws.data_ptr(), ws.numel(), _stream()),
          "brInBatchSoftmaxHardThreshold")


def inbatch_softmax_lse(Q, C, q_pos_ids, cand_ids, diag_offset, row_lse, loss_sum, thr=None, logq=None):
    qi, qt = _ids(q_pos_ids, "q_pos_ids"); ci, ct = _ids(cand_ids, "cand_ids")
    id_type = _same_id_type(qt, ct) if qi is not None else I32
    ws = _softmax_workspace(Q, C)
    if logq is not None:
        tsp, tpp = _thr_or_null(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxLseLogQ(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                  Q.shape[1], int(diag_offset), _f32(row_lse, "row_lse").data_ptr(), loss_sum.data_ptr(), tsp, tpp,
                                                  _logq(logq, C.shape[0]), ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxLseLogQ")
        return
    if thr is not None:
        tsp, tpp = _thr(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxLseHard(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                  Q.shape[1], int(diag_offset), _f32(row_lse, "row_lse").data_ptr(), loss_sum.data_ptr(), tsp, tpp,
                                                  ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxLseHard")
        return
    check(_lib.load().brInBatchSoftmaxLse(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                          Q.shape[1], int(diag_offset), _f32(row_lse, "row_lse").data_ptr(), loss_sum.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxLse")


def inbatch_softmax_lse_grad_q(Q, C, q_pos_ids, cand_ids, diag_offset, row_lse, loss_sum, dQ, thr=None, logq=None):
    """lse + loss + dQ in one sweep (online softmax): the training step's first softmax pass."""
    qi, qt = _ids(q_pos_ids, "q_pos_ids"); ci, ct = _ids(cand_ids, "cand_ids")
    id_type = _same_id_type(qt, ct) if qi is not None else I32
    ws = _softmax_workspace(Q, C)
    if logq is not None:
        tsp, tpp = _thr_or_null(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxLseGradQLogQ(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                       Q.shape[1], int(diag_offset), _f32(row_lse, "row_lse").data_ptr(), loss_sum.data_ptr(),
                                                       _f32(dQ, "dQ").data_ptr(), tsp, tpp, _logq(logq, C.shape[0]), ws.data_ptr(), ws.numel(), _stream()),
              "brInBatchSoftmaxLseGradQLogQ")
        return
    if thr is not None:
        tsp, tpp = _thr(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxLseGradQHard(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                       Q.shape[1], int(diag_offset), _f32(row_lse, "row_lse").data_ptr(), loss_sum.data_ptr(),
                                                       _f32(dQ, "dQ").data_ptr(), tsp, tpp, ws.data_ptr(), ws.numel(), _stream()),
              "brInBatchSoftmaxLseGradQHard")
        return
    check(_lib.load().brInBatchSoftmaxLseGradQ(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                               Q.shape[1], int(diag_offset), _f32(row_lse, "row_lse").data_ptr(), loss_sum.data_ptr(),
                                               _f32(dQ, "dQ").data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxLseGradQ")


def inbatch_softmax_grad(Q, C, q_pos_ids, cand_ids, diag_offset, row_lse, dQ=None, dC=None, thr=None, thr_slice=None, logq=None):
    """thr: the hard form (inbatch_softmax_hard_threshold on the same Q and C).  thr_slice = (c0, Bc_total): C and cand_ids are rows
    [c0, c0 + Bc) of the Bc_total candidates the thresholds were taken over (dC only; diag_offset relative to the slice, thr as the
    threshold sweep wrote it) - the arithmetic then follows Bc_total, as the sweep that formed the keys.
    logq: the log-Q form; with thr_slice it is the slice form (logq of the slice's rows; thr may then be None: the plain softmax)."""
    qi, qt = _ids(q_pos_ids, "q_pos_ids"); ci, ct = _ids(cand_ids, "cand_ids")
    id_type = _same_id_type(qt, ct) if qi is not None else I32
    ws = _softmax_workspace(Q, C)
    if logq is not None:
        if thr_slice is not None and (dQ is not None or dC is None):
            raise ValueError("thr_slice computes dC only")
        c0, total = (0, C.shape[0]) if thr_slice is None else (int(thr_slice[0]), int(thr_slice[1]))
        tsp, tpp = _thr_or_null(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxGradLogQ(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                   Q.shape[1], int(diag_offset), row_lse.data_ptr(), _p(dQ), _p(dC), tsp, tpp, _logq(logq, C.shape[0]),
                                                   c0, total, ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxGradLogQ")
        return
    if thr_slice is not None:
        if thr is None or dQ is not None or dC is None:
            raise ValueError("thr_slice goes with thr and computes dC only")
        tsp, tpp = _thr(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxGradHardSlice(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                        Q.shape[1], int(diag_offset), row_lse.data_ptr(), _p(dC), tsp, tpp, int(thr_slice[0]), int(thr_slice[1]),
                                                        ws.data_ptr(), ws.numel(), _stream()), "brInBatchSoftmaxGradHardSlice")
        return
    if thr is not None:
        tsp, tpp = _thr(thr, Q.shape[0])
        check(_lib.load().brInBatchSoftmaxGradHard(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                                   Q.shape[1], int(diag_offset), row_lse.data_ptr(), _p(dQ), _p(dC), tsp, tpp, ws.data_ptr(), ws.numel(),
                                                   _stream()), "brInBatchSoftmaxGradHard")
        return
    check(_lib.load().brInBatchSoftmaxGrad(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), _p(qi), _p(ci), id_type, Q.shape[0], C.shape[0],
                                           Q.shape[1], int(diag_offset), row_lse.data_ptr(), _p(dQ), _p(dC), ws.data_ptr(), ws.numel(), _stream()),
          "brInBatchSoftmaxGrad")


def score_matrix(Q, C, out=None):
    if out is None:
        out = torch.empty(Q.shape[0], C.shape[0], dtype=torch.float32, device=Q.device)
    check(_lib.load().brScoreMatrix(_f32(Q, "Q").data_ptr(), _f32(C, "C").data_ptr(), Q.shape[0], C.shape[0], Q.shape[1], out.data_ptr(),
                                    out.stride(0), _stream()), "brScoreMatrix")
    return out


def topk_rows(scores, k, exclude=None):
    """stable top-k per row: descending, ties keep the lower column (topKmetrics.py:59,68).  exclude = (off, idx), the CSR of
    truth_csr over the rows: those columns are never returned and slots past the remaining columns are (-inf, -1)
    (brTopKRowsExclude); exclude=None keeps brTopKRows."""
    U, I = scores.shape
    os_ = torch.empty(U, k, dtype=torch.float32, device=scores.device)
    oi = torch.empty(U, k, dtype=torch.int32, device=scores.device)
    if exclude is None:
        check(_lib.load().brTopKRows(_f32(scores, "scores").data_ptr(), U, I, int(k), os_.data_ptr(), oi.data_ptr(), _stream()), "brTopKRows")
        return os_, oi
    off, idx = _csr(exclude, U, "exclude")
    check(_lib.load().brTopKRowsExclude(_f32(scores, "scores").data_ptr(), U, I, int(k), off.data_ptr(), idx.data_ptr(), os_.data_ptr(),
                                        oi.data_ptr(), _stream()), "brTopKRowsExclude")
    return os_, oi


def _csr(csr, n_rows: int, name: str):
    off, idx = csr
    if (off.dtype != torch.int64 or idx.dtype != torch.int32 or not off.is_cuda or not idx.is_cuda or not off.is_contiguous()
            or not idx.is_contiguous() or off.dim() != 1 or off.shape[0] != n_rows + 1):
        raise TypeError(f"{name}: expected (off int64 [{n_rows + 1}], idx int32) contiguous device tensors (ops.truth_csr)")
    if idx.numel() == 0:          # a valid pointer for an empty list
        idx = torch.zeros(1, dtype=torch.int32, device=off.device)
    return off, idx


# ------------------------------------------------------------------------------ NeuMF catalogue top-k (csrc/recommend.hip)
def neumf_catalog_fold(theta, moving, n1: int, n2: int, n3: int, mf_first: int, bn_eps: float, out=None):
    """theta / moving: the engine's named views (W2 b2 g1 be1 W3 b3 g2 be2 W4 b4; mm1 mv1 mm2 mv2) -> the folded tower (BatchNorm into the
    next layer, head in a fixed order) that neumf_catalog_topk reads."""
    lib = _lib.load()
    n = int(lib.brNeumfCatalogTowerFloats(n1, n2, n3))
    if n < 0:
        raise ValueError(f"tower widths n1, n2 <= 128 and n3 <= 32 (got {n1}, {n2}, {n3})")
    dev = theta["W2"].device
    out = torch.empty(n, dtype=torch.float32, device=dev) if out is None else out
    t = [_f32(theta[k], k) for k in ("W2", "b2", "g1", "be1")] + [_f32(moving[k], k) for k in ("mm1", "mv1")]
    t += [_f32(theta[k], k) for k in ("W3", "b3", "g2", "be2")] + [_f32(moving[k], k) for k in ("mm2", "mv2")]
    t += [_f32(theta[k], k) for k in ("W4", "b4")]
    check(lib.brNeumfCatalogFold(*[x.data_ptr() for x in t], n1, n2, n3, int(mf_first), float(bn_eps), out.data_ptr(), _stream()),
          "brNeumfCatalogFold")
    return out


def neumf_catalog_project(table, ids, W1, n1: int, dim: int, item_first: int, user_side: bool, b1=None, col_major=False, err_flag=None):
    """[mlp | mf] rows of `ids` -> (len(ids) x (n1 + dim)) row-major, or ((n1 + dim) x len(ids)) with col_major: the row's half of the first
    layer (+ b1) followed by its mf half."""
    ids, id_type = _ids(ids, "ids")
    n = ids.shape[0]
    out = torch.empty((n1 + dim, n) if col_major else (n, n1 + dim), dtype=torch.float32, device=table.device)
    check(_lib.load().brNeumfCatalogProject(_f32(table, "table").data_ptr(), table.stride(0), table.shape[0], ids.data_ptr(), id_type, n, dim,
                                            _f32(W1, "W1").data_ptr(), n1, int(item_first), int(bool(user_side)), _p(b1), 1,
                                            out.data_ptr(), out.stride(0), int(bool(col_major)), _p(err_flag), _stream()),
          "brNeumfCatalogProject")
    return out


def neumf_catalog_topk(pu, pit, tower, dim: int, hidden, act: str, k: int, exclude=None, dump_logits=False, dump_probs=False):
    """pu (U x (n1 + dim)) and pit ((n1 + dim) x I) from neumf_catalog_project, tower from neumf_catalog_fold -> (scores (U, k) float32,
    index (U, k) int32 positions into the item list) [, logits (U, I)] [, probs (U, I)]."""
    n1, n2, n3 = hidden
    U, I = pu.shape[0], pit.shape[1]
    dev = pu.device
    lib = _lib.load()
    if not 1 <= int(k) <= 256:
        raise ValueError(f"k = {k}: 1 <= k <= 256")
    ws_bytes = int(lib.brNeumfCatalogTopKWorkspaceBytes(U, I, int(k)))
    if ws_bytes < 0:
        raise ValueError(f"neumf_catalog_topk: bad sizes U={U} I={I} k={k}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    os_ = torch.empty(U, k, dtype=torch.float32, device=dev)
    oi = torch.empty(U, k, dtype=torch.int32, device=dev)
    dl = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_logits else None
    dp = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_probs else None
    off, idx = _csr(exclude, U, "exclude") if exclude is not None else (None, None)
    check(lib.brNeumfCatalogTopK(_f32(pu, "pu").data_ptr(), pu.stride(0), _f32(pit, "pit").data_ptr(), pit.stride(0), U, I, dim, n1, n2, n3,
                                 ACT[act], _f32(tower, "tower").data_ptr(), _p(off), _p(idx), int(k), os_.data_ptr(), oi.data_ptr(), _p(dl),
                                 _p(dp), ws.data_ptr(), ws_bytes, _stream()), "brNeumfCatalogTopK")
    out = (os_, oi)
    if dump_logits:
        out += (dl,)
    if dump_probs:
        out += (dp,)
    return out


# ------------------------------------------------------------------------------ dot-product catalogue top-k (csrc/recommend_dot.hip)
def _rows_f32(t, name: str):
    """a 2-D float32 device matrix with unit column stride and row stride >= its width (a table as it is, or a column slice of one)"""
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{name}: expected a float32 device tensor, got {t.dtype} {t.device}")
    if t.shape[1] > 0 and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise TypeError(f"{name}: rows must be unit-stride with row stride >= {t.shape[1]} (got strides {tuple(t.stride())})")
    return t


DOT_MAX_DIM = 128          # widest rows of dot_catalog_topk / dot_catalog_auc (the whole-row kernels)
DOT_WIDE_MAX_DIM = 512     # ... of dot_catalog_topk_wide / dot_catalog_auc_wide (the block kernels)


def _dot_catalog_args(who: str, Q, C, k=None, max_dim=DOT_MAX_DIM):
    """the checks dot_catalog_topk / dot_catalog_auc and their _wide forms (`who`) make on Q, C (and k) -> (U, I, dim, ld_q, ld_c,
    device)"""
    for t, name in ((Q, "Q"), (C, "C")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a 2-D tensor")
    U, dim = Q.shape
    I = C.shape[0]
    if C.shape[1] != dim:
        raise ValueError(f"{who}: Q has dim {dim}, C has {C.shape[1]}")
    if not 1 <= dim <= max_dim:
        raise ValueError(f"{who}: dim = {dim}: 1 <= dim <= {max_dim}")
    if k is not None and not 1 <= int(k) <= 256:
        raise ValueError(f"k = {k}: 1 <= k <= 256")
    _rows_f32(Q, "Q"); _rows_f32(C, "C")
    if Q.device != C.device:
        raise ValueError(f"{who}: Q and C on different devices")
    return U, I, dim, (Q.stride(0) if U > 1 else dim), (C.stride(0) if I > 1 else dim), Q.device


def _wide_flags(force_wide) -> int:
    return _lib.parse_enums()["BR_DOT_FORCE_WIDE"] if force_wide else 0


def _dot_topk(who: str, wide: bool, Q, C, k, exclude, dump_scores, force_wide=False):
    """dot_catalog_topk (brDotCatalogTopK) and dot_catalog_topk_wide (wide: brDotCatalogTopKWide, with dim and the flags)"""
    U, I, dim, ld_q, ld_c, dev = _dot_catalog_args(who, Q, C, k, DOT_WIDE_MAX_DIM if wide else DOT_MAX_DIM)
    lib = _lib.load()
    ws_bytes = int(lib.brDotCatalogTopKWideWorkspaceBytes(U, I, dim, int(k)) if wide else lib.brDotCatalogTopKWorkspaceBytes(U, I, int(k)))
    if ws_bytes < 0:
        raise ValueError(f"{who}: bad sizes U={U} I={I} k={k}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    os_ = torch.empty(U, k, dtype=torch.float32, device=dev)
    oi = torch.empty(U, k, dtype=torch.int32, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_scores else None
    off, idx = _csr(exclude, U, "exclude") if exclude is not None else (None, None)
    fn, name = (lib.brDotCatalogTopKWide, "brDotCatalogTopKWide") if wide else (lib.brDotCatalogTopK, "brDotCatalogTopK")
    check(fn(Q.data_ptr(), ld_q, U, C.data_ptr(), ld_c, I, dim, _p(off), _p(idx), int(k), os_.data_ptr(), oi.data_ptr(), _p(dump),
             *((_wide_flags(force_wide),) if wide else ()), ws.data_ptr(), ws_bytes, _stream()), name)
    return (os_, oi, dump) if dump_scores else (os_, oi)


def dot_catalog_topk(Q, C, k, exclude=None, dump_scores=False):
    """Q (U x dim) user rows, C (I x dim) item rows (any row stride >= dim) -> (scores (U, k) float32, index (U, k) int32 positions
    into C) [, every pair's score (U, I)]: per user the k best Q[u] . C[i], best first, ties to the lower position, exclude positions
    (ops.truth_csr over the rows of Q) never returned, (-inf, -1) past the remaining candidates; the U x I matrix is not stored."""
    return _dot_topk("dot_catalog_topk", False, Q, C, k, exclude, dump_scores)


# ------------------------------------------------------------------------------ shard-local lists -> one list (csrc/recommend_merge.hip)
def _i32_dev(t, name: str):
    if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous int32 device tensor, got {t.dtype} {t.device}")
    return t


def csr_split_by_owner(off, idx, g2l):
    """(off int64 (rows + 1), idx int32): a CSR of ascending positions into a global candidate list; g2l int32 (n_global): global
    position -> this owner's local position or -1 -> (out_off (rows + 1), out_idx): the rows restricted to this owner's candidates in
    local positions (brCsrSplitByOwner).  out_idx keeps the input's capacity: only its first out_off[-1] entries mean anything (no
    host sync here to cut it)."""
    n_rows = off.shape[0] - 1
    off, idx = _csr((off, idx), n_rows, "csr")
    _i32_dev(g2l, "g2l")
    lib = _lib.load()
    ws_bytes = int(lib.brCsrSplitByOwnerWorkspaceBytes(n_rows))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=off.device)
    out_off = torch.empty(n_rows + 1, dtype=torch.int64, device=off.device)
    out_idx = torch.empty(max(idx.numel(), 1), dtype=torch.int32, device=off.device)
    check(lib.brCsrSplitByOwner(off.data_ptr(), idx.data_ptr(), n_rows, _p(g2l) if g2l.numel() else out_idx.data_ptr(), g2l.numel(),
                                out_off.data_ptr(), out_idx.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "brCsrSplitByOwner")
    return out_off, out_idx


def topk_lists_merge(scores, index, n_lists: int, n_users: int, k: int, l2g, l2g_off, list_stride=None, user_stride=None):
    """scores float32 / index int32: n_lists lists of k (score, local position) entries per user, entry e of list w of user u at element
    [w * list_stride + u * user_stride + e] (defaults: the (n_lists, n_users, k) stack of n_lists launches); l2g int32 / l2g_off int64
    (n_lists + 1): list w's local position l is global position l2g[l2g_off[w] + l], ascending per list -> (scores (n_users, k),
    index (n_users, k) int32 GLOBAL positions): the k best of the union, ties to the lower global position, (-inf, -1) past the
    entries there are (brTopKListsMerge)."""
    k, n_lists, n_users = int(k), int(n_lists), int(n_users)
    if not 1 <= k <= 256:
        raise ValueError(f"k = {k}: 1 <= k <= 256")
    user_stride = k if user_stride is None else int(user_stride)
    list_stride = n_users * user_stride if list_stride is None else int(list_stride)
    if scores.dtype != torch.float32 or not scores.is_cuda:
        raise TypeError("topk_lists_merge: scores must be a float32 device tensor")
    if index.dtype != torch.int32 or not index.is_cuda:
        raise TypeError("topk_lists_merge: index must be an int32 device tensor")
    if n_users:
        last = (n_lists - 1) * list_stride + (n_users - 1) * user_stride + k       # one past the last element the kernel reads
        for t, name in ((scores, "scores"), (index, "index")):
            if not t.is_contiguous() and t.dim() != 2:
                raise TypeError(f"topk_lists_merge: {name} must be contiguous or a column slice of a 2-D buffer")
            room = t.numel() if t.is_contiguous() else (t.shape[0] - 1) * t.stride(0) + t.shape[1]
            if room < last:
                raise ValueError(f"topk_lists_merge: {name} holds {room} elements, the strides reach {last}")
    if l2g_off.dtype != torch.int64 or not l2g_off.is_cuda or not l2g_off.is_contiguous() or l2g_off.numel() != n_lists + 1:
        raise TypeError(f"topk_lists_merge: l2g_off must be a contiguous int64 device tensor of {n_lists + 1} entries")
    _i32_dev(l2g, "l2g")
    dev = scores.device
    os_ = torch.empty(n_users, k, dtype=torch.float32, device=dev)
    oi = torch.empty(n_users, k, dtype=torch.int32, device=dev)
    if l2g.numel() == 0:           # a valid pointer for an empty map
        l2g = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.load().brTopKListsMerge(scores.data_ptr(), index.data_ptr(), list_stride, user_stride, n_lists, n_users, k, l2g.data_ptr(),
                                       l2g_off.data_ptr(), os_.data_ptr(), oi.data_ptr(), _stream()), "brTopKListsMerge")
    return os_, oi


# ------------------------------------------------------------------------------ dot-product catalogue AUC (csrc/auc_dot.hip)
def _dot_auc(who: str, wide: bool, Q, C, truth_off, truth_idx, dump_scores, force_wide=False):
    """dot_catalog_auc (brDotCatalogAuc) and dot_catalog_auc_wide (wide: brDotCatalogAucWide, with dim and the flags)"""
    U, I, dim, ld_q, ld_c, dev = _dot_catalog_args(who, Q, C, None, DOT_WIDE_MAX_DIM if wide else DOT_MAX_DIM)
    n_truth = truth_idx.numel() if isinstance(truth_idx, torch.Tensor) else 0
    off, idx = _csr((truth_off, truth_idx), U, "truth")
    lib = _lib.load()
    ws_bytes = int(lib.brDotCatalogAucWideWorkspaceBytes(U, I, dim, n_truth) if wide else lib.brDotCatalogAucWorkspaceBytes(U, I, n_truth))
    if ws_bytes < 0:
        raise ValueError(f"{who}: bad sizes U={U} I={I}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(U, dtype=torch.float32, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_scores else None
    fn, name = (lib.brDotCatalogAucWide, "brDotCatalogAucWide") if wide else (lib.brDotCatalogAuc, "brDotCatalogAuc")
    check(fn(Q.data_ptr(), ld_q, U, C.data_ptr(), ld_c, I, dim, off.data_ptr(), idx.data_ptr(), out.data_ptr(), _p(dump),
             *((_wide_flags(force_wide),) if wide else ()), ws.data_ptr(), ws_bytes, _stream()), name)
    return (out, dump) if dump_scores else out


def dot_catalog_auc(Q, C, truth_off, truth_idx, dump_scores=False):
    """Q (U x dim) user rows, C (I x dim) item rows (any row stride >= dim), truth (ops.truth_csr over the rows of Q: ascending
    positions into C) -> per-user AUC float32 (U,) [, every pair's score (U, I)]: full_auc of the scores Q[u] . C[i], equal bit for
    bit to full_auc(score_matrix(Q, C), truth_off, truth_idx) on the same scores, NaN where undefined; the U x I matrix is not stored."""
    return _dot_auc("dot_catalog_auc", False, Q, C, truth_off, truth_idx, dump_scores)


# ------------------------------------------------------------------------------ wide rows (csrc/recommend_dot_wide.hip, auc_dot.hip)
def dot_catalog_topk_wide(Q, C, k, exclude=None, dump_scores=False, force_wide=False):
    """dot_catalog_topk for 1 <= dim <= 512 (brDotCatalogTopKWide): the same arguments, results and score contract.  dim <= 128 runs
    dot_catalog_topk's launches unless force_wide, which sends those rows through the block kernels too (same bits: tests)."""
    return _dot_topk("dot_catalog_topk_wide", True, Q, C, k, exclude, dump_scores, force_wide)


def dot_catalog_auc_wide(Q, C, truth_off, truth_idx, dump_scores=False, force_wide=False):
    """dot_catalog_auc for 1 <= dim <= 512 (brDotCatalogAucWide): the same arguments, results and score contract.  dim <= 128 runs
    dot_catalog_auc's launches unless force_wide, which sends those rows through the block kernels too (same bits: tests)."""
    return _dot_auc("dot_catalog_auc_wide", True, Q, C, truth_off, truth_idx, dump_scores, force_wide)


def dot_topk_for(dim: int):
    """the catalogue top-k op the engines call at row width `dim`: the whole-row op up to 128 features exactly as before, the wide op
    above"""
    return dot_catalog_topk if dim <= DOT_MAX_DIM else dot_catalog_topk_wide


def dot_auc_for(dim: int):
    return dot_catalog_auc if dim <= DOT_MAX_DIM else dot_catalog_auc_wide


# ------------------------------------------------------------------------------ dot-product catalogue ranks (csrc/ranks_dot.hip)
RANK_MAX_KS = 8            # cutoffs of one rank_metrics call


def dot_catalog_ranks(Q, C, truth_off, truth_idx, exclude=None, dump_scores=False, force_wide=False):
    """Q (U x dim) user rows, C (I x dim) item rows (any row stride >= dim, 1 <= dim <= 512), truth (ops.truth_csr over the rows of Q:
    ascending positions into C), exclude: (off, idx) CSR over the rows of Q of positions never offered as candidates
    (topk_metrics.seen_csr) -> (above, tied) int32, one entry per truth entry in CSR order [, every pair's score (U, I)]: how many
    candidates (every non-excluded item but the entry itself, the user's other positives included) score above the positive and how
    many tie with it, counted exactly on the scores dot_catalog_auc / dot_catalog_topk form (same bits); the U x I matrix is not
    stored.  An excluded position that is a truth entry is still ranked (against the non-excluded others).  (-1, -1) for a positive
    whose score is NaN; a NaN candidate is never above and never tied.  force_wide as in dot_catalog_auc_wide (brDotCatalogRanks)."""
    U, I, dim, ld_q, ld_c, dev = _dot_catalog_args("dot_catalog_ranks", Q, C, None, DOT_WIDE_MAX_DIM)
    n_truth = truth_idx.numel() if isinstance(truth_idx, torch.Tensor) else 0
    off, idx = _csr((truth_off, truth_idx), U, "truth")
    xoff, xidx = _csr(exclude, U, "exclude") if exclude is not None else (None, None)
    lib = _lib.load()
    ws_bytes = int(lib.brDotCatalogRanksWorkspaceBytes(U, I, dim, n_truth))
    if ws_bytes < 0:
        raise ValueError(f"dot_catalog_ranks: bad sizes U={U} I={I} truth entries={n_truth}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    above = torch.empty(n_truth, dtype=torch.int32, device=dev)
    tied = torch.empty(n_truth, dtype=torch.int32, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_scores else None
    check(lib.brDotCatalogRanks(Q.data_ptr(), ld_q, U, C.data_ptr(), ld_c, I, dim, off.data_ptr(), idx.data_ptr(), n_truth, _p(xoff), _p(xidx),
                                above.data_ptr() if n_truth else ws.data_ptr(), tied.data_ptr() if n_truth else ws.data_ptr(), _p(dump),
                                _wide_flags(force_wide), ws.data_ptr(), ws_bytes, _stream()), "brDotCatalogRanks")
    return (above, tied, dump) if dump_scores else (above, tied)


def rank_metrics(above, tied, truth_off, ks):
    """above / tied int32 (one per truth entry) and truth_off int64 (U + 1) of dot_catalog_ranks, ks: 1 to 8 cutoffs k >= 1 -> dict of
    float32 device tensors (U,): "mrr" and per k "ndcg@k", "recall@k", "hr@k"; NaN for a user without positives.  The rank of a positive
    is r = 1 + above + tied - pessimistic: a tied candidate is taken to outrank the positive, so a model that scores everything equal
    earns nothing.  An entry with above = -1 has no rank: a miss that still counts in P.  NDCG@k = sum over r <= k of 1 / log2(1 + r)
    over the same sum for the ranks 1 .. min(P, k); recall@k = #{r <= k} / P; hr@k = [min r <= k]; mrr = 1 / min r, 0 without a ranked
    positive.  Summed in double on the device (brRankMetrics)."""
    import ctypes
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= RANK_MAX_KS:
        raise ValueError(f"rank_metrics: {len(ks)} cutoffs: 1 <= len(ks) <= {RANK_MAX_KS}")
    if min(ks) < 1 or max(ks) >= 1 << 31:
        raise ValueError(f"rank_metrics: ks = {ks}: every cutoff 1 <= k < 2^31")
    for t, name in ((above, "above"), (tied, "tied")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"rank_metrics: {name} must be a 1-D tensor")
    if above.shape != tied.shape:
        raise ValueError(f"rank_metrics: above has {above.numel()} entries, tied {tied.numel()}")
    if not isinstance(truth_off, torch.Tensor) or truth_off.dtype != torch.int64 or not truth_off.is_cuda or not truth_off.is_contiguous() \
            or truth_off.dim() != 1 or truth_off.numel() < 1:
        raise TypeError("rank_metrics: truth_off must be a contiguous int64 device tensor (U + 1)")
    _i32_dev(above, "above"); _i32_dev(tied, "tied")
    U, dev = truth_off.numel() - 1, truth_off.device
    mrr = torch.empty(U, dtype=torch.float32, device=dev)
    out = torch.empty(3, len(ks), U, dtype=torch.float32, device=dev)
    if above.numel() == 0:         # a valid pointer for an empty list
        above = tied = torch.zeros(1, dtype=torch.int32, device=dev)
    kk = (ctypes.c_int32 * len(ks))(*ks)
    if U:
        check(_lib.load().brRankMetrics(above.data_ptr(), tied.data_ptr(), truth_off.data_ptr(), U, ctypes.addressof(kk), len(ks), mrr.data_ptr(),
                                        out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream()), "brRankMetrics")
    res = {"mrr": mrr}
    for j, k in enumerate(ks):
        res[f"ndcg@{k}"], res[f"recall@{k}"], res[f"hr@{k}"] = out[0, j], out[1, j], out[2, j]
    return res


# ------------------------------------------------------------------------------ catalogue AUC counted at the item owners (csrc/auc_owner.hip)
# dot_catalog_auc[_wide] in four phases, for W owners that each hold a share of the candidates (parallel.auc_at_owners).
# force_wide as in dot_catalog_auc_wide; the positives and the count of one evaluation take the same value.
def _auc_list_args(who: str, U: int, list_off, sorted_, pcnt):
    """the checks the owner-side counts (`who`) make on the users' full lists (list_off / sorted_ / pcnt of auc_sort_pieces)"""
    if list_off.dtype != torch.int64 or not list_off.is_cuda or not list_off.is_contiguous() or list_off.numel() != U + 1:
        raise TypeError(f"{who}: list_off must be a contiguous int64 device tensor of {U + 1} entries")
    if sorted_.dtype != torch.float32 or not sorted_.is_cuda or not sorted_.is_contiguous() or sorted_.numel() < 1:
        raise TypeError(f"{who}: sorted_ must be a non-empty contiguous float32 device tensor")
    _i32_dev(pcnt, "pcnt")
    if pcnt.numel() != U:
        raise ValueError(f"{who}: pcnt has {pcnt.numel()} entries for {U} users")


def dot_auc_owner_positives(Q, C, pos_off, pos_idx, out=None, force_wide=False):
    """Q (U x dim), C (I_loc x dim): this owner's candidate rows; (pos_off, pos_idx): per user its positives among them in LOCAL
    positions (csr_split_by_owner) -> raw float32: raw[pos_off[u] + j] = the catalogue pass's score of the user's j-th entry, NaN for a
    position outside C.  out: a float32 device buffer of at least pos_off[-1] entries (default: one of pos_idx's capacity)."""
    U, I, dim, ld_q, ld_c, dev = _dot_catalog_args("dot_auc_owner_positives", Q, C, None, DOT_WIDE_MAX_DIM)
    n_cap = pos_idx.numel() if isinstance(pos_idx, torch.Tensor) else 0
    off, idx = _csr((pos_off, pos_idx), U, "positives")
    out = torch.empty(max(n_cap, 1), dtype=torch.float32, device=dev) if out is None else out
    if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise TypeError("dot_auc_owner_positives: out must be a contiguous float32 device tensor")
    check(_lib.load().brDotAucOwnerPositives(Q.data_ptr(), ld_q, U, C.data_ptr(), ld_c, I, dim, off.data_ptr(), idx.data_ptr(), out.data_ptr(),
                                             _wide_flags(force_wide), _stream()), "brDotAucOwnerPositives")
    return out


def auc_sort_pieces(raw, piece_off, list_off, cap: int):
    """raw float32 (any shape, contiguous), piece_off int64 (n_pieces, U + 1): piece w of user u is raw.view(-1)[piece_off[w, u] :
    piece_off[w, u + 1]]; list_off int64 (U + 1) -> (sorted float32 (cap + 1), pcnt int32 (U,)): per user the entries of all its pieces
    ascending at sorted[list_off[u]:], NaN dropped, their number in pcnt[u]; -1 for a user whose list lies past `cap` or whose pieces
    do not fit it (brAucSortPieces).  The pieces' order does not matter."""
    if raw.dtype != torch.float32 or not raw.is_cuda or not raw.is_contiguous():
        raise TypeError("auc_sort_pieces: raw must be a contiguous float32 device tensor")
    for t, name in ((piece_off, "piece_off"), (list_off, "list_off")):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
            raise TypeError(f"auc_sort_pieces: {name} must be a contiguous int64 device tensor")
    n_users = list_off.shape[0] - 1
    if piece_off.dim() != 2 or piece_off.shape[1] != n_users + 1:
        raise ValueError(f"auc_sort_pieces: piece_off must be (n_pieces, {n_users + 1})")
    n_pieces, cap, dev = piece_off.shape[0], int(cap), raw.device
    lib = _lib.load()
    ws_bytes = int(lib.brAucSortPiecesWorkspaceBytes(n_pieces, cap))
    if ws_bytes < 0:
        raise ValueError(f"auc_sort_pieces: n_pieces = {n_pieces}: 1 <= n_pieces <= 4096 (cap = {cap} >= 0)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    sorted_ = torch.empty(cap + 1, dtype=torch.float32, device=dev)
    pcnt = torch.empty(max(n_users, 1), dtype=torch.int32, device=dev)[:n_users]
    check(lib.brAucSortPieces(raw.data_ptr() if raw.numel() else sorted_.data_ptr(), raw.numel(), piece_off.data_ptr(), n_pieces, n_users,
                              list_off.data_ptr(), sorted_.data_ptr(), cap, pcnt.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
          "brAucSortPieces")
    return sorted_, pcnt


def dot_auc_owner_count(Q, C, skip_off, skip_idx, list_off, sorted_, pcnt, dump_scores=False, force_wide=False):
    """Q (U x dim), C (I_loc x dim): this owner's candidate rows; (skip_off, skip_idx): its positives per user, ascending LOCAL positions;
    list_off / sorted_ / pcnt of auc_sort_pieces: every user's FULL list -> per user the integer 2W over these candidates, int64 (U,)
    (the library's uint64: below 2^63 while P N < 2^62) [, every pair's score (U, I_loc)] (brDotAucOwnerCount)."""
    U, I, dim, ld_q, ld_c, dev = _dot_catalog_args("dot_auc_owner_count", Q, C, None, DOT_WIDE_MAX_DIM)
    off, idx = _csr((skip_off, skip_idx), U, "skip")
    _auc_list_args("dot_auc_owner_count", U, list_off, sorted_, pcnt)
    lib = _lib.load()
    ws_bytes = int(lib.brDotAucOwnerCountWorkspaceBytes(U, I, dim))
    if ws_bytes < 0:
        raise ValueError(f"dot_auc_owner_count: bad sizes U={U} I={I}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(U, dtype=torch.int64, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_scores else None
    check(lib.brDotAucOwnerCount(Q.data_ptr(), ld_q, U, C.data_ptr(), ld_c, I, dim, off.data_ptr(), idx.data_ptr(), list_off.data_ptr(),
                                 sorted_.data_ptr(), pcnt.data_ptr() if U else sorted_.data_ptr(), sorted_.numel() - 1, out.data_ptr() if U else sorted_.data_ptr(),
                                 _p(dump), _wide_flags(force_wide), ws.data_ptr(), ws_bytes, _stream()), "brDotAucOwnerCount")
    return (out, dump) if dump_scores else out


def auc_finalize_lists(part, n_lists: int, n_users: int, truth_off, pcnt, n_items: int, list_stride=None):
    """part int64: n_lists partial 2W per user, list w of user u at part.view(-1)[w * list_stride + u] (default stride n_users: the
    stack of n_lists counts, or the receive buffer of one all-to-all); truth_off int64 (n_users + 1): the GLOBAL truth offsets; pcnt of
    auc_sort_pieces for these users; n_items: the length of the whole candidate list -> AUC float32 (n_users,), NaN where undefined
    (brAucFinalizeLists)."""
    n_lists, n_users = int(n_lists), int(n_users)
    list_stride = n_users if list_stride is None else int(list_stride)
    if part.dtype != torch.int64 or not part.is_cuda or not part.is_contiguous():
        raise TypeError("auc_finalize_lists: part must be a contiguous int64 device tensor")
    if n_users and n_lists >= 1 and part.numel() < (n_lists - 1) * list_stride + n_users:
        raise ValueError(f"auc_finalize_lists: part holds {part.numel()} entries, the strides reach {(n_lists - 1) * list_stride + n_users}")
    if truth_off.dtype != torch.int64 or not truth_off.is_cuda or not truth_off.is_contiguous() or truth_off.numel() != n_users + 1:
        raise TypeError(f"auc_finalize_lists: truth_off must be a contiguous int64 device tensor of {n_users + 1} entries")
    _i32_dev(pcnt, "pcnt")
    if pcnt.numel() != n_users:
        raise ValueError(f"auc_finalize_lists: pcnt has {pcnt.numel()} entries for {n_users} users")
    out = torch.empty(n_users, dtype=torch.float32, device=part.device)
    valid = truth_off.data_ptr()           # a valid pointer where a tensor is empty
    check(_lib.load().brAucFinalizeLists(part.data_ptr() if part.numel() else valid, list_stride, n_lists, truth_off.data_ptr(),
                                         pcnt.data_ptr() if n_users else valid, n_users, int(n_items), out.data_ptr() if n_users else valid,
                                         _stream()), "brAucFinalizeLists")
    return out


# ------------------------------------------------------------------------------ NeuMF catalogue AUC (csrc/auc_neumf.hip)
# The operands of neumf_catalog_topk; the score of a pair is the probability that op's dump_probs shows, bit for bit.
def _neumf_catalog_args(who: str, pu, pit, tower, dim: int, hidden, act: str):
    """the checks the NeuMF catalogue AUC ops (`who`) make on their operands -> (U, I, n1, n2, n3, device)"""
    n1, n2, n3 = (int(n) for n in hidden)
    dim = int(dim)
    for t, name in ((pu, "pu"), (pit, "pit")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a 2-D tensor")
    if act not in ACT:
        raise ValueError(f"{who}: act = {act!r}: one of {sorted(ACT)}")
    if not (1 <= n1 <= 128 and 1 <= n2 <= 128 and 1 <= n3 <= 32):
        raise ValueError(f"{who}: tower widths n1, n2 <= 128 and n3 <= 32 (got {n1}, {n2}, {n3})")
    if not (1 <= dim and 2 * dim <= 256):
        raise ValueError(f"{who}: dim = {dim}: 1 <= dim, 2 * dim <= 256")
    _rows_f32(pu, "pu"); _rows_f32(pit, "pit")
    if not isinstance(tower, torch.Tensor) or tower.dtype != torch.float32 or not tower.is_cuda or not tower.is_contiguous():
        raise TypeError(f"{who}: tower must be a contiguous float32 device tensor (ops.neumf_catalog_fold)")
    if pu.shape[1] != n1 + dim or pit.shape[0] != n1 + dim:
        raise ValueError(f"{who}: pu must be (U, {n1 + dim}) and pit ({n1 + dim}, I) (got {tuple(pu.shape)}, {tuple(pit.shape)})")
    n_tower = int(_lib.load().brNeumfCatalogTowerFloats(n1, n2, n3))
    if tower.numel() != n_tower:
        raise ValueError(f"{who}: tower has {tower.numel()} floats, the widths ({n1}, {n2}, {n3}) need {n_tower}")
    if pu.device != pit.device or pu.device != tower.device:
        raise ValueError(f"{who}: pu, pit and tower on different devices")
    if pit.shape[1] < 1:
        raise ValueError(f"{who}: empty candidate list")
    return pu.shape[0], pit.shape[1], n1, n2, n3, pu.device


def _neumf_operands(pu, pit, U, I, dim, n1, n2, n3, act, tower):
    """the C-ABI's leading arguments (pu, ld_u, n_users, pit, ld_i, n_items, dim, n1, n2, n3, act, tower)"""
    return (pu.data_ptr() if U else tower.data_ptr(), pu.stride(0) if U > 1 else n1 + dim, U, pit.data_ptr(), pit.stride(0), I, int(dim), n1, n2,
            n3, ACT[act], tower.data_ptr())


def neumf_auc_positives(pu, pit, tower, dim: int, hidden, act: str, pos_off, pos_idx, out=None):
    """pu (U x (n1 + dim)), pit ((n1 + dim) x I_loc), tower: the operands of neumf_catalog_topk over these candidates; (pos_off,
    pos_idx): per user its positives among them, positions into pit (csr_split_by_owner on a row-sharded engine) -> raw float32:
    raw[pos_off[u] + j] = the catalogue pass's probability of the user's j-th entry, NaN for a position outside pit.  out: a float32
    device buffer of at least pos_off[-1] entries (default: one of pos_idx's capacity) (brNeumfAucPositives)."""
    U, I, n1, n2, n3, dev = _neumf_catalog_args("neumf_auc_positives", pu, pit, tower, dim, hidden, act)
    n_cap = pos_idx.numel() if isinstance(pos_idx, torch.Tensor) else 0
    off, idx = _csr((pos_off, pos_idx), U, "positives")
    out = torch.empty(max(n_cap, 1), dtype=torch.float32, device=dev) if out is None else out
    if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise TypeError("neumf_auc_positives: out must be a contiguous float32 device tensor")
    check(_lib.load().brNeumfAucPositives(*_neumf_operands(pu, pit, U, I, dim, n1, n2, n3, act, tower), off.data_ptr(), idx.data_ptr(),
                                          out.data_ptr(), _stream()), "brNeumfAucPositives")
    return out


def neumf_auc_count(pu, pit, tower, dim: int, hidden, act: str, skip_off, skip_idx, list_off, sorted_, pcnt, dump_probs=False):
    """the operands of neumf_auc_positives; (skip_off, skip_idx): the users' positives among these candidates, ascending positions;
    list_off / sorted_ / pcnt of auc_sort_pieces: every user's FULL list -> per user the integer 2W over these candidates, int64 (U,)
    (the library's uint64: below 2^63 while P N < 2^62) [, every pair's probability (U, I_loc)] (brNeumfAucCount)."""
    U, I, n1, n2, n3, dev = _neumf_catalog_args("neumf_auc_count", pu, pit, tower, dim, hidden, act)
    off, idx = _csr((skip_off, skip_idx), U, "skip")
    _auc_list_args("neumf_auc_count", U, list_off, sorted_, pcnt)
    lib = _lib.load()
    ws_bytes = int(lib.brNeumfAucCountWorkspaceBytes(U, I))
    if ws_bytes < 0:
        raise ValueError(f"neumf_auc_count: bad sizes U={U} I={I}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(U, dtype=torch.int64, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_probs else None
    check(lib.brNeumfAucCount(*_neumf_operands(pu, pit, U, I, dim, n1, n2, n3, act, tower), off.data_ptr(), idx.data_ptr(), list_off.data_ptr(),
                              sorted_.data_ptr(), pcnt.data_ptr() if U else sorted_.data_ptr(), sorted_.numel() - 1,
                              out.data_ptr() if U else sorted_.data_ptr(), _p(dump), ws.data_ptr(), ws_bytes, _stream()), "brNeumfAucCount")
    return (out, dump) if dump_probs else out


def neumf_catalog_auc(pu, pit, tower, dim: int, hidden, act: str, truth_off, truth_idx, dump_probs=False):
    """pu (U x (n1 + dim)) and pit ((n1 + dim) x I) from neumf_catalog_project, tower from neumf_catalog_fold, truth (ops.truth_csr over
    the rows of pu: ascending positions into the item list) -> per-user AUC float32 (U,) [, every pair's probability (U, I)]: full_auc
    of the probabilities neumf_catalog_topk ranks by, equal bit for bit to full_auc(its dump_probs, truth_off, truth_idx), NaN where
    undefined; the U x I matrix is not stored (brNeumfCatalogAuc)."""
    U, I, n1, n2, n3, dev = _neumf_catalog_args("neumf_catalog_auc", pu, pit, tower, dim, hidden, act)
    n_truth = truth_idx.numel() if isinstance(truth_idx, torch.Tensor) else 0
    off, idx = _csr((truth_off, truth_idx), U, "truth")
    lib = _lib.load()
    ws_bytes = int(lib.brNeumfCatalogAucWorkspaceBytes(U, I, n_truth))
    if ws_bytes < 0:
        raise ValueError(f"neumf_catalog_auc: bad sizes U={U} I={I}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(U, dtype=torch.float32, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_probs else None
    check(lib.brNeumfCatalogAuc(*_neumf_operands(pu, pit, U, I, dim, n1, n2, n3, act, tower), off.data_ptr(), idx.data_ptr(),
                                out.data_ptr() if U else ws.data_ptr(), _p(dump), ws.data_ptr(), ws_bytes, _stream()), "brNeumfCatalogAuc")
    return (out, dump) if dump_probs else out


# ------------------------------------------------------------------------------ NeuMF catalogue ranks (csrc/ranks_neumf.hip)
# dot_catalog_ranks' contract over the operands and the probabilities of neumf_catalog_auc; rank_metrics takes the integers.
def neumf_catalog_ranks(pu, pit, tower, dim: int, hidden, act: str, truth_off, truth_idx, exclude=None, dump_probs=False):
    """The operands of neumf_catalog_auc, truth (ops.truth_csr over the rows of pu: ascending positions into the item list), exclude:
    (off, idx) CSR over the rows of pu of positions never offered as candidates (topk_metrics.seen_csr) -> (above, tied) int32, one
    entry per truth entry in CSR order [, every pair's probability (U, I)]: how many candidates (every non-excluded item but the entry
    itself, the user's other positives included) have a probability above the positive's and how many tie with it, counted exactly on
    the probabilities neumf_catalog_auc / neumf_catalog_topk form (same bits); the U x I matrix is not stored.  An excluded position
    that is a truth entry is still ranked (against the non-excluded others).  (-1, -1) for a positive whose probability is NaN; a NaN
    candidate is never above and never tied (brNeumfCatalogRanks)."""
    U, I, n1, n2, n3, dev = _neumf_catalog_args("neumf_catalog_ranks", pu, pit, tower, dim, hidden, act)
    n_truth = truth_idx.numel() if isinstance(truth_idx, torch.Tensor) else 0
    off, idx = _csr((truth_off, truth_idx), U, "truth")
    xoff, xidx = _csr(exclude, U, "exclude") if exclude is not None else (None, None)
    lib = _lib.load()
    ws_bytes = int(lib.brNeumfCatalogRanksWorkspaceBytes(U, I, n_truth))
    if ws_bytes < 0:
        raise ValueError(f"neumf_catalog_ranks: bad sizes U={U} I={I} truth entries={n_truth}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    above = torch.empty(n_truth, dtype=torch.int32, device=dev)
    tied = torch.empty(n_truth, dtype=torch.int32, device=dev)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_probs else None
    check(lib.brNeumfCatalogRanks(*_neumf_operands(pu, pit, U, I, dim, n1, n2, n3, act, tower), off.data_ptr(), idx.data_ptr(), n_truth,
                                  _p(xoff), _p(xidx), above.data_ptr() if n_truth else ws.data_ptr(), tied.data_ptr() if n_truth else ws.data_ptr(),
                                  _p(dump), ws.data_ptr(), ws_bytes, _stream()), "brNeumfCatalogRanks")
    return (above, tied, dump) if dump_probs else (above, tied)


def _rank_bins_args(who: str, U: int, list_off, sorted_, pcnt, bins, ties):
    """the checks the phase entries of the ranks (`who`) make on the users' full lists and their bins -> cap"""
    _auc_list_args(who, U, list_off, sorted_, pcnt)
    cap = sorted_.numel() - 1
    for t, name in ((bins, "bins"), (ties, "ties")):
        _i32_dev(t, name)
        if t.dim() != 1 or t.numel() < max(cap + U, 1):
            raise ValueError(f"{who}: {name} must be 1-D with at least cap + U = {cap + U} entries (has {t.numel()})")
    return cap


def rank_bins(n_users: int, cap: int, device):
    """-> (bins, ties): the zeroed int32 bins and tie bins of `n_users` users whose lists lie in `cap` floats (n + 1 each per user)"""
    n = max(int(cap) + int(n_users), 1)
    return torch.zeros(n, dtype=torch.int32, device=device), torch.zeros(n, dtype=torch.int32, device=device)


def neumf_rank_count(pu, pit, tower, dim: int, hidden, act: str, skip_off, skip_idx, list_off, sorted_, pcnt, bins, ties, dump_probs=False):
    """The catalogue pass of neumf_catalog_ranks over the candidates one owner holds.  The operands of neumf_auc_positives; (skip_off,
    skip_idx): per user the owner's truth and excluded positions in one ascending list of LOCAL positions; list_off / sorted_ / pcnt of
    auc_sort_pieces: every user's FULL list; bins / ties of rank_bins: the call ADDS this owner's counts into them (user u's n + 1 bins
    from list_off[u] + u on) -> None [every pair's probability (U, I_loc)] (brNeumfRankCount)."""
    U, I, n1, n2, n3, dev = _neumf_catalog_args("neumf_rank_count", pu, pit, tower, dim, hidden, act)
    off, idx = _csr((skip_off, skip_idx), U, "skip")
    cap = _rank_bins_args("neumf_rank_count", U, list_off, sorted_, pcnt, bins, ties)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_probs else None
    check(_lib.load().brNeumfRankCount(*_neumf_operands(pu, pit, U, I, dim, n1, n2, n3, act, tower), off.data_ptr(), idx.data_ptr(),
                                       list_off.data_ptr(), sorted_.data_ptr(), pcnt.data_ptr() if U else sorted_.data_ptr(), cap,
                                       bins.data_ptr(), ties.data_ptr(), _p(dump), _stream()), "brNeumfRankCount")
    return dump


def dot_rank_count(Q, C, skip_off, skip_idx, list_off, sorted_, pcnt, bins, ties, dump_scores=False, force_wide=False):
    """The catalogue pass of dot_catalog_ranks over the candidates one owner holds.  Q (U x dim), C (I_loc x dim): this owner's candidate
    rows; (skip_off, skip_idx): per user the owner's truth and excluded positions in one ascending list of LOCAL positions; list_off /
    sorted_ / pcnt of auc_sort_pieces: every user's FULL list; bins / ties of rank_bins: the call ADDS this owner's counts into them
    (user u's n + 1 bins from list_off[u] + u on); force_wide as in dot_catalog_ranks -> None [every pair's score (U, I_loc)]
    (brDotRankCount)."""
    U, I, dim, ld_q, ld_c, dev = _dot_catalog_args("dot_rank_count", Q, C, None, DOT_WIDE_MAX_DIM)
    off, idx = _csr((skip_off, skip_idx), U, "skip")
    cap = _rank_bins_args("dot_rank_count", U, list_off, sorted_, pcnt, bins, ties)
    dump = torch.empty(U, I, dtype=torch.float32, device=dev) if dump_scores else None
    if U == 0:                     # no user, nothing to add (and no valid pointer for Q)
        return dump
    check(_lib.load().brDotRankCount(Q.data_ptr(), ld_q, U, C.data_ptr(), ld_c, I, dim, off.data_ptr(), idx.data_ptr(), list_off.data_ptr(),
                                     sorted_.data_ptr(), pcnt.data_ptr(), cap, bins.data_ptr(), ties.data_ptr(),
                                     _p(dump), _wide_flags(force_wide), _stream()), "brDotRankCount")
    return dump


def _rank_entry_args(who: str, U: int, entry_off, entry_idx, raw, exclude):
    off, idx = _csr((entry_off, entry_idx), U, "entries")
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.float32 or not raw.is_cuda or not raw.is_contiguous() or raw.dim() != 1:
        raise TypeError(f"{who}: raw must be a contiguous 1-D float32 device tensor")
    xoff, xidx = _csr(exclude, U, "exclude") if exclude is not None else (None, None)
    return off, idx, (raw if raw.numel() else torch.zeros(1, dtype=torch.float32, device=off.device)), xoff, xidx


def rank_bins_excluded(entry_off, entry_idx, exclude, raw, list_off, sorted_, pcnt, bins, ties):
    """(entry_off, entry_idx): the truth entries ranked here, raw: their scores, at least entry_off[-1] of them (neumf_auc_positives,
    dot_auc_owner_positives; entry_idx may have spare capacity behind them, as csr_split_by_owner leaves it), exclude:
    (off, idx) CSR in the positions of entry_idx (LOCAL ones at an owner); list_off / sorted_ / pcnt / bins / ties as neumf_rank_count:
    every entry that is also excluded takes 1 out of its bin and its tie bin, in place (brRankBinsExcluded)."""
    U = list_off.numel() - 1
    cap = _rank_bins_args("rank_bins_excluded", U, list_off, sorted_, pcnt, bins, ties)
    if exclude is None:
        raise ValueError("rank_bins_excluded: an exclusion CSR is required")
    off, idx, raw, xoff, xidx = _rank_entry_args("rank_bins_excluded", U, entry_off, entry_idx, raw, exclude)
    check(_lib.load().brRankBinsExcluded(off.data_ptr(), idx.data_ptr(), xoff.data_ptr(), xidx.data_ptr(), raw.data_ptr(), list_off.data_ptr(),
                                         sorted_.data_ptr(), pcnt.data_ptr() if U else sorted_.data_ptr(), cap, U, bins.data_ptr(), ties.data_ptr(),
                                         _stream()), "brRankBinsExcluded")


def rank_bins_finalize(entry_off, entry_idx, exclude, raw, list_off, sorted_, pcnt, bins, ties):
    """The arguments of rank_bins_excluded (exclude may be None) over the bins summed over all owners -> (above, tied) int32, one per
    entry of entry_idx (its capacity), (-1, -1) for an entry without a rank and past entry_off[-1].  The suffix sums are formed in `bins` IN PLACE: one call per copy of the
    bins (brRankBinsFinalize)."""
    U = list_off.numel() - 1
    cap = _rank_bins_args("rank_bins_finalize", U, list_off, sorted_, pcnt, bins, ties)
    off, idx, raw, xoff, xidx = _rank_entry_args("rank_bins_finalize", U, entry_off, entry_idx, raw, exclude)
    n = entry_idx.numel()
    above = torch.full((max(n, 1),), -1, dtype=torch.int32, device=off.device)
    tied = torch.full((max(n, 1),), -1, dtype=torch.int32, device=off.device)
    check(_lib.load().brRankBinsFinalize(off.data_ptr(), idx.data_ptr(), _p(xoff), _p(xidx), raw.data_ptr(), list_off.data_ptr(), sorted_.data_ptr(),
                                         pcnt.data_ptr() if U else sorted_.data_ptr(), cap, U, bins.data_ptr(), ties.data_ptr(), above.data_ptr(),
                                         tied.data_ptr(), _stream()), "brRankBinsFinalize")
    return above[:n], tied[:n]


# ------------------------------------------------------------------------------ 8f-1 evaluation: full AUC, MAP@k, hit counts
def truth_csr(n_users: int, user_rows, item_cols, device):
    """Ground truth of `n_users` rows as the CSR the eval kernels take: (offsets int64 (n_users + 1), column indices int32 ascending
    per user).  user_rows / item_cols: equal-length integer sequences (row index into the scored users, column index into the
    scored items); duplicates are dropped.  Host-side index plumbing (numpy), done once per evaluation."""
    import numpy as np
    u = np.asarray(user_rows, dtype=np.int64); c = np.asarray(item_cols, dtype=np.int64)
    key = np.unique(u * (int(c.max()) + 1 if c.size else 1) + c) if u.size else np.empty(0, np.int64)
    m = int(c.max()) + 1 if c.size else 1
    uu, cc = key // m, key % m
    off = np.zeros(n_users + 1, dtype=np.int64)
    np.add.at(off, uu + 1, 1)
    off = np.cumsum(off)
    return torch.from_numpy(off).to(device), torch.from_numpy(cc.astype(np.int32)).to(device)


def full_auc(scores, truth_off, truth_idx):
    """per-user roc_auc_score over all scored items (src/models/bpr.py:230-254); NaN where undefined."""
    U, I = scores.shape
    out = torch.empty(U, dtype=torch.float32, device=scores.device)
    check(_lib.load().brFullAuc(_f32(scores, "scores").data_ptr(), scores.stride(0), truth_off.data_ptr(), truth_idx.data_ptr(), U, I,
                                out.data_ptr(), _stream()), "brFullAuc")
    return out


def map_at_k(topk_index, truth_off, truth_idx, want_ap=True, want_hits=True):
    """(AP@k per user, hits per user) of top-k index lists (src/models/bpr.py:257-289; trainers/topKmetrics.py:85-93)."""
    U, k = topk_index.shape
    ap = torch.empty(U, dtype=torch.float32, device=topk_index.device) if want_ap else None
    hits = torch.empty(U, dtype=torch.int32, device=topk_index.device) if want_hits else None
    check(_lib.load().brMapAtK(topk_index.contiguous().data_ptr(), U, k, truth_off.data_ptr(), truth_idx.data_ptr(), _p(ap), _p(hits), _stream()),
          "brMapAtK")
    return ap, hits


# ------------------------------------------------------------------------------ 8f-2 batch construction on the device
def positives_csr(users, items, num_users: int, device):
    """The users' positives as CSR (offsets int64 (num_users + 1), items ascending per user, dtype of `items`): the membership
    structure of the rejection samplers.  Built once per dataset on the host (numpy lexsort: index plumbing, not the hot path)."""
    import numpy as np
    u = np.asarray(users.cpu() if torch.is_tensor(users) else users).astype(np.int64)
    i = np.asarray(items.cpu() if torch.is_tensor(items) else items).astype(np.int64)
    order = np.lexsort((i, u))
    u, i = u[order], i[order]
    keep = np.ones(len(u), bool)
    keep[1:] = (u[1:] != u[:-1]) | (i[1:] != i[:-1])
    u, i = u[keep], i[keep]
    off = np.zeros(num_users + 1, dtype=np.int64)
    np.add.at(off, u + 1, 1)
    dt = items.dtype if torch.is_tensor(items) else torch.int32
    return torch.from_numpy(np.cumsum(off)).to(device), torch.from_numpy(i).to(device).to(dt)


def bootstrap_dataset(users, items, n_neg: int, seed: int):
    """NeuMFModel.bootstrapDataset on the device -> (users, items, labels) of n + n_neg shuffled samples."""
    u, ut = _ids(users, "users"); i, it = _ids(items, "items")
    ty = _same_id_type(ut, it)
    n = u.shape[0]
    ou, oi = torch.empty(n + n_neg, dtype=u.dtype, device=u.device), torch.empty(n + n_neg, dtype=u.dtype, device=u.device)
    oy = torch.empty(n + n_neg, dtype=torch.float32, device=u.device)
    check(_lib.load().brBootstrapDataset(u.data_ptr(), i.data_ptr(), ty, n, int(n_neg), int(seed), ou.data_ptr(), oi.data_ptr(), oy.data_ptr(), _stream()),
          "brBootstrapDataset")
    return ou, oi, oy


def bpr_sample_triplets(users, items, pos_off, pos_items, neg_per_pos: int, seed: int, n_cand: int, cand_items=None, max_tries: int = 16):
    """Sampled BPR triplets -> (users, positives, negatives), n * neg_per_pos each."""
    u, ut = _ids(users, "users"); i, it = _ids(items, "items")
    ty = _same_id_type(ut, it)
    n = u.shape[0]
    T = n * int(neg_per_pos)
    ou, op, on = (torch.empty(T, dtype=u.dtype, device=u.device) for _ in range(3))
    check(_lib.load().brBprSampleTriplets(u.data_ptr(), i.data_ptr(), ty, n, int(neg_per_pos), pos_off.data_ptr(), pos_items.data_ptr(), _p(cand_items),
                                          int(n_cand), int(seed), int(max_tries), ou.data_ptr(), op.data_ptr(), on.data_ptr(), _stream()),
          "brBprSampleTriplets")
    return ou, op, on


def alias_table(weights, device=None):
    """Walker's alias table of `weights` (any non-negative numbers, not all zero) for brBprSampleNegatives -> (thresh uint32, alias
    int32), n each: a draw takes slot s uniformly and keeps it iff a second uniform u32 is < thresh[s], else alias[s].  Built on the
    host in numpy float64, deterministically (index plumbing, once per dataset).  thresh = min(floor(p * 2^32), 2^32 - 1) with p the
    slot's keep probability; where it saturates the slot is its own alias, so the kernel's strict `<` is exact; a zero weight gives
    thresh 0 (never kept) and is nobody's alias."""
    import numpy as np
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
    if w.size == 0 or np.isnan(w).any() or (w < 0).any() or not np.isfinite(w).all():
        raise ValueError("alias_table: weights must be finite and non-negative")
    tot = w.sum()
    if not tot > 0:
        raise ValueError("alias_table: all weights are zero")
    n = w.size
    p = w * (n / tot)                          # keep probabilities before pairing: mean 1
    alias = np.arange(n, dtype=np.int64)
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if p[i] >= 1.0]
    keep = np.ones(n, dtype=np.float64)
    while small and large:
        s, l = small.pop(), large[-1]
        keep[s], alias[s] = p[s], l
        p[l] -= 1.0 - p[s]                     # the large slot gives the small one's remainder
        if p[l] < 1.0:
            large.pop()
            small.append(l)
    # what is left (rounding) keeps its own slot with probability 1 - except a zero weight stranded among the small ones
    for s in small:
        if w[s] == 0.0:
            keep[s], alias[s] = 0.0, int(np.argmax(w))
    thresh = np.minimum(np.floor(keep * 4294967296.0), 4294967295.0)
    sat = thresh >= 4294967295.0
    alias[sat] = np.arange(n)[sat]
    dev = device if device is not None else (weights.device if torch.is_tensor(weights) else "cpu")
    return (torch.from_numpy(thresh.astype(np.uint32)).to(dev), torch.from_numpy(alias.astype(np.int32)).to(dev))


def bpr_sample_negatives(users, pos_off, pos_items, n_cand: int, seed: int, draw_step: int, pos0: int = 0, cand_items=None, alias=None, candidates: int = 1,
                         max_tries: int = 16, user=None, item=None, step_state=None, beta1=0.9, beta2=0.999, eps=1e-7, out=None, dump=False,
                         err_flag=None):
    """The negatives of one batch, drawn for this step (brBprSampleNegatives, csrc/sampling_step.hip): negative b is a pure function of
    (seed, draw_step, pos0 + b) - uniform over the candidates, or by `alias` = ops.alias_table(weights) - and, candidates = M > 1, the
    hardest of M candidates under the tables as of the last completed step.  user / item: (table,) for current tables (sweep / lazy
    Adam) or (table, m, v, last) for deferred ones (then step_state is needed); both None for M == 1.  -> out (B,) ids, and with
    dump=True also (cands (B, M) ids, scores (B, M) float32).  No host sync."""
    u, ty = _ids(users, "users")
    _, pt = _ids(pos_items, "pos_items")
    ty = _same_id_type(ty, pt)
    M, B, dev = int(candidates), u.shape[0], u.device
    if not 1 <= M <= 32:
        raise ValueError("candidates must be in [1, 32]")
    if not 1 <= int(max_tries) <= 256:
        raise ValueError("max_tries must be in [1, 256]")
    if pos_off.dtype != torch.int64 or not pos_off.is_cuda or not pos_off.is_contiguous():
        raise TypeError("pos_off: expected contiguous int64 device offsets")
    if cand_items is not None:
        _, ct = _ids(cand_items, "cand_items")
        ty = _same_id_type(ty, ct)
        if cand_items.shape[0] != n_cand:
            raise ValueError("cand_items must hold n_cand ids")
    thresh = alias_to = None
    if alias is not None:
        thresh, alias_to = alias
        if thresh.dtype != torch.uint32 or alias_to.dtype != torch.int32 or not (thresh.is_cuda and alias_to.is_cuda and thresh.is_contiguous() and alias_to.is_contiguous()) \
                or thresh.shape[0] != n_cand or alias_to.shape[0] != n_cand:
            raise TypeError("alias: (uint32 thresh, int32 alias) contiguous device tensors of n_cand entries (ops.alias_table)")
    tu = ti = (None, None, None, None)
    dim = 0
    if M > 1:
        if user is None or item is None:
            raise ValueError("candidates > 1 scores the candidates: the user and item tables are required")
        if len(user) != len(item) or len(user) not in (1, 4):
            raise ValueError("user / item: (table,) or (table, m, v, last), the same form for both")
        user, item = tuple(user), tuple(item)
        for t in user[:3] + item[:3]:
            _f32(t, "table / moment")
        for name, tab in (("user", user), ("item", item)):
            if tab[0].dim() != 2:
                raise ValueError(f"{name}: the table must be (rows, dim)")
            if len(tab) == 4:
                if tab[1].shape != tab[0].shape or tab[2].shape != tab[0].shape:
                    raise ValueError(f"{name}: m and v must have the table's shape")
                last = tab[3]
                if last.dtype != torch.int32 or not last.is_cuda or not last.is_contiguous() or last.dim() != 1 or last.shape[0] != tab[0].shape[0]:
                    raise TypeError(f"{name}: last must be a contiguous int32 device tensor with one entry per table row")
        if user[0].shape[1] != item[0].shape[1]:
            raise ValueError("the user and the item table must have the same dim")
        dim = user[0].shape[1]
        tu, ti = tuple(user) + (None,) * (4 - len(user)), tuple(item) + (None,) * (4 - len(item))
        if len(user) == 4 and step_state is None:
            raise ValueError("deferred tables need the step state")
    if out is None:
        out = torch.empty(B, dtype=u.dtype, device=dev)
    elif out.dtype != u.dtype or not out.is_contiguous() or out.shape[0] != B:
        raise TypeError("out: contiguous ids of the users' dtype, one per row")
    cands = torch.empty(B, M, dtype=u.dtype, device=dev) if dump else None
    scores = torch.empty(B, M, dtype=torch.float32, device=dev) if dump else None
    check(_lib.load().brBprSampleNegatives(u.data_ptr(), ty, B, int(pos0), int(draw_step) & 0xFFFFFFFF, pos_off.data_ptr(), pos_items.data_ptr(), pos_off.shape[0] - 1,
                                           _p(cand_items), int(n_cand), _p(thresh), _p(alias_to), int(seed), M, int(max_tries),
                                           _p(tu[0]), _p(tu[1]), _p(tu[2]), _p(tu[3]), 0 if tu[0] is None else tu[0].shape[0],
                                           _p(ti[0]), _p(ti[1]), _p(ti[2]), _p(ti[3]), 0 if ti[0] is None else ti[0].shape[0], dim,
                                           _p(step_state) if M > 1 and tu[1] is not None else 0, beta1, beta2, eps, out.data_ptr(), _p(cands), _p(scores),
                                           _p(err_flag), _stream()), "brBprSampleNegatives")
    return (out, cands, scores) if dump else out


def neumf_sample_batch(pos_users, pos_items, pos_off, pos_sorted_items, n_cand: int, neg_per_pos: int, seed: int, epoch: int, row0: int, batch: int,
                       cand_items=None, alias=None, max_tries: int = 16, out=None, err_flag=None):
    """Rows [row0, row0 + batch) of epoch `epoch` of the NeuMF fit, formed for this step (brNeumfSampleBatch, csrc/sampling_epoch.hip): a
    pure function of (seed, epoch, global row) - every positive (pos_users, pos_items) once per epoch with label 1 and neg_per_pos
    negatives per positive with label 0, uniform over the candidates or by `alias` = ops.alias_table(weights), re-drawn while they are
    positives of the user (pos_off / pos_sorted_items: ops.positives_csr).  out: optional (users, items, labels) to write into.
    -> (users, items, labels) of `batch` rows, ids in the positives' dtype, labels float32.  No host sync."""
    # (the dtypes first: a mismatch is refused wherever the tensors live)
    _same_id_type(*(t.dtype for t in (pos_users, pos_items, pos_sorted_items, cand_items) if t is not None))
    pu, ty = _ids(pos_users, "pos_users")
    pi, it = _ids(pos_items, "pos_items")
    _, pt = _ids(pos_sorted_items, "pos_sorted_items")
    ty = _same_id_type(ty, it, pt)
    if pu.dim() != 1 or pu.shape != pi.shape or pu.shape[0] < 1:
        raise ValueError("pos_users and pos_items: one id each per positive, at least one")
    n, r, B, dev = pu.shape[0], int(neg_per_pos), int(batch), pu.device
    if r < 0:
        raise ValueError("neg_per_pos must be >= 0")
    if not 1 <= int(max_tries) <= 256:
        raise ValueError("max_tries must be in [1, 256]")
    if pos_off.dtype != torch.int64 or not pos_off.is_cuda or not pos_off.is_contiguous():
        raise TypeError("pos_off: expected contiguous int64 device offsets")
    if n * (1 + r) >= 1 << 32:
        raise ValueError("an epoch of n (1 + neg_per_pos) rows must have fewer than 2^32")
    if int(row0) < 0 or B < 0 or int(row0) + B > n * (1 + r):
        raise ValueError("rows [row0, row0 + batch) must lie inside the epoch's n (1 + neg_per_pos) rows")
    if cand_items is not None:
        _, ct = _ids(cand_items, "cand_items")
        ty = _same_id_type(ty, ct)
        if cand_items.shape[0] != n_cand:
            raise ValueError("cand_items must hold n_cand ids")
    thresh = alias_to = None
    if alias is not None:
        thresh, alias_to = alias
        if thresh.dtype != torch.uint32 or alias_to.dtype != torch.int32 or not (thresh.is_cuda and alias_to.is_cuda and thresh.is_contiguous() and alias_to.is_contiguous()) \
                or thresh.shape[0] != n_cand or alias_to.shape[0] != n_cand:
            raise TypeError("alias: (uint32 thresh, int32 alias) contiguous device tensors of n_cand entries (ops.alias_table)")
    if out is None:
        ou, oi = torch.empty(B, dtype=pu.dtype, device=dev), torch.empty(B, dtype=pu.dtype, device=dev)
        oy = torch.empty(B, dtype=torch.float32, device=dev)
    else:
        ou, oi, oy = out
        for t in (ou, oi):
            if t.dtype != pu.dtype or not t.is_cuda or not t.is_contiguous() or t.numel() != B:
                raise TypeError("out: (users, items) contiguous device ids of the positives' dtype, one per row")
        _f32(oy, "out labels")
        if oy.numel() != B:
            raise TypeError("out: labels, one float32 per row")
    check(_lib.load().brNeumfSampleBatch(pu.data_ptr(), pi.data_ptr(), ty, n, r, pos_off.data_ptr(), pos_sorted_items.data_ptr(), pos_off.shape[0] - 1,
                                         _p(cand_items), int(n_cand), _p(thresh), _p(alias_to), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, int(row0), B,
                                         int(max_tries), ou.data_ptr(), oi.data_ptr(), oy.data_ptr(), _p(err_flag), _stream()), "brNeumfSampleBatch")
    return ou, oi, oy


def ncf_negatives(users, items, pos_off, pos_items, num_items: int, size: int, seed: int, oversample: float = 1.3, max_rounds: int = 8):
    """generateNegativeFeedback on the device: `size` DISTINCT (user, item) pairs outside the positives, users and items drawn by
    shuffling the two columns independently.  One host sync per round (the count of distinct valid candidates)."""
    u, ut = _ids(users, "users"); i, it = _ids(items, "items")
    ty = _same_id_type(ut, it)
    n, dev, lib = u.shape[0], u.device, _lib.load()
    n_cand = int(size * oversample) + n
    for _ in range(max_rounds):
        keys = torch.empty(n_cand, dtype=torch.int64, device=dev)
        check(lib.brNcfNegativeCandidates(u.data_ptr(), i.data_ptr(), ty, n, n_cand, pos_off.data_ptr(), pos_items.data_ptr(), int(num_items), int(seed),
                                          keys.data_ptr(), _stream()), "brNcfNegativeCandidates")
        wsb = int(lib.brSortUniqueWorkspaceBytes(n_cand))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        uniq = torch.empty(n_cand, dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib.brSortUniqueKeys64(keys.data_ptr(), n_cand, uniq.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, _stream()), "brSortUniqueKeys64")
        n_u = int(cnt.item())
        if n_u and int(uniq[n_u - 1].item()) == -1:      # the ~0 key of the rejected candidates sorts last
            n_u -= 1
        if n_u >= size:
            ou, oi = torch.empty(size, dtype=u.dtype, device=dev), torch.empty(size, dtype=u.dtype, device=dev)
            check(lib.brGatherPermutedPairs(uniq.data_ptr(), n_u, size, int(num_items), int(seed), ty, ou.data_ptr(), oi.data_ptr(), _stream()),
                  "brGatherPermutedPairs")
            return ou, oi
        n_cand = int(n_cand * 1.6) + n        # more rounds of column shuffles
    raise RuntimeError("ncf_negatives: not enough distinct negatives (is the interaction matrix nearly full?)")


# ------------------------------------------------------------------------------ implicit-feedback ALS (csrc/als.hip)
ALS_MAX_DIM = 128          # widest rows brGram / brAlsSolveRows take
ALS_CG_MAX_DIM = 512       # widest rows brGramWide / brAlsSolveRowsCg take (csrc/als_wide.hip)


def _ld(t) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def gram(Y, out=None):
    """G = Y^T Y (dim x dim float32, both triangles, exactly symmetric) of the rows x dim table Y (any row stride >= dim) on the
    fp32-input MFMA; the workgroups' partials are added in a fixed order in double: two calls give the same bits.  dim <= 128 is
    brGram; 129 .. 512 is brGramWide, the same contract in blocks of 128 columns."""
    if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
        raise ValueError("gram: Y must be a 2-D tensor")
    rows, dim = Y.shape
    if not 1 <= dim <= ALS_CG_MAX_DIM:
        raise ValueError(f"gram: dim = {dim}: 1 <= dim <= {ALS_CG_MAX_DIM}")
    _rows_f32(Y, "Y")
    if out is None:
        out = torch.empty(dim, dim, dtype=torch.float32, device=Y.device)
    elif tuple(out.shape) != (dim, dim):
        raise ValueError(f"gram: out must be ({dim}, {dim})")
    lib = _lib.load()
    size, run, name = (lib.brGramWorkspaceBytes, lib.brGram, "brGram") if dim <= ALS_MAX_DIM else (lib.brGramWideWorkspaceBytes, lib.brGramWide, "brGramWide")
    ws_bytes = int(size(rows, dim))
    if ws_bytes < 0:
        raise ValueError(f"gram: bad sizes rows={rows} dim={dim}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=Y.device)
    check(run(Y.data_ptr(), _ld(Y), rows, dim, _f32(out, "out").data_ptr(), ws.data_ptr(), ws_bytes, _stream()), name)
    return out


def als_solve_rows(Y, G, off, idx, reg, alpha, conf=None, out=None, err_flag=None):
    """One ALS half-step: for every row u of the CSR (off int64 [n_rows + 1], idx int32 positions into Y ascending per row -
    ops.truth_csr / als.csr_pair - conf float32 >= 0 per entry or None = 1), c_e = alpha * conf[e],
        out[u] = (G + reg I + sum_e c_e y_e y_e^T)^-1 sum_e (1 + c_e) y_e
    with G = ops.gram(Y); a row without entries gets exact zeros.  out: (n_rows, dim) float32, any row stride >= dim (columns past
    dim are left alone).  An idx outside Y sets BR_ERRFLAG_RANGE in err_flag and counts as absent."""
    if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
        raise ValueError("als_solve_rows: Y must be a 2-D tensor")
    n_y, dim = Y.shape
    if not 1 <= dim <= ALS_MAX_DIM:
        raise ValueError(f"als_solve_rows: dim = {dim}: 1 <= dim <= {ALS_MAX_DIM}")
    _rows_f32(Y, "Y")
    if tuple(G.shape) != (dim, dim):
        raise ValueError(f"als_solve_rows: G must be ({dim}, {dim})")
    _f32(G, "G")
    n_rows = off.shape[0] - 1
    off, idx_ = _csr((off, idx), n_rows, "csr")
    if conf is not None:
        if conf.dtype != torch.float32 or not conf.is_cuda or not conf.is_contiguous() or conf.shape != idx.shape:
            raise TypeError("als_solve_rows: conf must be a contiguous float32 device tensor, one value per idx entry")
        if conf.numel() == 0:
            conf = None
    if out is None:
        out = torch.empty(n_rows, dim, dtype=torch.float32, device=Y.device)
    elif out.dim() != 2 or out.shape[0] != n_rows or out.shape[1] < dim:
        raise ValueError(f"als_solve_rows: out must be ({n_rows}, >= {dim})")
    _rows_f32(out, "out")
    check(_lib.load().brAlsSolveRows(Y.data_ptr(), _ld(Y), n_y, dim, G.data_ptr(), off.data_ptr(), idx_.data_ptr(), _p(conf), float(alpha),
                                     float(reg), n_rows, out.data_ptr(), _ld(out), _p(err_flag), _stream()), "brAlsSolveRows")
    return out


def als_solve_rows_cg(Y, G, off, idx, reg, alpha, x, steps=3, conf=None, err_flag=None):
    """One ALS half-step by `steps` (1 .. 64) conjugate-gradient steps per row, in place on x (n_rows, >= dim) float32, any row stride
    >= dim (columns past dim are left alone): every row starts from its current vector (Takacs, Pilaszy, Tikk 2011; brAlsSolveRowsCg,
    csrc/als_wide.hip).  The operator A_u = G + reg I + sum_e c_e y_e y_e^T of als_solve_rows is applied, never formed, so rows up to
    ALS_CG_MAX_DIM = 512 features are taken.  CSR, conf, G = ops.gram(Y) and err_flag as for als_solve_rows; a row without entries
    gets exact zeros.  -> x."""
    if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
        raise ValueError("als_solve_rows_cg: Y must be a 2-D tensor")
    n_y, dim = Y.shape
    if not 1 <= dim <= ALS_CG_MAX_DIM:
        raise ValueError(f"als_solve_rows_cg: dim = {dim}: 1 <= dim <= {ALS_CG_MAX_DIM}")
    if not 1 <= int(steps) <= 64:
        raise ValueError(f"als_solve_rows_cg: steps = {steps}: 1 <= steps <= 64")
    _rows_f32(Y, "Y")
    if tuple(G.shape) != (dim, dim):
        raise ValueError(f"als_solve_rows_cg: G must be ({dim}, {dim})")
    _f32(G, "G")
    n_rows = off.shape[0] - 1
    off, idx_ = _csr((off, idx), n_rows, "csr")
    if conf is not None:
        if conf.dtype != torch.float32 or not conf.is_cuda or not conf.is_contiguous() or conf.shape != idx.shape:
            raise TypeError("als_solve_rows_cg: conf must be a contiguous float32 device tensor, one value per idx entry")
        if conf.numel() == 0:
            conf = None
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != n_rows or x.shape[1] < dim:
        raise ValueError(f"als_solve_rows_cg: x must be ({n_rows}, >= {dim})")
    _rows_f32(x, "x")
    check(_lib.load().brAlsSolveRowsCg(Y.data_ptr(), _ld(Y), n_y, dim, G.data_ptr(), off.data_ptr(), idx_.data_ptr(), _p(conf), float(alpha),
                                       float(reg), n_rows, x.data_ptr(), _ld(x), int(steps), _p(err_flag), _stream()), "brAlsSolveRowsCg")
    return x


# ------------------------------------------------------------------------------ ALS, the heavy rows (csrc/als_heavy.hip)
ALS_HEAVY_SLICE = 4096     # entries of a slice of brAlsNormalRows: one workgroup per slice and pair of 128-column blocks
ALS_HEAVY_ROWS = 256       # the recommended ALSEngine(heavy_rows=): the best of 256 .. 65 536 measured - a recommendation, not a default


def als_slice_prefix(off, rows, slice: int = ALS_HEAVY_SLICE):
    """-> int64 [len(rows) + 1]: the slices of `slice` entries of every listed row, as a prefix sum (torch ops on off's device)"""
    r = rows.long()
    n = (off[r + 1] - off[r] + (int(slice) - 1)) // int(slice)
    out = torch.zeros(r.shape[0] + 1, dtype=torch.int64, device=off.device)
    out[1:] = torch.cumsum(n, 0)
    return out


def als_normal_rows(Y, off, idx, alpha, rows, conf=None, slice=ALS_HEAVY_SLICE, err_flag=None, plan=None):
    """The normal matrix of the listed rows of the CSR, formed once by many workgroups (brAlsNormalRows): with c_e = alpha * conf[e]
        H[h] = sum_e c_e y_e y_e^T (float32 (n, dim, dim), bit-equal to its transpose),   b[h] = sum_e (1 + c_e) y_e (float64 (n, dim))
    over the entries of row rows[h].  rows: int32 device tensor, ascending and unique; slice: entries per workgroup, a multiple of 64;
    plan = (slice prefix int64 [n + 1] on the device, its last value as an int), made once per CSR (als.split_heavy) - None derives
    it here (a host sync).  CSR, conf and err_flag as for als_solve_rows; H[h] and b[h] do not depend on the other listed rows, and two
    calls give the same bits.  -> (H, b)"""
    if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
        raise ValueError("als_normal_rows: Y must be a 2-D tensor")
    n_y, dim = Y.shape
    if not 1 <= dim <= ALS_CG_MAX_DIM:
        raise ValueError(f"als_normal_rows: dim = {dim}: 1 <= dim <= {ALS_CG_MAX_DIM}")
    if int(slice) < 64 or int(slice) % 64:
        raise ValueError(f"als_normal_rows: slice = {slice} must be a multiple of 64, at least 64")
    _rows_f32(Y, "Y")
    n_rows = off.shape[0] - 1
    off, idx_ = _csr((off, idx), n_rows, "csr")
    if conf is not None:
        if conf.dtype != torch.float32 or not conf.is_cuda or not conf.is_contiguous() or conf.shape != idx.shape:
            raise TypeError("als_normal_rows: conf must be a contiguous float32 device tensor, one value per idx entry")
        if conf.numel() == 0:
            conf = None
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or not rows.is_cuda or not rows.is_contiguous() or rows.dim() != 1:
        raise TypeError("als_normal_rows: rows must be a contiguous int32 device vector")
    n = rows.shape[0]
    if plan is None:
        pre = als_slice_prefix(off, rows, slice)
        plan = (pre, int(pre[-1].item()))
    pre, n_slices = plan
    if pre.dtype != torch.int64 or not pre.is_cuda or not pre.is_contiguous() or tuple(pre.shape) != (n + 1,):
        raise TypeError(f"als_normal_rows: the slice prefix must be a contiguous int64 device vector of {n + 1}")
    H = torch.empty(n, dim, dim, dtype=torch.float32, device=Y.device)
    b = torch.empty(n, dim, dtype=torch.float64, device=Y.device)
    lib = _lib.load()
    ws_bytes = int(lib.brAlsNormalRowsWorkspaceBytes(int(n_slices), dim))
    if ws_bytes < 0:
        raise ValueError(f"als_normal_rows: bad sizes slices={n_slices} dim={dim}")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=Y.device)
    check(lib.brAlsNormalRows(Y.data_ptr(), _ld(Y), n_y, dim, off.data_ptr(), idx_.data_ptr(), _p(conf), float(alpha), n_rows, rows.data_ptr(),
                              pre.data_ptr(), n, int(n_slices), int(slice), H.data_ptr(), b.data_ptr(), ws.data_ptr(), ws_bytes, _p(err_flag),
                              _stream()), "brAlsNormalRows")
    return H, b


def als_solve_rows_dense_cg(G, H, b, reg, x0, steps=3, out=None):
    """`steps` (1 .. 64) conjugate-gradient steps of als_solve_rows_cg on the formed operators A_h = G + reg I + H[h] with right-hand
    sides b[h] (als_normal_rows), from x0 (n, dim) float32 contiguous (brAlsSolveRowsDenseCg): the sums in double, x rounded once.
    out: (n, >= dim) float32, any row stride >= dim (columns past dim are left alone).  -> out"""
    if not isinstance(G, torch.Tensor) or G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("als_solve_rows_dense_cg: G must be (dim, dim)")
    dim = G.shape[0]
    if not 1 <= dim <= ALS_CG_MAX_DIM:
        raise ValueError(f"als_solve_rows_dense_cg: dim = {dim}: 1 <= dim <= {ALS_CG_MAX_DIM}")
    if not 1 <= int(steps) <= 64:
        raise ValueError(f"als_solve_rows_dense_cg: steps = {steps}: 1 <= steps <= 64")
    _f32(G, "G")
    if not isinstance(H, torch.Tensor) or H.dim() != 3 or tuple(H.shape[1:]) != (dim, dim):
        raise ValueError(f"als_solve_rows_dense_cg: H must be (n, {dim}, {dim})")
    _f32(H, "H")
    n = H.shape[0]
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64 or not b.is_cuda or not b.is_contiguous() or tuple(b.shape) != (n, dim):
        raise TypeError(f"als_solve_rows_dense_cg: b must be a contiguous float64 device tensor ({n}, {dim})")
    if not isinstance(x0, torch.Tensor) or tuple(x0.shape) != (n, dim):
        raise ValueError(f"als_solve_rows_dense_cg: x0 must be ({n}, {dim})")
    _f32(x0, "x0")
    if out is None:
        out = torch.empty(n, dim, dtype=torch.float32, device=G.device)
    elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < dim:
        raise ValueError(f"als_solve_rows_dense_cg: out must be ({n}, >= {dim})")
    _rows_f32(out, "out")
    check(_lib.load().brAlsSolveRowsDenseCg(G.data_ptr(), H.data_ptr(), b.data_ptr(), dim, float(reg), x0.data_ptr(), n, int(steps),
                                            out.data_ptr(), _ld(out), _stream()), "brAlsSolveRowsDenseCg")
    return out
