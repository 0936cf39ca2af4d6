"""NeuMF training/inference engine on the HIP hot path (single GPU or one data-parallel rank).

Covers both reference graphs with one parametrisation:
  variant "A": trainers/NFC_plain.py:107-155  (concat [item,user], Dense 100/50/10 sigmoid,
               head concat [mf, mlp], BCE, Adam lr .005)
  variant "B": src/models/NeuMFModel.py:53-100 (concat [user,item], Dense F, F/2, F/4 relu,
               head concat [mlp, mf], MSE, Adam 1e-3)

Every arithmetic op is a libbinrec_hip.so launch (ops.py); torch only owns the buffers, the
stream and (data-parallel) the RCCL collectives.  One training step is the launch sequence in
`NeuMFEngine.train_step` — see DESIGN.md for the kernel-by-kernel data flow.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os

import torch

from . import _lib, ops
from .row_adam import RowAdam
from .sampler import CandidatePool

DENSE_ORDER = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "W3", "b3", "W4", "b4")
TABLES = ("user_mlp", "item_mlp", "user_mf", "item_mf")


@dataclasses.dataclass
class NeuMFConfig:
    variant: str = "A"
    dim: int = 10                       # latent_dim (NFC_plain.py:109) / numFactor (RModel.py:35)
    hidden: tuple | None = None
    lr: float | None = None
    dropout: float = 0.2                # NFC_plain.py:138,141,144 ; NeuMFModel.py:67,71,75
    bn_eps: float = 1e-3                # [TF-sem] Keras BatchNormalization defaults
    bn_momentum: float = 0.99
    beta1: float = 0.9                  # [TF-sem] Keras Adam defaults
    beta2: float = 0.999
    adam_eps: float = 1e-7
    optimizer: str = "adam_dense"       # "adam_dense" = Keras semantics (non-lazy sparse apply);
                                        # "adam_lazy"  = touched rows only (throughput deviation)
    dense_impl: str = "deferred"        # how adam_dense reaches the untouched rows: "deferred" = per-row catch-up
                                        # replay (same values, no per-step table sweep; include/binrec.h
                                        # "Deferred dense Adam"), "sweep" = one pass over the table per step
    replay: str | None = None           # deferred tables: "fast" (default; BR_REPLAY env overrides the default) = the cheaper form of the
                                        # g = 0 recurrence (include/binrec.h BR_REPLAY_FAST: ~1e-6 of a row's movement off the sweep),
                                        # "exact" = the sweep's own fp32 operations (tables bit-equal to dense_impl="sweep")
    seed: int = 0x5EED
    sync_bn: bool = True                # data-parallel: batch statistics over the GLOBAL batch

    def __post_init__(self):
        assert self.variant in ("A", "B")
        assert self.optimizer in ("adam_dense", "adam_lazy")
        assert self.dense_impl in ("deferred", "sweep")
        if self.replay is None:
            self.replay = os.environ.get("BR_REPLAY", "fast")
        assert self.replay in ("fast", "exact")
        if self.variant == "A":
            self.hidden = tuple(self.hidden) if self.hidden else (100, 50, 10)
            self.act, self.item_first, self.mf_first, self.loss = "sigmoid", 1, 1, "bce"
            self.lr = 0.005 if self.lr is None else self.lr
        else:
            self.hidden = tuple(self.hidden) if self.hidden else (self.dim, self.dim // 2, self.dim // 4)
            self.act, self.item_first, self.mf_first, self.loss = "relu", 0, 0, "mse"
            self.lr = 1e-3 if self.lr is None else self.lr

    def dense_shapes(self):
        n1, n2, n3 = self.hidden
        return {"W1": (2 * self.dim, n1), "b1": (n1,), "g1": (n1,), "be1": (n1,),
                "W2": (n1, n2), "b2": (n2,), "g2": (n2,), "be2": (n2,),
                "W3": (n2, n3), "b3": (n3,), "W4": (n3 + 1,), "b4": (1,)}


class _Flat:
    """One flat fp32 buffer with named views (dense parameters / their grads / Adam slots)."""

    def __init__(self, shapes: dict, device):
        self.offsets, off = {}, 0
        for k, shp in shapes.items():
            n = 1
            for s in shp:
                n *= s
            self.offsets[k] = (off, n, shp)
            off += n
        self.numel = off
        self.buf = torch.zeros(off, dtype=torch.float32, device=device)

    def view(self, k):
        off, n, shp = self.offsets[k]
        return self.buf[off:off + n].view(*shp)

    def slice(self, k0, k1):
        """contiguous span covering parameters k0..k1 (adjacent in the layout)."""
        o0 = self.offsets[k0][0]
        o1, n1, _ = self.offsets[k1]
        return self.buf[o0:o1 + n1]


class BatchSampler(CandidatePool):
    """What the per-step batch sampler (NeuMFEngine.sample_batch, csrc/sampling_epoch.hip) needs of a training set: the positives on the
    device, their CSR, the candidate items and - mode "popularity" - the alias table, exactly as bpr.NegativeSampler holds them
    (sampler.py).  An epoch is every positive once (label 1) and neg_per_pos negatives per positive (label 0), drawn again in every
    epoch: rows_per_epoch = n (1 + neg_per_pos) rows in a keyed order, none of them stored.  `epoch` is the next epoch to draw:
    KerasLikeNeuMF.fit(sampler=) advances it, so a second fit repeats no draw."""

    def __init__(self, users, items, n_users: int, neg_per_pos: int = 3, cand_items=None, mode: str = "uniform", power: float = 0.75, seed: int = 0,
                 max_tries: int = 16, n_items: int | None = None, device="cuda"):
        import numpy as np
        if int(neg_per_pos) < 0:
            raise ValueError("neg_per_pos must be >= 0")
        super().__init__(users, items, n_users, cand_items=cand_items, mode=mode, power=power, seed=seed, max_tries=max_tries, device=device, n_items=n_items)
        dt = self.pos_items.dtype
        as_dev = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))).to(self.device).to(dt).contiguous().view(-1)
        self.users, self.items = as_dev(users), as_dev(items)
        if self.users.shape != self.items.shape or self.users.shape[0] < 1:
            raise ValueError("users and items: one id each per positive, at least one")
        self.neg_per_pos = int(neg_per_pos)
        self.rows_per_epoch = int(self.users.shape[0]) * (1 + self.neg_per_pos)
        if self.rows_per_epoch >= 1 << 32:
            raise ValueError("an epoch of n (1 + neg_per_pos) rows must have fewer than 2^32")
        self.epoch = 0


class NeuMFEngine(RowAdam):
    def __init__(self, cfg: NeuMFConfig, num_user_rows: int, num_item_rows: int, device, max_batch: int,
                 id_dtype=torch.int32, init_seed: int = 0, dist=None):
        self.cfg, self.device, self.max_batch, self.id_dtype = cfg, torch.device(device), int(max_batch), id_dtype
        self.num_user_rows, self.num_item_rows = int(num_user_rows), int(num_item_rows)
        self.dist = dist                      # None, or the parallel.DistCtx of the row-sharded subclass
        if dist is not None and not self.sharded:
            # replicated tables would need every rank's row gradients (an all-gather of B x 2*dim per stream): the
            # multi-GPU form of this engine is the row-sharded one
            raise ValueError("a process group is only supported through parallel.make_sharded_engine (row-sharded tables)")
        D, (n1, n2, n3) = cfg.dim, cfg.hidden
        if 2 * D > 256 or max(n1, n2) > 128 or n3 > 32:
            raise ValueError("tower widths: 2*dim <= 256 (first layer, split-K above 128), n1, n2 <= 128 and n3 <= 32 in this build")
        dev = self.device
        g = torch.Generator(device="cpu").manual_seed(init_seed)
        # [TF-sem] Embedding init U(-0.05, 0.05); Dense glorot-uniform; bias 0; BN gamma 1 beta 0
        self._init_tables(g, init_seed)
        self.theta = _Flat(cfg.dense_shapes(), dev)
        for k, (_, _, shp) in self.theta.offsets.items():
            if k.startswith("W"):
                fi, fo = (shp[0], shp[1]) if len(shp) == 2 else (shp[0], 1)
                lim = math.sqrt(6.0 / (fi + fo))
                self.theta.view(k).copy_(((torch.rand(*shp, generator=g) * 2 - 1) * lim).to(dev))
            elif k.startswith("g"):
                self.theta.view(k).fill_(1.0)
        self.grad = _Flat(cfg.dense_shapes(), dev)
        self.adam_m = _Flat(cfg.dense_shapes(), dev)
        self.adam_v = _Flat(cfg.dense_shapes(), dev)
        self.fused_m = {k: torch.zeros_like(v) for k, v in self.fused.items()}
        self.fused_v = {k: torch.zeros_like(v) for k, v in self.fused.items()}
        self._tab_m = {"user_mlp": self.fused_m["user"][:, :D], "user_mf": self.fused_m["user"][:, D:],
                       "item_mlp": self.fused_m["item"][:, :D], "item_mf": self.fused_m["item"][:, D:]}
        self._tab_v = {"user_mlp": self.fused_v["user"][:, :D], "user_mf": self.fused_v["user"][:, D:],
                       "item_mlp": self.fused_v["item"][:, :D], "item_mf": self.fused_v["item"][:, D:]}
        self.moving_buf = torch.zeros(2 * n1 + 2 * n2, device=dev)      # [mm1 | mv1 | mm2 | mv2]
        self.moving = {"mm1": self.moving_buf[:n1], "mv1": self.moving_buf[n1:2 * n1],
                       "mm2": self.moving_buf[2 * n1:2 * n1 + n2], "mv2": self.moving_buf[2 * n1 + n2:]}
        self.moving["mv1"].fill_(1.0)
        self.moving["mv2"].fill_(1.0)
        self._alloc(self.max_batch)

    def local_rows(self, name: str) -> int:
        """rows of `name` held by this process (all of them without row-sharding)."""
        return self.num_user_rows if name.startswith("user") else self.num_item_rows

    def _init_tables(self, g, init_seed):
        """HBM layout: ONE allocation per id stream, rows = [mlp (dim) | mf (dim)] (512 B at dim 64), so
        a lookup touches one contiguous row instead of two; `self.tables` exposes the four reference
        tables (NFC_plain.py:115-126) as column views."""
        D, dev = self.cfg.dim, self.device
        self.fused = {}
        for si, stream in enumerate(("user", "item")):
            rows = self.local_rows(stream + "_mf")
            if rows * 2 * D > (1 << 26):   # big tables: draw on the device (same distribution)
                dg = torch.Generator(device=dev).manual_seed(init_seed + 7919 * (1 + si))
                t = torch.rand(rows, 2 * D, generator=dg, device=dev, dtype=torch.float32).mul_(0.1).sub_(0.05)
            else:
                t = (torch.rand(rows, 2 * D, generator=g) * 0.1 - 0.05).to(dev)
            self.fused[stream] = t
        self._make_views()

    def _make_views(self):
        D = self.cfg.dim
        self._tables = {"user_mlp": self.fused["user"][:, :D], "user_mf": self.fused["user"][:, D:],
                        "item_mlp": self.fused["item"][:, :D], "item_mf": self.fused["item"][:, D:]}

    # the four reference tables / their Adam slots as column views; reading them brings a deferred table up
    # to date first (self.fused* are the raw buffers)
    @property
    def tables(self):
        self.flush()
        return self._tables

    @property
    def tab_m(self):
        self.flush()
        return self._tab_m

    @property
    def tab_v(self):
        self.flush()
        return self._tab_v

    # ------------------------------------------------------------------ buffers
    def _alloc(self, B):
        cfg, dev = self.cfg, self.device
        D, (n1, n2, n3) = cfg.dim, cfg.hidden
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.x0, self.dot = f(B, 2 * D), f(B)
        pad4 = lambda n: (n + 3) & ~3      # rows of the hidden activations / their gradients are padded to 16 B (brNeumfStep)
        self.a1, self.a2, self.a3 = f(B, pad4(n1))[:, :n1], f(B, pad4(n2))[:, :n2], f(B, n3)
        self.logit, self.prob = f(B), f(B)
        self.da3, self.ddot = f(B, n3), f(B)
        self.gh2, self.gh1, self.dx0 = f(B, pad4(n2))[:, :n2], f(B, pad4(n1))[:, :n1], f(B, 2 * D)
        self.g_user, self.g_item = f(B, 2 * D), f(B, 2 * D)      # fused [mlp | mf] row gradients per stream
        # per-step double scratch: [stats1 | stats2 | bsum1 | bsum2], each [BR_STAT_REPLICAS][2n] (the kernels
        # spread their column-sum atomics over 8 replicas; consumers add them)
        R = ops.STAT_REPLICAS
        self.dstat = torch.zeros(R * (4 * n1 + 4 * n2), dtype=torch.float64, device=dev)
        o = 0
        self.stats1 = self.dstat[o:o + R * 2 * n1]; o += R * 2 * n1
        self.stats2 = self.dstat[o:o + R * 2 * n2]; o += R * 2 * n2
        self.bsum1 = self.dstat[o:o + R * 2 * n1]; o += R * 2 * n1
        self.bsum2 = self.dstat[o:o + R * 2 * n2]
        self.msums = torch.zeros(ops.SUM_SLOTS, ops.METRIC_SUMS, dtype=torch.float64, device=dev)   # [slot][loss, se, ae, correct, bce, tp, fp, fn] (epoch)
        self.bn_buf = f(4 * n1 + 4 * n2)      # [scale1|shift1|mean1|rstd1|scale2|shift2|mean2|rstd2]
        self.bn, o = {}, 0
        for k, n in (("scale1", n1), ("shift1", n1), ("mean1", n1), ("rstd1", n1), ("scale2", n2), ("shift2", n2), ("mean2", n2), ("rstd2", n2)):
            self.bn[k] = self.bn_buf[o:o + n]; o += n
        layers = ((2 * D, n1), (n1, n2), (n2, n3))
        # three slab regions [tail | layer 2 | layer 1] (the step driver lays them out; include/binrec.h)
        self.slabs = f(_lib.load().brNeumfStepSlabFloats(B, D, n1, n2, n3))
        self.dz_ws = f(max(ops.dense_backward_ws_floats(B, k, n) for k, n in layers))
        self.nsh = ops.head_slabs(B)
        self.hslabs = f(self.nsh * (n3 + 2))
        self.keep_bits = torch.empty(sum(ops.dropout_keep_words(B, k) for k in (2 * D, n1, n2)), dtype=torch.int32, device=dev)
        self._keep_widths = (2 * D, n1, n2)
        o1, o2 = ops.dropout_keep_words(B, 2 * D), ops.dropout_keep_words(B, 2 * D) + ops.dropout_keep_words(B, n1)
        self._keep_planes = [self.keep_bits[:o1], self.keep_bits[o1:o2], self.keep_bits[o2:]]
        self._keep_for = None                  # (step, row0) whose masks the planes hold (a training step prefetches the next one's)
        self.err = ops.new_err_flag(dev)
        self._alloc_sparse(B)
        self._init_row_adam({k: (self.fused[k], self.fused_m[k], self.fused_v[k]) for k in ("user", "item")}, cfg.optimizer, cfg.dense_impl,
                            cfg.lr, cfg.beta1, cfg.beta2, cfg.adam_eps, cfg.replay)
        self._build_step_struct()

    # ------------------------------------------------------------------ C step driver
    def _build_step_struct(self):
        """brNeumfStep (include/binrec.h): every pointer the fused step driver needs, filled once."""
        lib = _lib.load()

        class Step(ctypes.Structure):
            _fields_ = _lib.parse_struct("brNeumfStep")
        if ctypes.sizeof(Step) != lib.brNeumfStepSizeof():
            raise _lib.BinrecError("brNeumfStep layout mismatch between include/binrec.h and libbinrec_hip.so")
        cfg = self.cfg
        st = Step()
        st.user_rows, st.item_rows = self.local_rows("user_mf"), self.local_rows("item_mf")
        st.dim, (st.n1, st.n2, st.n3) = cfg.dim, cfg.hidden
        st.act, st.loss = ops.ACT[cfg.act], ops.LOSS[cfg.loss]
        st.item_first, st.mf_first = cfg.item_first, cfg.mf_first
        st.id_type = ops.I64 if self.id_dtype == torch.int64 else ops.I32
        # (row-sharded: the table optimizer runs from Python on the owner's shard, the driver never sees it)
        st.adam_dense = (2 if self.deferred else 1 if cfg.optimizer == "adam_dense" else 0) if not self.sharded else 0
        st.dropout, st.bn_eps, st.bn_momentum = cfg.dropout, cfg.bn_eps, cfg.bn_momentum
        st.seed = cfg.seed
        st.bn_local = 1 if (self.dist is not None and not cfg.sync_bn) else 0
        # a data-parallel host all-reduces `grad` between the reduction and the optimizer: per-replica BatchNorm reduces everything in one
        # launch at BNG (2); with global BatchNorm statistics dgamma / dbeta are already global when BNG writes them, AFTER the all-reduce of
        # the locally reduced dW (0: per-phase reductions)
        st.fused_final = 1 if self.dist is None else (0 if cfg.sync_bn else 2)
        st.beta1, st.beta2, st.adam_eps = cfg.beta1, cfg.beta2, cfg.adam_eps
        P = lambda t: t.data_ptr()
        st.user_tab, st.user_m, st.user_v = P(self.fused["user"]), P(self.fused_m["user"]), P(self.fused_v["user"])
        st.item_tab, st.item_m, st.item_v = P(self.fused["item"]), P(self.fused_m["item"]), P(self.fused_v["item"])
        if st.adam_dense == 1:
            st.user_mark, st.item_mark = P(self.mark["user"]), P(self.mark["item"])
        if self.deferred:
            if not self.sharded:
                st.user_last, st.item_last = P(self.last["user"]), P(self.last["item"])
            self._alloc_step_state(st)
        st.theta, st.grad, st.adam_m, st.adam_v = P(self.theta.buf), P(self.grad.buf), P(self.adam_m.buf), P(self.adam_v.buf)
        st.moving = P(self.moving_buf)
        for k in ("x0", "dot", "a1", "a2", "a3", "logit", "prob", "da3", "ddot", "gh2", "gh1", "dx0", "g_user", "g_item"):
            setattr(st, k, P(getattr(self, k)))
        st.bn, st.dstat, st.msums = P(self.bn_buf), P(self.dstat), P(self.msums)
        st.slabs, st.hslabs, st.err_flag, st.dz_ws = P(self.slabs), P(self.hslabs), P(self.err), P(self.dz_ws)
        st.keep_bits = P(self.keep_bits)
        self._bind_indexes(st)
        if not self.sharded and os.environ.get("BR_AUX_STREAM", "1") != "0":
            self.aux_stream = torch.cuda.Stream(device=self.device)     # the dedup sorts run beside fwd/bwd
            st.aux_stream = self.aux_stream.cuda_stream
        self.step_struct = st
        PH = self.PH = {k[6:]: v for k, v in _lib.parse_enums().items() if k.startswith("BR_PH_")}
        PH["OPT_ROWS"] = PH["ROWS_USER"] | PH["SWEEP_USER"] | PH["ROWS_ITEM"] | PH["SWEEP_ITEM"]
        self._graph = None
        self._graph_multi = None

    def _bind_indexes(self, st, ui=None, ii=None):
        """the step's index buffers: the engine's own, or (ui, ii) - a later step of a multi-step group (the segment scratch, written and
        read inside one step, stays the engine's)"""
        ui, ii = ui or self.user_index, ii or self.item_index
        st.u_sorted_ids, st.u_sorted_pos, st.u_ws, st.u_ws_bytes = ui.sorted_ids.data_ptr(), ui.sorted_pos.data_ptr(), ui.ws.data_ptr(), ui.ws_bytes
        st.i_sorted_ids, st.i_sorted_pos, st.i_ws, st.i_ws_bytes = ii.sorted_ids.data_ptr(), ii.sorted_pos.data_ptr(), ii.ws.data_ptr(), ii.ws_bytes
        st.u_seg_ws, st.i_seg_ws = self.user_index.seg_ws(2 * self.cfg.dim).data_ptr(), self.item_index.seg_ws(2 * self.cfg.dim).data_ptr()

    def _run(self, phases: int):
        _lib.check(_lib.load().brNeumfStepRun(ctypes.byref(self.step_struct), phases, ops._stream()), "brNeumfStepRun")

    def _check_batch(self, users, items, labels):
        for t in (users, items):
            if t.dtype != self.id_dtype or not t.is_cuda or not t.is_contiguous():
                raise TypeError(f"ids must be contiguous {self.id_dtype} device tensors")
        if labels is not None and (labels.dtype != torch.float32 or not labels.is_contiguous()):
            raise TypeError("labels must be contiguous float32")

    def _set_batch(self, users, items, labels, B, training, row0, batch_total):
        st = self.step_struct
        self._check_batch(users, items, labels)
        st.batch, st.batch_total, st.row0 = B, batch_total, row0
        st.users, st.items = users.data_ptr(), items.data_ptr()
        st.labels = labels.data_ptr() if labels is not None else None
        st.training, st.step = int(training), self.t
        st.alpha_t = ops.adam_alpha(self.cfg.lr, max(self.t, 1), self.cfg.beta1, self.cfg.beta2)
        # dropout planes: laid out for max_batch rows; a single-process training step prefetches the next step's planes beside its
        # Adam-rows kernel (brNeumfStep.keep_prefetch), and this step skips the generation if it is the one they were made for
        st.keep_rows = self.max_batch
        # 2 (default): the planes and the dense finalize ride in the Adam-rows launch's grid; BR_KEEP_PREFETCH=1: launches of their own
        # on the aux stream beside it (a fork / join inside the step's hipGraph; include/binrec.h keep_prefetch)
        st.keep_prefetch = int(os.environ.get("BR_KEEP_PREFETCH", "2")) if (training and self.dist is None and st.aux_stream) else 0
        st.keep_ready = 1 if (training and self._keep_for == (self.t, row0)) else 0

    def _alloc_sparse(self, B):
        dev = self.device
        self.user_index = ops.RowIndex(B, self.id_dtype, dev)
        self.item_index = ops.RowIndex(B, self.id_dtype, dev)

    def _alloc_step_state(self, st):
        """the device step state (made on first use: sweep and lazy tables need it only under graph replay) in the step struct, at t"""
        st.lr, st.step_state = self.cfg.lr, self._step_state().data_ptr()
        self._set_step_state()

    sharded = False   # the row-sharded subclass runs its own embed exchange (parallel.py)

    def _embed_forward(self, users, items, B):
        raise NotImplementedError   # only the sharded subclass routes the embed block through Python

    # ------------------------------------------------------------------ one optimizer step
    def train_step(self, users, items, labels, row0: int = 0, batch_total: int | None = None):
        """users/items: device int ids (B,), labels: device float32 (B,).  One brNeumfStepRun call on a
        single GPU (no host sync); with a process group the phases are interleaved with the BatchNorm /
        dense-gradient all-reduces and, when row-sharded, the embedding exchange."""
        cfg, PH = self.cfg, self.PH
        B = users.shape[0]
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch}")
        if B == 0:
            if self.dist is not None and self.dist.world > 1:
                # the peers are about to enter the step's collectives: returning here would leave them waiting forever
                raise ValueError("empty local batch in a data-parallel step: give every rank at least one pair (pad or drop the ragged tail)")
            return
        batch_total = B if batch_total is None else batch_total
        self.begin_steps(1)
        self.t += 1
        if self._graph is not None and B == self._graph["batch"] and row0 == 0 and batch_total == B:
            self._replay(users, items, labels)
            return
        self._set_batch(users, items, labels, B, True, row0, batch_total)
        if self.dist is None:
            self._run(PH["ALL"])
            self._keep_for = (self.t + 1, row0) if self.step_struct.keep_prefetch and cfg.dropout > 0 else None
            return
        self._dist_step(users, items, B)

    def _dist_step(self, users, items, B):
        """the launches and collectives of one data-parallel step (after _set_batch): no host sync with the fixed-capacity exchange, so the
        row-sharded engine can capture this body into a hipGraph (parallel.py ShardedNeuMFEngine.enable_graph)."""
        cfg, PH = self.cfg, self.PH
        d, sync = self.dist, cfg.sync_bn
        emb = 0 if self.sharded else PH["EMBED"]
        if self.sharded:
            if self.step_state is not None:
                # the lookup below replays against the device step counter: advance it first (the driver only does
                # so in a call that holds FWD1|EMBED); the same launch clears the step's double scratch
                self._advance_step_state(self.dstat)
            self._embed_forward(users, items, B)
        if not sync:
            # per-replica BatchNorm (what MirroredStrategy does with a plain BatchNormalization [TF-sem]): no collective
            # until the dense gradients, so the whole tower is one driver call
            self._run(PH["FWD1"] | PH["FWD2"] | PH["FWD3"] | PH["BWD2"] | PH["BWD1"] | PH["BNG"] | emb)
            d.all_reduce_sum(self.grad.buf)
        else:
            self._run(PH["FWD1"] | emb)
            d.all_reduce_sum(self.stats1)
            self._run(PH["FWD2"])
            d.all_reduce_sum(self.stats2)
            self._run(PH["FWD3"])
            d.all_reduce_sum(self.bsum2)
            self._run(PH["BWD2"])
            d.all_reduce_sum(self.bsum1)
            self._run(PH["BWD1"])
            # dgamma/dbeta are the BN-backward column sums: global once the sums are, so they are written AFTER
            # the sums' all-reduce and BEFORE nothing else needs them
            d.all_reduce_sum(self.grad.buf)
            self._run(PH["BNG"])
        if self.sharded:
            self._embed_backward_apply(users, items, B)
        else:
            self._run(PH["OPT_TABLES"] | PH["EMBED"] | PH["INDEX"] | PH["OPT_ROWS"])
        self._run(PH["OPT_DENSE"])

    # ------------------------------------------------------------------ hipGraph replay of the step
    PHASE_ORDER = ("FWD1", "FWD2", "FWD3", "BWD2", "BWD1", "BNG", "OPT_TABLES", "ROWS_USER", "SWEEP_USER", "ROWS_ITEM",
                   "SWEEP_ITEM", "OPT_DENSE")

    def enable_graph(self, batch: int | None = None, eager_phases: tuple = (), keep_graph: bool = False):
        """Capture the single-GPU training step for batches of exactly `batch` pairs into a hipGraph and
        replay it from `train_step` (other batch sizes keep the eager launch sequence).  The two per-step
        scalars (dropout step counter, Adam alpha_t) then live in device memory (brNeumfStep.step_state)
        and are advanced by a 1-thread kernel at the top of the step; ids/labels are read from the static
        buffers `in_users / in_items / in_labels` (train_step copies into them unless it is handed
        exactly those tensors).
        eager_phases: consecutive names from PHASE_ORDER that stay OUTSIDE the graphs (graph A -> eager launches
        -> graph B) so that HIP events can bracket them; timed events cannot be recorded inside a capture on
        ROCm 7.2 (bench.py's fallback when the runtime refuses event-record nodes).
        keep_graph: keep the captured hipGraph_t alive beside its executable (torch.cuda.CUDAGraph(keep_graph=True)) - node handles
        placed during the capture (brProbeGraph*) stay valid for hipGraphExec*SetEvent."""
        if self.dist is not None:
            raise ValueError("graph replay covers the single-GPU step (collectives run between the phases otherwise)")
        B = self.max_batch if batch is None else int(batch)
        if not 0 < B <= self.max_batch:
            raise ValueError("graph batch must be in (0, max_batch]")
        dev, st, PH = self.device, self.step_struct, self.PH
        if getattr(self, "in_users", None) is None or self.in_users.shape[0] != B:
            # (kept across captures of the same batch size: an earlier capture that is still replayed reads these very buffers)
            self.in_users = torch.zeros(B, dtype=self.id_dtype, device=dev)
            self.in_items = torch.zeros(B, dtype=self.id_dtype, device=dev)
            self.in_labels = torch.zeros(B, dtype=torch.float32, device=dev)
        self._alloc_step_state(st)
        # every kernel of the step runs once outside a capture first (code objects load on first launch);
        # the model state is put back afterwards
        keep = self._snapshot_for_dry_run()
        keep_sums = self.msums.clone()
        self._set_step_state()
        self._set_batch(self.in_users, self.in_items, self.in_labels, B, True, 0, B)
        self._run(PH["ALL"])
        torch.cuda.synchronize(dev)
        self._restore_after_dry_run(keep)
        self.msums.copy_(keep_sums)
        del keep
        self._set_batch(self.in_users, self.in_items, self.in_labels, B, True, 0, B)
        st.keep_ready = 1 if st.keep_prefetch else 0      # replays find the planes the previous step (or _replay itself) left
        if eager_phases:
            order = self.PHASE_ORDER
            idx = sorted(order.index(n) for n in eager_phases)
            if idx != list(range(idx[0], idx[-1] + 1)):
                raise ValueError("eager_phases must be consecutive in PHASE_ORDER")
            mask = lambda names: sum(PH[n] for n in names)
            # EMBED modifies FWD1 / OPT_TABLES wherever they land; the dedup sorts go with FWD1 (aux stream)
            parts = [(mask(order[:idx[0]]), True), (mask(order[idx[0]:idx[-1] + 1]), False), (mask(order[idx[-1] + 1:]), True)]
            parts = [(m | PH["EMBED"] | (PH["INDEX"] if m & PH["FWD1"] else 0), cap) for m, cap in parts if m]
        else:
            parts = [(PH["ALL"], True)]
        graphs = []
        for ph, cap in parts:
            if not cap:
                graphs.append(None)
                continue
            g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run(ph)
            if keep_graph:
                g.instantiate()
            graphs.append(g)
        parts = [ph for ph, _ in parts]
        # the capture itself executes nothing, but the dry run above advanced the device step counter
        self._set_step_state()
        self._keep_for = None                 # the dry run above left another step's planes
        self._graph = {"batch": B, "parts": parts, "graphs": graphs}

    def disable_graph(self):
        self._graph = None
        self._graph_multi = None

    def enable_graph_multi(self, batch: int | None = None, steps: int = 4, keep_graph: bool = False, probe_tag: int | None = None):
        """Capture `steps` consecutive training steps as ONE hipGraph (`train_steps` replays it): a training loop whose batches are already
        on the device - `fit()` over resident arrays, bench.py - then pays the per-launch costs of a graph (the gap between two graph
        launches, ~8 us here, and the staging launch) once per `steps` steps instead of once per step.  Everything that differs between
        the steps of a group lives on the device (step counter, alpha_t, the alpha ring, the dropout planes the previous step's
        Adam-rows launch prefetched); the group's ids / labels are staged by one brStageBatch launch into static buffers of `steps`
        batches.  Needs the single-step graph (captured here if absent: it runs the dry step that loads every code object).
        Where the step takes the fused lookup + index path (brNeumfGroupIndexPlan: batch > 16 384, deferred tables, embed_dim 64 / 128,
        planes prefetched or no dropout, steps <= 8) the group's first step builds the row index of every step and the later steps
        launch neither sorts nor a rank; the returned dict's "sets" then holds each step's (user index, item index, double scratch),
        else None.  BR_GROUP_INDEX=0 at capture: every step builds its own index, as in the single-step graph.
        probe_tag: bench.py's measurement - only the LAST step of the group carries the event-record nodes around that kernel (a tag
        that step does not launch - the fused lookup + index call, once the head has built the index - places none)."""
        S = int(steps)
        if S < 2:
            raise ValueError("enable_graph_multi: steps >= 2 (enable_graph is the single-step form)")
        B = self.max_batch if batch is None else int(batch)
        if self._graph is None or self._graph["batch"] != B or len(self._graph["graphs"]) != 1 or self._graph["graphs"][0] is None:
            self.enable_graph(B)
        dev, st, PH = self.device, self.step_struct, self.PH
        gm = getattr(self, "_graph_multi", None)
        if gm is None or gm["S"] != S or gm["batch"] != B:
            self.in_users_m = torch.zeros(S * B, dtype=self.id_dtype, device=dev)
            self.in_items_m = torch.zeros(S * B, dtype=self.id_dtype, device=dev)
            self.in_labels_m = torch.zeros(S * B, dtype=torch.float32, device=dev)
            gm = None
        lib = _lib.load()
        batch_of = lambda k: (self.in_users_m[k * B:(k + 1) * B], self.in_items_m[k * B:(k + 1) * B], self.in_labels_m[k * B:(k + 1) * B])
        # The group's index built once, at its head (include/binrec.h brNeumfStep.group_size; BR_GROUP_INDEX=0: every step its own, as
        # the single-step graph has it): the ids of all S steps are in the static buffers before the group's first kernel runs, so the
        # head's lookup launch carries the chunk sorts of all 2 S id streams and ONE chunk-rank launch ranks them; steps 2..S are the
        # plain lookup and no rank.  Every step then has index buffers and BatchNorm double scratch of its own (step 0: the engine's),
        # kept with the capture - an earlier capture of the same S and batch that is still replayed shares them.
        self._set_batch(*batch_of(0), B, True, 0, B)
        st.keep_ready = 1 if st.keep_prefetch else 0
        sets = None
        if lib.brNeumfGroupIndexPlan(ctypes.byref(st), S) > 0:
            sets = gm.get("sets") if gm is not None else None
            if sets is None:
                sets = [(self.user_index, self.item_index, self.dstat)]
                sets += [(ops.RowIndex(self.max_batch, self.id_dtype, dev), ops.RowIndex(self.max_batch, self.id_dtype, dev), torch.zeros_like(self.dstat))
                         for _ in range(S - 1)]

            class GroupSet(ctypes.Structure):
                _fields_ = _lib.parse_struct("brNeumfGroupSet")
            if ctypes.sizeof(GroupSet) != lib.brNeumfGroupSetSizeof():
                raise _lib.BinrecError("brNeumfGroupSet layout mismatch between include/binrec.h and libbinrec_hip.so")
            arr = (GroupSet * S)()
            for k, (ui, ii, ds) in enumerate(sets):
                uk, ik, _ = batch_of(k)
                arr[k].users, arr[k].items, arr[k].dstat = uk.data_ptr(), ik.data_ptr(), ds.data_ptr()
                arr[k].u_sorted_ids, arr[k].u_sorted_pos, arr[k].u_ws = ui.sorted_ids.data_ptr(), ui.sorted_pos.data_ptr(), ui.ws.data_ptr()
                arr[k].i_sorted_ids, arr[k].i_sorted_pos, arr[k].i_ws = ii.sorted_ids.data_ptr(), ii.sorted_pos.data_ptr(), ii.ws.data_ptr()
        g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
        try:
            if sets is not None:
                st.group_size, st.group_sets = S, ctypes.addressof(arr)      # (a host array: read while the calls below are captured)
            with torch.cuda.graph(g):
                for k in range(S):
                    self._set_batch(*batch_of(k), B, True, 0, B)
                    st.keep_ready = 1 if st.keep_prefetch else 0
                    if sets is not None:
                        st.group_pos = k
                        self._bind_indexes(st, sets[k][0], sets[k][1])
                        st.dstat = sets[k][2].data_ptr()
                    if probe_tag is not None and k == S - 1:
                        lib.brProbeGraphSelect(int(probe_tag))
                    self._run(PH["ALL"])
        finally:
            if probe_tag is not None:
                lib.brProbeGraphSelect(-1)
            # the step struct as the single-step graph and the eager step know it
            st.group_size, st.group_pos, st.group_sets = 0, 0, None
            self._bind_indexes(st)
            st.dstat = self.dstat.data_ptr()
        if keep_graph:
            g.instantiate()
        self._set_batch(self.in_users, self.in_items, self.in_labels, B, True, 0, B)     # the single-step graph's view of the step struct
        st.keep_ready = 1 if st.keep_prefetch else 0
        self._graph_multi = {"S": S, "batch": B, "graph": g, "sets": sets}
        return self._graph_multi

    def train_steps(self, users, items, labels):
        """`steps` training steps in one graph launch (enable_graph_multi): users / items / labels hold the group's batches back to back,
        (steps * batch,) or (steps, batch), contiguous device tensors.  Equal to `steps` calls of train_step on the slices."""
        gm = getattr(self, "_graph_multi", None)
        if gm is None:
            raise RuntimeError("train_steps: enable_graph_multi first")
        S, B = gm["S"], gm["batch"]
        if users.numel() != S * B or items.numel() != S * B or labels.numel() != S * B:
            raise ValueError(f"train_steps: {S} batches of {B} pairs expected")
        self._check_batch(users, items, labels)
        cfg = self.cfg
        self.begin_steps(S)
        if users.data_ptr() != self.in_users_m.data_ptr() or items.data_ptr() != self.in_items_m.data_ptr() or labels.data_ptr() != self.in_labels_m.data_ptr():
            _lib.check(_lib.load().brStageBatch(self.in_users_m.data_ptr(), self.in_items_m.data_ptr(), self.in_labels_m.data_ptr(), users.data_ptr(),
                                                items.data_ptr(), labels.data_ptr(), self.step_struct.id_type, S * B, ops._stream()), "brStageBatch")
        prefetching = cfg.dropout > 0 and self.step_struct.aux_stream
        if prefetching and self._keep_for != (self.t + 1, 0):
            ops.dropout_keep_bits(cfg.dropout, cfg.seed, self.t + 1, 0, self.max_batch, (0, 1, 2), self._keep_widths, self._keep_planes)
        self.t += S
        gm["graph"].replay()
        self._keep_for = (self.t + 1, 0) if prefetching else None

    def sample_batch(self, sampler: BatchSampler, epoch: int, row0: int, B: int, out=None):
        """Rows [row0, row0 + B) of epoch `epoch` of `sampler`, formed now for train_step / train_steps: a pure function of
        (sampler.seed, epoch, global row), so a rank of the row-sharded engine asks for its own slice of the global batch and the ranks'
        slices are the single-device epoch.  One launch beside the step (outside a captured graph), no host sync.  out: optional
        (users, items, labels) buffers of B rows.  -> (users, items, labels) in the engine's id dtype and float32."""
        if sampler.users.dtype != self.id_dtype:
            raise TypeError(f"the sampler holds {sampler.users.dtype} ids, the engine takes {self.id_dtype}")
        return ops.neumf_sample_batch(sampler.users, sampler.items, sampler.pos_off, sampler.pos_items, sampler.n_cand, sampler.neg_per_pos, sampler.seed,
                                      epoch, row0, B, cand_items=sampler.cand_items, alias=sampler.alias, max_tries=sampler.max_tries, out=out,
                                      err_flag=self.err)

    def _snapshot_for_dry_run(self):
        """what enable_graph's dry-run step can change.  Per-step sweep: every table row moves, so the whole (flushed) state.  Deferred /
        lazy tables: only the rows the static input buffers name move - those rows with their moments and `last`, the dense state and
        the host counters are kept, NOT flushed: a capture in the middle of a run leaves every other row's lag as it is (state_dict()
        would flush the tables: 42 GB cloned and every lag reset at config 5's shard size)."""
        if self.cfg.optimizer == "adam_dense" and not self.deferred:
            return {"full": {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.state_dict().items()}}
        ids = {"user": self.in_users, "item": self.in_items}
        snap = {"rows": self._snapshot_rows({k: torch.unique(i).long().clamp_(0, self.fused[k].shape[0] - 1) for k, i in ids.items()}),
                "host": (self.t, self._flush_t, self._stale)}
        snap["dense"] = [t.clone() for t in (self.theta.buf, self.adam_m.buf, self.adam_v.buf, self.moving_buf)]
        return snap

    def _restore_after_dry_run(self, snap):
        if "full" in snap:
            self.load_state_dict(snap["full"])
            return
        self._restore_rows(snap["rows"])
        for dst, src in zip((self.theta.buf, self.adam_m.buf, self.adam_v.buf, self.moving_buf), snap["dense"]):
            dst.copy_(src)
        self.t, self._flush_t, self._stale = snap["host"]
        self._set_step_state()

    def _replay(self, users, items, labels):
        if users.data_ptr() != self.in_users.data_ptr() or items.data_ptr() != self.in_items.data_ptr() or labels.data_ptr() != self.in_labels.data_ptr():
            self._check_batch(users, items, labels)
            _lib.check(_lib.load().brStageBatch(self.in_users.data_ptr(), self.in_items.data_ptr(), self.in_labels.data_ptr(), users.data_ptr(),
                                                items.data_ptr(), labels.data_ptr(), self.step_struct.id_type, users.shape[0], ops._stream()),
                       "brStageBatch")
        gr = self._graph
        cfg = self.cfg
        prefetching = cfg.dropout > 0 and self.step_struct.aux_stream
        if prefetching and self._keep_for != (self.t, 0):
            # first replay (or the previous step ran another path): the graph expects this step's planes to be there
            ops.dropout_keep_bits(cfg.dropout, cfg.seed, self.t, 0, self.max_batch, (0, 1, 2), self._keep_widths, self._keep_planes)
            self._keep_for = (self.t, 0)
        for ph, g in zip(gr["parts"], gr["graphs"]):
            if g is None:
                self._set_batch(self.in_users, self.in_items, self.in_labels, gr["batch"], True, 0, gr["batch"])
                self.step_struct.keep_ready = 1 if prefetching else 0
                self._run(ph)
            else:
                g.replay()
        self._keep_for = (self.t + 1, 0) if prefetching else None

    def row_grad_views(self, B):
        """name -> (tensor, row stride): the MLP halves are views of dx0, the MF halves of g_user / g_item.
        (Inspection helper for tests.  Single-GPU deferred mode: the step never writes the MF gradients out - the optimizer
        launch forms ddot[b] * partner row as it reads the stashed rows (brAdamRowsSortedPair hi_scale) - so they are
        formed here, with the same single fp32 multiply.)"""
        D = self.cfg.dim
        uo, io = (D, 0) if self.cfg.item_first else (0, D)
        dx0 = self.dx0[:B]
        gu, gi = self.g_user[:B, D:], self.g_item[:B, D:]
        if self.deferred and not self.sharded:
            dd = self.ddot[:B, None]
            gu, gi = dd * gi, dd * gu
        return {"user_mlp": (dx0[:, uo:uo + D], 2 * D), "item_mlp": (dx0[:, io:io + D], 2 * D),
                "user_mf": (gu, 2 * D), "item_mf": (gi, 2 * D)}

    def _embed_backward_apply(self, users, items, B):
        """B1 row gradients of the 4 tables, S1 dedup index, O1 Adam on the (fused) tables."""
        cfg, t, D = self.cfg, self._tables, self.cfg.dim
        ops.neumf_embed_backward(t["user_mf"], t["item_mf"], users, items, cfg.item_first, None, self.ddot[:B],
                                 self.g_user[:B, D:], self.g_item[:B, D:])
        self.user_index.build(users, self.num_user_rows)
        self.item_index.build(items, self.num_item_rows)
        rg = self.row_grad_views(B)
        self._adam_tables({"user": (rg["user_mlp"][0], 2 * D, rg["user_mf"][0], 2 * D),
                           "item": (rg["item_mlp"][0], 2 * D, rg["item_mf"][0], 2 * D)})

    def _adam_tables(self, rg, replayed=None):
        """rg: stream -> (mlp-half grads, stride, mf-half grads, stride), aligned with the positions the
        indexes were built on.  One launch per fused table (+ the dense sweep in Keras mode).
        replayed: stream -> the fused rows as this step's deferred gather wrote them, by the same positions (a row-sharded owner:
        the rows it served) - the optimizer then replays the moments only."""
        cfg, D = self.cfg, self.cfg.dim
        if (self.deferred and replayed is not None and rg["user"][2] is None and rg["item"][2] is None
                and self.user_index.n == self.item_index.n and rg["user"][1] == rg["item"][1] == 2 * D
                and replayed["user"].stride(0) == replayed["item"].stride(0)):
            # fixed-capacity exchange: both streams have the same number of slots -> the two shards in ONE launch (each alone leaves
            # HBM half idle: random 512-B rows behind a dependent chain per row)
            ops.adam_rows_sorted_deferred_pair_replayed(
                self.fused["user"], self.fused_m["user"], self.fused_v["user"], self.last["user"], self.user_index, rg["user"][0], replayed["user"],
                self.fused["item"], self.fused_m["item"], self.fused_v["item"], self.last["item"], self.item_index, rg["item"][0], replayed["item"],
                D, self.step_state, cfg.beta1, cfg.beta2, cfg.adam_eps)
            return
        for k, idx in (("user", self.user_index), ("item", self.item_index)):
            g0, ld0, g1, ld1 = rg[k]
            self._adam_rows(k, idx, g0, ld0, g1, ld1, D if g1 is not None else 0, None if replayed is None else replayed[k])
            self._adam_sweep(k)

    # ------------------------------------------------------------------ inference
    def _infer(self, users, items, labels, n):
        PH = self.PH
        self.flush()
        self._set_batch(users, items, labels, n, False, 0, n)
        if self.sharded:
            self._embed_forward(users, items, n)
            self._run(PH["FWD1"] | PH["FWD2"] | PH["FWD3"])
        else:
            self._run(PH["FWD1"] | PH["FWD2"] | PH["FWD3"] | PH["EMBED"])

    def predict(self, users, items, out=None):
        """sigmoid output of the graph in inference mode (moving BN stats, no dropout)."""
        B = users.shape[0]
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        for s in range(0, B, self.max_batch):
            e = min(B, s + self.max_batch)
            self._infer(users[s:e], items[s:e], None, e - s)
            out[s:e].copy_(self.prob[:e - s])
        return out

    def _catalog_ids(self, users, items, every_item=True):
        """What recommend and full_auc do first: flush, then `users` and `items` as contiguous device id tensors of one integer dtype.
        items None: every item row - or None itself with every_item=False (an owner of a row-sharded engine enumerates its own rows)."""
        dev = self.device
        self.flush()                         # deferred-Adam rows lag until then (as _infer)
        users = torch.as_tensor(users, device=dev)
        if users.dtype not in (torch.int32, torch.int64):
            users = users.to(self.id_dtype)
        if items is None and every_item:
            items = torch.arange(self.num_item_rows, dtype=users.dtype, device=dev)
        if items is not None:
            items = torch.as_tensor(items, device=dev)
            items = (items if items.dtype == users.dtype else items.to(users.dtype)).contiguous()
        return users.contiguous(), items

    def _catalog_tower(self):
        """-> (the dense parameters by name, the tower with BatchNorm folded in: csrc/recommend.hip brNeumfCatalogFold)"""
        cfg = self.cfg
        th = {name: self.theta.view(name) for name in self.theta.offsets}
        return th, ops.neumf_catalog_fold(th, self.moving, *cfg.hidden, cfg.mf_first, cfg.bn_eps)

    def _catalog_project(self, th, table, ids, user_side):
        """first-layer projection of rows `ids` of `table`: users row-major with the bias, items column-major"""
        cfg = self.cfg
        if user_side:
            return ops.neumf_catalog_project(table, ids, th["W1"], cfg.hidden[0], cfg.dim, cfg.item_first, True, b1=th["b1"], err_flag=self.err)
        return ops.neumf_catalog_project(table, ids, th["W1"], cfg.hidden[0], cfg.dim, cfg.item_first, False, col_major=True, err_flag=self.err)

    def _catalog_operands(self, users, items):
        """-> (users, items, tower, pu, pit): what the fused catalogue kernels take"""
        users, items = self._catalog_ids(users, items)
        th, tower = self._catalog_tower()
        return users, items, tower, self._catalog_project(th, self.fused["user"], users, True), self._catalog_project(th, self.fused["item"], items, False)

    def recommend(self, users, k, items=None, exclude=None, dump_logits=None):
        """The k best items of every user of `users` in inference mode (the sigmoid output predict returns), without scoring pairs
        one by one: the first layer is split into a user and an item projection, BatchNorm folded into the next layer, and one fused
        launch scores, masks and selects (csrc/recommend.hip).  items: the candidate ids (None: every item row); exclude: (off, idx)
        CSR over `users` of candidate POSITIONS never to return (ops.truth_csr; topk_metrics.seen_csr maps raw ids).
        -> (scores (U, k) float32, index (U, k) int32 positions into `items`) on the device, best first, ties to the lower position;
        slots past the remaining candidates are (-inf, -1).  dump_logits=True also returns every pair's head logit (U x I).
        (The row-sharded engine overrides this with a collective of the same contract: parallel.py recommend_at_owners.)"""
        cfg = self.cfg
        users, items, tower, pu, pit = self._catalog_operands(users, items)
        return ops.neumf_catalog_topk(pu, pit, tower, cfg.dim, tuple(cfg.hidden), cfg.act, k, exclude=exclude, dump_logits=bool(dump_logits))

    PAIR_CHUNK = 1 << 22        # pairs per predict call of full_auc(method="pairs")

    def full_auc(self, users, truth, items=None, dump_probs=False, method="fused"):
        """Per-user ROC AUC over the whole candidate list (full_auc, src/models/bpr.py:230-254) of the probabilities predict returns, in
        inference mode.  truth: (off, idx) CSR over `users` of the candidate POSITIONS that are positives (ops.truth_csr); items: the
        candidate ids (None: every item row).  -> float32 (U,) on the device, NaN where undefined (no positives, or nothing else).
        method="fused" (default): recommend's set-up, then one fused evaluation that never forms the U x I matrix (csrc/auc_neumf.hip);
        dump_probs=True also returns every pair's probability (U x I).  method="pairs": the stand-in it replaces - every pair through
        predict in chunks, the U x I matrix, ops.full_auc - kept as the cross-check and the benchmark's baseline.
        (The row-sharded engine overrides this with a collective of the same contract: parallel.py auc_at_owners.)"""
        if method not in ("fused", "pairs"):
            raise ValueError(f"method must be 'fused' or 'pairs', got {method!r}")
        cfg = self.cfg
        off, idx = truth
        users, items = self._catalog_ids(users, items)
        U, I = users.shape[0], items.shape[0]
        if I < 1:
            raise ValueError("full_auc: empty candidate list")
        if method == "pairs":
            probs = torch.empty(U, I, dtype=torch.float32, device=self.device)
            flat = probs.view(-1)
            rows = max(1, self.PAIR_CHUNK // I)
            for u0 in range(0, U, rows):
                u1 = min(U, u0 + rows)
                self.predict(users[u0:u1].repeat_interleave(I), items.repeat(u1 - u0), out=flat[u0 * I:u1 * I])
            auc = ops.full_auc(probs, *ops._csr((off, idx), U, "truth"))
            return (auc, probs) if dump_probs else auc
        users, items, tower, pu, pit = self._catalog_operands(users, items)
        return ops.neumf_catalog_auc(pu, pit, tower, cfg.dim, tuple(cfg.hidden), cfg.act, off, idx, dump_probs=bool(dump_probs))

    def catalog_ranks(self, users, truth, items=None, exclude=None, dump_probs=False):
        """Per truth entry, in CSR order, the exact (above, tied) int32 counts of the probability predict returns over the whole candidate
        list, in inference mode: recommend's set-up, then one fused evaluation without the U x I matrix (ops.neumf_catalog_ranks,
        csrc/ranks_neumf.hip).  truth / items as in full_auc; exclude: (off, idx) CSR over `users` of candidate POSITIONS never offered
        (topk_metrics.seen_csr): an excluded truth entry is still ranked, against the others.  dump_probs=True also returns every pair's
        probability (U x I).
        (The row-sharded engine overrides this with a collective of the same contract: parallel.py ranks_at_owners.)"""
        cfg = self.cfg
        users, items, tower, pu, pit = self._catalog_operands(users, items)
        return ops.neumf_catalog_ranks(pu, pit, tower, cfg.dim, tuple(cfg.hidden), cfg.act, truth[0], truth[1], exclude=exclude,
                                       dump_probs=bool(dump_probs))

    def rank_metrics(self, users, truth, ks=(10,), items=None, exclude=None):
        """{"mrr", "ndcg@k", "recall@k", "hr@k"} per user (float32 (U,) on the device) over the whole candidate list, from the exact
        ranks of catalog_ranks: r = 1 + above + tied - pessimistic: a tied candidate is taken to outrank the positive, so a model that
        scores everything equal earns nothing.  ks: up to 8 cutoffs; NaN for a user without positives (ops.rank_metrics)."""
        above, tied = self.catalog_ranks(users, truth, items=items, exclude=exclude)
        return ops.rank_metrics(above, tied, truth[0], ks)

    def evaluate_batch(self, users, items, labels):
        """inference-mode forward + loss/metric sums accumulated into self.msums (no grads)."""
        self._infer(users, items, labels, users.shape[0])

    def pop_metrics(self, n_samples: int) -> dict:
        """Host sync: the compiled metrics since the last call - mean loss / mse / mae / binary_accuracy (RModel.py:20) and the
        rest of trainers/NFC_plain.py:155: binary_crossentropy, true/false positives/negatives at threshold 0.5."""
        s = self.msums.sum(dim=0).cpu().tolist()
        self.msums.zero_()
        n = max(1, n_samples)
        return {"loss": s[0] / n, "mse": s[1] / n, "mae": s[2] / n, "binary_accuracy": s[3] / n, "binary_crossentropy": s[4] / n,
                "true_positives": s[5], "false_positives": s[6], "false_negatives": s[7], "true_negatives": n_samples - s[5] - s[6] - s[7]}

    def check_ids(self):
        ops.raise_if_flag(self.err)

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        self.flush()
        sd = {"t": self.t, "theta": self.theta.buf, "adam_m": self.adam_m.buf, "adam_v": self.adam_v.buf}
        for k in ("user", "item"):
            sd["table." + k], sd["table." + k + ".m"], sd["table." + k + ".v"] = self.fused[k], self.fused_m[k], self.fused_v[k]
        sd.update(self.moving)
        return sd

    def load_state_dict(self, sd: dict):
        self.t = int(sd["t"])
        for k, dst in (("theta", self.theta.buf), ("adam_m", self.adam_m.buf), ("adam_v", self.adam_v.buf)):
            dst.copy_(sd[k])
        for k in ("user", "item"):
            self.fused[k].copy_(sd["table." + k]); self.fused_m[k].copy_(sd["table." + k + ".m"]); self.fused_v[k].copy_(sd["table." + k + ".v"])
        for k in self.moving:
            self.moving[k].copy_(sd[k])
        self._reset_lags()

    def load_numpy_params(self, p: dict):
        """Load a parameter dict in the oracle's naming (tests / golden fixtures)."""
        for k in TABLES:
            self.tables[k].copy_(torch.as_tensor(p[k], dtype=torch.float32))
        for k in DENSE_ORDER:
            self.theta.view(k).copy_(torch.as_tensor(p[k], dtype=torch.float32).reshape(self.theta.view(k).shape))
        for k in self.moving:
            self.moving[k].copy_(torch.as_tensor(p[k], dtype=torch.float32))
