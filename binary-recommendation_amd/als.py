"""Implicit-feedback ALS (Hu, Koren, Volinsky 2008, "Collaborative Filtering for Implicit Feedback Datasets") on the HIP hot path:
the weighted matrix factorisation behind `implicit` and Spark's ALS(implicitPrefs=True).  No negative sampler, no learning rate, no
optimiser state: every unobserved pair is a weak negative in closed form, through the Gram matrix of the other side.

One half-step solves every row of one side against the other side's table Y (csrc/als.hip):
    G = Y^T Y (ops.gram),   x_u = (G + reg I + sum_e c_e y_e y_e^T)^-1 sum_e (1 + c_e) y_e (ops.als_solve_rows),  c_e = alpha * conf_e
and an epoch is the user half-step followed by the item half-step on the transposed CSR.  solver="cg" replaces the exact solve by a few
conjugate-gradient steps from the row's current vector (ops.als_solve_rows_cg, csrc/als_wide.hip): no dim x dim matrix
per row, rows up to 512 features.  heavy_rows= takes the few rows with very many entries out of that kernel (one wave per row): their
normal matrices are formed once by many workgroups and the same recurrence runs on them (split_heavy, ops.als_normal_rows,
ops.als_solve_rows_dense_cg, csrc/als_heavy.hip).  The result is a (user table, item table)
pair of float rows: the fused catalogue kernels of the dot-product models (top-k, AUC, exact ranks) serve it unchanged.  Single device.
"""
from __future__ import annotations

import torch

from . import ops


def csr_pair(users, items, n_users: int, n_items: int, device, conf=None):
    """The observed pairs as the two CSRs a half-step takes -> (user_csr, item_csr), each (off int64 [rows + 1], idx int32 ascending
    and unique per row, conf float32 per entry or None): the items of every user, and - the transpose - the users of every item.
    Duplicate pairs are merged: binary data has no counts; a given conf (float, >= 0, one per pair) is summed over them.  torch ops on
    `device` ("cpu" runs the same code on the host)."""
    dev = torch.device(device)
    u = torch.as_tensor(users).to(dev).long().view(-1)
    i = torch.as_tensor(items).to(dev).long().view(-1)
    if u.shape != i.shape:
        raise ValueError("csr_pair: users and items must have one length")
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= n_users or int(i.min()) < 0 or int(i.max()) >= n_items):
        raise IndexError("csr_pair: id out of range")
    key = u * int(n_items) + i
    c_u = None
    if conf is None:
        key = torch.unique(key)                               # sorted
    else:
        c = torch.as_tensor(conf).to(dev).view(-1)
        if c.shape != u.shape:
            raise ValueError("csr_pair: conf must have one value per pair")
        # sorted by pair, then the sum of every run of equal pairs in the order given (a prefix sum in double: no atomics)
        key, order = torch.sort(key, stable=True)
        cum = torch.cumsum(c[order].double(), 0)
        last = torch.ones_like(key, dtype=torch.bool)
        last[:-1] = key[1:] != key[:-1]
        ends = cum[last]
        c_u = (ends - torch.cat([ends.new_zeros(1), ends[:-1]])).float()
        key = key[last]
    uu, ii = key // int(n_items), key % int(n_items)

    def offsets(rows, n):
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
        return off
    user_csr = (offsets(uu, n_users), ii.to(torch.int32).contiguous(), c_u)
    order = torch.argsort(ii * int(n_users) + uu)             # distinct keys: one order
    item_csr = (offsets(ii, n_items), uu[order].to(torch.int32).contiguous(), None if c_u is None else c_u[order].contiguous())
    return user_csr, item_csr


def _csr3(csr):
    return (csr[0], csr[1], csr[2] if len(csr) > 2 else None)


HEAVY_WS_BYTES = 256 << 20      # H, b and the partial workspace of one batch of heavy rows, at most (a row above it stands alone)


def heavy_row_bytes(n_slices: int, dim: int) -> int:
    """H (float32 dim x dim), b (float64 dim) and the partials of a row of n_slices slices: ops.als_normal_rows allocates this much"""
    nb = (dim + 127) // 128
    return dim * dim * 4 + dim * 8 + n_slices * (nb * (nb + 1) // 2 * 65536 + dim * 8)


class HeavyBatch:
    """consecutive heavy rows [lo, hi) of a HeavyCSR: their ids (int32 and int64), slice prefix from 0 and slice count"""

    def __init__(self, lo, hi, rows, slice_off, n_slices):
        self.lo, self.hi, self.rows, self.rows_long, self.slice_off, self.n_slices = lo, hi, rows, rows.long(), slice_off, n_slices


class HeavyCSR:
    """A CSR with its heavy rows (more than `threshold` entries) set apart (split_heavy):
    csr        the CSR as given, (off, idx, conf or None)
    rows       int32, ascending: the heavy rows
    light      (off, idx, conf) over ALL rows with the heavy rows emptied, idx / conf compacted: the kernels of the plain path run it
               unchanged and give the heavy rows exact zeros (the CSR itself where no row is heavy)
    slice      entries per slice, slice_off: int64 [len(rows) + 1] prefix of the slices of the heavy rows
    batches    [HeavyBatch]: consecutive heavy rows whose H, b and partial workspace stay under ws_bytes at `dim` features (plan)"""

    def __init__(self, csr, threshold, rows, light, slice, slice_off, row_slices):
        self.csr, self.threshold, self.rows, self.light, self.slice, self.slice_off = csr, threshold, rows, light, slice, slice_off
        self._row_slices = row_slices            # host: slices of every heavy row
        self.dim = self.ws_bytes = None
        self.batches = []

    def plan(self, dim: int, ws_bytes: int = HEAVY_WS_BYTES):
        """the batches for rows of `dim` features under `ws_bytes` (host arithmetic; no sync)"""
        bounds, lo, used = [], 0, 0
        for h, ns in enumerate(self._row_slices):
            need = heavy_row_bytes(ns, dim)
            if h > lo and used + need > ws_bytes:
                bounds.append((lo, h))
                lo, used = h, 0
            used += need
        if len(self._row_slices) > lo:
            bounds.append((lo, len(self._row_slices)))
        self.batches = [HeavyBatch(lo, hi, self.rows[lo:hi], (self.slice_off[lo:hi + 1] - self.slice_off[lo]).contiguous(),
                                   sum(self._row_slices[lo:hi])) for lo, hi in bounds]
        self.dim, self.ws_bytes = int(dim), int(ws_bytes)
        return self


def split_heavy(csr, threshold: int, dim: int = None, heavy_ws_bytes: int = HEAVY_WS_BYTES, slice: int = None) -> HeavyCSR:
    """Set the rows of `csr` with more than `threshold` entries apart -> HeavyCSR, made once per CSR (host syncs).  dim: the row width the
    batches are planned for (None: ops.ALS_CG_MAX_DIM, the widest; HeavyCSR.plan re-plans).  torch ops on the CSR's device ("cpu" runs
    the same code on the host)."""
    slice = ops.ALS_HEAVY_SLICE if slice is None else int(slice)
    if int(threshold) < 1:
        raise ValueError(f"split_heavy: threshold = {threshold} must be >= 1")
    if slice < 64 or slice % 64:
        raise ValueError(f"split_heavy: slice = {slice} must be a multiple of 64, at least 64")
    off, idx, conf = _csr3(csr)
    lens = off[1:] - off[:-1]
    heavy = lens > int(threshold)
    rows = torch.nonzero(heavy).view(-1).to(torch.int32)
    if rows.numel() == 0:
        light = (off, idx, conf)
    else:
        keep = ~torch.repeat_interleave(heavy, lens)
        light_off = torch.zeros_like(off)
        light_off[1:] = torch.cumsum(torch.where(heavy, torch.zeros_like(lens), lens), 0)
        light = (light_off, idx[keep].contiguous(), None if conf is None else conf[keep].contiguous())
    slice_off = ops.als_slice_prefix(off, rows, slice)
    row_slices = (slice_off[1:] - slice_off[:-1]).tolist()
    h = HeavyCSR((off, idx, conf), int(threshold), rows, light, slice, slice_off, row_slices)
    return h.plan(ops.ALS_CG_MAX_DIM if dim is None else int(dim), heavy_ws_bytes)


class ALSEngine:
    """Tables `user` (num_users x num_factor) and `item` (num_items x num_factor), float32, N(0, 0.01) from init_seed; reg = the
    ridge term lambda > 0, alpha = the confidence slope (an observed pair weighs 1 + alpha * conf).
    solver = "cholesky" (the default): every row is solved exactly, num_factor <= ops.ALS_MAX_DIM = 128.
    solver = "cg": cg_steps (1 .. 64) conjugate-gradient steps per row and half-step, warm-started from the row's vector, num_factor <=
    ops.ALS_CG_MAX_DIM = 512.  Above 128 features only the fused serving forms exist (recommend, full_auc, catalog_ranks,
    rank_metrics): predict_scores stops at 128, as for BPR.
    heavy_rows = None (the default) | int >= 1, solver="cg" only: prepare(csr) sets the rows with more than heavy_rows entries apart
    and a half-step takes them through their formed normal matrices, in batches of at most heavy_ws_bytes of device memory
    (ops.ALS_HEAVY_ROWS is the measured recommendation)."""

    def __init__(self, num_users: int, num_items: int, num_factor: int, device, reg: float = 0.01, alpha: float = 40.0, init_seed: int = 0,
                 solver: str = "cholesky", cg_steps: int = 3, heavy_rows=None, heavy_ws_bytes: int = HEAVY_WS_BYTES):
        if solver not in ("cholesky", "cg"):
            raise ValueError(f"solver must be 'cholesky' or 'cg', got {solver!r}")
        if heavy_rows is not None:
            if isinstance(heavy_rows, bool) or not isinstance(heavy_rows, int) or heavy_rows < 1:
                raise ValueError(f"heavy_rows = {heavy_rows!r}: None or an int >= 1")
            if solver != "cg":
                raise ValueError("heavy_rows needs solver='cg'")
        self.heavy_rows, self.heavy_ws_bytes = heavy_rows, int(heavy_ws_bytes)
        max_dim = ops.ALS_MAX_DIM if solver == "cholesky" else ops.ALS_CG_MAX_DIM
        if not 1 <= int(num_factor) <= max_dim:
            raise ValueError(f"num_factor = {num_factor}: 1 <= num_factor <= {max_dim} with solver={solver!r}")
        if not 1 <= int(cg_steps) <= 64:
            raise ValueError(f"cg_steps = {cg_steps}: 1 <= cg_steps <= 64")
        if not (reg > 0 and alpha >= 0):
            raise ValueError("reg must be > 0 and alpha >= 0")
        self.device, self.dim, self.reg, self.alpha = torch.device(device), int(num_factor), float(reg), float(alpha)
        self.solver, self.cg_steps = solver, int(cg_steps)
        self.id_dtype = torch.int32
        g = torch.Generator(device="cpu").manual_seed(init_seed)
        self.user = (torch.randn(num_users, self.dim, generator=g) * 0.01).to(self.device)
        self.item = (torch.randn(num_items, self.dim, generator=g) * 0.01).to(self.device)
        self._gram = torch.empty(self.dim, self.dim, dtype=torch.float32, device=self.device)
        self.err = ops.new_err_flag(self.device)

    # ---- training ----
    def prepare(self, csr):
        """What half_step / epoch should be given for `csr`: with heavy_rows set, the HeavyCSR of it (split_heavy, once per CSR; host
        syncs); else csr itself."""
        if self.heavy_rows is None:
            return csr
        return split_heavy(csr, self.heavy_rows, dim=self.dim, heavy_ws_bytes=self.heavy_ws_bytes)

    def half_step(self, side: str, csr):
        """Solve every row of `side` ("user" | "item") against the other table, in place: gram, then the fused per-row solve (Cholesky,
        or cg_steps conjugate-gradient steps from the rows as they stand).  csr:
        (off, idx[, conf]) over the rows of `side` with positions into the other table (csr_pair), or the HeavyCSR of one (prepare;
        solver="cg"): its light rows take the same kernel, its heavy rows ops.als_normal_rows + ops.als_solve_rows_dense_cg.  No host
        sync."""
        if side not in ("user", "item"):
            raise ValueError(f"side must be 'user' or 'item', got {side!r}")
        X, Y = (self.user, self.item) if side == "user" else (self.item, self.user)
        heavy = csr if isinstance(csr, HeavyCSR) else None
        if heavy is not None:
            if self.solver != "cg":
                raise ValueError("half_step: a HeavyCSR needs solver='cg'")
            if heavy.dim != self.dim or heavy.ws_bytes != self.heavy_ws_bytes:
                heavy.plan(self.dim, self.heavy_ws_bytes)
            csr = heavy.light
        off, idx, conf = _csr3(csr)
        if off.shape[0] != X.shape[0] + 1:
            raise ValueError(f"half_step({side!r}): the CSR has {off.shape[0] - 1} rows, the table {X.shape[0]}")
        if heavy is not None and heavy.batches:
            x0 = X.index_select(0, heavy.rows.long())          # before the light pass zeroes these rows
        G = ops.gram(Y, out=self._gram)
        if self.solver == "cg":
            ops.als_solve_rows_cg(Y, G, off, idx, self.reg, self.alpha, X, steps=self.cg_steps, conf=conf, err_flag=self.err)
            if heavy is not None:
                f_off, f_idx, f_conf = heavy.csr
                for bt in heavy.batches:
                    H, b = ops.als_normal_rows(Y, f_off, f_idx, self.alpha, bt.rows, conf=f_conf, slice=heavy.slice, err_flag=self.err,
                                               plan=(bt.slice_off, bt.n_slices))
                    X.index_copy_(0, bt.rows_long, ops.als_solve_rows_dense_cg(G, H, b, self.reg, x0[bt.lo:bt.hi], steps=self.cg_steps))
        else:
            ops.als_solve_rows(Y, G, off, idx, self.reg, self.alpha, conf=conf, out=X, err_flag=self.err)

    def epoch(self, user_csr, item_csr):
        self.half_step("user", user_csr)
        self.half_step("item", item_csr)

    def objective(self, user_csr) -> float:
        """L = sum_obs [(1 + c)(1 - s)^2 - s^2] + <X^T X, Y^T Y>_F + reg (tr X^T X + tr Y^T Y), s = x_u . y_i: the double sum over all
        U x I pairs is the Frobenius product of the two Gram matrices, so nothing of size U x I is formed.  Host sync."""
        off, idx, conf = _csr3(user_csr)
        gx, gy = ops.gram(self.user).double(), ops.gram(self.item).double()
        total = (gx * gy).sum() + self.reg * (torch.diagonal(gx).sum() + torch.diagonal(gy).sum())
        if idx.numel():
            rows = torch.repeat_interleave(torch.arange(off.shape[0] - 1, device=self.device), off[1:] - off[:-1])
            xu = ops.gather_rows([self.user], [rows], err_flag=self.err)[0]
            yi = ops.gather_rows([self.item], [idx], err_flag=self.err)[0]
            s = ops.row_dot(xu, yi).double()
            c = self.alpha * (conf.double() if conf is not None else torch.ones_like(s))
            total = total + ((1.0 + c) * (1.0 - s) ** 2 - s * s).sum()
        return float(total.item())

    # ---- serving: the surface of BPREngine, on the same fused catalogue kernels ----
    def predict_scores(self, user_ids, item_ids=None):
        """user vectors x item matrix^T (rows up to 128 features, ops.score_matrix)"""
        u = ops.gather_rows([self.user], [user_ids])[0]
        it = self.item if item_ids is None else ops.gather_rows([self.item], [item_ids])[0]
        return ops.score_matrix(u, it)

    def recommend(self, users, k, items=None, exclude=None, dump_scores=False):
        """The k best items of every user of `users` by the dot score predict_scores returns, without the U x I matrix: one fused
        launch scores, masks and selects (ops.dot_catalog_topk, csrc/recommend_dot.hip).  items: the candidate ids (None: the item
        table in place); exclude: (off, idx) CSR over `users` of candidate POSITIONS never to return (topk_metrics.seen_csr).
        -> (scores (U, k) float32, index (U, k) int32 positions into `items`) on the device, best first, ties to the lower position;
        slots past the remaining candidates are (-inf, -1).  Ids outside the tables set self.err (check_ids raises)."""
        q, c = self._catalog_rows(users, items)
        return ops.dot_topk_for(q.shape[1])(q, c, k, exclude=exclude, dump_scores=dump_scores)

    def full_auc(self, users, truth, items=None, dump_scores=False):
        """Per-user full AUC of the dot scores predict_scores returns, without the U x I matrix (ops.dot_catalog_auc, csrc/auc_dot.hip).
        truth: (off, idx) CSR over `users` of candidate POSITIONS, ascending (ops.truth_csr); items: the candidate ids (None: the item
        table in place).  -> float32 (U,) on the device, NaN for a user without positives or without negatives.  Ids outside the
        tables set self.err (check_ids raises)."""
        q, c = self._catalog_rows(users, items)
        return ops.dot_auc_for(q.shape[1])(q, c, truth[0], truth[1], dump_scores=dump_scores)

    def catalog_ranks(self, users, truth, items=None, exclude=None, dump_scores=False):
        """Per truth entry, in the order of the CSR, how many candidates score above it and how many tie with it, over the whole
        catalogue and without the U x I matrix (ops.dot_catalog_ranks, csrc/ranks_dot.hip).  truth / items as in full_auc; exclude:
        (off, idx) CSR over `users` of candidate POSITIONS never offered (topk_metrics.seen_csr): an excluded truth entry is still
        ranked, against the others.  -> (above, tied) int32 on the device, (-1, -1) for a positive whose score is NaN.  Ids outside
        the tables set self.err (check_ids raises)."""
        q, c = self._catalog_rows(users, items)
        return ops.dot_catalog_ranks(q, c, truth[0], truth[1], exclude=exclude, dump_scores=dump_scores)

    def rank_metrics(self, users, truth, ks=(10,), items=None, exclude=None):
        """Per-user MRR and, for every cutoff of ks (at most 8), NDCG@k, recall@k and hit rate@k over the whole catalogue, from the exact
        ranks of catalog_ranks: r = 1 + above + tied - pessimistic: a tied candidate is taken to outrank the positive, so a model that
        scores everything equal earns nothing.  -> {"mrr", "ndcg@k", "recall@k", "hr@k"} float32 (U,) on the device, NaN for a user
        without positives (ops.rank_metrics)."""
        above, tied = self.catalog_ranks(users, truth, items=items, exclude=exclude)
        return ops.rank_metrics(above, tied, truth[0], ks)

    def _catalog_rows(self, users, items):
        """-> (the rows of `users`, the rows of `items` or the item table in place) that recommend / full_auc score"""
        users, items = self._recommend_ids(users, items)
        q = ops.gather_rows([self.user], [users], err_flag=self.err)[0]
        c = self.item if items is None else ops.gather_rows([self.item], [items], err_flag=self.err)[0]
        return q, c

    def _recommend_ids(self, users, items):
        users = torch.as_tensor(users, device=self.device)
        if users.dtype not in (torch.int32, torch.int64):
            users = users.to(self.id_dtype)
        if items is not None:
            items = torch.as_tensor(items, device=self.device)
            if items.dtype != users.dtype:
                items = items.to(users.dtype)
            items = items.contiguous()
        return users.contiguous(), items

    def check_ids(self):
        ops.raise_if_flag(self.err)

    STATE_TABLES = ("user", "item")

    def state_dict(self) -> dict:
        return {k: getattr(self, k) for k in self.STATE_TABLES}

    def load_state_dict(self, sd: dict):
        for k in self.STATE_TABLES:
            getattr(self, k).copy_(sd[k])
