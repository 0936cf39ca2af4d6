"""Row-sharded embedding tables over the GPUs of one node (one process per GPU, RCCL over xGMI).

The reference only mirrors every variable on every worker (MultiWorkerMirroredStrategy,
src/models/RModel.py:119: all-reduce of dense AND whole-table gradients).  MI355X-first
(SURVEY.md §8e): each table is row-sharded, owner(r) = r mod W, local row = r div W (balances
Zipf heads); per step and id stream
   all-to-all #1  ids      requester -> owner   (B/W * 4 B per stream: latency-bound)
   all-to-all #2  rows     owner -> requester   (direct xGMI links, all 7 peers concurrently)
   all-to-all #3  row grads requester -> owner  (same volume), owner dedups + runs Adam locally
and one small all-reduce of the flat dense gradient (~75 KB) plus the BatchNorm column sums.

`ShardExchange` is backend-agnostic index plumbing (torch index ops + torch.distributed); the
row gather / optimizer compute is injected, so the product path passes the HIP ops and the
CPU tests (gloo, world_size 2) pass the oracle.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


class DistCtx:
    """Thin wrapper over a torch.distributed process group ("nccl" == RCCL on ROCm)."""

    def __init__(self, group=None, force_collectives: bool = False):
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.backend = dist.get_backend(group)
        # a 1-rank group normally short-cuts every collective to a local copy; force_collectives issues them anyway
        # (rehearsal of the RCCL call paths on a one-GPU box: tests/test_gpu_nccl_world1.py, bench.py BR_BENCH_FORCE_SHARDED)
        self.local = self.world == 1 and not force_collectives

    def _stage(self, t):
        # gloo has no device-side collectives for every op: stage through the host there
        return self.backend == "gloo" and t.is_cuda

    def all_reduce_sum(self, t: torch.Tensor):
        if self.local:
            return t
        if self._stage(t):
            c = t.cpu()
            dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.group)
            t.copy_(c)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def all_to_all(self, out: torch.Tensor, inp: torch.Tensor, out_splits, in_splits):
        """Row-wise all_to_all_single (splits count rows of dim 0)."""
        if self.local:
            out.copy_(inp)
            return out
        if self._stage(inp):
            co, ci = torch.empty(out.shape, dtype=out.dtype), inp.cpu()
            dist.all_to_all_single(co, ci, list(out_splits), list(in_splits), group=self.group)
            out.copy_(co)
        else:
            dist.all_to_all_single(out, inp.contiguous(), list(out_splits), list(in_splits), group=self.group)
        return out

    def all_to_all_equal(self, out: torch.Tensor, inp: torch.Tensor):
        """all_to_all_single with equal, static splits (dim 0 of both is a multiple of the world size): no split lists, no counts."""
        if self.local:
            out.copy_(inp)
        elif self._stage(inp):
            co = torch.empty(out.shape, dtype=out.dtype)
            dist.all_to_all_single(co, inp.cpu(), group=self.group)
            out.copy_(co)
        else:
            dist.all_to_all_single(out, inp, group=self.group)
        return out

    def all_gather_rows(self, inp: torch.Tensor) -> torch.Tensor:
        out = torch.empty((self.world * inp.shape[0],) + tuple(inp.shape[1:]), dtype=inp.dtype, device=inp.device)
        if self.local:
            out.copy_(inp)
        elif self._stage(inp):
            co = torch.empty(out.shape, dtype=out.dtype)
            dist.all_gather_into_tensor(co, inp.cpu(), group=self.group)
            out.copy_(co)
        else:
            dist.all_gather_into_tensor(out, inp.contiguous(), group=self.group)
        return out

    def barrier(self):
        if not self.local:
            dist.barrier(group=self.group)


def shard_rows(total_rows: int, rank: int, world: int) -> int:
    """rows r with r % world == rank."""
    return (total_rows - rank + world - 1) // world if total_rows > rank else 0


class ShardExchange:
    """One id stream of one step: who owns what, in which order rows travel.

    bucket order = batch positions stably sorted by owner; `order[j]` is the batch position of
    bucket slot j, `inv[b]` the bucket slot of batch position b.
    """

    def __init__(self, ctx: DistCtx):
        self.ctx = ctx

    def plan(self, ids: torch.Tensor):
        if ids.is_cuda:
            return ShardExchange.plan_pair(self, ids)
        # host tensors (CPU unit tests of the exchange logic): the same plan with torch ops
        W = self.ctx.world
        dest = (ids % W).to(torch.int64)
        _, order = torch.sort(dest, stable=True)
        # rows per destination; NOT torch.bincount: it sizes its output from a device max => a hidden host sync per call
        counts = (dest.unsqueeze(1) == torch.arange(W, device=dest.device).unsqueeze(0)).sum(0)
        self.order = order
        self.inv = torch.empty_like(order)
        self.inv[order] = torch.arange(order.numel(), device=order.device, dtype=order.dtype)
        self.send_local = torch.div(ids, W, rounding_mode="floor")[order].contiguous()
        self.send_counts_t = counts
        return self

    def _scratch(self, n, ids):
        """device scratch of the planning kernels, grown on demand"""
        if getattr(self, "_cap", -1) < n or self._dtype != ids.dtype:
            from . import _lib
            cap = int(n * 1.25) + 64
            dev, W = ids.device, self.ctx.world
            e = lambda dt: torch.empty(cap, dtype=dt, device=dev)
            self._dest, self._sdest, self._send = e(ids.dtype), e(ids.dtype), e(ids.dtype)
            self._order, self._inv = e(torch.int32), e(torch.int32)
            self._counts = torch.zeros(W, dtype=torch.int64, device=dev)
            self._ws_bytes = int(_lib.load().brRowIndexWorkspaceBytes(cap, 1 if ids.dtype == torch.int64 else 0))
            self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=dev)
            self._cap, self._dtype = cap, ids.dtype

    @staticmethod
    def plan_pair(xa: "ShardExchange", ids_a: torch.Tensor, xb: "ShardExchange" = None, ids_b: torch.Tensor = None):
        """Plan one stream, or two equally long ones in shared launches (brShardPlanPair: 4 launches instead of ~10 torch ops
        per stream)."""
        from . import _lib, ops
        n, W = ids_a.shape[0], xa.ctx.world
        if xb is not None and ids_b.shape[0] != n:
            xa.plan(ids_a); xb.plan(ids_b)
            return xa, xb
        for x, ids in ((xa, ids_a),) + (((xb, ids_b),) if xb is not None else ()):
            if not ids.is_contiguous() or ids.dtype not in (torch.int32, torch.int64):
                raise TypeError("ids must be contiguous int32 / int64 device tensors")
            x._scratch(n, ids)
        P = lambda t: t.data_ptr()
        b = xb if xb is not None else xa
        wsb = min(xa._ws_bytes, b._ws_bytes)
        _lib.check(_lib.load().brShardPlanPair(P(ids_a), P(ids_b) if xb is not None else None, ops.I64 if ids_a.dtype == torch.int64 else ops.I32, n, W,
                                               P(xa._dest), P(b._dest), P(xa._sdest), P(b._sdest), P(xa._order), P(b._order), P(xa._ws), P(b._ws), wsb,
                                               P(xa._inv), P(b._inv), P(xa._send), P(b._send), P(xa._counts), P(b._counts), ops._stream()),
                   "brShardPlanPair")
        for x in (xa,) + ((xb,) if xb is not None else ()):
            x.order, x.inv, x.send_local, x.send_counts_t = x._order[:n], x._inv[:n], x._send[:n], x._counts
        return (xa, xb) if xb is not None else xa

    def exchange_counts(self, *others: "ShardExchange"):
        """ONE host sync for all streams of the step: send/recv row counts per peer."""
        ctx, W = self.ctx, self.ctx.world
        plans = (self,) + others
        S = len(plans)
        sc = torch.stack([p.send_counts_t for p in plans]).to(torch.int64)          # (S, W)
        if not ctx.local:
            # peer-major layout (inp[d*S + s] = sc[s][d]) so ONE all_to_all moves every stream's count
            out = torch.empty(W * S, dtype=torch.int64, device=sc.device)
            ctx.all_to_all(out, sc.t().contiguous().view(-1), [S] * W, [S] * W)
            rc = out.view(W, S).t().contiguous()                                    # rc[s][src]
        else:
            rc = sc.clone()
        sc_h, rc_h = sc.cpu().tolist(), rc.cpu().tolist()
        for p, s, r in zip(plans, sc_h, rc_h):
            p.send_counts, p.recv_counts = s, r
            p.n_recv = int(sum(r))
        return self

    def send_ids(self) -> torch.Tensor:
        """all-to-all #1: local row ids to their owners -> ids this rank must serve."""
        out = torch.empty(self.n_recv, dtype=self.send_local.dtype, device=self.send_local.device)
        self.recv_local = self.ctx.all_to_all(out, self.send_local, self.recv_counts, self.send_counts)
        return self.recv_local

    def return_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """all-to-all #2: rows served (n_recv, D) -> rows requested, in bucket order (B, D)."""
        out = torch.empty((self.order.numel(), rows.shape[1]), dtype=rows.dtype, device=rows.device)
        return self.ctx.all_to_all(out, rows, self.send_counts, self.recv_counts)

    def send_row_grads(self, grads_bucket_order: torch.Tensor) -> torch.Tensor:
        """all-to-all #3: per-pair row gradients (bucket order) -> owners, aligned with recv_local."""
        out = torch.empty((self.n_recv, grads_bucket_order.shape[1]), dtype=grads_bucket_order.dtype,
                          device=grads_bucket_order.device)
        return self.ctx.all_to_all(out, grads_bucket_order, self.recv_counts, self.send_counts)


class PaddedExchange:
    """Both id streams of a NeuMF step through ONE all-to-all per phase, duplicate ids merged, a FIXED number of slots per peer
    (brShardDedupPlanPair): ids out, rows back, row gradients out = 3 collectives per step (+ the dense all-reduce), every split equal
    and static, every buffer allocated once, nothing about the step read back by the host - the launches and collectives of a step
    are enqueued without a sync and can be captured into a hipGraph (the exact exchange above needs the per-peer row counts on the
    host before it can post its first all-to-all).
    Layout of every exchanged buffer: [peer][stream: user | item][cap] slots (ids: one id per slot; rows / gradients: `dim` floats
    per slot).  An owner serves each DISTINCT id of a batch once (a Zipf batch with one id on thousands of positions costs one slot);
    the requester sums the row gradients of an id's positions (ordered, two-level) into its slot before they travel.  Pad slots
    carry the owner's spare table row (gradient 0).  More than `cap` distinct ids of one stream for one owner: the surplus ids get
    no slot - the step reads zeros for them and sends no gradient, nothing collides - and a device flag that the engine's
    check_ids() turns into an error (cap = 1.25 x batch / world: uniform ids at batch 65 536 / 8 ranks sit 20 sigma below it, skewed
    ids further still; only a batch whose DISTINCT ids crowd onto one owner can overflow)."""

    def __init__(self, ctx: DistCtx, max_batch: int, id_dtype, device, total_rows, dim: int, factor: float = 1.25):
        from . import _lib, ops
        W = ctx.world
        self.ctx, self.W, self.dim, self.id_dtype, self.total_rows = ctx, W, int(dim), id_dtype, tuple(int(r) for r in total_rows)
        cap = max_batch if W == 1 else min(max_batch, (int(max_batch / W * factor) + 64) // 64 * 64)
        self.cap, self.n_slots = cap, W * cap                 # slots per stream; the merged buffers hold 2 * n_slots
        self.id_type = ops.I64 if id_dtype == torch.int64 else ops.I32
        e = lambda n, dt: torch.empty(n, dtype=dt, device=device)
        B, S = max_batch, 2 * self.n_slots
        self.keys, self.skeys = [e(B, id_dtype) for _ in range(2)], [e(B, id_dtype) for _ in range(2)]
        self.spos, self.urank, self.slot = ([e(B, torch.int32) for _ in range(2)] for _ in range(3))
        self.first = [torch.zeros(W + 1, dtype=torch.int32, device=device) for _ in range(2)]
        self.ws_bytes = int(_lib.load().brRowIndexWorkspaceBytes(B, self.id_type))
        self.ws = [e(self.ws_bytes, torch.uint8) for _ in range(2)]
        self.seg_ws = [e(int(_lib.load().brSegmentScratchFloats(B, self.dim)), torch.float32) for _ in range(2)]
        self.send_ids_buf, self.recv_ids = e(S, id_dtype), e(S, id_dtype)
        f = lambda: torch.empty(S, self.dim, dtype=torch.float32, device=device)
        self.served, self.rows, self.gpad, self.grecv = f(), f(), f(), f()
        self.seg = (cap, 2 * cap, 0, cap)                     # (seg_len, seg_stride, offset of the user half, of the item half): common.h seg_phys

    def plan(self, ids_a, ids_b, err_flag):
        from . import _lib, ops
        n = ids_a.shape[0]
        if ids_b.shape[0] != n or n > self.keys[0].shape[0]:
            raise ValueError("PaddedExchange.plan: both streams must have the same length <= max_batch")
        P = lambda t: t.data_ptr()
        _lib.check(_lib.load().brShardDedupPlanPair(
            P(ids_a), P(ids_b), self.id_type, n, self.W, self.cap, self.total_rows[0], self.total_rows[1], P(self.keys[0]), P(self.keys[1]),
            P(self.skeys[0]), P(self.skeys[1]), P(self.spos[0]), P(self.spos[1]), P(self.ws[0]), P(self.ws[1]), self.ws_bytes, P(self.urank[0]), P(self.urank[1]),
            P(self.first[0]), P(self.first[1]), P(self.send_ids_buf), P(self.slot[0]), P(self.slot[1]), P(self.gpad), self.dim, P(err_flag), ops._stream()),
            "brShardDedupPlanPair")
        self.n = n
        return self

    def send_ids(self):
        """all-to-all #1: every owner's distinct local row ids of both streams -> the ids this rank serves ([source][stream][cap])."""
        return self.ctx.all_to_all_equal(self.recv_ids, self.send_ids_buf)

    def return_rows(self):
        """all-to-all #2: self.served (filled by the owner-side gather, slot for slot) -> self.rows in the requester's slot numbering."""
        return self.ctx.all_to_all_equal(self.rows, self.served)

    def send_row_grads(self, g0_a, g1_a, g0_b, g1_b, ldg, hi_scale, split):
        """the per-id sums of the step's row gradients into the send slots (brSegmentSumToSlotsPair: columns [0, split) from g0, the
        rest hi_scale[position] * g1 - the NeuMF step passes the MLP halves of dx0, the partner streams' stashed MF rows and ddot),
        then all-to-all #3 -> self.grecv on the owners, slot for slot with recv_ids."""
        from . import _lib, ops
        P = lambda t: 0 if t is None else t.data_ptr()
        _lib.check(_lib.load().brSegmentSumToSlotsPair(P(self.skeys[0]), P(self.spos[0]), P(self.slot[0]), P(g0_a), P(g1_a), P(self.skeys[1]), P(self.spos[1]),
                                                       P(self.slot[1]), P(g0_b), P(g1_b), ldg, ldg, P(hi_scale), self.id_type, self.n, self.dim, split, P(self.gpad),
                                                       P(self.seg_ws[0]), P(self.seg_ws[1]), ops._stream()), "brSegmentSumToSlotsPair")
        return self.ctx.all_to_all_equal(self.grecv, self.gpad)


# ---------------------------------------------------------------------------------------------------------------------
# Checkpoint / restore of row-sharded engines.  The reference writes ONE SavedModel: the chief to
# checkpoints/<model>/cp, every other worker to a temporary cp/workertemp_<id> that it deletes again, because all its variables
# are mirrored (src/models/RModel.py:139,175-196).  Here every rank OWNS different table rows, so every rank writes its shard:
#   <path>.shard<rank>-of-<world>.pt   state_dict() of the rank's engine (row r of a table = global row r * world + rank)
#   <path>.meta.json                   written by rank 0: world size, names of the row-sharded entries
# Restore accepts any world size: with the same one a rank reads its own file, otherwise every saved shard is read and the
# global rows are dealt out again (owner = row mod new world; also world 1 = the single-GPU engines).
# ---------------------------------------------------------------------------------------------------------------------
def _shard_file(path, rank, world):
    return f"{path}.shard{rank:03d}-of-{world:03d}.pt"


def save_sharded(engine, path, ctx: "DistCtx", sharded_keys):
    """sharded_keys: state_dict entries whose dim 0 is row-sharded (tables and their optimizer slots)."""
    import json
    import os
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    sd = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in engine.state_dict().items()}
    torch.save(sd, _shard_file(path, ctx.rank, ctx.world))
    if ctx.rank == 0:
        with open(path + ".meta.json", "w") as f:
            json.dump({"world": ctx.world, "sharded_keys": list(sharded_keys)}, f)
    ctx.barrier()


def load_sharded(engine, path, rank: int, world: int, global_rows: dict):
    """global_rows: {sharded key: rows of the GLOBAL table}.  Works for any saved world size."""
    import json
    with open(path + ".meta.json") as f:
        meta = json.load(f)
    W0, keys = int(meta["world"]), set(meta["sharded_keys"])

    def fit(sd):
        """row-sharded entries cut / zero-padded to the engine's row count (an engine with the padded exchange has a spare row)"""
        have = engine.state_dict()
        for k in keys:
            want = have[k].shape[0]
            if sd[k].shape[0] > want:
                sd[k] = sd[k][:want]
            elif sd[k].shape[0] < want:
                sd[k] = torch.cat([sd[k], torch.zeros((want - sd[k].shape[0],) + tuple(sd[k].shape[1:]), dtype=sd[k].dtype)])
        return sd

    if W0 == world:
        engine.load_state_dict(fit(torch.load(_shard_file(path, rank, world), map_location="cpu", weights_only=True)))
        return
    shards = [torch.load(_shard_file(path, r, W0), map_location="cpu", weights_only=True) for r in range(W0)]
    sd = {}
    for k, v in shards[0].items():
        if k not in keys:
            sd[k] = v                                     # replicated (dense parameters, counters)
            continue
        rows = int(global_rows[k])
        full = torch.zeros((rows,) + tuple(v.shape[1:]), dtype=v.dtype)
        for r in range(W0):
            n = shard_rows(rows, r, W0)
            if n:
                full[r::W0] = shards[r][k][:n]
        mine = full[rank::world]
        sd[k] = mine if mine.shape[0] else torch.zeros((1,) + tuple(v.shape[1:]), dtype=v.dtype)
    engine.load_state_dict(fit(sd))


# ---------------------------------------------------------------------------------------------------------------------
# Catalogue top-k scored where the item rows live.  The candidate rows never travel: every rank scores the queries
# of ALL ranks against the candidates it owns with the single-device fused launch, the k-entry lists go back to the rank that
# asked, and brTopKListsMerge merges each user's W lists under the launch's own order - bit for bit the single-device lists.
# ---------------------------------------------------------------------------------------------------------------------
def gather_global_rows(ctx: DistCtx, ids: torch.Tensor, serve, width: int):
    """rows `ids` (global ids, any owner) of a row-sharded table -> (len(ids), width) on this rank, through the id -> owner exchange
    of the training step; serve(local_rows) -> the owner's rows.  A collective."""
    from . import ops
    x = ShardExchange(ctx)
    if ids.numel():
        x.plan(ids)
    else:                                   # nothing to ask for, but the peers' requests are still served: the empty plan
        x.order = x.inv = torch.empty(0, dtype=torch.int32, device=ids.device)
        x.send_local, x.send_counts_t = ids, torch.zeros(ctx.world, dtype=torch.int64, device=ids.device)
    x.exchange_counts()
    served = x.send_ids()
    empty = torch.empty(0, width, dtype=torch.float32, device=ids.device)
    back = x.return_rows(serve(served) if served.numel() else empty)            # bucket order
    return ops.gather_rows([back], [x.inv.to(ids.dtype)])[0] if ids.numel() else empty


def _all_gather_ragged(ctx: DistCtx, t: torch.Tensor, counts):
    """rank r contributes counts[r] rows of t's shape -> the rows of all ranks, rank after rank (padded to the longest for the
    collective, the pads dropped again)."""
    if ctx.local:
        return t
    m = max(counts)
    pad = torch.zeros((m,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[:t.shape[0]].copy_(t)
    g = ctx.all_gather_rows(pad)
    return torch.cat([g[r * m:r * m + c] for r, c in enumerate(counts)]) if m else g


def _owners_meta(ctx: DistCtx, what: str, n_users: int, n_csr: int, items, k: int):
    """What every rank of an owner-side catalogue collective must know about the others, in ONE small all-gather and one host sync: the
    user and CSR entry counts (n_csr = -1: this rank passes no CSR), and that the candidate lists agree (length, k and a
    position-weighted checksum of the ids; a mismatch raises on every rank) -> (user counts, CSR counts) per rank."""
    I, dev = items.shape[0], items.device
    fp = (items.to(torch.int64) * (torch.arange(I, device=dev, dtype=torch.int64) % 65521 + 1)).sum()
    meta = torch.tensor([[n_users, n_csr, I, k, 0]], dtype=torch.int64).to(dev)
    meta[0, 4] = fp
    meta = ctx.all_gather_rows(meta).cpu().tolist()
    if any(m[2:] != meta[0][2:] for m in meta):
        raise ValueError(f"{what} on a row-sharded engine: every rank must pass the same items and k "
                         f"(rank {ctx.rank} sees (len, k, checksum) = {[m[2:] for m in meta]})")
    return [int(m[0]) for m in meta], [int(m[1]) for m in meta]


def _all_gather_csr(ctx: DistCtx, off, idx, n_users: int, u_counts, c_counts):
    """the per-user CSRs (off, idx) of all ranks -> one CSR over the users of all ranks, rank after rank (off None: this rank has no
    lists, its users get empty ones).  Depends only on what the meta gather told every rank: a rank without users or candidates still
    takes part."""
    dev = idx.device
    lens = (off[1:] - off[:-1]) if off is not None else torch.zeros(n_users, dtype=torch.int64, device=dev)
    off_all = torch.zeros(sum(u_counts) + 1, dtype=torch.int64, device=dev)
    off_all[1:] = _all_gather_ragged(ctx, lens, u_counts).cumsum(0)
    return off_all, _all_gather_ragged(ctx, idx, [max(c, 0) for c in c_counts]).contiguous()


class _CandidatePlan:
    """This rank's share of a candidate list every rank holds: positions p with items[p] mod W == rank in ascending p (the exchange
    plan's bucket order is the W ascending local -> global maps one after the other), local row items[p] div W."""

    def __init__(self, ctx: DistCtx, items):
        W, r, dev = ctx.world, ctx.rank, items.device
        plan = ShardExchange(ctx).plan(items)
        self.n_global = items.shape[0]
        self.l2g = plan.order.to(torch.int32).contiguous()
        self.l2g_off = torch.zeros(W + 1, dtype=torch.int64, device=dev)
        self.l2g_off[1:] = plan.send_counts_t.to(torch.int64).cumsum(0)
        self.lo, self.hi = (int(v) for v in self.l2g_off[r:r + 2].cpu().tolist())
        self.n_loc = self.hi - self.lo
        self.local_rows = plan.send_local[self.lo:self.hi].contiguous()

    def split_csr(self, off, idx):
        """a CSR of global positions cut down to this rank's candidates, in its local positions (brCsrSplitByOwner)"""
        from . import ops
        g2l = torch.full((self.n_global,), -1, dtype=torch.int32, device=off.device)
        g2l[self.l2g[self.lo:self.hi].long()] = torch.arange(self.n_loc, dtype=torch.int32, device=off.device)
        return ops.csr_split_by_owner(off, idx, g2l)


def recommend_at_owners(ctx: DistCtx, users, items, n_item_rows: int, k: int, exclude, fetch_user_rows, queries_of, candidates_of, score):
    """The single-device `recommend` contract on row-sharded tables.  A collective, like predict_scores: every rank calls it with
    its own `users` (device ids; counts may differ and may be 0), the SAME `items` (device ids in any order, None = every item row)
    and optionally an exclusion CSR (off, idx) over its own users in positions of `items`; it gets (scores (U_r, k) float32,
    index (U_r, k) int32 positions into `items`) for its users.  The engine supplies
      fetch_user_rows(ids) -> this rank's users' table rows (the id -> owner exchange, gather_global_rows)
      queries_of(rows)     -> the query rows the fused launch reads, from the user rows of ALL ranks
      candidates_of(local) -> the candidate operand of the launch from this rank's own item rows `local` (ids div W)
      score(q, c, k, excl) -> (scores, index) of the fused launch over q x c."""
    from . import ops
    W, dev = ctx.world, users.device
    k = int(k)
    if not 1 <= k <= 256:
        raise ValueError(f"k = {k}: 1 <= k <= 256")
    if items is None:
        items = torch.arange(n_item_rows, dtype=users.dtype, device=dev)
    U, I = users.shape[0], items.shape[0]
    if I < 1:
        raise ValueError("recommend: empty candidate list")
    has_ex = exclude is not None
    if has_ex:
        ex_off, ex_idx = ops._csr(exclude, U, "exclude")
        ex_idx = ex_idx[:int(exclude[1].numel())]
    u_counts, e_counts = _owners_meta(ctx, "recommend", U, int(exclude[1].numel()) if has_ex else -1, items, k)
    U_all = sum(u_counts)
    if U_all == 0:
        return torch.empty(0, k, dtype=torch.float32, device=dev), torch.empty(0, k, dtype=torch.int32, device=dev)
    # 1. the queries of all ranks on every rank
    rows_all = _all_gather_ragged(ctx, fetch_user_rows(users), u_counts)
    q_all = queries_of(rows_all)
    # 2. this rank's candidates
    plan = _CandidatePlan(ctx, items)
    # 3. the exclusion lists of all ranks on every rank
    csr_all = None
    if any(c >= 0 for c in e_counts):
        csr_all = _all_gather_csr(ctx, ex_off if has_ex else None, ex_idx if has_ex else torch.empty(0, dtype=torch.int32, device=dev), U,
                                  u_counts, e_counts)
    if plan.n_loc:
        cand = candidates_of(plan.local_rows)
        excl = plan.split_csr(*csr_all) if csr_all is not None else None
        s_loc, p_loc = score(q_all, cand, k, excl)
    else:                        # no candidate of the list lives here: empty lists for everybody
        s_loc = torch.full((U_all, k), float("-inf"), dtype=torch.float32, device=dev)
        p_loc = torch.full((U_all, k), -1, dtype=torch.int32, device=dev)
    # 4. [score bits | positions] of every user back to its rank in one all-to-all, then the merge reads the receive buffer in place:
    #    list w of user u at row w * U + u
    send = torch.cat([s_loc.view(torch.int32), p_loc], dim=1)
    recv = torch.empty(W * U, 2 * k, dtype=torch.int32, device=dev)
    ctx.all_to_all(recv, send, [U] * W, u_counts)
    if U == 0:
        return torch.empty(0, k, dtype=torch.float32, device=dev), torch.empty(0, k, dtype=torch.int32, device=dev)
    return ops.topk_lists_merge(recv.view(torch.float32), recv[:, k:], W, U, k, plan.l2g, plan.l2g_off, list_stride=U * 2 * k, user_stride=2 * k)


def _sorted_positives_at_owners(ctx: DistCtx, plan: "_CandidatePlan", q_all, off_all, idx_all, T_all: int, candidates_of, positives):
    """What auc_at_owners and ranks_at_owners share behind the gathered queries and truth lists: this rank's candidates, its share
    of every user's positives in its local positions, and every user's full sorted list of positives on every rank.  Every owner's
    per-user counts, then its raw scores, go to every rank: each piece padded to the longest (one host sync to learn it), and the
    lists are sorted from the receive buffer in place.  A rank that owns no candidate of the list has no positives but joins both
    all-gathers.  -> (cand, pos_off, pos_idx: None on such a rank; raw: this rank's piece (1, max(longest, 1)); sorted_, pcnt)."""
    from . import ops
    W, dev, U_all = ctx.world, q_all.device, off_all.shape[0] - 1
    cand = pos_off = pos_idx = None
    if plan.n_loc:
        cand = candidates_of(plan.local_rows)
        pos_off, pos_idx = plan.split_csr(off_all, idx_all)
        lens = (pos_off[1:] - pos_off[:-1]).to(torch.int32)
    else:
        lens = torch.zeros(U_all, dtype=torch.int32, device=dev)
    lens_all = ctx.all_gather_rows(lens.view(1, U_all)).to(torch.int64)
    m = int(lens_all.sum(1).max().item())
    raw = torch.zeros(1, max(m, 1), dtype=torch.float32, device=dev)
    if plan.n_loc and m:
        positives(q_all, cand, pos_off, pos_idx, raw)
    raw_all = ctx.all_gather_rows(raw) if m else raw.repeat(W, 1)
    piece_off = torch.zeros(W, U_all + 1, dtype=torch.int64, device=dev)
    piece_off[:, 1:] = lens_all.cumsum(1)
    piece_off += (torch.arange(W, dtype=torch.int64, device=dev) * raw.shape[1]).view(W, 1)
    sorted_, pcnt = ops.auc_sort_pieces(raw_all, piece_off, off_all, T_all)
    return cand, pos_off, pos_idx, raw, sorted_, pcnt


# ---------------------------------------------------------------------------------------------------------------------
# Full-catalogue AUC counted where the item rows live: recommend_at_owners' turn for full_auc.  Every rank scores the
# positives it owns, the raw scores of all owners are sorted into every user's full list on every rank, each rank counts the queries
# of ALL ranks against its own candidates, and the integer partial counts go back to the rank that asked: they add up exactly, so the
# one division gives the single-device float bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def auc_at_owners(ctx: DistCtx, users, items, n_item_rows: int, truth, fetch_user_rows, queries_of, candidates_of, dim: int = None,
                  force_wide: bool = False, positives=None, count=None):
    """The single-device `full_auc` contract on row-sharded tables.  A collective: every rank calls it with its own `users` (device
    ids; counts may differ and may be 0), the SAME `items` (None = every item row) and the truth CSR (off, idx) over its own users in
    ascending positions of `items` (ops.truth_csr); it gets the float32 AUCs of its users, NaN where undefined.  fetch_user_rows,
    queries_of and candidates_of as in recommend_at_owners; dim: the width of the query and candidate rows (checked when given).
    positives(q, cand, pos_off, pos_idx, out) and count(q, cand, skip_off, skip_idx, list_off, sorted_, pcnt): the model's scoring
    phases over this rank's candidates (defaults: the dot-product ones, ops.dot_auc_owner_positives / ops.dot_auc_owner_count with
    force_wide; NeuMF passes ops.neumf_auc_positives / ops.neumf_auc_count over its projected operands)."""
    from . import ops
    if positives is None:
        positives = lambda q, c, po, pi, out: ops.dot_auc_owner_positives(q, c, po, pi, out=out, force_wide=force_wide)
    if count is None:
        count = lambda q, c, so, si, lo, srt, pc: ops.dot_auc_owner_count(q, c, so, si, lo, srt, pc, force_wide=force_wide)
    W, r, dev = ctx.world, ctx.rank, users.device
    if items is None:
        items = torch.arange(n_item_rows, dtype=users.dtype, device=dev)
    U, I = users.shape[0], items.shape[0]
    if I < 1:
        raise ValueError("full_auc: empty candidate list")
    n_truth = int(truth[1].numel())
    t_off, t_idx = ops._csr(truth, U, "truth")
    t_idx = t_idx[:n_truth]
    # 1. user and truth counts, and that the candidate lists agree
    u_counts, t_counts = _owners_meta(ctx, "full_auc", U, n_truth, items, 0)
    U_all = sum(u_counts)
    if U_all == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    # 2. the queries and the truth lists (global positions) of all ranks on every rank
    q_all = queries_of(_all_gather_ragged(ctx, fetch_user_rows(users), u_counts))
    if dim is not None and q_all.shape[1] != dim:
        raise ValueError(f"full_auc: the query rows have {q_all.shape[1]} features, dim = {dim}")
    off_all, idx_all = _all_gather_csr(ctx, t_off, t_idx, U, u_counts, t_counts)
    T_all = sum(t_counts)
    # 3, 4. this rank's candidates and its share of every user's positives; every user's full sorted list on every rank
    plan = _CandidatePlan(ctx, items)
    cand, pos_off, pos_idx, _raw, sorted_, pcnt = _sorted_positives_at_owners(ctx, plan, q_all, off_all, idx_all, T_all, candidates_of, positives)
    # 5. all queries x the local candidates: one integer 2W per user
    if plan.n_loc:
        w2 = count(q_all, cand, pos_off, pos_idx, off_all, sorted_, pcnt)
    else:
        w2 = torch.zeros(U_all, dtype=torch.int64, device=dev)
    # 6. the partials of every user back to its rank in one all-to-all; the finalize reads the receive buffer in place: list w of user
    #    u at w * U + u
    recv = torch.empty(W * U, dtype=torch.int64, device=dev)
    ctx.all_to_all(recv, w2, [U] * W, u_counts)
    if U == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    u0 = sum(u_counts[:r])
    return ops.auc_finalize_lists(recv, W, U, t_off, pcnt[u0:u0 + U], I, list_stride=U)


# ---------------------------------------------------------------------------------------------------------------------
# Exact catalogue ranks counted where the item rows live: auc_at_owners' turn for catalog_ranks.  Steps 1 to 4 are
# auc_at_owners': every user's full sorted list of positives on every rank.  Then each rank counts the queries of ALL ranks against its
# own candidates into bins laid out by the GLOBAL truth offsets, the integer bins are summed over the ranks, each rank finalizes the
# truth entries it owns (it holds their raw scores) and the (above, tied) pairs are put together: integers add exactly, so the result
# is the single-device one entry for entry.
# ---------------------------------------------------------------------------------------------------------------------
def csr_union(a, b, n_cols: int):
    """two CSRs (off, idx) over the same rows, per row ascending unique positions in [0, n_cols) (idx may have spare capacity behind
    off[-1], as csr_split_by_owner leaves it) -> the CSR of their union per row, ascending.  Two host syncs (the entry counts)."""
    n_rows, dev = a[0].shape[0] - 1, a[0].device
    keys = []
    for off, idx in (a, b):
        n = int(off[-1].item())
        rows = torch.repeat_interleave(torch.arange(n_rows, dtype=torch.int64, device=dev), off[1:] - off[:-1], output_size=n)
        keys.append(rows * n_cols + idx[:n].to(torch.int64))
    k = torch.unique(torch.cat(keys))                       # sorted: by row, then by position
    off = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.bincount(k // n_cols, minlength=n_rows).cumsum(0)
    return off, (k % n_cols).to(torch.int32).contiguous()


def ranks_at_owners(ctx: DistCtx, users, items, n_item_rows: int, truth, exclude, fetch_user_rows, queries_of, candidates_of, count, positives):
    """The single-device `catalog_ranks` contract on row-sharded tables.  A collective: every rank calls it with its own `users` (device
    ids; counts may differ and may be 0), the SAME `items` (None = every item row), the truth CSR (off, idx) over its own users in
    ascending positions of `items` and optionally an exclusion CSR of the same kind; it gets (above, tied) int32 for its own truth
    entries, in CSR order.  fetch_user_rows, queries_of and candidates_of as in recommend_at_owners; the model's two scoring phases over
    this rank's candidates: positives(q, cand, pos_off, pos_idx, out) (ops.neumf_auc_positives; the dot-product models:
    ops.dot_auc_owner_positives) and count(q, cand, skip_off, skip_idx, list_off, sorted_, pcnt, bins, ties) (ops.neumf_rank_count;
    ops.dot_rank_count), which adds into the bins."""
    from . import ops
    r, dev = ctx.rank, users.device
    if items is None:
        items = torch.arange(n_item_rows, dtype=users.dtype, device=dev)
    U, I = users.shape[0], items.shape[0]
    if I < 1:
        raise ValueError("catalog_ranks: empty candidate list")
    n_truth = int(truth[1].numel())
    t_off, t_idx = ops._csr(truth, U, "truth")
    t_idx = t_idx[:n_truth]
    has_ex = exclude is not None
    if has_ex:
        ex_off, ex_idx = ops._csr(exclude, U, "exclude")
        ex_idx = ex_idx[:int(exclude[1].numel())]
    none = torch.empty(0, dtype=torch.int32, device=dev)
    # 1. user, truth and exclusion counts, and that the candidate lists agree
    u_counts, t_counts = _owners_meta(ctx, "catalog_ranks", U, n_truth, items, 0)
    _u, e_counts = _owners_meta(ctx, "catalog_ranks", U, int(exclude[1].numel()) if has_ex else -1, items, 0)
    U_all, T_all = sum(u_counts), sum(t_counts)
    if U_all == 0:
        return none, none.clone()
    # 2. the queries, the truth lists and the exclusion lists (global positions) of all ranks on every rank
    q_all = queries_of(_all_gather_ragged(ctx, fetch_user_rows(users), u_counts))
    off_all, idx_all = _all_gather_csr(ctx, t_off, t_idx, U, u_counts, t_counts)
    any_ex = any(c >= 0 for c in e_counts)
    if any_ex:
        x_all = _all_gather_csr(ctx, ex_off if has_ex else None, ex_idx if has_ex else none, U, u_counts, e_counts)
    # 3, 4. this rank's candidates, its share of every user's excluded positions and positives in its local positions; every user's
    #    full sorted list of positives on every rank
    plan = _CandidatePlan(ctx, items)
    excl = plan.split_csr(*x_all) if plan.n_loc and any_ex else None
    cand, pos_off, pos_idx, raw, sorted_, pcnt = _sorted_positives_at_owners(ctx, plan, q_all, off_all, idx_all, T_all, candidates_of, positives)
    # 5. all queries x the local candidates into zeroed bins over the global lists, then this rank's excluded positives out of them
    bins, ties = ops.rank_bins(U_all, T_all, dev)
    if plan.n_loc:
        skip = csr_union((pos_off, pos_idx), excl, plan.n_loc) if excl is not None else (pos_off, pos_idx)
        count(q_all, cand, skip[0], skip[1], off_all, sorted_, pcnt, bins, ties)
        if excl is not None:
            ops.rank_bins_excluded(pos_off, pos_idx, excl, raw.view(-1), off_all, sorted_, pcnt, bins, ties)
    # 6. the integer bins of all owners summed on every rank
    ctx.all_reduce_sum(bins)
    ctx.all_reduce_sum(ties)
    # 7. every owner finalizes the entries it holds (entry CSR: its split CSR, raw: its own piece; list CSR: the global one) and puts
    #    them where they stand in the global truth order: brCsrSplitByOwner keeps the input order, so its entries are the global ones
    #    with g2l >= 0, in order.  1 + value, 0 where another rank owns the entry: the sum over the ranks is 1 + the owner's value
    out = torch.zeros(2, max(T_all, 1), dtype=torch.int32, device=dev)
    if plan.n_loc and T_all:
        a_loc, t_loc = ops.rank_bins_finalize(pos_off, pos_idx, excl, raw.view(-1), off_all, sorted_, pcnt, bins, ties)
        g2l = torch.full((I,), -1, dtype=torch.int32, device=dev)
        g2l[plan.l2g[plan.lo:plan.hi].long()] = torch.arange(plan.n_loc, dtype=torch.int32, device=dev)
        g = idx_all.long()
        own = ((g >= 0) & (g < I)) & (g2l[g.clamp(0, I - 1)] >= 0)
        slot = (own.cumsum(0) - 1).clamp(min=0)
        out[0, :T_all] = torch.where(own, a_loc[slot] + 1, 0)
        out[1, :T_all] = torch.where(own, t_loc[slot] + 1, 0)
    ctx.all_reduce_sum(out)
    out -= 1                     # an entry no rank owns (a position outside the list) keeps -1
    t0 = sum(t_counts[:r])
    return out[0, t0:t0 + n_truth].contiguous(), out[1, t0:t0 + n_truth].contiguous()


def make_sharded_engine(base_cls):
    """ShardedNeuMFEngine = NeuMFEngine with its embed / table-optimizer hooks replaced by the
    row-sharded exchange.  (Factory so this module stays importable without the HIP library.)"""
    from . import ops
    from .neumf import TABLES

    class ShardedNeuMFEngine(base_cls):
        sharded = True

        def __init__(self, cfg, num_user_rows, num_item_rows, device, max_batch, ctx: DistCtx, **kw):
            self.ctx = ctx
            self.full_tables = kw.pop("full_tables", None)   # tests: {name: full (rows, D) tensor} to slice
            # "padded" (default): fixed per-peer capacity, no host sync in the step (PaddedExchange); "exact": row counts over the host
            self.exchange = kw.pop("exchange", "padded")
            self.exchange_capacity = float(kw.pop("exchange_capacity", 1.25))
            if self.exchange not in ("padded", "exact"):
                raise ValueError("exchange must be 'padded' or 'exact'")
            super().__init__(cfg, num_user_rows, num_item_rows, device, max_batch, dist=ctx, **kw)
            self.xu, self.xi = ShardExchange(ctx), ShardExchange(ctx)
            if self.exchange == "padded":
                self.px = PaddedExchange(ctx, max_batch, self.id_dtype, self.device, (num_user_rows, num_item_rows), 2 * cfg.dim, self.exchange_capacity)
                self._grow_index(self.px.n_slots)

        def owned_rows(self, name):
            total = self.num_user_rows if name.startswith("user") else self.num_item_rows
            return shard_rows(total, self.ctx.rank, self.ctx.world)

        def local_rows(self, name):
            """rows of this rank's table tensors: the rows it owns (+ the spare row the pad slots of the padded exchange point at)"""
            return max(1, self.owned_rows(name)) + (1 if self.exchange == "padded" else 0)

        def _init_tables(self, g, init_seed):
            if self.full_tables is not None:     # tests: slice the rows this rank owns out of global tables
                D = self.cfg.dim
                self.fused = {}
                for stream in ("user", "item"):
                    full = torch.cat([self.full_tables[stream + "_mlp"], self.full_tables[stream + "_mf"]], dim=1)
                    t = full[self.ctx.rank::self.ctx.world].contiguous().to(self.device)
                    t = t if t.shape[0] else torch.zeros(1, 2 * D, device=self.device)
                    if self.exchange == "padded":
                        t = torch.cat([t, torch.zeros(1, 2 * D, device=self.device)])
                    self.fused[stream] = t
                self._make_views()
                return
            super()._init_tables(g, init_seed + 104729 * self.ctx.rank)

        def _alloc_sparse(self, B):
            # an owner can receive more than B ids in a step; indexes are (re)grown on demand
            self._idx_cap = 0
            self._grow_index(2 * B)

        def _grow_index(self, n):
            if n > self._idx_cap:
                self._idx_cap = int(n * 1.25) + 64
                self.user_index = ops.RowIndex(self._idx_cap, self.id_dtype, self.device)
                self.item_index = ops.RowIndex(self._idx_cap, self.id_dtype, self.device)
                if hasattr(self, "step_struct"):
                    self._bind_indexes(self.step_struct)

        def _embed_forward(self, users, items, B):
            D = self.cfg.dim
            if self.exchange == "padded":
                x, cfg = self.px, self.cfg
                x.plan(users, items, self.err)
                rid = x.send_ids()                                 # all-to-all #1 (both streams)
                S, (sl, ss_, ou_, oi_) = x.n_slots, x.seg
                # the owner-side dedup indexes depend only on the ids just received: both in shared launches on a side stream,
                # beside the lookup / MLP, joined before the Adam-rows kernels
                main = torch.cuda.current_stream(self.device)
                if getattr(self, "_side", None) is None:
                    self._side, self._ev_ids, self._ev_index = torch.cuda.Stream(device=self.device), torch.cuda.Event(), torch.cuda.Event()
                self._ev_ids.record(main)
                self._side.wait_event(self._ev_ids)
                with torch.cuda.stream(self._side):
                    # every source's segment arrives sorted (distinct local rows in key order, pads = the spare row last): the index is a
                    # merge of W sorted runs, no sort (BR_MERGE_INDEX=0: the chunk-sort build, A/B)
                    if os.environ.get("BR_MERGE_INDEX", "1") != "0":
                        ops.row_index_merge_pair_seg(self.user_index, self.local_rows("user_mf"), self.item_index, self.local_rows("item_mf"), rid, S, x.seg, self.err)
                    else:
                        ops.row_index_build_pair_seg(self.user_index, self.local_rows("user_mf"), self.item_index, self.local_rows("item_mf"), rid, S, x.seg)
                    self._ev_index.record(self._side)
                # owner-side G1 on the fused [mlp | mf] rows (512 B at dim 64): both shards, one launch, straight into the slots
                if self.deferred and 2 * D in (64, 128, 256):
                    ops.gather_rows_deferred_pair_seg(self.fused["user"], self.fused_m["user"], self.fused_v["user"], self.last["user"],
                                                      self.fused["item"], self.fused_m["item"], self.fused_v["item"], self.last["item"], rid, x.served, S, x.seg,
                                                      self.step_state, cfg.beta1, cfg.beta2, cfg.adam_eps, err_flag=self.err)
                elif self.deferred:      # other row widths: the row-group gather per stream, through contiguous copies of the stream's slots
                    W, cap = x.W, x.cap
                    for k, stream in enumerate(("user", "item")):
                        ids_k = rid.view(W, 2, cap)[:, k].contiguous().view(-1)
                        rows_k = self.rows_as_of_previous_step(stream, ids_k)
                        x.served.view(W, 2, cap, 2 * D)[:, k].copy_(rows_k.view(W, cap, 2 * D))
                else:
                    ops.gather_rows_pair_seg(self.fused["user"], self.fused["item"], rid, x.served, S, x.seg, err_flag=self.err)
                rows = x.return_rows()                             # all-to-all #2 (both streams)
                self.pos_u, self.pos_i = x.slot[0][:B], x.slot[1][:B]
                if self.id_dtype != torch.int32:
                    self.pos_u, self.pos_i = self.pos_u.to(self.id_dtype), self.pos_i.to(self.id_dtype)
                # requester side: the fused embed kernel with the received slots as its "tables" (ids = slots; an id without a slot reads
                # zeros - flagged by the plan, not here); the MF rows of every pair are stashed by position for the backward
                ops.neumf_embed_forward(rows[:, :D], rows[:, :D], rows[:, D:], rows[:, D:], self.pos_u, self.pos_i, self.cfg.item_first,
                                        self.x0[:B], self.dot[:B], None, stash=(self.g_user[:B, D:], self.g_item[:B, D:]))
                return
            xu, xi = ShardExchange.plan_pair(self.xu, users, self.xi, items)
            xu.exchange_counts(xi)                     # the step's one host sync (variable split sizes)
            ru, ri = xu.send_ids(), xi.send_ids()      # all-to-all #1
            empty = torch.empty(0, 2 * D, device=self.device)
            # owner-side G1 on the fused [mlp | mf] rows (512 B at dim 64)
            gu = self.rows_as_of_previous_step("user", ru) if ru.numel() else empty
            gi = self.rows_as_of_previous_step("item", ri) if ri.numel() else empty
            self._served = {"user": gu, "item": gi}    # kept for the optimizer: this rank's rows replayed to step t-1, by received slot
            self.r_user, self.r_item = xu.return_rows(gu), xi.return_rows(gi)      # all-to-all #2
            self.pos_u = xu.inv.to(self.id_dtype)
            self.pos_i = xi.inv.to(self.id_dtype)
            # requester-side: same fused embed kernel, "tables" = received rows, ids = bucket slots
            ops.neumf_embed_forward(self.r_user[:, :D], self.r_item[:, :D], self.r_user[:, D:], self.r_item[:, D:], self.pos_u,
                                    self.pos_i, self.cfg.item_first, self.x0[:B], self.dot[:B], self.err)

        # ------------------------------------------------------------------ hipGraph replay of the sharded step
        def enable_graph(self, batch: int | None = None):
            """Replay the row-sharded step - its ~25 launches AND its four RCCL collectives - as ONE hipGraph per step for local batches
            of exactly `batch` pairs.  Needs the fixed-capacity exchange (no host sync in the step) and deferred tables (every per-step
            scalar in the device step state).  The first such step runs eagerly on the static input buffers (every kernel and every
            collective once outside a capture), then the step's body is captured; a runtime / backend that refuses the capture (gloo
            stages its collectives through the host) keeps the eager sequence - `graph_active` tells which."""
            if self.exchange != "padded" or not self.deferred:
                raise ValueError("graph replay of the sharded step needs exchange='padded' and optimizer='adam_dense' with dense_impl='deferred'")
            B = self.max_batch if batch is None else int(batch)
            if not 0 < B <= self.max_batch:
                raise ValueError("graph batch must be in (0, max_batch]")
            dev = self.device
            self.in_users = torch.zeros(B, dtype=self.id_dtype, device=dev)
            self.in_items = torch.zeros(B, dtype=self.id_dtype, device=dev)
            self.in_labels = torch.zeros(B, dtype=torch.float32, device=dev)
            self._sgraph = {"batch": B, "graph": None, "key": None, "refused": None}

        def disable_graph(self):
            self._sgraph = None

        @property
        def graph_active(self) -> bool:
            g = getattr(self, "_sgraph", None)
            return bool(g and g["graph"] is not None)

        def train_step(self, users, items, labels, row0: int = 0, batch_total: int | None = None):
            g = getattr(self, "_sgraph", None)
            B = users.shape[0]
            self._moving_dirty = True            # (per-replica BatchNorm: this rank's moving statistics move apart from the others')
            if g is None or B != g["batch"]:
                return super().train_step(users, items, labels, row0=row0, batch_total=batch_total)
            from . import _lib
            bt = B if batch_total is None else batch_total
            self._check_batch(users, items, labels)
            _lib.check(_lib.load().brStageBatch(self.in_users.data_ptr(), self.in_items.data_ptr(), self.in_labels.data_ptr(), users.data_ptr(), items.data_ptr(),
                                                labels.data_ptr(), self.step_struct.id_type, B, ops._stream()), "brStageBatch")
            if g["graph"] is not None and g["key"] == (row0, bt):
                self.begin_steps(1)
                self.t += 1
                g["graph"].replay()
                return
            super().train_step(self.in_users, self.in_items, self.in_labels, row0=row0, batch_total=bt)      # eager: also the warm-up of the capture
            if g["graph"] is None and g["refused"] is None:
                self._capture_step(g, B, row0, bt)

        def _capture_step(self, g, B, row0, bt):
            ctx = self.ctx
            if not ctx.local and ctx.backend != "nccl":
                g["refused"] = f"backend {ctx.backend}: collectives are staged through the host"
                return
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            try:
                self._set_batch(self.in_users, self.in_items, self.in_labels, B, True, row0, bt)
                with torch.cuda.graph(graph):
                    self._dist_step(self.in_users, self.in_items, B)
                g["graph"], g["key"] = graph, (row0, bt)
            except Exception as exc:  # noqa: BLE001 - the runtime refused (a collective or a launch that cannot be captured): eager from here on
                g["refused"] = f"{type(exc).__name__}: {exc}"
                try:
                    torch.cuda.synchronize(self.device)
                except Exception:  # noqa: BLE001
                    pass

        SHARDED_KEYS = ("table.user", "table.user.m", "table.user.v", "table.item", "table.item.m", "table.item.v")

        def save_sharded(self, path):
            """model.save for the row-sharded engine (every rank writes its shard; see save_sharded above)."""
            save_sharded(self, path, self.ctx, self.SHARDED_KEYS)

        def load_sharded(self, path):
            rows = {k: (self.num_user_rows if ".user" in k else self.num_item_rows) for k in self.SHARDED_KEYS}
            load_sharded(self, path, self.ctx.rank, self.ctx.world, rows)

        def state_dict(self):
            """Per-replica BatchNorm (sync_bn=False) updates the moving statistics from each rank's own batch: reconcile them first
            (MirroredStrategy keeps them as ON_READ variables aggregated by MEAN [TF-sem]), so every rank saves / predicts the same."""
            self.sync_moving_stats()
            return super().state_dict()

        def sync_moving_stats(self):
            """a COLLECTIVE when per-replica BatchNorm has trained since the last call (every rank must then reach it: state_dict(),
            save_sharded(), predict() and evaluate_batch() of a sharded engine are collectives anyway); a no-op otherwise, so repeated
            reads between two training steps cost nothing and cannot hang a lone reader."""
            if self.ctx.world > 1 and not self.cfg.sync_bn and getattr(self, "_moving_dirty", False):
                self.ctx.all_reduce_sum(self.moving_buf)
                self.moving_buf.div_(self.ctx.world)
            self._moving_dirty = False

        def _infer(self, users, items, labels, n):
            self.sync_moving_stats()
            return super()._infer(users, items, labels, n)

        def _owner_catalog(self, users, items):
            """What the collectives recommend and full_auc set up alike: -> (users, items, folded tower, and the three callables
            *_at_owners take: user rows through gather_global_rows, the user projection of fetched rows, the column-major item
            projection of local rows)"""
            users, items = self._catalog_ids(users, items, every_item=False)
            self.sync_moving_stats()
            th, tower = self._catalog_tower()
            D, dev = self.cfg.dim, self.device
            fetch = lambda ids: gather_global_rows(self.ctx, ids, lambda loc: ops.gather_rows([self.fused["user"]], [loc], err_flag=self.err)[0], 2 * D)
            queries_of = lambda rows: self._catalog_project(th, rows, torch.arange(rows.shape[0], dtype=torch.int32, device=dev), True)
            candidates_of = lambda loc: self._catalog_project(th, self.fused["item"], loc, False)
            return users, items, tower, fetch, queries_of, candidates_of

        def recommend(self, users, k, items=None, exclude=None, dump_logits=None):
            """NeuMFEngine.recommend on the row-sharded tables (recommend_at_owners): a collective - every rank calls it with its own
            users (any number, also none), the same `items` and k, and gets the single-device lists of ITS users bit for bit.  Every
            owner projects and scores only the items whose rows it holds; user rows travel out, k-entry lists travel back."""
            if dump_logits:
                raise NotImplementedError("recommend(dump_logits=True) on the row-sharded engine is not supported: no rank forms the "
                                          "logits of another owner's items; score with a single-device engine")
            cfg, hidden = self.cfg, tuple(self.cfg.hidden)
            users, items, tower, fetch, queries_of, candidates_of = self._owner_catalog(users, items)
            return recommend_at_owners(self.ctx, users, items, self.num_item_rows, k, exclude, fetch, queries_of, candidates_of,
                                       lambda q, c, kk, ex: ops.neumf_catalog_topk(q, c, tower, cfg.dim, hidden, cfg.act, kk, exclude=ex))

        def full_auc(self, users, truth, items=None, dump_probs=False, method="fused"):
            """NeuMFEngine.full_auc on the row-sharded tables (auc_at_owners): a collective - every rank calls it with its own users
            (any number, also none), their truth CSR and the same `items`, and gets the single-device floats of ITS users bit for bit.
            Every owner projects, scores and counts only the items whose rows it holds; user rows, the positives' probabilities and
            one integer count per user travel."""
            if dump_probs:
                raise NotImplementedError("full_auc(dump_probs=True) on the row-sharded engine is not supported: no rank forms the "
                                          "probabilities of another owner's items; score with a single-device engine")
            if method != "fused":
                raise NotImplementedError(f"full_auc(method={method!r}) on the row-sharded engine is not supported: predict is a collective "
                                          "over pairs, every rank's tables hold a share of the rows; use method='fused'")
            cfg, hidden = self.cfg, tuple(self.cfg.hidden)
            users, items, tower, fetch, queries_of, candidates_of = self._owner_catalog(users, items)
            return auc_at_owners(
                self.ctx, users, items, self.num_item_rows, truth, fetch, queries_of, candidates_of,
                positives=lambda q, c, po, pi, out: ops.neumf_auc_positives(q, c, tower, cfg.dim, hidden, cfg.act, po, pi, out=out),
                count=lambda q, c, so, si, lo, srt, pc: ops.neumf_auc_count(q, c, tower, cfg.dim, hidden, cfg.act, so, si, lo, srt, pc))

        def catalog_ranks(self, users, truth, items=None, exclude=None, dump_probs=False):
            """NeuMFEngine.catalog_ranks on the row-sharded tables (ranks_at_owners): a collective - every rank calls it with its own
            users (any number, also none), their truth CSR (and optionally their exclusion CSR) and the same `items`, and gets the
            single-device integers of ITS truth entries.  Every owner projects, scores and counts only the items whose rows it holds;
            user rows, the positives' probabilities and the integer bins travel."""
            if dump_probs:
                raise NotImplementedError("catalog_ranks(dump_probs=True) on the row-sharded engine is not supported: no rank forms the "
                                          "probabilities of another owner's items; score with a single-device engine")
            cfg, hidden = self.cfg, tuple(self.cfg.hidden)
            users, items, tower, fetch, queries_of, candidates_of = self._owner_catalog(users, items)
            return ranks_at_owners(
                self.ctx, users, items, self.num_item_rows, truth, exclude, fetch, queries_of, candidates_of,
                count=lambda q, c, so, si, lo, srt, pc, b, t: ops.neumf_rank_count(q, c, tower, cfg.dim, hidden, cfg.act, so, si, lo, srt, pc, b, t),
                positives=lambda q, c, po, pi, out: ops.neumf_auc_positives(q, c, tower, cfg.dim, hidden, cfg.act, po, pi, out=out))

        def _embed_backward_apply(self, users, items, B):
            cfg, D = self.cfg, self.cfg.dim
            if self.exchange == "padded":
                # per-id sums of the row gradients [mlp half of dx0 | ddot * the partner's stashed MF row] into the send slots
                x = self.px
                uo, io = (D, 0) if cfg.item_first else (0, D)
                dx0 = self.dx0[:B]
                og = x.send_row_grads(dx0[:, uo:], self.g_item[:B, D:], dx0[:, io:], self.g_user[:B, D:], 2 * D, self.ddot[:B], D)      # + all-to-all #3
                torch.cuda.current_stream(self.device).wait_event(self._ev_index)
                # x.served still holds the rows this rank served for these very slots = its rows replayed to step t-1; the indexes carry
                # physical slot numbers, so both tables read the one received buffer
                self._adam_tables({"user": (og, 2 * D, None, 0), "item": (og, 2 * D, None, 0)},
                                  replayed={"user": x.served, "item": x.served} if self.deferred else None)
                return
            gu, gi = self.g_user[:B], self.g_item[:B]
            # fused per-pair row gradients [mlp | mf] (the MLP halves are copied out of dx0 here)
            ops.neumf_embed_backward(self.r_user[:, D:], self.r_item[:, D:], self.pos_u, self.pos_i, cfg.item_first,
                                     self.dx0[:B], self.ddot[:B], gu[:, D:], gi[:, D:], gu[:, :D], gi[:, :D])
            xu, xi = self.xu, self.xi
            # batch order -> bucket order, then all-to-all #3 to the owners
            bu = ops.gather_rows([gu], [xu.order.to(self.id_dtype)])[0]
            bi = ops.gather_rows([gi], [xi.order.to(self.id_dtype)])[0]
            ou, oi = xu.send_row_grads(bu), xi.send_row_grads(bi)
            self._grow_index(max(xu.n_recv, xi.n_recv))
            self.user_index.build(xu.recv_local, self.local_rows("user_mf"))
            self.item_index.build(xi.recv_local, self.local_rows("item_mf"))
            rep = getattr(self, "_served", None) if self.deferred else None
            if rep is not None and (rep["user"].shape[0] != xu.n_recv or rep["item"].shape[0] != xi.n_recv or not xu.n_recv or not xi.n_recv):
                rep = None
            self._adam_tables({"user": (ou, 2 * D, None, 0), "item": (oi, 2 * D, None, 0)}, replayed=rep)
            self._served = None

    return ShardedNeuMFEngine


def make_sharded_two_tower(base_cls):
    """ShardedTwoTowerEngine = trainers/twoTower.py on W GPUs (BASELINE config 4): embedding tables
    row-sharded (owner = id mod W, all-to-all ids / rows / row grads as for NeuMF), towers replicated
    (dense gradients all-reduced), and GLOBAL in-batch negatives: every rank scores its B queries against
    the all-gathered W*B candidates (streaming LSE, never materialised), and its B candidates against
    the all-gathered queries for dC — no reduce-scatter needed."""
    from . import ops

    class ShardedTwoTowerEngine(base_cls):
        def __init__(self, embed_dim, nbr_item, nbr_user, semb, device, max_batch, ctx: DistCtx, full_tables=None, **kw):
            self.ctx, self._full_tables = ctx, full_tables
            self.user_rows_global, self.item_rows_global = nbr_user + 2, nbr_item + 2
            super().__init__(embed_dim, nbr_item, nbr_user, semb, device, max_batch, **kw)     # tables and slots: this rank's shard only
            self.dist = ctx
            self._full_tables = None
            self.xu, self.xi = ShardExchange(ctx), ShardExchange(ctx)
            cap = int(2.5 * self.max_batch) + 64
            self.user_index, self.item_index = ops.RowIndex(cap, self.id_dtype, self.device), ops.RowIndex(cap, self.id_dtype, self.device)
            self._idx_cap = cap

        def _init_tables(self, user_rows, item_rows, g):
            """only the rows this rank owns (r mod W == rank): a slice of `full_tables` (tests), else drawn with a rank-offset
            seed - peak memory per GPU is the shard, not the replicated model"""
            r, W = self.ctx.rank, self.ctx.world
            gl = torch.Generator(device="cpu").manual_seed(int(g.initial_seed()) + 104729 * (r + 1))
            for name, rows in (("user_emb", user_rows), ("item_emb", item_rows)):
                if self._full_tables is not None:
                    shard = self._full_tables[name][r::W].contiguous().to(self.device)
                else:
                    shard = (torch.rand(shard_rows(rows, r, W), self.E, generator=gl) * 0.1 - 0.05).to(self.device)
                setattr(self, name, shard if shard.shape[0] else torch.zeros(1, self.E, device=self.device))

        SHARDED_KEYS = ("user_emb", "item_emb", "user_acc", "item_acc", "user_v", "item_v")

        def _start_indexes(self, users, items):
            pass                                    # the owners index the ids they receive (_apply_tables)

        def save_sharded(self, path):
            save_sharded(self, path, self.ctx, [k for k in self.SHARDED_KEYS if k in self.state_dict()])

        def load_sharded(self, path):
            rows = {k: (self.user_rows_global if k.startswith("user") else self.item_rows_global) for k in self.SHARDED_KEYS}
            load_sharded(self, path, self.ctx.rank, self.ctx.world, rows)

        def _lookup(self, users, items, B):
            xu, xi = ShardExchange.plan_pair(self.xu, users, self.xi, items)
            xu.exchange_counts(xi)
            ru, ri = xu.send_ids(), xi.send_ids()
            E = self.E
            empty = torch.empty(0, E, device=self.device)
            gu = ops.gather_rows([self.user_emb], [ru], err_flag=self.err)[0] if ru.numel() else empty
            gi = ops.gather_rows([self.item_emb], [ri], err_flag=self.err)[0] if ri.numel() else empty
            bu, bi = xu.return_rows(gu), xi.return_rows(gi)                      # bucket order
            ops.gather_rows([bu, bi], [xu.inv.to(self.id_dtype), xi.inv.to(self.id_dtype)], [self.eu[:B], self.ei[:B]])

        def _tower(self, rows, tower):
            out = torch.empty(rows.shape[0], self.S, device=self.device)
            Wt, bt = self.W(tower)
            ops.dense_forward(rows, Wt, bt, out, "linear")
            return out

        def recommend(self, users, k, items=None, exclude=None):
            """TwoTowerEngine.recommend on the row-sharded tables (recommend_at_owners): a collective - every rank calls it with its own
            users (any number, also none), the same `items` (None: every row of the item table) and k, and gets the single-device
            lists of ITS users bit for bit.  Every owner applies the item tower to the candidates whose rows it holds only."""
            users = users.contiguous()
            if items is not None:
                items = (items if items.dtype == users.dtype else items.to(users.dtype)).contiguous()
            return recommend_at_owners(
                self.ctx, users, items, self.item_rows_global, k, exclude,
                lambda ids: gather_global_rows(self.ctx, ids, lambda loc: ops.gather_rows([self.user_emb], [loc], err_flag=self.err)[0], self.E),
                lambda rows: self._tower(rows, "user"),
                lambda loc: self._tower(ops.gather_rows([self.item_emb], [loc], err_flag=self.err)[0], "item"),
                lambda q, c, kk, ex: ops.dot_catalog_topk(q, c, kk, exclude=ex))

        def catalog_ranks(self, users, truth, items=None, exclude=None):
            """TwoTowerEngine.catalog_ranks on the row-sharded tables (ranks_at_owners): a collective - every rank calls it with its own
            users (any number, also none), their truth CSR (and optionally their exclusion CSR) and the same `items` (None: every row
            of the item table), and gets the single-device integers of ITS truth entries.  Every owner applies the item tower to the
            candidates whose rows it holds only, as recommend does, and counts them there (ops.dot_rank_count)."""
            users = users.contiguous()
            if items is not None:
                items = (items if items.dtype == users.dtype else items.to(users.dtype)).contiguous()
            return ranks_at_owners(
                self.ctx, users, items, self.item_rows_global, truth, exclude,
                lambda ids: gather_global_rows(self.ctx, ids, lambda loc: ops.gather_rows([self.user_emb], [loc], err_flag=self.err)[0], self.E),
                lambda rows: self._tower(rows, "user"),
                lambda loc: self._tower(ops.gather_rows([self.item_emb], [loc], err_flag=self.err)[0], "item"),
                count=lambda q, c, so, si, lo, srt, pc, b, t: ops.dot_rank_count(q, c, so, si, lo, srt, pc, b, t),
                positives=lambda q, c, po, pi, out: ops.dot_auc_owner_positives(q, c, po, pi, out=out))

        def rank_metrics(self, users, truth, ks=(10,), items=None, exclude=None):
            """TwoTowerEngine.rank_metrics as a collective, from the ranks of catalog_ranks: every rank gets the floats of ITS users."""
            above, tied = self.catalog_ranks(users, truth, items=items, exclude=exclude)
            return ops.rank_metrics(above, tied, truth[0], ks)

        def _softmax(self, q, c, items, B, dq, dc):
            ctx = self.ctx
            off = ctx.rank * B
            c_all, ids_all = ctx.all_gather_rows(c.contiguous()), ctx.all_gather_rows(items.contiguous())
            q = self._scaled_q(q, B)
            # log-Q: the table is replicated (item rows x 4 bytes), so b of ALL candidates is a local gather from the gathered ids - no collective
            b_all = None
            if self.cand_log_q is not None:
                if getattr(self, "_logq_all", None) is None or self._logq_all.numel() < ids_all.shape[0]:
                    self._logq_all = torch.empty(max(ids_all.shape[0], ctx.world * self.max_batch), dtype=torch.float32, device=self.device)
                b_all = self._logq(ids_all, self._logq_all[:ids_all.shape[0]])
            thr = self._hard_thr(q, c_all, items, ids_all, off, B, logq=b_all)       # my queries against ALL candidates: the stripe sweep
            if dq is None:
                ops.inbatch_softmax_lse(q, c_all, items, ids_all, off, self.lse[:B], self.loss_slots, thr=thr, logq=b_all)
                return
            ops.inbatch_softmax_lse_grad_q(q, c_all, items, ids_all, off, self.lse[:B], self.loss_slots, dq, thr=thr, logq=b_all)     # lse + loss + dQ in one sweep
            q_all, lse_all = ctx.all_gather_rows(q.contiguous()), ctx.all_gather_rows(self.lse[:B].contiguous())
            # the thresholds of ALL queries: their columns count over c_all, of which my candidates are rows [off, off + B) - and the dC sweep
            # runs on the arithmetic of the stripe sweep that formed them (chosen from c_all's row count, not from B)
            thr_all = None if thr is None else (ctx.all_gather_rows(thr[0].contiguous()), ctx.all_gather_rows(thr[1].contiguous()))
            # dC of MY candidates against ALL queries: query g's positive is my candidate g - rank*B.  (log-Q: the slice form also without
            # thresholds - the arithmetic of a log-Q call follows the whole candidate count)
            ops.inbatch_softmax_grad(q_all, c.contiguous(), ids_all, items, -off, lse_all, None, dc, thr=thr_all,
                                     thr_slice=None if (thr is None and b_all is None) else (off, c_all.shape[0]),
                                     logq=None if b_all is None else b_all[off:off + B])
            self._unscale_dq(dq)

        def _apply_tables(self, users, items, B):
            xu, xi = self.xu, self.xi
            bu = ops.gather_rows([self.deu[:B]], [xu.order.to(self.id_dtype)])[0]
            bi = ops.gather_rows([self.dei[:B]], [xi.order.to(self.id_dtype)])[0]
            ou, oi = xu.send_row_grads(bu), xi.send_row_grads(bi)
            if max(xu.n_recv, xi.n_recv) > self._idx_cap:
                self._idx_cap = int(1.25 * max(xu.n_recv, xi.n_recv)) + 64
                self.user_index, self.item_index = ops.RowIndex(self._idx_cap, self.id_dtype, self.device), ops.RowIndex(self._idx_cap, self.id_dtype, self.device)
            self.user_index.build(xu.recv_local, self.user_emb.shape[0])
            self.item_index.build(xi.recv_local, self.item_emb.shape[0])
            self._opt_rows(self.user_emb, self.user_acc, getattr(self, "user_v", None), self.user_index, ou)
            self._opt_rows(self.item_emb, self.item_acc, getattr(self, "item_v", None), self.item_index, oi)

    return ShardedTwoTowerEngine


def make_sharded_bpr(base_cls):
    """ShardedBPREngine = src/models/BPRModel.py on W GPUs: the user and the (shared) item table are row-sharded
    (owner = id mod W).  Per step the three id streams travel as two exchanges - users (B ids) and [pos | neg] (2B ids):
    ids -> owners, owner-side gather, rows back; the fused triplet kernel then runs on the received rows (positions as
    ids), and the per-triplet row gradients go back to the owners, which dedup (one sort per table over the
    contributions of all ranks) and apply Adam.  The loss is the mean over the GLOBAL batch (batch_total)."""
    from . import ops

    class ShardedBPREngine(base_cls):
        def __init__(self, num_users, num_items, num_factor, device, max_batch, ctx: DistCtx, full_tables=None, **kw):
            self.ctx, self._full_tables = ctx, full_tables
            self.num_users_global, self.num_items_global = int(num_users), int(num_items)
            super().__init__(num_users, num_items, num_factor, device, max_batch, **kw)      # tables, slots, marks: this rank's shard only
            self._full_tables = None
            self.xu, self.xi = ShardExchange(ctx), ShardExchange(ctx)
            B = self.max_batch
            self._idx_cap = int(5 * B) + 64
            self.user_index, self.item_index = ops.RowIndex(self._idx_cap, self.id_dtype, self.device), ops.RowIndex(self._idx_cap, self.id_dtype, self.device)
            self.pos_b = torch.arange(2 * B, device=self.device).to(self.id_dtype)

        def _init_tables(self, num_users, num_items, init_seed):
            """only the rows this rank owns: a slice of `full_tables` (tests), else drawn with a rank-offset seed"""
            r, W = self.ctx.rank, self.ctx.world
            g = torch.Generator(device="cpu").manual_seed(init_seed + 104729 * (r + 1))
            for name, rows in (("user", num_users), ("item", num_items)):
                if self._full_tables is not None:
                    shard = self._full_tables[name][r::W].contiguous().to(self.device)
                else:
                    shard = (torch.rand(shard_rows(rows, r, W), self.dim, generator=g) * 0.1 - 0.05).to(self.device)
                setattr(self, name, shard if shard.shape[0] else torch.zeros(1, self.dim, device=self.device))

        def train_step(self, users, pos, neg, batch_total: int | None = None):
            B = users.shape[0]
            if B > self.max_batch:
                raise ValueError("batch exceeds max_batch")
            ctx, D = self.ctx, self.dim
            self.begin_steps(1)
            if self.deferred:
                self._advance_step_state()                           # device step counter / alpha ring (the owner-side replay reads them)
            self.t += 1
            bt = B * ctx.world if batch_total is None else batch_total
            ids2 = self.item_ids[:2 * B]
            ids2[:B].copy_(pos)
            ids2[B:].copy_(neg)
            xu, xi = self.xu.plan(users), self.xi.plan(ids2)
            xu.exchange_counts(xi)                                   # the step's one host sync
            ru, ri = xu.send_ids(), xi.send_ids()
            empty = torch.empty(0, D, device=self.device)
            gu = self.rows_as_of_previous_step("user", ru) if ru.numel() else empty       # owner side of the lookup
            gi = self.rows_as_of_previous_step("item", ri) if ri.numel() else empty
            bu, bi = xu.return_rows(gu), xi.return_rows(gi)          # bucket order
            if B == 0:
                eu, ei = empty, empty
            else:
                eu = ops.gather_rows([bu], [xu.inv.to(self.id_dtype)])[0]            # batch order (B x D)
                ei = ops.gather_rows([bi], [xi.inv.to(self.id_dtype)])[0]            # [pos rows | neg rows] (2B x D)
                ar = self.pos_b[:B]
                ops.bpr_forward_backward(eu, ei, ar, ar, ar + B, 1.0 / bt, self.loss_slots, self.g_user[:B], self.g_item[:2 * B],
                                         self.per_triplet[:B], self.err)
            # row gradients: batch order -> bucket order -> owners
            gub = ops.gather_rows([self.g_user[:B]], [xu.order.to(self.id_dtype)])[0] if B else empty
            gib = ops.gather_rows([self.g_item[:2 * B]], [xi.order.to(self.id_dtype)])[0] if B else empty
            ou, oi = xu.send_row_grads(gub), xi.send_row_grads(gib)
            if max(xu.n_recv, xi.n_recv) > self._idx_cap:
                self._idx_cap = int(1.25 * max(xu.n_recv, xi.n_recv)) + 64
                self.user_index, self.item_index = ops.RowIndex(self._idx_cap, self.id_dtype, self.device), ops.RowIndex(self._idx_cap, self.id_dtype, self.device)
            for name, idx, ex, og, served in (("user", self.user_index, xu, ou, gu), ("item", self.item_index, xi, oi, gi)):
                if ex.n_recv:
                    idx.build(ex.recv_local, getattr(self, "_" + name).shape[0])
                    # (the rows this rank served for these positions = its rows replayed to step t-1)
                    self._adam_rows(name, idx, og, D, replayed=served if served.shape[0] == ex.n_recv else None)
                self._adam_sweep(name)
            self.n_seen += B

        def _sampler_tables(self):
            """sample_negatives with candidates == 1 reads no table and works as on one device (with pos0 = the slice's global row
            offset the negatives do not depend on the world size); scoring M > 1 candidates does not"""
            raise NotImplementedError("hard negatives (candidates > 1) on the row-sharded engine: the candidate rows live at their owners "
                                      "(an id-to-owner exchange of B x M rows, or scoring at the owners: DESIGN.md section 7)")

        def _gather_global(self, name, ids):
            """rows `ids` (global ids, any owner) of the row-sharded table `name` -> (len(ids), dim) on this rank."""
            x = ShardExchange(self.ctx).plan(ids)
            x.exchange_counts()
            served = x.send_ids()
            empty = torch.empty(0, self.dim, device=self.device)
            rows = ops.gather_rows([getattr(self, name)], [served], err_flag=self.err)[0] if served.numel() else empty
            back = x.return_rows(rows)                                               # bucket order
            return ops.gather_rows([back], [x.inv.to(self.id_dtype)])[0] if ids.numel() else empty

        def predict_scores(self, user_ids, item_ids=None):
            """bpr_predict (src/models/bpr.py:122-133) on row-sharded tables: the user vectors (and the item rows, all of them when
            item_ids is None) come through the same id -> owner exchange as the training step; every rank must call this (it is a
            collective) and gets the scores of ITS user_ids."""
            u = self._gather_global("user", user_ids)
            if item_ids is None:
                item_ids = torch.arange(self.num_items_global, device=self.device).to(self.id_dtype)
            it = self._gather_global("item", item_ids)
            return ops.score_matrix(u, it)

        def _catalog_rows(self, users, items):
            """The rows BPREngine.recommend / full_auc score, on row-sharded tables: the user rows (and the candidate rows, every item
            when items is None) come through the id -> owner exchange of predict_scores, then the fused launch runs locally.  So both
            are collectives here: every rank calls them and gets the lists / AUCs of ITS users.  (No flush() of its own: _gather_global
            reads the tables through the flushing properties when this rank serves rows.)"""
            users, items = self._recommend_ids(users, items)
            u = self._gather_global("user", users.to(self.id_dtype))
            if items is None:
                items = torch.arange(self.num_items_global, device=self.device)
            it = self._gather_global("item", items.to(self.id_dtype))
            return u, it

        def recommend(self, users, k, items=None, exclude=None, dump_scores=False, catalog="gather"):
            """BPREngine.recommend as a collective.  catalog="gather" (default): every candidate row is pulled to every rank
            (_catalog_rows) and each rank scores its users alone; "owners": every rank scores the users of ALL ranks against the
            candidates whose rows it holds and the k-entry lists are merged (recommend_at_owners) - the same lists bit for bit, with
            U x dim user rows and U x W x k list entries on the wire instead of I x dim candidate rows per rank."""
            if catalog not in ("gather", "owners"):
                raise ValueError(f"catalog must be 'gather' or 'owners', got {catalog!r}")
            if catalog == "gather":
                return super().recommend(users, k, items=items, exclude=exclude, dump_scores=dump_scores)
            if dump_scores:
                raise NotImplementedError("recommend(catalog='owners', dump_scores=True): no rank forms the scores of another owner's items")
            users, items = self._recommend_ids(users, items)
            self.flush()                         # deferred-Adam rows lag until then
            rows_of = lambda name: (lambda loc: ops.gather_rows([getattr(self, "_" + name)], [loc], err_flag=self.err)[0])
            return recommend_at_owners(self.ctx, users, items, self.num_items_global, k, exclude,
                                       lambda ids: gather_global_rows(self.ctx, ids, rows_of("user"), self.dim),
                                       lambda rows: rows, rows_of("item"),
                                       lambda q, c, kk, ex: ops.dot_topk_for(self.dim)(q, c, kk, exclude=ex))

        def full_auc(self, users, truth, items=None, dump_scores=False, catalog="gather"):
            """BPREngine.full_auc as a collective.  catalog="gather" (default): every candidate row is pulled to every rank
            (_catalog_rows) and each rank evaluates its users alone; "owners": every rank counts the users of ALL ranks against the
            candidates whose rows it holds and the integer partial counts are summed (auc_at_owners) - the same floats bit for bit, with
            U x dim user rows, the truth lists and their scores and U partials on the wire instead of I x dim candidate rows per rank."""
            if catalog not in ("gather", "owners"):
                raise ValueError(f"catalog must be 'gather' or 'owners', got {catalog!r}")
            if catalog == "gather":
                return super().full_auc(users, truth, items=items, dump_scores=dump_scores)
            if dump_scores:
                raise NotImplementedError("full_auc(catalog='owners', dump_scores=True): no rank forms the scores of another owner's items")
            users, items = self._recommend_ids(users, items)
            self.flush()                         # deferred-Adam rows lag until then
            rows_of = lambda name: (lambda loc: ops.gather_rows([getattr(self, "_" + name)], [loc], err_flag=self.err)[0])
            return auc_at_owners(self.ctx, users, items, self.num_items_global, truth,
                                 lambda ids: gather_global_rows(self.ctx, ids, rows_of("user"), self.dim),
                                 lambda rows: rows, rows_of("item"), self.dim)

        def catalog_ranks(self, users, truth, items=None, exclude=None, dump_scores=False, catalog="gather"):
            """BPREngine.catalog_ranks as a collective.  catalog="gather" (default): every candidate row is pulled to every rank
            (_catalog_rows) and each rank ranks its users alone; "owners": every rank counts the users of ALL ranks against the
            candidates whose rows it holds and the integer bins are summed (ranks_at_owners; the count: ops.dot_rank_count, the whole-row
            kernels up to 128 features and the block kernels above, as everywhere) - the same integers entry for entry, with U x dim
            user rows, the truth and exclusion lists, the positives' scores and two int32 bins per truth entry and user on the wire
            instead of I x dim candidate rows per rank."""
            if catalog not in ("gather", "owners"):
                raise ValueError(f"catalog must be 'gather' or 'owners', got {catalog!r}")
            if catalog == "gather":
                return super().catalog_ranks(users, truth, items=items, exclude=exclude, dump_scores=dump_scores)
            if dump_scores:
                raise NotImplementedError("catalog_ranks(catalog='owners', dump_scores=True): no rank forms the scores of another owner's items")
            users, items = self._recommend_ids(users, items)
            self.flush()                         # deferred-Adam rows lag until then
            rows_of = lambda name: (lambda loc: ops.gather_rows([getattr(self, "_" + name)], [loc], err_flag=self.err)[0])
            return ranks_at_owners(self.ctx, users, items, self.num_items_global, truth, exclude,
                                   lambda ids: gather_global_rows(self.ctx, ids, rows_of("user"), self.dim),
                                   lambda rows: rows, rows_of("item"),
                                   count=lambda q, c, so, si, lo, srt, pc, b, t: ops.dot_rank_count(q, c, so, si, lo, srt, pc, b, t),
                                   positives=lambda q, c, po, pi, out: ops.dot_auc_owner_positives(q, c, po, pi, out=out))

        def rank_metrics(self, users, truth, ks=(10,), items=None, exclude=None, catalog="gather"):
            """BPREngine.rank_metrics as a collective, from the ranks of catalog_ranks(catalog=...): the same floats either way."""
            above, tied = self.catalog_ranks(users, truth, items=items, exclude=exclude, catalog=catalog)
            return ops.rank_metrics(above, tied, truth[0], ks)

        SHARDED_KEYS = ("user", "item", "user_m", "user_v", "item_m", "item_v")

        def save_sharded(self, path):
            save_sharded(self, path, self.ctx, self.SHARDED_KEYS)

        def load_sharded(self, path):
            rows = {k: (self.num_users_global if k.startswith("user") else self.num_items_global) for k in self.SHARDED_KEYS}
            load_sharded(self, path, self.ctx.rank, self.ctx.world, rows)

    return ShardedBPREngine
