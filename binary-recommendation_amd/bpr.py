"""BPR pairwise model on the HIP hot path — src/models/BPRModel.py:49-74,124-144 and the
stand-alone src/models/bpr.py:141-201.

Graph: shared item embedding (positive + negative lookups), user embedding, Lambda triplet loss
`1 - sigmoid(u.p - u.n)` (NOT -log sigmoid: BPRModel.py:144), identityLoss = mean (BPRModel.py:124-126),
Adam(1e-3) (BPRModel.py:70).  One fused launch does the 3 gathers, 2 dots, the loss partials and the
3 per-triplet row gradients; the shared item table receives its two IndexedSlices concatenated
[pos rows | neg rows] and deduplicated by one sort over the 2B ids.
"""
from __future__ import annotations

import os

import torch

from . import _lib, ops
from .row_adam import RowAdam
from .sampler import CandidatePool


class NegativeSampler(CandidatePool):
    """What the per-step negative sampler (BPREngine.sample_negatives, csrc/sampling_step.hip) needs of a training set: the positives'
    CSR (ops.positives_csr), the candidate item ids (None: 0..n_items-1 with n_items = the largest positive item + 1) and, mode
    "popularity", Walker's alias table of count(item)^power over the given positives, restricted to the candidates (sampler.py).
    candidates = M > 1: dynamic negative sampling - every step draws M candidates per triplet and trains on the one the current model
    scores highest."""

    def __init__(self, users, items, n_users: int, cand_items=None, mode: str = "uniform", candidates: int = 1, power: float = 0.75, seed: int = 0,
                 max_tries: int = 16, device="cuda", n_items: int | None = None):
        if mode not in ("uniform", "popularity"):
            raise ValueError("mode must be 'uniform' or 'popularity'")
        if not 1 <= int(candidates) <= 32:
            raise ValueError("candidates must be in [1, 32]")
        self.candidates = int(candidates)
        super().__init__(users, items, n_users, cand_items=cand_items, mode=mode, power=power, seed=seed, max_tries=max_tries, device=device, n_items=n_items)


class BPREngine(RowAdam):
    """optimizer "adam_dense" = Keras' non-lazy sparse Adam (every row of both tables moves every step [TF-sem]); dense_impl
    "deferred" (default) reaches the untouched rows by per-row replay (include/binrec.h "Deferred dense Adam": the lookup replays a
    row's missing g = 0 steps in registers, the optimizer launch applies them, flush() brings every row to the current step before
    anything else reads the tables) instead of sweeping 6 x 4 B per table element per step ("sweep"); bit-equal tables."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-7

    def __init__(self, num_users: int, num_items: int, num_factor: int, device, max_batch: int, lr: float = 1e-3,
                 optimizer: str = "adam_dense", id_dtype=torch.int32, init_seed: int = 0, dense_impl: str = "deferred", replay: str | None = None):
        assert optimizer in ("adam_dense", "adam_lazy") and dense_impl in ("deferred", "sweep")
        self.replay = os.environ.get("BR_REPLAY", "fast") if replay is None else replay      # NeuMFConfig.replay: form of the deferred replay
        assert self.replay in ("fast", "exact")
        self.device, self.max_batch, self.lr, self.optimizer, self.id_dtype = torch.device(device), int(max_batch), lr, optimizer, id_dtype
        self.dim = int(num_factor)
        dev = self.device
        self._init_tables(num_users, num_items, init_seed)
        self.user_m, self.user_v = torch.zeros_like(self._user), torch.zeros_like(self._user)
        self.item_m, self.item_v = torch.zeros_like(self._item), torch.zeros_like(self._item)
        B = self.max_batch
        self.g_user = torch.empty(B, self.dim, device=dev)
        self.g_item = torch.empty(2 * B, self.dim, device=dev)
        self.per_triplet = torch.empty(B, device=dev)
        self.loss_slots = torch.zeros(ops.SUM_SLOTS, dtype=torch.float64, device=dev)
        self.item_ids = torch.empty(2 * B, dtype=id_dtype, device=dev)
        self.user_index = ops.RowIndex(B, id_dtype, dev)
        self.item_index = ops.RowIndex(2 * B, id_dtype, dev)
        self._side_index = ops.SideIndexes(dev)
        self.err = ops.new_err_flag(dev)
        self._init_row_adam({"user": (self._user, self.user_m, self.user_v), "item": (self._item, self.item_m, self.item_v)}, optimizer,
                            dense_impl, lr, self.BETA1, self.BETA2, self.EPS, self.replay)
        if self.deferred:
            self.r_user = torch.empty(B, self.dim, device=dev)            # rows as of the previous step (replayed in registers)
            self.r_item = torch.empty(2 * B, self.dim, device=dev)
            self.pos_b = torch.arange(2 * B, device=dev).to(id_dtype)
        self.n_seen = 0

    # the tables as a caller sees them: flushed (deferred mode) before they are handed out
    @property
    def user(self):
        self.flush()
        return self._user

    @user.setter
    def user(self, t):
        self._user = t

    @property
    def item(self):
        self.flush()
        return self._item

    @item.setter
    def item(self, t):
        self._item = t

    def _init_tables(self, num_users, num_items, init_seed):
        """[TF-sem] Keras Embedding init U(-0.05, 0.05).  (A hook: the row-sharded engine allocates only its shard.)"""
        g = torch.Generator(device="cpu").manual_seed(init_seed)
        self._user = (torch.rand(num_users, self.dim, generator=g) * 0.1 - 0.05).to(self.device)
        self._item = (torch.rand(num_items, self.dim, generator=g) * 0.1 - 0.05).to(self.device)

    def train_step(self, users, pos, neg, batch_total: int | None = None):
        """fit step (BPRModel.py:109): users/pos/neg device ids (B,). No host sync."""
        B = users.shape[0]
        if B == 0:
            return
        if B > self.max_batch:
            raise ValueError("batch exceeds max_batch")
        ids2 = self.item_ids[:2 * B]
        for t in (users, pos, neg):
            if t.dtype != self.id_dtype or not t.is_cuda or not t.is_contiguous() or t.shape[0] != B:
                raise TypeError(f"ids must be contiguous {self.id_dtype} device tensors of one length")
        self.begin_steps(1)
        # [pos | neg] side by side (the shared item table gets one index over both): one launch instead of two copies
        _lib.check(_lib.load().brStageBatch(ids2.data_ptr(), ids2[B:].data_ptr(), None, pos.data_ptr(), neg.data_ptr(), None,
                                            ops.I64 if self.id_dtype == torch.int64 else ops.I32, B, ops._stream()), "brStageBatch")
        gr = getattr(self, "_graph", None)
        if gr is not None and B == gr["batch"] and (batch_total is None or batch_total == B):
            gr["users"].copy_(users)
            self.t += 1
            gr["graph"].replay()
            self.n_seen += B
            return
        self.t += 1
        self._step_body(users, ids2, B, B if batch_total is None else batch_total)
        self.n_seen += B

    def enable_graph(self, batch: int | None = None):
        """Replay the step for batches of exactly `batch` triplets as ONE hipGraph (for hosts whose per-launch overhead is the bound:
        at batch 65 536 on MI355X the eager step is GPU-bound at 0.195 ms and the replay, with its two forked index branches, takes
        0.214 ms).  Deferred dense Adam only: then every per-step scalar (step counter, alpha) lives in the device step state.  The
        user ids are copied into a static buffer per step."""
        if not self.deferred:
            raise ValueError("graph replay needs optimizer='adam_dense' with dense_impl='deferred' (per-step scalars on the device)")
        B = self.max_batch if batch is None else int(batch)
        if not 0 < B <= self.max_batch:
            raise ValueError("graph batch must be in (0, max_batch]")
        users = torch.zeros(B, dtype=self.id_dtype, device=self.device)
        ids2 = self.item_ids[:2 * B]
        ids2.zero_()
        # every kernel runs once outside a capture first (code objects load on first launch); the model state is put back afterwards.
        # The dry run's ids are all 0: it moves row 0 of each table and nothing else (deferred tables) - that row, with its moments and
        # `last`, is what is kept.  NOT state_dict(): that flushes, and a flush in the middle of a run resets every row's lag (and, with the
        # fast replay, is no longer bit-neutral: one catch-up over (s, t] and two over (s, u], (u, t] round differently).
        z = torch.zeros(1, dtype=torch.long, device=self.device)
        keep = self._snapshot_rows({"user": z, "item": z})
        keep_loss = self.loss_slots.clone()

        def restore():
            self._restore_rows(keep)
            self.loss_slots.copy_(keep_loss)
            self._set_step_state()
        self._step_body(users, ids2, B, B)
        torch.cuda.synchronize(self.device)
        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_body(users, ids2, B, B)
        restore()                               # (the capture executes nothing; this re-syncs the device step counter after the dry run)
        self._graph = {"batch": B, "users": users, "graph": g}

    def disable_graph(self):
        self._graph = None

    def _step_body(self, users, ids2, B, bt):
        """the step's launches (ids2 = [pos | neg] already in place)"""
        gi = self.g_item[:2 * B]
        U, I = self._user, self._item
        # one-wave-per-row shapes at a batch that fills the chip: the chunk sorts of both id streams ride in the gather's launch, the
        # chunk-rank launch advances the step state - five launches on one stream, no fork (include/binrec.h brGatherRowsDeferredPairWithIndex)
        fused = self.deferred and self.dim in (64, 128, 256) and B >= 1024 and 2 * B <= 524288 and max(U.shape[0], I.shape[0]) < (1 << 31) - 2 \
            and os.environ.get("BR_FUSED_SORT", "1") != "0"
        if fused:
            hp = (self.BETA1, self.BETA2, self.EPS)
            ru, ri = ops.gather_rows_deferred_pair_with_index(U, self.user_m, self.user_v, self.last["user"], users, self.r_user[:B], self.user_index,
                                                              I, self.item_m, self.item_v, self.last["item"], ids2, self.r_item[:2 * B], self.item_index,
                                                              self.step_state, self.lr, *hp, err_flag=self.err)
            ar = self.pos_b[:B]
            ops.bpr_forward_backward(ru, ri, ar, ar, self.pos_b[B:2 * B], 1.0 / bt, self.loss_slots, self.g_user[:B], gi, self.per_triplet[:B], self.err)
            ops.adam_rows_sorted_deferred_pair_replayed(U, self.user_m, self.user_v, self.last["user"], self.user_index, self.g_user[:B], ru,
                                                        I, self.item_m, self.item_v, self.last["item"], self.item_index, gi, ri, 0, self.step_state, *hp)
            return
        if self.deferred:
            self._advance_step_state()
        # the two dedup indexes depend only on the ids: each on a side stream of its own (their sort kernels fill 8 and 16 CUs), beside
        # the lookups and the triplet kernel; joined before the optimizer launches.  (On the launch stream they were 92 of the step's 248 us.)
        main = torch.cuda.current_stream(self.device)
        self._side_index.start(main, ((self.user_index, users, U.shape[0]), (self.item_index, ids2, I.shape[0])))
        ru = ri = None
        if self.deferred:
            hp = (self.BETA1, self.BETA2, self.EPS)
            pair = self.dim in (64, 128, 256)       # one-wave-per-row shapes: both tables served / updated by one launch each
            if pair:
                ru, ri = ops.gather_rows_deferred_pair(U, self.user_m, self.user_v, self.last["user"], users, self.r_user[:B],
                                                       I, self.item_m, self.item_v, self.last["item"], ids2, self.r_item[:2 * B], self.step_state, *hp, err_flag=self.err)
            else:
                ru = self.rows_as_of_previous_step("user", users, out=self.r_user[:B])
                ri = self.rows_as_of_previous_step("item", ids2, out=self.r_item[:2 * B])
            ar = self.pos_b[:B]
            ops.bpr_forward_backward(ru, ri, ar, ar, self.pos_b[B:2 * B], 1.0 / bt, self.loss_slots, self.g_user[:B], gi, self.per_triplet[:B], self.err)
            self._side_index.join(main)
            # the gathered rows ARE the tables' rows replayed to step t-1: the optimizer takes theta from them and replays m, v only
            if pair:
                ops.adam_rows_sorted_deferred_pair_replayed(U, self.user_m, self.user_v, self.last["user"], self.user_index, self.g_user[:B], ru,
                                                            I, self.item_m, self.item_v, self.last["item"], self.item_index, gi, ri, 0, self.step_state, *hp)
                return
        else:
            ops.bpr_forward_backward(U, I, users, ids2[:B], ids2[B:], 1.0 / bt, self.loss_slots, self.g_user[:B], gi, self.per_triplet[:B], self.err)
            self._side_index.join(main)
        self._adam_rows("user", self.user_index, self.g_user[:B], self.dim, replayed=ru)
        self._adam_rows("item", self.item_index, gi, self.dim, replayed=ri)
        self._adam_sweep("user")
        self._adam_sweep("item")

    def sample_negatives(self, users, pos, sampler: NegativeSampler, pos0: int = 0, out=None, dump: bool = False):
        """The negatives of the NEXT train_step's batch (users, pos), drawn now: negative b is a pure function of (sampler.seed, the
        completed steps self.t, pos0 + b) and - sampler.candidates > 1 - the hardest of the candidates under the tables as of the last
        completed step (deferred rows are replayed in registers, nothing is written).  One launch beside the step (outside a captured
        graph), no host sync.  -> neg (B,), with dump=True also (cands (B, M), scores (B, M)).  `pos` is not read: the positives a
        negative must avoid are the sampler's CSR."""
        M = sampler.candidates
        user = item = None
        if M > 1:
            user, item = self._sampler_tables()
        return ops.bpr_sample_negatives(users, sampler.pos_off, sampler.pos_items, sampler.n_cand, sampler.seed, self.t, pos0=pos0, cand_items=sampler.cand_items,
                                        alias=sampler.alias, candidates=M, max_tries=sampler.max_tries, user=user, item=item,
                                        step_state=self.step_state if self.deferred else None, beta1=self.BETA1, beta2=self.BETA2, eps=self.EPS,
                                        out=out, dump=dump, err_flag=self.err)

    def _sampler_tables(self):
        """the tables as sample_negatives scores against them (row-sharded engines refuse: parallel.py)"""
        if self.deferred:
            return (self._user, self.user_m, self.user_v, self.last["user"]), (self._item, self.item_m, self.item_v, self.last["item"])
        return (self._user,), (self._item,)

    def pop_loss(self) -> float:
        """Host sync: mean triplet loss since the last call."""
        s = float(self.loss_slots.sum().item())
        n = max(1, self.n_seen)
        self.loss_slots.zero_()
        self.n_seen = 0
        return s / n

    def predict_scores(self, user_ids, item_ids=None):
        """bpr_predict (src/models/bpr.py:122-133): user vectors x item matrix^T."""
        u = ops.gather_rows([self.user], [user_ids])[0]
        it = self.item if item_ids is None else ops.gather_rows([self.item], [item_ids])[0]
        return ops.score_matrix(u, it)

    def recommend(self, users, k, items=None, exclude=None, dump_scores=False):
        """The k best items of every user of `users` by the dot score predict_scores returns, without the U x I matrix: one fused
        launch scores, masks and selects (ops.dot_catalog_topk, csrc/recommend_dot.hip; rows wider than 128 features:
        ops.dot_catalog_topk_wide, csrc/recommend_dot_wide.hip, up to 512).  items: the candidate ids (None: the item
        table in place); exclude: (off, idx) CSR over `users` of candidate POSITIONS never to return (topk_metrics.seen_csr).
        -> (scores (U, k) float32, index (U, k) int32 positions into `items`) on the device, best first, ties to the lower position;
        slots past the remaining candidates are (-inf, -1).  Ids outside the tables set self.err (check_ids raises).  On the row-sharded
        engine (parallel.py) this is a collective: every rank calls it and gets the lists of ITS users."""
        q, c = self._catalog_rows(users, items)
        return ops.dot_topk_for(q.shape[1])(q, c, k, exclude=exclude, dump_scores=dump_scores)

    def full_auc(self, users, truth, items=None, dump_scores=False):
        """Per-user full AUC (src/models/bpr.py:230-254) of the dot scores predict_scores returns, without the U x I matrix: the fused
        launches of ops.dot_catalog_auc (csrc/auc_dot.hip; rows wider than 128 features: ops.dot_catalog_auc_wide).  truth: (off, idx)
        CSR over `users` of candidate POSITIONS, ascending (ops.truth_csr); items: the candidate ids (None: the item table in place).  -> float32 (U,) on the device, NaN for a user
        without positives or without negatives.  Ids outside the tables set self.err (check_ids raises).  On the row-sharded engine
        (parallel.py) this is a collective: every rank calls it and gets the AUCs of ITS users."""
        q, c = self._catalog_rows(users, items)
        return ops.dot_auc_for(q.shape[1])(q, c, truth[0], truth[1], dump_scores=dump_scores)

    def catalog_ranks(self, users, truth, items=None, exclude=None, dump_scores=False):
        """Per truth entry, in the order of the CSR, how many candidates score above it and how many tie with it, over the whole
        catalogue and without the U x I matrix (ops.dot_catalog_ranks, csrc/ranks_dot.hip; rows up to 512 features).  truth / items as
        in full_auc; exclude: (off, idx) CSR over `users` of candidate POSITIONS never offered (topk_metrics.seen_csr): an excluded
        truth entry is still ranked, against the others.  -> (above, tied) int32 on the device, (-1, -1) for a positive whose score is
        NaN.  Ids outside the tables set self.err (check_ids raises).  On the row-sharded engine this is a collective (every rank
        calls it and gets the counts of ITS users), through the gathered rows or counted at the item owners (parallel.py: catalog=)."""
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
        """-> (the rows of `users`, the rows of `items` or the item table in place) that recommend / full_auc score (row-sharded
        engines override this: parallel.py)"""
        self.flush()                         # deferred-Adam rows lag until then
        users, items = self._recommend_ids(users, items)
        q = ops.gather_rows([self._user], [users], err_flag=self.err)[0]
        c = self._item if items is None else ops.gather_rows([self._item], [items], err_flag=self.err)[0]
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

    # tables + Adam slots (model.save / restoreFromLatestCheckPoint, RModel.py:139,172); row-sharded engines hold their shard
    STATE_TABLES = ("user", "item", "user_m", "user_v", "item_m", "item_v")

    def state_dict(self) -> dict:
        self.flush()
        sd = {"t": self.t}
        sd.update({k: getattr(self, k) for k in self.STATE_TABLES})
        return sd

    def load_state_dict(self, sd: dict):
        self.t = int(sd["t"])
        for k in self.STATE_TABLES:
            getattr(self, "_" + k if k in ("user", "item") else k).copy_(sd[k])
        self._reset_lags()
