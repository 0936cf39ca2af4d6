"""-m gpu: exact full-catalogue ranks for NeuMF (csrc/ranks_neumf.hip, csrc/rank_bins.h, NeuMFEngine.catalog_ranks / rank_metrics,
ShardedNeuMFEngine.catalog_ranks, NeuMFModel.rank_metrics).

No tolerance on the integers: (above, tied) equal torch `>` / `==` counts on the call's own dump_probs entry for entry, the dump equals
brNeumfCatalogAuc's bit for bit (one text of the scoring loop), other grids and other splits give the same integers, and W owners over
parts of the candidates give the single launch's.  The metrics are those integers through rank_metrics_numpy (float64), each stored
float32 once: one float32 rounding of a value in [0, 1] is the bound.

Two ranks on one card over gloo (child processes, each under its own time limit, never run again)."""
import importlib.util
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RANK_LDS_CAP = 512      # kNeumfRankLdsCap: a user's sorted positives and its bins sit in LDS up to this many


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


N = _load("test_gpu_neumf_auc")          # _engine / _operands / _built_users / _dev_csr / _same_bits / CASES, and R: the owner maps
D = _load("test_gpu_ranks_dot")          # _count: torch `>` / `==` under the candidate mask
C = _load("test_ranks_dot_cpu")          # rank_metrics_numpy
R = N.R
F32_EPS = float(np.finfo(np.float32).eps)


def _m(name):
    return import_module("binary-recommendation_amd." + name)


def _excl_over(rng, off, idx, I, dev, n=40, skip=()):
    """an exclusion CSR that overlaps the truth: per user n random positions and the user's first three truth entries; the users of
    `skip` exclude nothing"""
    rows = []
    for u in range(len(off) - 1):
        rows.append(np.empty(0, np.int64) if u in skip else np.union1d(rng.choice(I, n, replace=False), idx[off[u]:off[u] + 3]))
    xoff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return N._dev_csr(xoff, np.concatenate(rows).astype(np.int32), dev)


def _same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# --------------------------------------------------------------------------------------------------------------- 1: exact against the dump
# padded widths 8 and 128, 56 (A's default tower) and 16, both variants (A: sigmoid, B: relu - the engine offers no other), both id dtypes
TOWERS = [("A", 10, (24, 8, 4), torch.int32), ("B", 64, (128, 128, 32), torch.int32), ("A", 64, None, torch.int64), ("B", 32, None, torch.int32),
          ("B", 16, (40, 40, 8), torch.int64)]


@pytest.mark.parametrize("variant,dim,hidden,idt", TOWERS)
def test_exact_against_the_dump(dev, variant, dim, hidden, idt):
    ops = _m("ops")
    rng = np.random.default_rng(dim + (0 if hidden is None else hidden[1]))
    I = N.LDS_CAP + 303                                               # not a multiple of 64
    items = rng.permutation(I + 100)[:I]
    spec, p, eng = N._engine(dev, variant, dim, 50, I + 100, seed=dim, id_dtype=idt, hidden=hidden)
    off, idx = N._built_users(rng, I)         # 9 users: none, every candidate, P = 1, P = 70, P past both LDS caps, four random lists
    U = len(off) - 1
    assert U % 4 and I % 64 and np.diff(off).max() > RANK_LDS_CAP and 0 < np.diff(off)[5:].min() < RANK_LDS_CAP
    users = torch.as_tensor(rng.integers(0, 50, U), dtype=idt, device=dev)
    pu, pit, tower, tail = N._operands(eng, users, torch.as_tensor(items, dtype=idt, device=dev))
    toff, tidx = N._dev_csr(off, idx, dev)
    auc_dump = ops.neumf_catalog_auc(pu, pit, tower, *tail, toff, tidx, dump_probs=True)[1]
    for ex in (None, _excl_over(rng, off, idx, I, dev, skip=(3,))):
        above, tied, dump = ops.neumf_catalog_ranks(pu, pit, tower, *tail, toff, tidx, exclude=ex, dump_probs=True)
        eng.check_ids()
        assert above.dtype == tied.dtype == torch.int32 and above.shape == tied.shape == (len(idx),)
        assert N._same_bits(dump, auc_dump)                           # the score is the AUC's: one text
        assert _same((above, tied), D._count(dump, toff, tidx, ex)), (variant, dim, ex is not None)
        assert _same((above, tied), ops.neumf_catalog_ranks(pu, pit, tower, *tail, toff, tidx, exclude=ex))      # without the dump
        assert (above >= 0).all()
    # the engine surface returns the same
    e = eng.catalog_ranks(users, (toff, tidx), items=torch.as_tensor(items, dtype=idt, device=dev), exclude=ex, dump_probs=True)
    assert _same(e[:2], (above, tied)) and N._same_bits(e[2], dump)


# --------------------------------------------------------------------------------------------------------------- 2, 3: ties, non-finite
def test_ties_and_saturation(dev):
    """test_gpu_neumf_auc.test_ties' construction: 700 positions name five rows, and a head saturated to exact 0.0 / 1.0"""
    ops = _m("ops")
    rng = np.random.default_rng(3)
    I, U = 1500, 21
    items = rng.permutation(I)
    items[200:900] = items[np.arange(200, 900) % 5]
    rows = [np.sort(rng.choice(I, int(rng.integers(1, 400)), replace=False)) for _ in range(U)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    toff, tidx = N._dev_csr(off, idx, dev)
    ex = _excl_over(rng, off, idx, I, dev)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    for variant, saturate in (("A", False), ("B", True), ("A", True)):
        spec, p = N._params(variant, 32, 50, I, seed=9)
        if saturate:
            p = dict(p)
            w4 = np.zeros_like(p["W4"])
            w4.reshape(-1)[0 if spec.head_concat[0] == "mf" else -1] = 3000.0
            p["W4"], p["b4"] = w4, np.zeros_like(p["b4"])
        _s, _p, eng = N._engine(dev, variant, 32, 50, I, seed=9, p=p)
        pu, pit, tower, tail = N._operands(eng, users, torch.as_tensor(items, dtype=torch.int32, device=dev))
        for x in (None, ex):
            above, tied, dump = ops.neumf_catalog_ranks(pu, pit, tower, *tail, toff, tidx, exclude=x, dump_probs=True)
            if saturate:
                assert ((dump == 0.0).float().mean() > 0.25) and ((dump == 1.0).float().mean() > 0.25)
            assert (tied > 0).float().mean() > (0.5 if saturate else 0.25), (variant, saturate, float((tied > 0).float().mean()))
            assert _same((above, tied), D._count(dump, toff, tidx, x)), (variant, saturate, x is not None)


def test_non_finite(dev):
    """test_gpu_neumf_auc.test_non_finite_scores' rows: a NaN, a +inf and a -inf in item rows that are positives of some users and
    candidates of the others.  A NaN positive gets (-1, -1); a NaN candidate is never counted"""
    ops = _m("ops")
    rng = np.random.default_rng(4)
    I, U, dim = 700, 24, 32
    for variant in ("A", "B"):
        spec, p, eng = N._engine(dev, variant, dim, 50, I, seed=12)
        eng.fused["item"][10, dim + 3] = float("nan")
        eng.fused["item"][11, dim + 5] = float("inf")
        eng.fused["item"][12, dim] = float("-inf")
        items = rng.permutation(I)
        where = np.empty(I, np.int64); where[items] = np.arange(I)
        rows = []
        for u in range(U):
            base = set(rng.choice(I, 15, replace=False).tolist()) - {int(where[10]), int(where[11]), int(where[12])}
            for bit, i in enumerate((10, 11, 12)):
                if (u >> bit) & 1:
                    base.add(int(where[i]))
            rows.append(np.sort(np.fromiter(base, np.int64)))
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        toff, tidx = N._dev_csr(off, idx, dev)
        users = torch.arange(U, dtype=torch.int32, device=dev)
        pu, pit, tower, tail = N._operands(eng, users, torch.as_tensor(items, dtype=torch.int32, device=dev))
        above, tied, dump = ops.neumf_catalog_ranks(pu, pit, tower, *tail, toff, tidx, dump_probs=True)
        assert torch.isnan(dump[:, int(where[10])]).all()
        nan_pos = tidx == int(where[10])
        assert int(nan_pos.sum()) == U // 2
        assert (above[nan_pos] == -1).all() and (tied[nan_pos] == -1).all()
        ranked = above >= 0                                                # (an infinite row may have met a zero: NaN too)
        assert ranked.float().mean() > 0.8 and torch.equal(ranked, tied >= 0)
        assert _same((above, tied), D._count(dump, toff, tidx)), variant       # torch compares: a NaN candidate is never above, never tied
        # every candidate is above, tied or below the positive, but the NaN ones: they are in none of the three
        rws = torch.from_numpy(np.repeat(np.arange(U), np.diff(off))).to(dev)
        s = dump[rws, tidx.long()]
        below = (dump[rws] < s[:, None]).sum(1)
        n_nan = torch.isnan(dump).sum(1)[rws]
        assert (n_nan[ranked] >= 1).any()
        assert torch.equal((above.long() + tied.long() + below + 1)[ranked], (I - n_nan)[ranked])


# --------------------------------------------------------------------------------------------------------------- 4: plan independence
def test_plan_independence(dev):
    """single users (many item splits, the LDS path and the global-bin path) and a 7-user subset (another grid) give the integers of the
    full call"""
    ops, A = _m("ops"), _load("test_gpu_auc_dot")
    U, I = 600, 20000
    spec, p, eng = N._engine(dev, "A", 64, U, I, seed=5)
    sizes = np.random.default_rng(5).integers(0, 40, U)
    sizes[7] = RANK_LDS_CAP + 300
    off, idx = A._truth(sizes, I, dev, seed=5)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    pu, pit, tower, tail = N._operands(eng, users, torch.arange(I, dtype=torch.int32, device=dev))
    full = ops.neumf_catalog_ranks(pu, pit, tower, *tail, off, idx)
    o, x = off.cpu().numpy(), idx.cpu().numpy()
    assert (full[0] >= 0).all()
    for u in (0, 1, 7, 257, U - 1):
        t = torch.from_numpy(x[o[u]:o[u + 1]]).to(dev)
        one = ops.neumf_catalog_ranks(pu[u:u + 1], pit, tower, *tail, torch.tensor([0, len(t)], dtype=torch.int64, device=dev), t)
        assert _same(one, (full[0][o[u]:o[u + 1]], full[1][o[u]:o[u + 1]])), u
    some = np.array([7, 3, 599, 100, 101, 102, 8])
    so, sx = ops.truth_csr(len(some), np.repeat(np.arange(len(some)), sizes[some]), np.concatenate([x[o[u]:o[u + 1]] for u in some]), dev)
    part = ops.neumf_catalog_ranks(pu[torch.from_numpy(some).to(dev)].contiguous(), pit, tower, *tail, so, sx)
    sel = torch.from_numpy(np.concatenate([np.arange(o[u], o[u + 1]) for u in some])).to(dev)
    assert _same(part, (full[0][sel], full[1][sel]))


# --------------------------------------------------------------------------------------------------------------- 4b: the wave cursor
def test_rows_that_fill_or_straddle_a_window(dev):
    """the one cursor of the three catalogue kernels (neumf_score.h WaveCursor) on rows that are empty, sit at either end, fill the
    64-item window [64, 128), cross a window boundary or name every item, each as the truth row and as the exclusion row; 200 items are
    three full windows and a tail of 8, and the plan gives every window its own split, so all cursors but the first start inside a row"""
    ops = _m("ops")
    I, k = 200, 64
    rows = [np.empty(0, np.int64), np.array([0]), np.array([I - 1]), np.arange(64, 128), np.arange(60, 71), np.arange(I)]
    U = len(rows)
    assert U % 4
    ws = int(ops._lib.load().brNeumfCatalogTopKWorkspaceBytes(U, I, k))       # 2 x (U x splits x k) entries of 4 bytes, a multiple of 256
    assert ws // (2 * U * k * 4) == 4 and ws % (2 * U * k * 4) == 0              # 4 splits
    spec, p, eng = N._engine(dev, "A", 10, 50, I, seed=21)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    pu, pit, tower, tail = N._operands(eng, users, torch.arange(I, dtype=torch.int32, device=dev))

    def csr(shift):
        r = rows[shift:] + rows[:shift]
        return N._dev_csr(np.concatenate([[0], np.cumsum([len(x) for x in r])]), np.concatenate(r), dev)

    toff, tidx = csr(0)
    auc, dump = ops.neumf_catalog_auc(pu, pit, tower, *tail, toff, tidx, dump_probs=True)
    assert N._equal(auc, ops.full_auc(dump, toff, tidx))
    assert torch.equal(torch.isnan(auc).cpu(), torch.tensor([True, False, False, False, False, True]))
    for shift in (0, 3):                                                       # the rows excluded for their own user, and for another
        ex = csr(shift)
        ts, ti, probs = ops.neumf_catalog_topk(pu, pit, tower, *tail, k, exclude=ex, dump_probs=True)
        assert N._same_bits(probs, dump)
        assert _same((ts, ti), ops.topk_rows(probs, k, exclude=ex)), shift
        full = (U - 1 - shift) % U                                             # the user whose exclusion row names every item
        assert (ts[full] == -float("inf")).all() and (ti[full] == -1).all()
        for x in (None, ex):
            above, tied, d = ops.neumf_catalog_ranks(pu, pit, tower, *tail, toff, tidx, exclude=x, dump_probs=True)
            assert N._same_bits(d, dump)
            assert _same((above, tied), D._count(dump, toff, tidx, x)), (shift, x is not None)
    eng.check_ids()


# --------------------------------------------------------------------------------------------------------------- 5: the phase entries
def _through_owners(dev, W, items, eng, users, off, idx, xoff, xidx, idt, dump=None):
    """ranks_at_owners by hand over the W parts of `items`: every owner's positives, the full lists, neumf_rank_count per part into
    shared bins, rank_bins_excluded per part, then rank_bins_finalize per part on its own copy of the summed bins, scattered back"""
    ops, par = _m("ops"), _m("parallel")
    maps, g2l = R.owner_maps(items, W)
    toff, tidx = N._dev_csr(off, idx, dev)
    ex = N._dev_csr(xoff, xidx, dev)
    ids = torch.as_tensor(items, dtype=idt, device=dev)
    U, T = users.shape[0], len(idx)
    pu, _none, tower, tail = N._operands(eng, users, None)
    parts = {}
    for r in range(W):
        if len(maps[r]) == 0:               # an owner without a candidate of the list: no piece, no counts
            continue
        pit = N._operands(eng, None, ids[torch.from_numpy(maps[r].astype(np.int64)).to(dev)].contiguous())[1]
        g = torch.from_numpy(g2l[r]).to(dev)
        po, pi = ops.csr_split_by_owner(toff, tidx, g)
        xo, xi = ops.csr_split_by_owner(ex[0], ex[1], g)
        parts[r] = (pit, po, pi, xo, xi, ops.neumf_auc_positives(pu, pit, tower, *tail, po, pi), g)
    m = max(1, max(int(v[1][-1]) for v in parts.values()))
    buf = torch.full((W, m), 123.0, device=dev)
    piece_off = torch.zeros(W, U + 1, dtype=torch.int64, device=dev)
    for r in range(W):
        if r in parts:
            n = int(parts[r][1][-1])
            buf[r, :n] = parts[r][5][:n]
            piece_off[r, 1:] = (parts[r][1][1:] - parts[r][1][:-1]).cumsum(0)
        piece_off[r] += r * m
    sorted_, pcnt = ops.auc_sort_pieces(buf, piece_off, toff, T)
    bins, ties = ops.rank_bins(U, T, dev)
    for r, (pit, po, pi, xo, xi, raw, g) in parts.items():
        so, si = par.csr_union((po, pi), (xo, xi), pit.shape[1])
        d = ops.neumf_rank_count(pu, pit, tower, *tail, so, si, toff, sorted_, pcnt, bins, ties, dump_probs=dump is not None)
        if dump is not None:
            assert N._same_bits(d, dump[:, torch.from_numpy(maps[r].astype(np.int64)).to(dev)])
        ops.rank_bins_excluded(po, pi, (xo, xi), raw, toff, sorted_, pcnt, bins, ties)
    above = torch.full((T,), -1, dtype=torch.int32, device=dev)
    tied = above.clone()
    for r, (pit, po, pi, xo, xi, raw, g) in parts.items():
        a, t = ops.rank_bins_finalize(po, pi, (xo, xi), raw, toff, sorted_, pcnt, bins.clone(), ties)
        own, n = g[tidx.long()] >= 0, int(po[-1])
        assert int(own.sum()) == n
        above[own], tied[own] = a[:n], t[:n]
    return above, tied


@pytest.mark.parametrize("W,empty", [(2, False), (3, False), (3, True)])
def test_phase_entries_over_virtual_owners(dev, W, empty):
    ops = _m("ops")
    rng = np.random.default_rng(7 * W + empty)
    rows, I = 4000, 1900
    spec, p, eng = N._engine(dev, "A" if W == 2 else "B", 32, 50, rows, seed=W)
    pool = np.flatnonzero(np.arange(rows) % 3 != 2) if empty else np.arange(rows)      # empty: no id of residue 2, owner 2 holds nothing
    items = rng.permutation(pool)[:I]
    assert (sum(len(m) == 0 for m in R.owner_maps(items, W)[0]) == 1) == empty
    off, idx = R.built_users(rng, items, W, big=(100, RANK_LDS_CAP + 200))
    U = len(off) - 1
    users = torch.as_tensor(rng.integers(0, 50, U), dtype=torch.int32, device=dev)
    toff, tidx = N._dev_csr(off, idx, dev)
    xoff, xidx = _excl_over(rng, off, idx, I, dev, skip=(4,))
    pu, pit, tower, tail = N._operands(eng, users, torch.as_tensor(items, dtype=torch.int32, device=dev))
    want = ops.neumf_catalog_ranks(pu, pit, tower, *tail, toff, tidx, exclude=(xoff, xidx), dump_probs=True)
    got = _through_owners(dev, W, items, eng, users, off, idx, xoff.cpu().numpy(), xidx.cpu().numpy(), torch.int32, dump=want[2])
    eng.check_ids()
    assert _same(got, want[:2])
    assert _same(want[:2], D._count(want[2], toff, tidx, (xoff, xidx)))


# --------------------------------------------------------------------------------------------------------------- 6: the engine
def _close_to_numpy(res, above, tied, off, ks):
    """ops.rank_metrics' float32 vectors against rank_metrics_numpy (float64) on the same integers: values in [0, 1] stored float32
    once, NaN in the same places"""
    want = C.rank_metrics_numpy(above.cpu().numpy(), tied.cpu().numpy(), off.cpu().numpy(), ks)
    assert set(res) == set(want)
    for name, w in want.items():
        g = res[name].double().cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= F32_EPS).all(), (name, np.abs(g[ok] - w[ok]).max())
    return want


def test_engine_rank_metrics(dev):
    A = _load("test_gpu_auc_dot")
    U, I, ks = 64, 5000, (1, 10, 100)
    spec, p, eng = N._engine(dev, "A", 64, U, I, seed=30)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    sizes = np.random.default_rng(30).integers(0, 50, U)
    truth = A._truth(sizes, I, dev, seed=30)
    above, tied, dump = eng.catalog_ranks(users, truth, dump_probs=True)
    assert _same((above, tied), D._count(dump, *truth))
    res = eng.rank_metrics(users, truth, ks=ks)
    eng.check_ids()
    _close_to_numpy(res, above, tied, truth[0], ks)
    assert torch.equal(torch.isnan(res["mrr"]).cpu(), torch.from_numpy(sizes == 0))
    # hit@k agrees with membership in recommend(k)'s list where no tie stands at the cutoff
    off, idx = truth[0].cpu().numpy(), truth[1].cpu().numpy()
    for k in (1, 10, 100):
        _ts, ti = eng.recommend(users, k)
        top = torch.sort(dump, dim=1, descending=True)[0]
        clear = (top[:, k - 1] != top[:, k]).cpu().numpy() & (sizes > 0)
        assert clear.sum() > U // 2
        ti = ti.cpu().numpy()
        member = np.array([len(set(ti[u].tolist()) & set(idx[off[u]:off[u + 1]].tolist())) > 0 for u in range(U)])
        assert np.array_equal(res[f"hr@{k}"].cpu().numpy()[clear] == 1.0, member[clear]), k
    with pytest.raises(ValueError):
        eng.rank_metrics(users, truth, ks=tuple(range(1, 10)))          # more than 8 cutoffs


def test_engine_flushes_deferred_rows_and_checks_ids(dev):
    A, T = _load("test_gpu_auc_dot"), _load("test_gpu_neumf")
    B, U, I = 48, 1500, 400
    sw, de = T._two_engines(dev, B, U, I)                            # the same model by per-step sweep and by deferred replay ("exact")
    rng = np.random.default_rng(5)
    td = lambda a, dt: torch.from_numpy(a).to(dev).to(dt)
    for step in range(6):
        uu, ii = rng.integers(0, U, B), rng.integers(0, I, B)
        yy = (rng.random(B) < 0.3).astype(np.float32)
        for e in (sw, de):
            e.train_step(td(uu, torch.int32), td(ii, torch.int32), td(yy, torch.float32))
    assert de.deferred and de._stale
    users = torch.arange(0, 1500, 5, dtype=torch.int32, device=dev)
    truth = A._truth(np.random.default_rng(2).integers(0, 30, 300), I, dev, seed=2)
    a = de.catalog_ranks(users, truth)                               # no explicit flush: catalog_ranks flushes
    neumf = _m("neumf")
    fresh = neumf.NeuMFEngine(de.cfg, U, I, dev, max_batch=B)
    fresh.load_state_dict(de.state_dict())                           # (state_dict flushes: the rows as they are)
    assert _same(a, fresh.catalog_ranks(users, truth))
    assert _same(a, sw.catalog_ranks(users, truth))
    assert _same(a, de.catalog_ranks(users.long(), truth, items=torch.arange(I, dtype=torch.int64, device=dev)))
    de.check_ids()
    de.catalog_ranks(torch.tensor([0, U], dtype=torch.int32, device=dev), A._truth([1, 1], I, dev))
    with pytest.raises(IndexError):
        de.check_ids()
    de.rank_metrics(users[:2], A._truth([1, 1], 2, dev), items=torch.tensor([1, -1], dtype=torch.int32, device=dev))
    with pytest.raises(IndexError):
        de.check_ids()


# --------------------------------------------------------------------------------------------------------------- 7: 2 ranks, gloo staging
def _check_engine(rank, world, ctx, dev):
    par, neumf = _m("parallel"), _m("neumf")
    G, S = _load("test_gpu_sharded_recommend"), _load("test_gpu_sharded_auc")
    U, I, dim = 50, 300, 16
    for variant, idt, exchange in (("A", torch.int32, "padded"), ("B", torch.int64, "exact")):
        spec, p, single = N._engine(dev, variant, dim, U, I, seed=4, id_dtype=idt)
        p["item_mlp"][50:200] = p["item_mlp"][np.arange(50, 200) % 4]; p["item_mf"][50:200] = p["item_mf"][np.arange(50, 200) % 4]
        single.load_numpy_params(p)                                       # ties across the two owners
        sh = par.make_sharded_engine(neumf.NeuMFEngine)(single.cfg, U, I, dev, 4096, ctx, full_tables={k: torch.from_numpy(p[k]) for k in neumf.TABLES},
                                                        id_dtype=idt, exchange=exchange)
        sh.theta.buf.copy_(single.theta.buf)
        for k in single.moving:
            sh.moving[k].copy_(single.moving[k])
        # unequal user counts, one rank without users, a rank that owns no candidate of the list; with and without an exclusion CSR
        for counts, how, excl in (((13, 5), "perm", True), ((7, 0), None, True), ((0, 9), "perm", False), ((6, 4), "even", True),
                                  ((2, 3), "one", False)):
            rng = np.random.default_rng(23 + len(how or ""))
            users = torch.as_tensor(G._rank_users(rng, rank, U, counts), dtype=idt, device=dev)
            items, n_it = G._items(rng, how, I, idt, dev)
            truth = S._rank_truth(np.random.default_rng(200 + rank), counts[rank], n_it, dev)
            ex = S._rank_truth(np.random.default_rng(300 + rank), counts[rank], n_it, dev) if excl else None
            got = sh.catalog_ranks(users, truth, items=items, exclude=ex)
            assert got[0].shape == got[1].shape == (truth[1].numel(),) and got[0].dtype == torch.int32
            if counts[rank]:
                want = single.catalog_ranks(users, truth, items=items, exclude=ex)
                assert _same(got, want), (variant, counts, how, got, want)
                if how == "perm":
                    assert (want[1] > 0).any()
            res = sh.rank_metrics(users, truth, ks=(1, 10), items=items, exclude=ex)       # a collective too: every rank calls it
            if counts[rank]:
                _close_to_numpy(res, want[0], want[1], truth[0], (1, 10))
        sh.check_ids()
        with pytest.raises(NotImplementedError, match="dump_probs"):
            sh.catalog_ranks(users, truth, dump_probs=True)


def _check_model(rank, world, ctx, dev):
    import torch.distributed as dist
    par, neumf, models = _m("parallel"), _m("neumf"), _m("models")
    U, I, dim = 50, 300, 16
    m = models.NeuMFModel(device="cuda:0", max_batch=4096)
    m.compileModel(None, U, I, dim)
    eng = m.model.engine
    assert getattr(eng, "sharded", False) and eng.ctx.world == world
    shards = [None] * world
    dist.all_gather_object(shards, {k: eng.tables[k].cpu() for k in neumf.TABLES})
    ref = neumf.NeuMFEngine(eng.cfg, U, I, dev, 4096, id_dtype=torch.int32)
    for k in neumf.TABLES:
        rows = U if k.startswith("user") else I
        for r in range(world):
            ref.tables[k][r::world] = shards[r][k][:par.shard_rows(rows, r, world)].to(dev)
    th = eng.theta.buf.cpu()
    dist.broadcast(th, 0)                 # (an untrained model: make sure both ranks score with one tower)
    eng.theta.buf.copy_(th)
    ref.theta.buf.copy_(eng.theta.buf)
    for k in ref.moving:
        ref.moving[k].copy_(eng.moving[k])
    m1 = models.NeuMFModel(device="cuda:0", max_batch=4096)
    m1.model = models.KerasLikeNeuMF(ref)
    rng = np.random.default_rng(8)
    items = rng.permutation(I)[:150].tolist()
    rng = np.random.default_rng(80 + rank)
    gt = [(int(u), [items[j] for j in rng.choice(150, int(rng.integers(0, 30)), replace=False)]) for u in rng.integers(0, U, [9, 4][rank])]
    gt[0] = (gt[0][0], [items[3]])
    assert m.rank_metrics(gt, items, ks=(1, 10, 50)) == m1.rank_metrics(gt, items, ks=(1, 10, 50))


def _worker(rank, world, port, kind, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dev = torch.device("cuda:0")
        ctx = _m("parallel").DistCtx()
        {"engine": _check_engine, "model": _check_model}[kind](rank, world, ctx, dev)
        torch.cuda.synchronize()
        ctx.barrier()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()[-2500:]))
    finally:
        try:
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001
            pass


@pytest.mark.parametrize("kind", ["engine", "model"])
def test_sharded_catalog_ranks_two_ranks_one_gpu(dev, kind):
    """2 ranks (3 GPU processes with this one); every child has its own time limit and is never run again"""
    world, port = 2, N._free_port()
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    procs = [ctxm.Process(target=_worker, args=(r, world, port, kind, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=300) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
        for p in procs:      # never leave a child behind: the interpreter would wait for it at exit
            if p.is_alive():
                p.kill()
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}: {r[1]}"


# --------------------------------------------------------------------------------------------------------------- 8: the model surface
def test_neumf_model_surface(dev):
    models = _m("models")
    U, I, ks = 60, 400, (1, 5, 20)
    spec, p, eng = N._engine(dev, "B", 16, U, I, seed=14)
    m = models.NeuMFModel(device="cuda:0", max_batch=4096)
    m.model = models.KerasLikeNeuMF(eng)
    rng = np.random.default_rng(14)
    items = rng.permutation(I)[:250].tolist()
    gt = [(int(u), [items[j] for j in rng.choice(250, int(rng.integers(1, 30)), replace=False)]) for u in rng.integers(0, U, 17)]
    gt[0], gt[1] = (gt[0][0], []), (gt[1][0], [items[3]])           # one user without positives: 16 users count
    users = torch.as_tensor([u for u, _ in gt], dtype=eng.id_dtype, device=dev)
    col = {it: j for j, it in enumerate(items)}
    off, idx = _m("ops").truth_csr(len(gt), [r for r, (_u, t) in enumerate(gt) for _ in t], [col[q] for _u, t in gt for q in t], dev)
    ids = torch.as_tensor(items, dtype=eng.id_dtype, device=dev)
    got = m.rank_metrics(gt, items, ks=ks)
    per_user = eng.rank_metrics(users, (off, idx), ks=ks, items=ids)
    assert got == models._mean_over_users_with_positives(per_user)
    above, tied, dump = eng.catalog_ranks(users, (off, idx), items=ids, dump_probs=True)
    assert _same((above, tied), D._count(dump, off, idx))
    want = _close_to_numpy(per_user, above, tied, off, ks)
    has = np.array([len(t) > 0 for _u, t in gt])
    assert has.sum() == 16 and np.isnan(want["mrr"][0])
    for name, w in want.items():                                     # the user without positives is left out of the mean
        assert abs(got[name] - w[has].mean()) <= F32_EPS, name
    assert set(got) == {"mrr"} | {f"{n}@{k}" for n in ("ndcg", "recall", "hr") for k in ks}
    # excludeSeen: the training split's products are no candidates
    m._seen = (np.array([gt[2][0], gt[2][0]]), np.array([items[0], gt[2][1][0]]))
    seen = m.rank_metrics(gt, items, ks=ks, excludeSeen=True)
    assert seen["mrr"] >= got["mrr"]                                 # fewer candidates: no rank gets worse
    outside = next(i for i in range(I) if i not in col)
    with pytest.raises(ValueError, match="is not in list"):
        m.rank_metrics([(3, [items[0], outside])], items)
