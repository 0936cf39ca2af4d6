"""-m gpu: catalogue top-k and AUC for rows wider than 128 features (csrc/recommend_dot_wide.hip, csrc/auc_dot_wide.hip,
ops.dot_catalog_topk_wide / dot_catalog_auc_wide, BPREngine / ShardedBPREngine / BPRModel at the reference's latent_dim = 350): scores
against float64, the block kernels against the whole-row kernels bit for bit, exact integer rows, one accumulator chain across the
feature blocks, selection, strides, plan independence, AUC against brFullAuc bit for bit, the surfaces, scale and memory.

The reference of the model-surface checks is float64 (the numpy MAP and the float64 Mann-Whitney AUC of test_gpu_recommend_dot.py /
test_gpu_auc_dot.py), not method="matrix": brScoreMatrix stops at 128 features, so predict_scores and every method="matrix" call
refuse a 350-wide model."""
import importlib.util
import os
import socket
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WIDE_DIMS = [129, 130, 131, 200, 256, 257, 350, 384, 511, 512]


def _m(name):
    return import_module("binary-recommendation_amd." + name)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bound(Q, C):
    """1e-5 * sum_j |q_j c_j| per pair (float64): the project's bar.  The fp32 chain itself stays near 2.5e-7 of that sum."""
    return 1e-5 * (Q.double().abs() @ C.double().abs().T)


def _empty_csr(U, dev):
    return torch.zeros(U + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)


def _reference(dump, k, exclude=None):
    """brTopKRows (or brTopKRowsExclude) over the dumped scores: the selection the fused kernel must reproduce bit for bit"""
    ops = _m("ops")
    if exclude is None and k > dump.shape[1]:
        exclude = _empty_csr(dump.shape[0], dump.device)          # (the padded form: slots past the items are (-inf, -1))
    return ops.topk_rows(dump, k, exclude=exclude)


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert _bits(x, y)


def _truth(sizes, I, dev, seed=0):
    """ops.truth_csr with sizes[u] distinct random positions per user"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(len(sizes)), sizes)
    cols = np.concatenate([rng.choice(I, int(p), replace=False) for p in sizes] + [np.zeros(0, np.int64)])
    return _m("ops").truth_csr(len(sizes), rows, cols, dev)


def _nan_equal(a, b):
    """bit for bit, NaN in the same places"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and _bits(a[~torch.isnan(a)], b[~torch.isnan(b)])


# ---------------------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("dim", WIDE_DIMS)
def test_scores_against_float64(dev, dim):
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(dim)
    for U, I in ((1, 4097), (37, 1000), (1000, 37), (4097, 1)):
        Q = torch.randn(U, dim, generator=g).to(dev)
        C = torch.randn(I, dim, generator=g).to(dev)
        s, i, dump = ops.dot_catalog_topk_wide(Q, C, 10, dump_scores=True)
        ref = Q.double() @ C.double().T
        ratio = ((dump.double() - ref).abs() / (_bound(Q, C) * 1e5)).max().item()
        print(f"dim {dim} {U}x{I}: worst |err| / sum|q c| = {ratio:.3e}")
        assert torch.all((dump.double() - ref).abs() <= _bound(Q, C)), (U, I)
        _assert_same((s, i), _reference(dump, 10))


@pytest.mark.parametrize("dim", [1, 33, 64, 100, 128])
def test_forced_wide_equals_narrow(dev, dim):
    """BR_DOT_FORCE_WIDE sends rows the whole-row kernels take through the block kernels: the same bits, top-k and AUC; without the
    flag the wide ops ARE the narrow launches"""
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(100 + dim)
    for U, I in ((1, 4097), (37, 1000), (300, 2000)):
        Q = torch.randn(U, dim, generator=g).to(dev)
        C = torch.randn(I, dim, generator=g).to(dev)
        for k in (10, 100, 256):
            want = ops.dot_catalog_topk(Q, C, k, dump_scores=True)
            _assert_same(ops.dot_catalog_topk_wide(Q, C, k, dump_scores=True, force_wide=True), want)
            _assert_same(ops.dot_catalog_topk_wide(Q, C, k, dump_scores=True), want)
        sizes = np.random.default_rng(dim).choice([0, 1, 2, 7, 200, I], U)
        off, idx = _truth(sizes, I, dev, seed=dim)
        want = ops.dot_catalog_auc(Q, C, off, idx, dump_scores=True)
        for force in (True, False):
            got = ops.dot_catalog_auc_wide(Q, C, off, idx, dump_scores=True, force_wide=force)
            assert _nan_equal(got[0], want[0]) and _bits(got[1], want[1]), (U, I, force)


@pytest.mark.parametrize("dim", [129, 257, 350, 512])
def test_exact_blocks(dev, dim):
    """integer rows: every fp32 partial sum is exact, so the scores equal the int64 product - a block dropped, doubled or padded
    wrongly shows; then rows that are non-zero in one feature only (the last one, the first of the second and of the third block)"""
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(dim)
    U, I = 70, 700
    Qi = torch.randint(-3, 4, (U, dim), generator=g)
    Ci = torch.randint(-3, 4, (I, dim), generator=g)
    want = (Qi @ Ci.T).to(dev)
    dump = ops.dot_catalog_topk_wide(Qi.float().to(dev), Ci.float().to(dev), 10, dump_scores=True)[2]
    assert torch.equal(dump.long(), want) and torch.equal(dump, want.float())
    for f in (dim - 1, 128, 256):
        if f >= dim:
            continue
        Q1, C1 = torch.zeros_like(Qi), torch.zeros_like(Ci)
        Q1[:, f], C1[:, f] = Qi[:, f] + 4, Ci[:, f] + 4          # (1..7: no zero column)
        dump = ops.dot_catalog_topk_wide(Q1.float().to(dev), C1.float().to(dev), 10, dump_scores=True)[2]
        assert torch.equal(dump.long(), (Q1 @ C1.T).to(dev)), f
        off, idx = _truth(np.full(U, 5), I, dev, seed=f)
        auc, adump = ops.dot_catalog_auc_wide(Q1.float().to(dev), C1.float().to(dev), off, idx, dump_scores=True)
        assert torch.equal(adump, dump) and _nan_equal(auc, ops.full_auc(dump, off, idx))


@pytest.mark.parametrize("dim", [129, 350, 512])
def test_one_chain_across_blocks(dev, dim):
    """2^24 at feature 0, then 1.0 once per MFMA k-step from feature 128 on, against an all-ones item: in ONE chain every + 1 rounds
    away (2^24 + 1 is a tie that rounds to even) and the score is exactly 2^24; summing each block apart and adding the sums gives
    2^24 + the count of ones"""
    ops = _m("ops")
    q = torch.zeros(3, dim)
    q[0, 0] = q[2, 0] = 2.0 ** 24
    q[0, 128::4] = 1.0
    q[1, 128::4] = 1.0                                           # the ones alone: their count, exactly
    C = torch.ones(50, dim)
    n_ones = len(range(128, dim, 4))
    s, i, dump = ops.dot_catalog_topk_wide(q.to(dev), C.to(dev), 5, dump_scores=True)
    assert torch.all(dump[0] == 16777216.0), dump[0, :4]
    assert torch.all(dump[1] == float(n_ones)) and torch.all(dump[2] == 16777216.0)
    off, idx = _truth(np.array([3, 3, 3]), 50, dev)
    assert torch.equal(ops.dot_catalog_auc_wide(q.to(dev), C.to(dev), off, idx, dump_scores=True)[1], dump)


# ------------------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("k", [1, 10, 100, 256])
def test_selection_equals_topk_rows(dev, k):
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(k)
    for U, I in ((1, 5000), (37, 1000), (300, 4097), (5, 100)):
        Q = torch.randn(U, 350, generator=g).to(dev)
        C = torch.randn(I, 350, generator=g).to(dev)
        s, i, dump = ops.dot_catalog_topk_wide(Q, C, k, dump_scores=True)
        _assert_same((s, i), _reference(dump, k))
        if k > I:
            assert torch.all(i[:, I:] == -1) and torch.all(torch.isneginf(s[:, I:]))
            assert torch.all(i[:, :I] >= 0)
        # with exclusion: every third user drops a random tenth of the items, one user drops everything
        rng = np.random.default_rng(k)
        rows, cols = [], []
        for u in range(0, U, 3):
            c = rng.choice(I, size=max(1, I // 10), replace=False) if u != 3 else np.arange(I)
            rows += [u] * len(c); cols += c.tolist()
        ex = ops.truth_csr(U, rows, cols, dev)
        s, i, dump2 = ops.dot_catalog_topk_wide(Q, C, k, exclude=ex, dump_scores=True)
        assert _bits(dump2, dump)
        _assert_same((s, i), ops.topk_rows(dump, k, exclude=ex))
        if U > 3:
            assert torch.all(i[3] == -1) and torch.all(torch.isneginf(s[3]))


def test_ties_across_item_splits(dev):
    """identical best rows on both sides of split and window boundaries: the lower position comes first"""
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(7)
    I, dim = 5000, 350
    C = torch.rand(I, dim, generator=g) * 2 - 1
    dup = [31, 32, 63, 64, 127, 128, 1023, 1024, 2500, 4999]
    C[dup] = 2.0                                              # the best row for every user with positive features
    C[[100, 101, 3000]] = C[7].clone()                        # plain ties elsewhere in the list
    C = C.to(dev)
    for U in (1, 300):
        Q = (torch.rand(U, dim, generator=g) * 0.9 + 0.1).to(dev)
        for k in (5, 10, 40, 256):
            s, i, dump = ops.dot_catalog_topk_wide(Q, C, k, dump_scores=True)
            _assert_same((s, i), _reference(dump, k))
            n = min(k, len(dup))
            assert torch.all(i[:, :n] == torch.tensor(dup[:n], dtype=torch.int32, device=dev)), (U, k)
            assert torch.all(s[:, :n] == s[:, :1])


def test_stride_larger_than_dim(dev):
    """a column slice of a wider table (16-B aligned rows and not: the scalar-load path) gives the packed rows' result bit for bit"""
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(1)
    for dim, ld, off in ((350, 352, 0), (350, 351, 1), (129, 131, 0)):
        Qw = torch.randn(300, ld, generator=g).to(dev)
        Cw = torch.randn(1500, ld, generator=g).to(dev)
        Q, C = Qw[:, off:dim + off], Cw[:, off:dim + off]
        assert Q.stride(0) == ld and C.stride(0) == ld
        _assert_same(ops.dot_catalog_topk_wide(Q, C, 20, dump_scores=True), ops.dot_catalog_topk_wide(Q.contiguous(), C.contiguous(), 20, dump_scores=True))
        t_off, t_idx = _truth(np.random.default_rng(ld).choice([0, 3, 40], 300), 1500, dev)
        a = ops.dot_catalog_auc_wide(Q, C, t_off, t_idx, dump_scores=True)
        b = ops.dot_catalog_auc_wide(Q.contiguous(), C.contiguous(), t_off, t_idx, dump_scores=True)
        assert _nan_equal(a[0], b[0]) and _bits(a[1], b[1])
        assert torch.all((a[1].double() - Q.double() @ C.double().T).abs() <= _bound(Q, C))


def test_plan_independence(dev):
    """a user scored alone and among 300 users gets the same list bits; the dump of a sub-catalogue equals those columns of the whole"""
    ops = _m("ops")
    g = torch.Generator(device="cpu").manual_seed(13)
    Q = torch.randn(300, 350, generator=g).to(dev)
    C = torch.randn(6000, 350, generator=g).to(dev)
    for k in (10, 100):
        full = ops.dot_catalog_topk_wide(Q, C, k, dump_scores=True)
        for sel in ([0], [299], list(range(100, 163))):
            idx = torch.tensor(sel, device=dev)
            part = ops.dot_catalog_topk_wide(Q[idx].contiguous(), C, k, dump_scores=True)
            _assert_same(part, tuple(t[idx] for t in full))
        for lo, hi in ((0, 1), (17, 2048), (4001, 6000)):
            sub = ops.dot_catalog_topk_wide(Q, C[lo:hi], k, dump_scores=True)[2]
            assert _bits(sub, full[2][:, lo:hi].contiguous())


# ------------------------------------------------------------------------------------------------------------------------------- AUC
@pytest.mark.parametrize("dim", [129, 350, 512])
def test_auc_bit_exact_against_full_auc_of_the_dump(dev, dim):
    ops = _m("ops")
    U, I = 300, 5000
    rng = np.random.default_rng(dim)
    g = torch.Generator(device="cpu").manual_seed(dim)
    Q = torch.randn(U, dim, generator=g).to(dev)
    C = torch.randn(I, dim, generator=g).to(dev)
    mixed = rng.choice([0, 1, 2, 7, 200, 2500, I - 1, I], U)
    small = rng.choice([0, 1, 2, 7], U)                                # every wave's lists fit in LDS
    for sizes in (mixed, small):
        off, idx = _truth(sizes, I, dev, seed=dim)
        auc, dump = ops.dot_catalog_auc_wide(Q, C, off, idx, dump_scores=True)
        assert _nan_equal(auc, ops.full_auc(dump, off, idx))
        assert torch.isnan(auc[torch.from_numpy((sizes == 0) | (sizes == I)).to(dev)]).all()
        assert not torch.isnan(auc[torch.from_numpy((sizes > 0) & (sizes < I)).to(dev)]).any()
        assert _nan_equal(auc, ops.dot_catalog_auc_wide(Q, C, off, idx))   # the dump changes nothing
        assert _bits(dump, ops.dot_catalog_topk_wide(Q, C, 1, dump_scores=True)[2])   # one score per pair, whichever kernel forms it
    # several splits: one user against the whole catalogue, the same value
    one = ops.dot_catalog_auc_wide(Q[7:8], C, torch.stack([off[7] - off[7], off[8] - off[7]]), idx[int(off[7]):int(off[8])].contiguous())
    assert _nan_equal(one, auc[7:8])


def test_auc_ties_and_non_finite_scores(dev):
    ops = _m("ops")
    U, I, dim = 120, 3000, 350
    g = torch.Generator(device="cpu").manual_seed(3)
    Q = torch.zeros(U, dim); C = torch.zeros(I, dim)
    cols = torch.randperm(dim, generator=g)[:8]                        # few non-zero integer features: many ties
    Q[:, cols] = torch.randint(-2, 3, (U, 8), generator=g).float()
    C[:, cols] = torch.randint(-2, 3, (I, 8), generator=g).float()
    C[1000:2000] = C[:1000]
    sizes = np.random.default_rng(3).choice([0, 1, 3, 50, 700, I], U)
    off, idx = _truth(sizes, I, dev, seed=3)
    auc, dump = ops.dot_catalog_auc_wide(Q.to(dev), C.to(dev), off, idx, dump_scores=True)
    assert torch.equal(dump.long(), (Q.long() @ C.long().T).to(dev))
    assert _nan_equal(auc, ops.full_auc(dump, off, idx))
    # NaN and +-inf scores
    Q = torch.rand(40, dim, generator=g) + 0.1
    C = torch.randn(700, dim, generator=g)
    Q[5] = float("nan")
    C[10, 300] = float("inf"); C[11, 0] = float("-inf"); C[12:20, 200] = float("inf")
    C[30, 1] = float("inf"); C[30, 349] = float("-inf")                # inf - inf: NaN for every user
    sizes = np.full(40, 30); sizes[7] = 0; sizes[8] = 700
    off, idx = _truth(sizes, 700, dev, seed=4)
    auc, dump = ops.dot_catalog_auc_wide(Q.to(dev), C.to(dev), off, idx, dump_scores=True)
    assert torch.isnan(dump[5]).all() and torch.isinf(dump[torch.arange(40) != 5][:, 10]).all() and torch.isnan(dump[:, 30]).all()
    assert _nan_equal(auc, ops.full_auc(dump, off, idx))
    assert float(auc[5]) == 0.0                                        # NaN user: no pair counts


def test_auc_against_float64(dev):
    A = _load("test_gpu_auc_dot")
    ops = _m("ops")
    U, I, dim = 256, 5000, 350
    g = torch.Generator(device="cpu").manual_seed(9)
    Q = torch.randn(U, dim, generator=g).to(dev)
    C = torch.randn(I, dim, generator=g).to(dev)
    off, idx = _truth(np.random.default_rng(9).integers(1, 60, U), I, dev, seed=9)
    auc = ops.dot_catalog_auc_wide(Q, C, off, idx)
    want = A._auc64(Q.double() @ C.double().T, off, idx)
    diff = abs(float(auc.double().mean()) - float(want.mean()))
    print(f"mean AUC fused {float(auc.double().mean()):.9f} float64 {float(want.mean()):.9f} diff {diff:.3e}")
    assert diff <= 1e-6


# --------------------------------------------------------------------------------------------------------------------------- surface
def _trained(dev, U=300, I=500, dim=350):
    bpr = _m("bpr")
    eng = bpr.BPREngine(U, I, dim, dev, max_batch=256, init_seed=5)
    rng = np.random.default_rng(3)
    td = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    for _ in range(3):
        eng.train_step(td(rng.integers(0, U, 256)), td(rng.integers(0, I, 256)), td(rng.integers(0, I, 256)))
    return eng


def test_bpr_engine_at_350(dev):
    ops = _m("ops")
    eng = _trained(dev)
    users = torch.arange(0, 300, 3, dtype=torch.int32, device=dev)
    s, i, dump = eng.recommend(users, 20, dump_scores=True)
    _assert_same((s, i), _reference(dump, 20))
    _assert_same((s, i), eng.recommend(users.long(), 20))
    q = eng.user[users.long()].contiguous()
    assert torch.all((dump.double() - q.double() @ eng.item.double().T).abs() <= _bound(q, eng.item))
    ex = _truth(np.random.default_rng(1).integers(0, 40, len(users)), 500, dev, seed=1)
    _assert_same(eng.recommend(users, 20, exclude=ex), ops.topk_rows(dump, 20, exclude=ex))
    sub = torch.tensor([499, 3, 250, 7], dtype=torch.int64, device=dev)
    s4, i4, d4 = eng.recommend(users, 4, items=sub, dump_scores=True)
    _assert_same((s4, i4), _reference(d4, 4))
    assert _bits(d4, dump[:, sub].contiguous())
    truth = _truth(np.random.default_rng(2).choice([0, 1, 5, 30], len(users)), 500, dev, seed=2)
    auc, adump = eng.full_auc(users, truth, dump_scores=True)
    assert _bits(adump, dump) and _nan_equal(auc, ops.full_auc(dump, *truth))
    eng.check_ids()
    eng.recommend(torch.tensor([0, 300], dtype=torch.int32, device=dev), 5)
    with pytest.raises(IndexError):
        eng.check_ids()


def test_bpr_model_surface_at_350(dev, tmp_path, monkeypatch):
    import pandas as pd
    G, A = _load("test_gpu_recommend_dot"), _load("test_gpu_auc_dot")
    models, tkm = _m("models"), _m("topk_metrics")
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    U, I, n = 120, 80, 4000
    u = rng.integers(0, U, n); i = (u * 7 + rng.integers(0, 5, n)) % I
    pd.DataFrame({"CUSTOMER_ID": u, "PRODUCT_ID": i, "MATERIAL": i, "QUANTITY": 1}).to_csv(tmp_path / "sdata.csv", index=False)
    m = models.BPRModel(device="cuda:0", max_batch=4096)
    m.epochs, m.numFactor = 2, 350
    m.train(str(tmp_path / "sdata.csv"), 50000, {})
    assert m.model.dim == 350
    seen = {}
    for a, b in zip(m.trainDf.CUSTOMER_ID.tolist(), m.trainDf.PRODUCT_ID.tolist()):
        seen.setdefault(int(a), set()).add(str(b))
    cust = [int(c) for c in m.getPredictableUsers()[:30]]
    recs = m.recommendForUsers(cust, 5, excludeSeen=True)
    assert len(recs) == len(cust)
    for c, lst in zip(cust, recs):
        assert lst and not {it for it, _s in lst} & seen.get(c, set())
        assert lst == m.predictForUser(c, 5, excludeSeen=True)
        assert all(float(a[1]) >= float(b[1]) for a, b in zip(lst, lst[1:]))
    rows = tkm.topKRatings(5, m, cust, m.productIds)
    assert [[str(it) for _s, it in lst] for _u, lst in rows] == [[it for it, _s in lst] for lst in m.recommendForUsers(cust, 5, excludeSeen=False)]
    # MAP@k and full AUC through the fused path against float64 scores
    items = [int(x) for x in m.productIds]
    gt = [(int(c), [int(x) for x in m.testDf[m.testDf.CUSTOMER_ID == c].PRODUCT_ID.tolist()]) for c in cust]
    e = m.model
    Qu = e.user[torch.tensor([c for c, _ in gt], device=e.device)].double()
    Ci = e.item[torch.tensor(items, device=e.device)].double()
    S = Qu @ Ci.T
    col = {it: j for j, it in enumerate(items)}
    truth = [{col[p] for p in t if p in col} for _c, t in gt]
    got = m.mean_average_precision_k(gt, items, k=10, method="fused")
    want = G._map_numpy(S.cpu().numpy(), truth, [len(t) for _c, t in gt], 10)
    print(f"MAP@10 fused {got:.9f} float64 {want:.9f}")
    assert got == pytest.approx(want, abs=1e-6)
    rows_ = [n for n, t in enumerate(truth) for _ in t]
    off, idx = _m("ops").truth_csr(len(gt), rows_, [p for t in truth for p in t], e.device)
    per = A._auc64(S, off, idx)
    gt_in = [(c, [p for p in t if p in col]) for c, t in gt]           # (full_auc raises for a true item outside `items`, as bpr.py:247)
    got, want = m.full_auc(gt_in, items, method="fused"), float(np.nanmean(per))
    print(f"full AUC fused {got:.9f} float64 {want:.9f}")
    assert got == pytest.approx(want, abs=1e-6)


# --------------------------------------------------------------------------------------------------------------------------- sharded
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("k", [10, 256])
def test_virtual_ranks_equal_the_whole_catalogue(dev, W, k):
    """the candidate list dealt to W owners on one device (test_gpu_sharded_recommend.py): the wide launch per part, the exclusion CSR
    cut down to each part, the W lists merged - bit for bit the launch over the whole list"""
    ops = _m("ops")
    SH = _load("test_gpu_sharded_recommend")
    rng = np.random.default_rng(7 * W + k)
    U, rows, I, dim = 70, 2000, 1500, 350
    T = torch.from_numpy(rng.standard_normal((rows, dim)).astype(np.float32)).to(dev)
    T[:5] *= 2.5
    T[200:900] = T[(torch.arange(200, 900, device=dev) % 5)]        # duplicated rows on every owner: equal scores meet in the merge
    Q = torch.from_numpy(rng.standard_normal((U, dim)).astype(np.float32)).to(dev)
    items = rng.permutation(rows)[:I]
    ids = torch.as_tensor(items, dtype=torch.int64, device=dev)
    C = ops.gather_rows([T], [ids])[0]
    for ex_np in (None, SH._exclusion(rng, U, items, W, dev)):
        want_s, want_p = ops.dot_catalog_topk_wide(Q, C, k, exclude=None if ex_np is None else ex_np[2])

        def launch(pos, ex):
            part = ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
            return ops.dot_catalog_topk_wide(Q, part, k, exclude=ex)
        got_s, got_p = SH._through_owners(dev, W, items, U, k, ex_np, launch)
        assert torch.equal(got_p, want_p) and _bits(got_s, want_s)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        par, bpr = _m("parallel"), _m("bpr")
        dev = torch.device("cuda:0")
        ctx = par.DistCtx()
        U, I, dim = 60, 333, 350
        g = torch.Generator().manual_seed(dim)
        full = {"user": torch.randn(U, dim, generator=g), "item": torch.randn(I, dim, generator=g)}
        full["item"][50:200] = full["item"][torch.arange(50, 200) % 4]          # ties across the two owners
        sh = par.make_sharded_bpr(bpr.BPREngine)(U, I, dim, dev, 256, ctx, full_tables=full)
        single = bpr.BPREngine(U, I, dim, dev, 256)
        single._user.copy_(full["user"]); single._item.copy_(full["item"])
        rng = np.random.default_rng(23)
        mine = torch.from_numpy(rng.permutation(U)[rank::world][:20].astype(np.int32)).to(dev)
        sub = torch.from_numpy(rng.permutation(I)[:200].astype(np.int32)).to(dev)
        for k in (10, 256):
            for items, n_it in ((None, I), (sub, 200)):
                ex = _truth(np.random.default_rng(k + rank).integers(0, n_it // 3, len(mine)), n_it, dev, seed=k)
                for e in (None, ex):
                    want = single.recommend(mine, k, items=items, exclude=e)
                    _assert_same(sh.recommend(mine, k, items=items, exclude=e, catalog="owners"), want)
                    _assert_same(sh.recommend(mine, k, items=items, exclude=e, catalog="gather"), want)
        truth = _truth(np.random.default_rng(5 + rank).choice([0, 2, 9], len(mine)), I, dev, seed=5)
        assert _nan_equal(sh.full_auc(mine, truth), single.full_auc(mine, truth))
        sh.check_ids()
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


def test_sharded_bpr_engine_at_350_two_ranks(dev):
    """2 ranks on one card over gloo; every child has its own time limit and is never run again"""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    procs = [ctxm.Process(target=_sharded_worker, args=(r, world, port, q)) for r in range(world)]
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


# ------------------------------------------------------------------------------------------------------------------ scale and memory
def test_scale_and_memory(dev):
    ops, bpr = _m("ops"), _m("bpr")
    U, I, dim, k = 65536, 100000, 350, 10
    eng = bpr.BPREngine(U, I, dim, dev, max_batch=1024)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    s, i = eng.recommend(users, k)
    torch.cuda.synchronize()
    eng.check_ids()
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"allocator peak rose by {rise / 2**20:.0f} MiB; the U x I matrix is {U * I * 4 / 2**20:.0f} MiB")
    assert rise < U * I * 4 / 8, rise
    assert s.shape == (U, k) and torch.all(i >= 0)
    sample = torch.from_numpy(np.random.default_rng(0).choice(U, 64, replace=False)).to(dev)
    q = eng.user[sample].contiguous()
    ss, si, dump = ops.dot_catalog_topk_wide(q, eng.item, k, dump_scores=True)      # the sampled users' score rows, by themselves
    assert torch.all((dump.double() - q.double() @ eng.item.double().T).abs() <= _bound(q, eng.item))
    _assert_same((s[sample], i[sample]), ops.topk_rows(dump, k))
