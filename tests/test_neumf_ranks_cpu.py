"""-m "not gpu": the surface of the exact full-catalogue ranks for NeuMF (include/binrec.h "Catalogue ranks for NeuMF",
csrc/ranks_neumf.hip, csrc/rank_bins.h, ops.neumf_catalog_ranks / neumf_rank_count / rank_bins_excluded / rank_bins_finalize,
parallel.ranks_at_owners).

The five entries are declared, exported and bound; every argument outside the limits is refused before any launch (the pointers below
are never followed); the workspace is -1 outside the limits; no users is BR_OK; ops rejects wrong shapes, dtypes and host tensors; and
a numpy restatement of ranks_at_owners (candidates dealt round-robin to W owners, per-owner bins over the global lists, their sum, the
finalize per owner, the scatter back by g2l >= 0 order) reproduces direct counting."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

NEW = ("brNeumfCatalogRanksWorkspaceBytes", "brNeumfCatalogRanks", "brNeumfRankCount", "brRankBinsExcluded", "brRankBinsFinalize")
ERR_ARG, ERR_WS = -1, -4
BIG = (1 << 31) - 2            # n_truth (or cap) with which n_truth + n_users reaches 2^31


@pytest.fixture(scope="module")
def lib():
    import_module("binary-recommendation_amd.build").build_library(verbose=False)
    return import_module("binary-recommendation_amd._lib")


def test_new_entry_points_are_declared_bound_and_exported(lib):
    ops, par, neumf, models = (import_module("binary-recommendation_amd." + m) for m in ("ops", "parallel", "neumf", "models"))
    protos = lib.parse_header()
    assert set(NEW) <= set(protos), set(NEW) - set(protos)
    assert protos["brNeumfCatalogRanksWorkspaceBytes"][0] is ctypes.c_int64
    assert protos["brNeumfCatalogRanksWorkspaceBytes"][2] == ["n_users", "n_items", "n_truth"]
    head = ["pu", "ld_u", "n_users", "pit", "ld_i", "n_items", "dim", "n1", "n2", "n3", "act", "tower"]
    assert protos["brNeumfCatalogRanks"][2] == head + ["truth_off", "truth_idx", "n_truth", "excl_off", "excl_idx", "out_above", "out_tied",
                                                        "dump_probs", "ws", "ws_bytes", "stream"]
    assert protos["brNeumfRankCount"][2] == head + ["skip_off", "skip_idx", "list_off", "sorted", "pcnt", "cap", "bins", "ties", "dump_probs",
                                                     "stream"]
    lists = ["entry_off", "entry_idx", "excl_off", "excl_idx", "raw", "list_off", "sorted", "pcnt", "cap", "n_users", "bins", "ties"]
    assert protos["brRankBinsExcluded"][2] == lists + ["stream"]
    assert protos["brRankBinsFinalize"][2] == lists + ["above", "tied", "stream"]
    for name in ("neumf_catalog_ranks", "neumf_rank_count", "rank_bins_excluded", "rank_bins_finalize", "rank_bins", "rank_metrics"):
        assert callable(getattr(ops, name)), name
    assert callable(neumf.NeuMFEngine.catalog_ranks) and callable(neumf.NeuMFEngine.rank_metrics) and callable(models.NeuMFModel.rank_metrics)
    assert callable(par.ranks_at_owners)
    sh = par.make_sharded_engine(neumf.NeuMFEngine)
    assert sh.catalog_ranks is not neumf.NeuMFEngine.catalog_ranks            # the collective, not the inherited one
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(cdll, name), name


P = 8          # a non-null pointer that is never followed: every call below fails its argument check first, or has no user


def _head(p=P, pit=P, tower=P, U=4, I=100, dim=32, n1=64, n2=32, n3=16, act=2, ld_u=None, ld_i=None):
    return [p, n1 + dim if ld_u is None else ld_u, U, pit, I if ld_i is None else ld_i, I, dim, n1, n2, n3, act, tower]


def _ranks(off=P, idx=P, n_truth=16, xoff=0, xidx=0, above=P, tied=P, ws=P, ws_bytes=1 << 24, **kw):
    return _head(**kw) + [off, idx, n_truth, xoff, xidx, above, tied, 0, ws, ws_bytes, 0]


def _count(soff=P, sidx=P, loff=P, sorted_=P, pcnt=P, cap=10, bins=P, ties=P, **kw):
    return _head(**kw) + [soff, sidx, loff, sorted_, pcnt, cap, bins, ties, 0, 0]


def _bins(entry, eoff=P, eidx=P, xoff=P, xidx=P, raw=P, loff=P, sorted_=P, pcnt=P, cap=10, U=4, bins=P, ties=P, above=P, tied=P):
    a = [eoff, eidx, xoff, xidx, raw, loff, sorted_, pcnt, cap, U, bins, ties]
    return a + ([above, tied, 0] if entry == "brRankBinsFinalize" else [0])


# what the entries over the NeuMF operands refuse: null operands, dim / n1 / n2 / n3 past the limits, n_items 0 and 2^31, short strides,
# a bad activation
_COMMON = [dict(p=0), dict(pit=0), dict(tower=0), dict(dim=0), dict(dim=129, n1=8), dict(n1=0), dict(n1=129), dict(n2=0), dict(n2=129),
           dict(n3=0), dict(n3=33), dict(I=0), dict(I=1 << 31), dict(U=-1), dict(ld_u=95), dict(ld_i=99), dict(act=7)]
_OWN = {"brNeumfCatalogRanks": [dict(off=0), dict(idx=0), dict(above=0), dict(tied=0), dict(ws=0), dict(xoff=P), dict(xidx=P), dict(n_truth=-1),
                                dict(n_truth=BIG)],
        "brNeumfRankCount": [dict(soff=0), dict(sidx=0), dict(loff=0), dict(sorted_=0), dict(pcnt=0), dict(bins=0), dict(ties=0), dict(cap=-1),
                             dict(cap=BIG)]}
_MAKE = {"brNeumfCatalogRanks": _ranks, "brNeumfRankCount": _count}


@pytest.mark.parametrize("entry,kw", [(e, kw) for e in _MAKE for kw in _COMMON + _OWN[e]],
                         ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_bad_arguments_are_refused_before_any_launch(lib, entry, kw):
    L = lib.load()
    assert getattr(L, entry)(*_MAKE[entry](**kw)) == ERR_ARG
    assert L.brGetLastError().decode().startswith(entry)


@pytest.mark.parametrize("entry", ["brRankBinsExcluded", "brRankBinsFinalize"])
def test_bin_entries_refuse_bad_arguments(lib, entry):
    L = lib.load()
    bad = [dict(eoff=0), dict(eidx=0), dict(raw=0), dict(loff=0), dict(sorted_=0), dict(pcnt=0), dict(bins=0), dict(ties=0), dict(cap=-1),
           dict(cap=BIG), dict(U=-1), dict(xoff=0), dict(xidx=0)]           # (one exclusion pointer without the other)
    if entry == "brRankBinsFinalize":
        bad += [dict(above=0), dict(tied=0)]
    else:
        bad += [dict(xoff=0, xidx=0)]                                      # the excluded-positives kernel needs an exclusion CSR
    for kw in bad:
        assert getattr(L, entry)(*_bins(entry, **kw)) == ERR_ARG, kw
        assert L.brGetLastError().decode().startswith(entry)
    assert getattr(L, entry)(*_bins(entry, U=0)) == 0                      # no users: BR_OK


def test_workspace_and_no_users(lib):
    L = lib.load()
    q = L.brNeumfCatalogRanksWorkspaceBytes
    for U, I in ((-1, 100), (4, 0), (4, 1 << 31)):
        assert q(U, I, 10) == -1
    assert q(4, 100, -1) == -1 and q(4, 100, BIG) == -1 and q(1 << 30, 100, 1 << 30) == -1
    assert q(4, 100, BIG - 4) > 0                                          # n_truth + n_users = 2^31 - 2: inside
    # monotone in the truth entries: raw scores, sorted lists, two bins per entry and the sort's scratch, 4 bytes each; two bins per user
    sizes = [q(64, 1000, n) for n in (0, 1, 100, 10000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[-1] - sizes[0] >= 5 * 4 * (1 << 20)
    assert q(1 << 20, 1000, 100) - q(64, 1000, 100) >= 3 * 4 * ((1 << 20) - 64) - 3 * 256
    assert q(64, 100000, 100) == q(64, 1000, 100)                          # (the bins do not depend on the split plan)
    # a short workspace: BR_ERR_WORKSPACE with the entry's name, before any launch
    assert L.brNeumfCatalogRanks(*_ranks(ws_bytes=q(4, 100, 16) - 1)) == ERR_WS
    assert L.brGetLastError().decode().startswith("brNeumfCatalogRanks") and "workspace" in L.brGetLastError().decode()
    assert L.brNeumfCatalogRanks(*_ranks(U=0, n_truth=0, ws_bytes=q(0, 100, 0))) == 0
    assert L.brNeumfRankCount(*_count(U=0)) == 0


def test_ops_and_surface_reject_wrong_arguments(lib):
    import torch
    ops, models, par, neumf = (import_module("binary-recommendation_amd." + m) for m in ("ops", "models", "parallel", "neumf"))
    n1, n2, n3, dim = 16, 8, 4, 8
    tower = torch.zeros(int(lib.load().brNeumfCatalogTowerFloats(n1, n2, n3)))
    pu, pit = torch.zeros(4, n1 + dim), torch.zeros(n1 + dim, 20)
    off, idx = torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    lst, pcnt, bins = torch.zeros(1), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    calls = {"neumf_catalog_ranks": lambda a, b, t, d=dim, h=(n1, n2, n3), act="relu": ops.neumf_catalog_ranks(a, b, t, d, h, act, off, idx),
             "neumf_rank_count": lambda a, b, t, d=dim, h=(n1, n2, n3), act="relu": ops.neumf_rank_count(a, b, t, d, h, act, off, idx, off, lst, pcnt,
                                                                                                          bins, bins)}
    for name, call in calls.items():
        with pytest.raises(TypeError):
            call(pu, pit, tower)                                    # host tensors
        with pytest.raises(TypeError):
            call(pu.double(), pit, tower)                           # dtype
        with pytest.raises(ValueError):
            call(pu[0], pit, tower)                                 # not 2-D
        with pytest.raises(ValueError):
            call(pu, pit, tower, h=(129, n2, n3))                   # tower widths past the limits
        with pytest.raises(ValueError):
            call(pu, pit, tower, h=(n1, n2, 33))
        with pytest.raises(ValueError):
            call(pu, pit, tower, d=129)                             # 2 * dim > 256
        with pytest.raises(ValueError):
            call(pu, pit, tower, act="tanh")
        with pytest.raises(TypeError):
            call(pu, pit.t(), tower)                                # the item side must be feature-major with unit stride along the items
    # the bin ops: host tensors and wrong dtypes are refused before the library is called
    raw = torch.zeros(1)
    for fn in (ops.rank_bins_excluded, ops.rank_bins_finalize):
        with pytest.raises(TypeError):
            fn(off, idx, (off, idx), raw, off, lst, pcnt, bins, bins)
        with pytest.raises(TypeError):
            fn(off, idx, (off, idx), raw, off.int(), lst, pcnt, bins, bins)
    # the model surface: a true item outside `items` raises as full_auc does, before the engine is touched
    m = models.NeuMFModel.__new__(models.NeuMFModel)
    with pytest.raises(ValueError, match="not in list"):
        m.rank_metrics([(0, [7])], [1, 2])
    # the row-sharded engine refuses what no rank can form, before any collective
    sh = par.make_sharded_engine(neumf.NeuMFEngine)
    with pytest.raises(NotImplementedError, match="dump_probs"):
        sh.catalog_ranks(object(), None, None, dump_probs=True)


# ------------------------------------------------------------------------------------------------------------ ranks_at_owners in numpy
def direct_ranks(scores, off, idx, xoff=None, xidx=None):
    """the contract, counted directly: per truth entry (u, p) over the candidates i != p that are not excluded for u"""
    above, tied = np.full(len(idx), -1, np.int64), np.full(len(idx), -1, np.int64)
    for u in range(len(off) - 1):
        cand = np.ones(scores.shape[1], bool)
        if xoff is not None:
            cand[xidx[xoff[u]:xoff[u + 1]]] = False
        for e in range(off[u], off[u + 1]):
            p = idx[e]
            if not 0 <= p < scores.shape[1] or np.isnan(scores[u, p]):
                continue
            c = cand.copy()
            c[p] = False
            with np.errstate(invalid="ignore"):
                above[e], tied[e] = (scores[u, c] > scores[u, p]).sum(), (scores[u, c] == scores[u, p]).sum()
    return above, tied


def _split(off, idx, g2l):
    """brCsrSplitByOwner: the rows restricted to the owner's candidates, local positions, input order"""
    rows = [[g2l[p] for p in idx[off[u]:off[u + 1]] if 0 <= p < len(g2l) and g2l[p] >= 0] for u in range(len(off) - 1)]
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.asarray([p for r in rows for p in r], np.int64)


def owners_ranks(scores, off, idx, xoff, xidx, W):
    """ranks_at_owners restated: candidates dealt round-robin to W owners; every owner counts its candidates into bins over the users'
    FULL sorted lists (n + 1 bins per user from off[u] + u on), takes its excluded positives out, the bins are summed, every owner
    finalizes its own entries and they go back into global truth order by g2l >= 0"""
    U, I = scores.shape
    T = len(idx)
    lists = []
    for u in range(U):
        v = np.asarray([scores[u, p] for p in idx[off[u]:off[u + 1]] if 0 <= p < I], np.float32)
        lists.append(np.sort(v[~np.isnan(v)]))
    maps = [np.arange(r, I, W) for r in range(W)]
    sum_bins, sum_ties = np.zeros(T + U, np.int64), np.zeros(T + U, np.int64)
    parts = []
    for r in range(W):
        g2l = np.full(I, -1, np.int64)
        g2l[maps[r]] = np.arange(len(maps[r]))
        po, pi = _split(off, idx, g2l)
        xo, xi = _split(xoff, xidx, g2l) if xoff is not None else (None, None)
        bins, ties = np.zeros(T + U, np.int64), np.zeros(T + U, np.int64)
        for u in range(U):
            v, n = lists[u], len(lists[u])
            if n == 0:
                continue
            skip = set(pi[po[u]:po[u + 1]].tolist()) | (set(xi[xo[u]:xo[u + 1]].tolist()) if xo is not None else set())
            for l, g in enumerate(maps[r]):
                s = scores[u, g]
                if l in skip or np.isnan(s) or s < v[0]:
                    continue
                if s > v[-1]:
                    bins[off[u] + u + n] += 1
                    continue
                lo = int(np.searchsorted(v, s, "left"))
                bins[off[u] + u + lo] += 1
                ties[off[u] + u + lo] += v[lo] == s
            if xo is not None:                                   # rank_bins_excluded over the owner's own entries
                ex = set(xi[xo[u]:xo[u + 1]].tolist())
                for l in pi[po[u]:po[u + 1]]:
                    s = scores[u, maps[r][l]]
                    if l in ex and not np.isnan(s):
                        lo = int(np.searchsorted(v, s, "left"))
                        bins[off[u] + u + lo] -= 1
                        ties[off[u] + u + lo] -= 1
        sum_bins += bins
        sum_ties += ties
        parts.append((g2l, po, pi, xo, xi))
    above, tied = np.full(T, -1, np.int64), np.full(T, -1, np.int64)
    for r, (g2l, po, pi, xo, xi) in enumerate(parts):
        a_loc, t_loc = np.full(len(pi), -1, np.int64), np.full(len(pi), -1, np.int64)
        for u in range(U):                                       # rank_bins_finalize on the owner's copy of the summed bins
            v, n = lists[u], len(lists[u])
            if n == 0:
                continue
            S = np.cumsum(sum_bins[off[u] + u:off[u] + u + n + 1][::-1])[::-1]
            ex = set(xi[xo[u]:xo[u + 1]].tolist()) if xo is not None else set()
            for e in range(po[u], po[u + 1]):
                s = scores[u, maps[r][pi[e]]]
                if np.isnan(s):
                    continue
                lo, hi = int(np.searchsorted(v, s, "left")), int(np.searchsorted(v, s, "right"))
                a_loc[e] = S[hi] + (n - hi)
                t_loc[e] = sum_ties[off[u] + u + lo] + (hi - lo) - (0 if pi[e] in ex else 1)
        own = np.asarray([0 <= p < I and g2l[p] >= 0 for p in idx], bool)
        assert own.sum() == len(pi)
        above[own], tied[own] = a_loc, t_loc
    return above, tied


@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("exclusion", [False, True])
def test_the_owner_path_restated_in_numpy_reproduces_direct_counting(W, exclusion):
    rng = np.random.default_rng(40 + W)
    U, I = 7, 90
    scores = rng.integers(-3, 4, (U, I)).astype(np.float32)                 # few values: ties everywhere
    scores[:, 7], scores[:, 11], scores[2, 20:40] = np.nan, np.inf, -np.inf
    rows = [np.empty(0, np.int64), np.arange(I), np.array([7]), np.array([5, 7, 11, 30])]     # none, every candidate, a NaN positive alone, mixed
    rows += [np.sort(rng.choice(I, int(rng.integers(1, 30)), replace=False)) for _ in range(U - 4)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int64)
    xoff = xidx = None
    if exclusion:                                                           # overlaps the truth; user 4 excludes nothing
        xrows = [np.sort(np.union1d(rng.choice(I, 12, replace=False), rows[u][:3])) if u != 4 else np.empty(0, np.int64) for u in range(U)]
        xoff = np.concatenate([[0], np.cumsum([len(r) for r in xrows])]).astype(np.int64)
        xidx = np.concatenate(xrows).astype(np.int64)
    want = direct_ranks(scores, off, idx, xoff, xidx)
    assert (want[1] > 0).sum() > len(idx) // 2 and (want[0][off[2]:off[3]] == -1).all()
    got = owners_ranks(scores, off, idx, xoff, xidx, W)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # an owner without a candidate: W past the list's length leaves owners empty, the result stands
    if W == 3:
        sc = scores[:, :2]
        o2 = np.array([0, 1, 2], np.int64)
        want2 = direct_ranks(sc[:2], o2, np.array([0, 1], np.int64))
        got2 = owners_ranks(sc[:2], o2, np.array([0, 1], np.int64), None, None, 3)     # owner 2 holds no candidate
        assert np.array_equal(got2[0], want2[0]) and np.array_equal(got2[1], want2[1])
