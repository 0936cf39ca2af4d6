"""-m "not gpu": the surface of the dot-product catalogue ranks counted at the item owners (include/binrec.h "Catalogue ranks at the item
owners", csrc/ranks_owner.hip, ops.dot_rank_count, ShardedBPREngine / ShardedTwoTowerEngine.catalog_ranks, BPRModel.rank_metrics(catalog=)).

brDotRankCount is declared, exported and bound; every argument outside the limits is refused before any launch (the pointers below are
never followed); no users is BR_OK; the engines and the model refuse what they cannot do before anything touches a device; and a numpy
restatement of the owner bin rule the header states, summed over W owners and finalized, reproduces brute-force (above, tied)."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

ERR_ARG = -1
BIG = (1 << 31) - 2            # a cap with which cap + n_users reaches 2^31


@pytest.fixture(scope="module")
def lib():
    import_module("binary-recommendation_amd.build").build_library(verbose=False)
    return import_module("binary-recommendation_amd._lib")


def test_entry_point_is_declared_bound_and_exported(lib):
    ops, par, bpr, tt = (import_module("binary-recommendation_amd." + m) for m in ("ops", "parallel", "bpr", "two_tower"))
    protos = lib.parse_header()
    assert protos["brDotRankCount"][0] is ctypes.c_int
    assert protos["brDotRankCount"][2] == ["Q", "ld_q", "n_users", "C", "ld_c", "n_items", "dim", "skip_off", "skip_idx", "list_off", "sorted",
                                           "pcnt", "cap", "bins", "ties", "dump_scores", "flags", "stream"]
    # brDotAucOwnerCount's operands up to the list, brNeumfRankCount's from the skip CSR to the bins
    assert protos["brDotRankCount"][2][:13] == protos["brDotAucOwnerCount"][2][:13]
    assert protos["brDotRankCount"][2][7:15] == protos["brNeumfRankCount"][2][12:20]
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "brDotRankCount")
    assert callable(ops.dot_rank_count)
    sb, st = par.make_sharded_bpr(bpr.BPREngine), par.make_sharded_two_tower(tt.TwoTowerEngine)
    assert sb.catalog_ranks is not bpr.BPREngine.catalog_ranks and sb.rank_metrics is not bpr.BPREngine.rank_metrics
    assert callable(tt.TwoTowerEngine.catalog_ranks)
    assert st.catalog_ranks is not tt.TwoTowerEngine.catalog_ranks and st.rank_metrics is not tt.TwoTowerEngine.rank_metrics


P = 8          # a non-null pointer that is never followed: every call below fails its argument check first, or has no user


def _count(Q=P, C=P, U=4, I=100, dim=32, ld_q=None, ld_c=None, soff=P, sidx=P, loff=P, sorted_=P, pcnt=P, cap=10, bins=P, ties=P, flags=0):
    return [Q, dim if ld_q is None else ld_q, U, C, dim if ld_c is None else ld_c, I, dim, soff, sidx, loff, sorted_, pcnt, cap, bins, ties, 0,
            flags, 0]


_BAD = [dict(Q=0), dict(C=0), dict(soff=0), dict(sidx=0), dict(loff=0), dict(sorted_=0), dict(pcnt=0), dict(bins=0), dict(ties=0),   # null pointers
        dict(dim=0), dict(dim=513), dict(flags=2), dict(flags=-1), dict(cap=-1), dict(cap=BIG), dict(cap=1 << 40), dict(U=-1),
        dict(U=1 << 31, cap=0), dict(I=0), dict(I=1 << 31), dict(ld_q=31), dict(ld_c=31)]


@pytest.mark.parametrize("kw", _BAD, ids=lambda kw: ",".join(f"{k}={x}" for k, x in kw.items()))
def test_bad_arguments_are_refused_before_any_launch(lib, kw):
    L = lib.load()
    assert L.brDotRankCount(*_count(**kw)) == ERR_ARG
    assert L.brGetLastError().decode().startswith("brDotRankCount")
    with pytest.raises(lib.BinrecError):
        lib.check(ERR_ARG, "brDotRankCount")


def test_no_users_and_the_limits_inside(lib):
    L = lib.load()
    assert lib.parse_enums()["BR_DOT_FORCE_WIDE"] == 1                     # (flags=2 above is an unknown flag)
    assert L.brDotRankCount(*_count(U=0)) == 0
    assert L.brDotRankCount(*_count(U=0, dim=512, flags=1)) == 0
    assert L.brDotRankCount(*_count(U=0, cap=BIG + 1)) == 0                # cap + n_users = 2^31 - 1: inside


def test_ops_engines_and_model_reject_what_they_cannot_do(lib):
    import torch
    ops, par, models, bpr = (import_module("binary-recommendation_amd." + m) for m in ("ops", "parallel", "models", "bpr"))
    Q, C = torch.zeros(4, 8), torch.zeros(20, 8)
    off, idx = torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    lst, pcnt, bins = torch.zeros(1), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.dot_rank_count(Q, C, off, idx, off, lst, pcnt, bins, bins)       # host tensors
    with pytest.raises(TypeError):
        ops.dot_rank_count(Q.double(), C, off, idx, off, lst, pcnt, bins, bins)
    with pytest.raises(ValueError):
        ops.dot_rank_count(Q[0], C, off, idx, off, lst, pcnt, bins, bins)    # not 2-D
    with pytest.raises(ValueError):
        ops.dot_rank_count(Q, torch.zeros(20, 9), off, idx, off, lst, pcnt, bins, bins)
    with pytest.raises(ValueError):
        ops.dot_rank_count(torch.zeros(4, 513), torch.zeros(20, 513), off, idx, off, lst, pcnt, bins, bins)
    # the row-sharded engine: a bad catalog and a dump no rank can form, before any collective
    sb = par.make_sharded_bpr(bpr.BPREngine)
    e = sb.__new__(sb)                                                       # (never initialised: the checks come first)
    with pytest.raises(ValueError, match="catalog"):
        e.catalog_ranks(None, None, catalog="everywhere")
    with pytest.raises(ValueError, match="catalog"):
        e.rank_metrics(None, None, catalog="everywhere")
    with pytest.raises(NotImplementedError, match="dump_scores"):
        e.catalog_ranks(None, None, dump_scores=True, catalog="owners")
    # the model surface: "owners" needs a row-sharded engine; a bad value is refused as full_auc refuses it
    m = models.BPRModel.__new__(models.BPRModel)
    m.model = object()                                                       # (an engine without a process group: no `ctx`)
    with pytest.raises(ValueError, match="row-sharded"):
        m.rank_metrics([(0, [1])], [1, 2], catalog="owners")
    with pytest.raises(ValueError, match="catalog"):
        m.rank_metrics([(0, [1])], [1, 2], catalog="everywhere")


# ------------------------------------------------------------------------------------------------------------ the bin rule in numpy
def brute(scores, off, idx, xoff, xidx):
    """(above, tied) per truth entry, counted directly over the candidates i != p that are not excluded for u; (-1, -1) for NaN"""
    above, tied = np.full(len(idx), -1, np.int64), np.full(len(idx), -1, np.int64)
    for u in range(len(off) - 1):
        cand = np.ones(scores.shape[1], bool)
        if xoff is not None:
            cand[xidx[xoff[u]:xoff[u + 1]]] = False
        for e in range(off[u], off[u + 1]):
            s = scores[u, idx[e]]
            if np.isnan(s):
                continue
            c = cand.copy(); c[idx[e]] = False
            with np.errstate(invalid="ignore"):
                above[e], tied[e] = (scores[u, c] > s).sum(), (scores[u, c] == s).sum()
    return above, tied


def owner_bins(scores_loc, skip, lists, list_off, bins, ties):
    """brDotRankCount as include/binrec.h states it, for one owner: scores_loc (U, I_loc), skip[u]: the local positions not counted,
    lists[u]: the user's FULL ascending list v (n entries); user u's n + 1 bins start at list_off[u] + u.  ADDS into bins / ties"""
    for u in range(scores_loc.shape[0]):
        v = lists[u]; n = len(v)
        if n == 0:
            continue
        b0 = list_off[u] + u
        for l in range(scores_loc.shape[1]):
            s = scores_loc[u, l]
            if l in skip[u] or np.isnan(s) or s < v[0]:                  # skipped; NaN or below v_0: touches nothing
                continue
            if s > v[-1]:                                                # above v_{n-1}: bin n
                bins[b0 + n] += 1
                continue
            lo = int((v < s).sum())                                      # v_0 <= s <= v_{n-1}: bin #{v < s} ...
            bins[b0 + lo] += 1
            if v[lo] == s:                                               # ... and the tie bin of that index when v_lo == s
                ties[b0 + lo] += 1


@pytest.mark.parametrize("W", [1, 2, 3, 5])
@pytest.mark.parametrize("exclusion", [False, True])
def test_the_owner_bin_rule_summed_and_finalized_is_the_brute_force_count(W, exclusion):
    rng = np.random.default_rng(60 + W)
    U, I = 8, 120
    scores = rng.integers(-4, 5, (U, I)).astype(np.float32)                 # nine values: ties everywhere
    scores[:, 9], scores[:, 13], scores[3, 40:60] = np.nan, np.inf, -np.inf
    rows = [np.empty(0, np.int64), np.arange(I), np.array([9]), np.array([5, 9, 13, 41])]      # none, every candidate, a NaN positive alone, mixed
    rows += [np.sort(rng.choice(I, int(rng.integers(1, 40)), replace=False)) for _ in range(U - 4)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int64)
    xoff = xidx = None
    if exclusion:                                                           # overlaps the truth; user 4 excludes nothing
        xr = [np.union1d(rng.choice(I, 15, replace=False), rows[u][:3]) if u != 4 else np.empty(0, np.int64) for u in range(U)]
        xoff = np.concatenate([[0], np.cumsum([len(r) for r in xr])]).astype(np.int64)
        xidx = np.concatenate(xr).astype(np.int64)
    want = brute(scores, off, idx, xoff, xidx)
    assert (want[1] > 0).sum() > len(idx) // 2 and (want[0][off[2]:off[3]] == -1).all()
    T = len(idx)
    lists = []
    for u in range(U):
        v = scores[u, idx[off[u]:off[u + 1]]]
        lists.append(np.sort(v[~np.isnan(v)]))
    owners = [np.flatnonzero(np.arange(I) % W == r) for r in range(W)]      # candidate positions of owner r, ascending
    bins, ties = np.zeros(T + U, np.int64), np.zeros(T + U, np.int64)
    for own in owners:
        local = {int(g): l for l, g in enumerate(own)}
        skip = []
        for u in range(U):
            s = {local[int(p)] for p in idx[off[u]:off[u + 1]] if int(p) in local}
            if exclusion:
                s |= {local[int(p)] for p in xidx[xoff[u]:xoff[u + 1]] if int(p) in local}
            skip.append(s)
        owner_bins(scores[:, own], skip, lists, off, bins, ties)            # every owner adds into the same bins
    # brRankBinsExcluded over all entries, then brRankBinsFinalize: suffix sums, the list terms, the entry itself
    above, tied = np.full(T, -1, np.int64), np.full(T, -1, np.int64)
    for u in range(U):
        v, n, b0 = lists[u], len(lists[u]), off[u] + u
        ex = set(xidx[xoff[u]:xoff[u + 1]].tolist()) if exclusion else set()
        for e in range(off[u], off[u + 1]):
            s = scores[u, idx[e]]
            if idx[e] in ex and not np.isnan(s):
                lo = int(np.searchsorted(v, s, "left"))
                bins[b0 + lo] -= 1; ties[b0 + lo] -= 1
    for u in range(U):
        v, n, b0 = lists[u], len(lists[u]), off[u] + u
        if n == 0:
            continue
        S = np.cumsum(bins[b0:b0 + n + 1][::-1])[::-1]
        ex = set(xidx[xoff[u]:xoff[u + 1]].tolist()) if exclusion else set()
        for e in range(off[u], off[u + 1]):
            s = scores[u, idx[e]]
            if np.isnan(s):
                continue
            lo, hi = int(np.searchsorted(v, s, "left")), int(np.searchsorted(v, s, "right"))
            above[e] = S[hi] + (n - hi)
            tied[e] = ties[b0 + lo] + (hi - lo) - (0 if idx[e] in ex else 1)
    assert np.array_equal(above, want[0]) and np.array_equal(tied, want[1])
