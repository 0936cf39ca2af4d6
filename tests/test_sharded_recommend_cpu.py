"""-m "not gpu": the rules behind the catalogue top-k of the row-sharded engines (include/binrec.h brCsrSplitByOwner /
brTopKListsMerge, parallel.py recommend_at_owners), restated in numpy and checked on hand-made cases; the GPU tests
(test_gpu_sharded_recommend.py) hold the kernels to these restatements.

  split_ref : an exclusion CSR over the global candidate list -> one owner's CSR in its local positions
  topk_ref  : brTopKRowsExclude's selection (score desc, ties to the lower position, strict >, (-inf, -1) pads)
  merge_ref : W lists of k (score, local position) entries with ascending local -> global maps -> one list of k (score, global
              position) entries under the same compare

and the argument that makes the sharded result equal the single-device one: the candidates dealt r::W, top-k per part, split + map +
merge == top-k of the whole list, entry for entry."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

NEG_INF = np.float32(-np.inf)


def beats(s, p, ts, tp):
    """csrc/topk_list.h: strict >, ties keep the lower position (False whenever s is NaN)"""
    return bool(s > ts or (s == ts and p < tp))


def split_ref(off, idx, g2l):
    """rows of (off, idx) restricted to the positions with g2l >= 0, renamed to g2l's local positions, order kept"""
    out_off, out_idx = [0], []
    for u in range(len(off) - 1):
        for g in idx[off[u]:off[u + 1]]:
            if 0 <= g < len(g2l) and g2l[g] >= 0:
                out_idx.append(int(g2l[g]))
        out_off.append(len(out_idx))
    return np.asarray(out_off, np.int64), np.asarray(out_idx, np.int32)


def _insert(lst, k, s, p):
    """offer (s, p) to a list sorted by `beats`, at most k entries"""
    pos = sum(1 for (ls, lp) in lst if beats(ls, lp, s, p))
    if pos < k and not np.isnan(s):
        lst.insert(pos, (s, p))
        del lst[k:]


def _pad(lst, k):
    s = np.full(k, NEG_INF, np.float32)
    p = np.full(k, -1, np.int32)
    for e, (ls, lp) in enumerate(lst):
        s[e], p[e] = ls, lp
    return s, p


def topk_ref(scores, k, off=None, idx=None):
    """scores (U, I) -> (U, k) scores / positions: brTopKRowsExclude"""
    U, I = scores.shape
    S, P = np.empty((U, k), np.float32), np.empty((U, k), np.int32)
    for u in range(U):
        ex = set(idx[off[u]:off[u + 1]].tolist()) if off is not None else ()
        lst = []
        for p in range(I):
            if p not in ex:
                _insert(lst, k, scores[u, p], p)
        S[u], P[u] = _pad(lst, k)
    return S, P


def merge_ref(scores, pos, maps, k):
    """scores / pos (W, U, k), maps[w] = ascending local -> global positions of list w -> (U, k) scores / GLOBAL positions"""
    W, U, _ = scores.shape
    S, P = np.empty((U, k), np.float32), np.empty((U, k), np.int32)
    for u in range(U):
        lst = []
        for w in range(W):
            for e in range(k):
                lp = pos[w, u, e]
                if 0 <= lp < len(maps[w]):           # -1: that shard ran out of candidates
                    _insert(lst, k, scores[w, u, e], int(maps[w][lp]))
        S[u], P[u] = _pad(lst, k)
    return S, P


def owner_maps(items, W):
    """positions p of `items` with items[p] mod W == r in ascending p, for every r; and the inverse map of each"""
    items = np.asarray(items)
    maps = [np.flatnonzero(items % W == r).astype(np.int32) for r in range(W)]
    g2l = []
    for m in maps:
        g = np.full(len(items), -1, np.int32)
        g[m] = np.arange(len(m), dtype=np.int32)
        g2l.append(g)
    return maps, g2l


def sharded_topk_ref(scores, items, W, k, off=None, idx=None):
    """top-k per owner on its columns + split + merge: what recommend_at_owners computes"""
    maps, g2l = owner_maps(items, W)
    U = scores.shape[0]
    Ss, Ps = np.full((W, U, k), NEG_INF, np.float32), np.full((W, U, k), -1, np.int32)
    for r in range(W):
        if len(maps[r]):
            lo, li = split_ref(off, idx, g2l[r]) if off is not None else (None, None)
            Ss[r], Ps[r] = topk_ref(scores[:, maps[r]], k, lo, li)
    return merge_ref(Ss, Ps, maps, k)


# ------------------------------------------------------------------------------------------------------------ hand-made cases
def test_split_hand_made():
    # 7 candidates dealt over 3 owners by id = position: owner 1 holds positions 1, 4 -> local 0, 1
    _maps, g2l = owner_maps(np.arange(7), 3)
    off = np.array([0, 3, 3, 7, 8], np.int64)                 # row 1 is empty
    idx = np.array([0, 1, 4, 1, 2, 3, 6, 5], np.int32)
    o, i = split_ref(off, idx, g2l[1])
    assert o.tolist() == [0, 2, 2, 3, 3] and i.tolist() == [0, 1, 0]          # row 3 has nothing of owner 1: emptied
    o, i = split_ref(off, idx, g2l[0])                                        # owner 0: positions 0, 3, 6 -> 0, 1, 2
    assert o.tolist() == [0, 1, 1, 3, 3] and i.tolist() == [0, 1, 2]
    o, i = split_ref(off, idx, g2l[2])                                        # owner 2: positions 2, 5 -> 0, 1
    assert o.tolist() == [0, 0, 0, 1, 2] and i.tolist() == [0, 1]
    # one owner (W = 1): the CSR itself
    _m, g1 = owner_maps(np.arange(7), 1)
    o, i = split_ref(off, idx, g1[0])
    assert o.tolist() == off.tolist() and i.tolist() == idx.tolist()
    # a candidate list in non-id order: ids [5, 2, 8, 3] on 2 owners -> owner 0 holds positions 1, 2; owner 1 positions 0, 3
    _m, g = owner_maps(np.array([5, 2, 8, 3]), 2)
    o, i = split_ref(np.array([0, 4], np.int64), np.array([0, 1, 2, 3], np.int32), g[1])
    assert o.tolist() == [0, 2] and i.tolist() == [0, 1]


def test_merge_ties_across_owners_go_to_the_lower_global_position():
    # two owners, k = 3; equal scores everywhere: the order is the global position alone
    maps = [np.array([0, 2, 4], np.int32), np.array([1, 3], np.int32)]
    s = np.full((2, 1, 3), 1.0, np.float32)
    p = np.array([[[0, 1, 2]], [[0, 1, -1]]], np.int32)
    s[1, 0, 2] = NEG_INF
    S, P = merge_ref(s, p, maps, 3)
    assert P.tolist() == [[0, 1, 2]] and S.tolist() == [[1.0, 1.0, 1.0]]
    # a higher score on the later owner wins whatever its position
    s[1, 0, 1] = 2.0
    S, P = merge_ref(s, p, maps, 3)
    assert P.tolist() == [[3, 0, 1]] and S.tolist() == [[2.0, 1.0, 1.0]]


def test_merge_padding_never_wins_and_fills_the_tail():
    maps = [np.array([0, 3], np.int32), np.array([1], np.int32), np.array([2], np.int32)]
    k = 4                                                     # larger than every shard
    s = np.full((3, 1, k), NEG_INF, np.float32)
    p = np.full((3, 1, k), -1, np.int32)
    s[0, 0, :2], p[0, 0, :2] = [0.5, -1.5], [1, 0]
    s[1, 0, :1], p[1, 0, :1] = [-2.0], [0]
    # owner 2: everything excluded -> an all-pad list
    S, P = merge_ref(s, p, maps, k)
    assert P.tolist() == [[3, 0, 1, -1]] and S[0, :3].tolist() == [0.5, -1.5, -2.0] and S[0, 3] == NEG_INF
    # a REAL candidate whose score is -inf is an entry (it beats a pad, as in brTopKRows); a pad with a finite score is still a pad
    s[2, 0, 0], p[2, 0, 0] = NEG_INF, 0
    s[1, 0, 1], p[1, 0, 1] = 9.0, -1
    S, P = merge_ref(s, p, maps, k)
    assert P.tolist() == [[3, 0, 1, 2]] and S[0, 3] == NEG_INF
    # no entry at all: an all-pad result
    S, P = merge_ref(np.full((3, 1, k), NEG_INF, np.float32), np.full((3, 1, k), -1, np.int32), maps, k)
    assert P.tolist() == [[-1] * k] and np.all(S == NEG_INF)


def test_merge_nan_keeps_the_place_beats_gives_it():
    # `beats` is False for a NaN candidate: it never enters a list (brTopKRows does the same)
    maps = [np.array([0, 1], np.int32)]
    S, P = merge_ref(np.array([[[np.nan, 1.0]]], np.float32), np.array([[[0, 1]]], np.int32), maps, 2)
    assert P.tolist() == [[1, -1]] and S[0, 0] == 1.0 and S[0, 1] == NEG_INF


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [1, 4, 40])
def test_sharded_selection_equals_the_whole_catalogue(W, k):
    """scores with many ties, candidate ids in non-id order, exclusion lists that empty whole shards and whole rows, k above the shard
    size: top-k per owner + split + merge == top-k of the whole list"""
    rng = np.random.default_rng(100 * W + k)
    U, I = 9, 37
    scores = rng.integers(-3, 4, (U, I)).astype(np.float32)          # 7 distinct values over 37 columns: ties everywhere
    scores[1, :5] = NEG_INF
    items = rng.permutation(4 * I)[:I]
    rows = []
    for u in range(U):
        if u == 0:
            rows.append(np.arange(I))                                  # everything excluded
        elif u == 2:
            rows.append(np.empty(0, np.int64))                         # an empty row
        elif u == 3:
            rows.append(np.flatnonzero(items % W == 0))                # empties owner 0
        else:
            rows.append(np.sort(rng.choice(I, rng.integers(0, I), replace=False)))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    want = topk_ref(scores, k, off, idx)
    got = sharded_topk_ref(scores, items, W, k, off, idx)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])
    want = topk_ref(scores, k)
    got = sharded_topk_ref(scores, items, W, k)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


# ------------------------------------------------------------------------------------------------------------ the C-ABI surface
NEW = ("brCsrSplitByOwnerWorkspaceBytes", "brCsrSplitByOwner", "brTopKListsMerge")


def test_new_entry_points_are_declared_bound_and_exported():
    lib = import_module("binary-recommendation_amd._lib")
    ops = import_module("binary-recommendation_amd.ops")
    par = import_module("binary-recommendation_amd.parallel")
    protos = lib.parse_header()
    assert set(NEW) <= set(protos), set(NEW) - set(protos)
    assert protos["brCsrSplitByOwnerWorkspaceBytes"][0] is ctypes.c_int64
    assert protos["brTopKListsMerge"][2] == ["scores", "index", "list_stride", "user_stride", "n_lists", "n_users", "k", "l2g", "l2g_off",
                                             "out_scores", "out_index", "stream"]
    assert callable(ops.csr_split_by_owner) and callable(ops.topk_lists_merge) and callable(par.recommend_at_owners)
    built = import_module("binary-recommendation_amd.build").build_library(verbose=False)
    cdll = ctypes.CDLL(built)
    for name in NEW:
        assert hasattr(cdll, name), name


def test_new_entry_points_refuse_bad_sizes_before_any_launch():
    import_module("binary-recommendation_amd.build").build_library(verbose=False)
    h = import_module("binary-recommendation_amd._lib").load()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its argument check first
    assert h.brTopKListsMerge(None, None, 0, 1, 1, 1, 1, None, None, None, None, None) == -1 and b"brTopKListsMerge" in h.brGetLastError()
    for k in (0, 257):
        assert h.brTopKListsMerge(one, one, 0, 300, 2, 1, k, one, one, one, one, None) == -1
    assert h.brTopKListsMerge(one, one, 0, 4, 0, 1, 4, one, one, one, one, None) == -1           # no list
    assert h.brTopKListsMerge(one, one, 0, 3, 2, 1, 4, one, one, one, one, None) == -1           # user_stride < k
    assert h.brTopKListsMerge(one, one, 0, 4, 64, 0, 4, one, one, one, one, None) == 0           # no user: nothing to launch
    assert h.brCsrSplitByOwner(None, None, 1, None, 1, None, None, None, 0, None) == -1 and b"brCsrSplitByOwner" in h.brGetLastError()
    assert h.brCsrSplitByOwner(one, one, 1, one, 1 << 31, one, one, one, 1 << 20, None) == -1    # n_global >= 2^31
    assert h.brCsrSplitByOwner(one, one, 4, one, 10, ctypes.c_void_p(16), ctypes.c_void_p(24), one, 8, None) == -4    # workspace too small
    assert h.brCsrSplitByOwnerWorkspaceBytes(-1) == -1 and h.brCsrSplitByOwnerWorkspaceBytes(0) == 0
    assert h.brCsrSplitByOwnerWorkspaceBytes(33) == 512
