"""-m gpu: the full-catalogue AUC of the row-sharded engines, counted where the item rows live (csrc/auc_owner.hip, parallel.py
auc_at_owners).

One process, W virtual ranks (the pattern of test_gpu_sharded_recommend.py): the candidate list is dealt to W owners by id mod W on one
device and the four phases run per part - brCsrSplitByOwner + brDotAucOwnerPositives, brAucSortPieces over the pieces of all parts,
brDotAucOwnerCount, brAucFinalizeLists over the W partial counts.  The result must equal the launch over the whole list
(ops.dot_auc_for(dim)) BIT FOR BIT with the same NaN mask, and the numpy restatement of test_sharded_auc_cpu.py on the whole launch's
dumped scores: no tolerance in this file but the float64 comparison's 1e-6 (test_gpu_auc_dot.py::test_scale_against_float64's bar).

Two ranks on one card over gloo (child processes, each under its own time limit, never run again): ShardedBPREngine.full_auc(catalog=
"owners") returns for each rank's users what the single-device engine returns, and BPRModel.full_auc under the group the same float."""
import importlib.util
import os
import socket
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("test_sharded_auc_cpu")        # owner_maps / built_users / sharded_auc_ref: the numpy restatement


def _m(name):
    return import_module("binary-recommendation_amd." + name)


def _equal(a, b):
    """bit for bit, NaN in the same places"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


def _through_owners(dev, W, items, Q, rows_of, off, idx, force_wide=False, order=None, dump=None, pad=0):
    """the four phases over the W parts of `items` (rows_of(positions) -> that part's candidate rows) -> (auc (U,), sorted, pcnt).
    order: the order the owners' pieces lie in the sort's input; dump: the whole launch's (U, I) scores, every part's dump_scores is held
    to its columns; pad: extra entries between the owners' partial counts (the finalize reads a strided buffer)"""
    ops = _m("ops")
    maps, g2l = R.owner_maps(items, W)
    toff, tidx = torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev)
    U, T = Q.shape[0], len(idx)
    parts, raws, lens = {}, [], []
    for r in range(W):
        if len(maps[r]) == 0:               # an owner without a candidate of the list: no piece, a zero count
            raws.append(torch.empty(0, device=dev)); lens.append(torch.zeros(U, dtype=torch.int64, device=dev))
            continue
        C = rows_of(maps[r].astype(np.int64))
        po, pi = ops.csr_split_by_owner(toff, tidx, torch.from_numpy(g2l[r]).to(dev))
        raw = ops.dot_auc_owner_positives(Q, C, po, pi, force_wide=force_wide)
        parts[r] = (C, po, pi)
        raws.append(raw[:int(po[-1])]); lens.append(po[1:] - po[:-1])
    # the all-gather's receive buffer: one row per owner, padded to the longest piece
    order = list(range(W)) if order is None else list(order)
    m = max(1, max(x.numel() for x in raws))
    buf = torch.full((W, m), 123.0, device=dev)
    piece_off = torch.zeros(W, U + 1, dtype=torch.int64, device=dev)
    for slot, r in enumerate(order):
        buf[slot, :raws[r].numel()] = raws[r]
        piece_off[slot, 1:] = lens[r].cumsum(0)
        piece_off[slot] += slot * m
    sorted_, pcnt = ops.auc_sort_pieces(buf, piece_off, toff, T)
    stride = U + pad
    w2 = torch.full((W * stride,), 7, dtype=torch.int64, device=dev)       # (the pads must never be read)
    for r in range(W):
        if r in parts:
            C, po, pi = parts[r]
            got = ops.dot_auc_owner_count(Q, C, po, pi, toff, sorted_, pcnt, dump_scores=dump is not None, force_wide=force_wide)
            if dump is not None:
                got, d = got
                assert torch.equal(d.view(torch.int32), dump[:, torch.from_numpy(maps[r].astype(np.int64)).to(dev)].contiguous().view(torch.int32))
            w2[r * stride:r * stride + U] = got
        else:
            w2[r * stride:r * stride + U] = 0
    return ops.auc_finalize_lists(w2, W, U, toff, pcnt, len(items), list_stride=stride), sorted_, pcnt


def _table(rng, rows, dim, dev):
    T = torch.from_numpy(rng.standard_normal((rows, dim)).astype(np.float32)).to(dev)
    T[200:900] = T[(torch.arange(200, 900, device=dev) % 5)]        # duplicated rows on every owner: equal scores everywhere
    return T


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("dim,idt", [(64, torch.int32), (50, torch.int64), (350, torch.int64), (129, torch.int32)])
def test_virtual_ranks_equal_the_whole_catalogue(dev, W, dim, idt):
    """a shuffled subset of the rows as candidates; the built users (no positives, every candidate, all on owner 0, all on the last
    owner, P > 64 and P > 2048: the multi-chunk sort and the lists past the LDS cap); every part's dump against the whole dump"""
    ops = _m("ops")
    rng = np.random.default_rng(7 * W + dim)
    rows, I = 4000, 2600
    T = _table(rng, rows, dim, dev)
    items = rng.permutation(rows)[:I]
    ids = torch.as_tensor(items, dtype=idt, device=dev)
    off, idx = R.built_users(rng, items, W, big=(100, 2100))
    U = len(off) - 1
    assert (np.diff(off)[-2:] == [100, 2100]).all() and np.diff(off)[0] == 0 and np.diff(off)[1] == I
    Q = torch.from_numpy(rng.standard_normal((U, dim)).astype(np.float32)).to(dev)
    C = ops.gather_rows([T], [ids])[0]
    toff, tidx = torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev)
    want, dump = ops.dot_auc_for(dim)(Q, C, toff, tidx, dump_scores=True)
    rows_of = lambda pos: ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
    got, _s, pcnt = _through_owners(dev, W, items, Q, rows_of, off, idx, dump=dump, pad=3)
    assert torch.isnan(want[:2]).all() and not torch.isnan(want[4:]).any()
    assert _equal(got, want), (got, want)
    assert pcnt.cpu().tolist() == np.diff(off).tolist()
    assert R.same_bits(got.cpu().numpy(), R.sharded_auc_ref(dump.cpu().numpy(), off, idx, items, W))


def test_an_owner_without_candidates(dev):
    """W = 8 over ids of three residue classes: five owners hold no candidate and send zeros"""
    ops = _m("ops")
    rng = np.random.default_rng(3)
    ids_all = np.concatenate([8 * np.arange(100), 8 * np.arange(100) + 1, 8 * np.arange(100) + 5])
    items = rng.permutation(ids_all)[:250]
    assert sum(len(m) == 0 for m in R.owner_maps(items, 8)[0]) == 5
    T = _table(rng, 1000, 64, dev)
    ids = torch.as_tensor(items, dtype=torch.int32, device=dev)
    off, idx = R.built_users(rng, items, 8, big=(100,))
    Q = torch.from_numpy(rng.standard_normal((len(off) - 1, 64)).astype(np.float32)).to(dev)
    want = ops.dot_catalog_auc(Q, ops.gather_rows([T], [ids])[0], torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev))
    rows_of = lambda pos: ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
    assert _equal(_through_owners(dev, 8, items, Q, rows_of, off, idx)[0], want)


@pytest.mark.parametrize("W,dim", [(2, 64), (3, 350)])
def test_ties_across_owners(dev, W, dim):
    """an item row under two ids of different residues, one copy a positive and the other not: the tie is counted on another owner than
    the one that scored the positive"""
    ops = _m("ops")
    rng = np.random.default_rng(W)
    I, U = 600, 40
    T = torch.from_numpy(rng.standard_normal((I, dim)).astype(np.float32)).to(dev)
    T[1:I:2] = T[0:I - 1:2]                                          # ids 2j and 2j + 1 share a row; (2j) % W != (2j + 1) % W
    items = rng.permutation(I)
    where = np.empty(I, np.int64); where[items] = np.arange(I)       # id -> position
    rows = []
    for u in range(U):
        j = rng.choice(I // 2, 12, replace=False)
        pos_ids, twin_ids = 2 * j + (u % 2), 2 * j + 1 - (u % 2)
        assert ((pos_ids % W) != (twin_ids % W)).all() and not set(pos_ids) & set(twin_ids)   # every user has such pairs
        rows.append(np.sort(where[pos_ids]))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    ids = torch.as_tensor(items, dtype=torch.int64, device=dev)
    Q = torch.from_numpy(rng.standard_normal((U, dim)).astype(np.float32)).to(dev)
    C = ops.gather_rows([T], [ids])[0]
    want, dump = ops.dot_auc_for(dim)(Q, C, torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev), dump_scores=True)
    d = dump.cpu().numpy()
    for u in range(U):                                                # the pair's scores are equal bits, one a positive, one not
        p = idx[off[u]:off[u + 1]]
        twins = where[items[p] ^ 1]
        assert np.array_equal(d[u, p].view(np.int32), d[u, twins].view(np.int32)) and not set(twins) & set(p)
    rows_of = lambda pos: ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
    assert _equal(_through_owners(dev, W, items, Q, rows_of, off, idx)[0], want)


@pytest.mark.parametrize("dim", [64, 350])
def test_non_finite_scores(dev, dim):
    """an item row with a NaN and one with an inf, each a positive of some users and a negative of the others, on different owners"""
    ops = _m("ops")
    rng = np.random.default_rng(dim)
    W, I, U = 3, 500, 24
    T = torch.from_numpy(rng.standard_normal((I, dim)).astype(np.float32)).to(dev)
    T[10, 3], T[11, 5], T[12, 0] = float("nan"), float("inf"), float("-inf")          # ids 10, 11, 12: owners 1, 2, 0
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
    ids = torch.as_tensor(items, dtype=torch.int32, device=dev)
    Q = torch.from_numpy(rng.standard_normal((U, dim)).astype(np.float32)).to(dev)
    C = ops.gather_rows([T], [ids])[0]
    want, dump = ops.dot_auc_for(dim)(Q, C, torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev), dump_scores=True)
    assert torch.isnan(dump[:, int(where[10])]).all() and torch.isinf(dump[:, int(where[11])]).all()
    rows_of = lambda pos: ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
    got, _s, pcnt = _through_owners(dev, W, items, Q, rows_of, off, idx, dump=dump)
    assert _equal(got, want)
    assert pcnt.cpu().tolist() == [int(n) - (u & 1) for u, n in enumerate(np.diff(off))]       # the NaN positive is dropped from the list
    assert R.same_bits(got.cpu().numpy(), R.sharded_auc_ref(dump.cpu().numpy(), off, idx, items, W))


def test_forced_wide_equals_narrow(dev):
    ops = _m("ops")
    rng = np.random.default_rng(11)
    W, I, dim = 3, 1500, 64
    T = _table(rng, 2000, dim, dev)
    items = rng.permutation(2000)[:I]
    ids = torch.as_tensor(items, dtype=torch.int32, device=dev)
    off, idx = R.built_users(rng, items, W, big=(100,))
    Q = torch.from_numpy(rng.standard_normal((len(off) - 1, dim)).astype(np.float32)).to(dev)
    rows_of = lambda pos: ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
    narrow, s_n, p_n = _through_owners(dev, W, items, Q, rows_of, off, idx)
    wide, s_w, p_w = _through_owners(dev, W, items, Q, rows_of, off, idx, force_wide=True)
    assert _equal(wide, narrow) and torch.equal(p_n, p_w)
    assert torch.equal(s_n[:len(idx)].view(torch.int32), s_w[:len(idx)].view(torch.int32))     # (no NaN here: every list is full)
    C = ops.gather_rows([T], [ids])[0]
    assert _equal(wide, ops.dot_catalog_auc_wide(Q, C, torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev), force_wide=True))


def test_sort_from_pieces_does_not_depend_on_their_order(dev):
    ops = _m("ops")
    rng = np.random.default_rng(13)
    W, I, dim = 8, 2600, 50
    T = _table(rng, 3000, dim, dev)
    T[7, 2] = float("nan")
    items = rng.permutation(3000)[:I]
    ids = torch.as_tensor(items, dtype=torch.int64, device=dev)
    off, idx = R.built_users(rng, items, W, big=(100, 2100))
    Q = torch.from_numpy(rng.standard_normal((len(off) - 1, dim)).astype(np.float32)).to(dev)
    rows_of = lambda pos: ops.gather_rows([T], [ids[torch.from_numpy(pos).to(dev)].contiguous()])[0]
    a, s_a, p_a = _through_owners(dev, W, items, Q, rows_of, off, idx)
    for order in (list(reversed(range(W))), rng.permutation(W).tolist()):
        b, s_b, p_b = _through_owners(dev, W, items, Q, rows_of, off, idx, order=order)
        assert torch.equal(p_a, p_b) and _equal(a, b)
        o, n = off, p_a.cpu().numpy()
        keep = torch.from_numpy(np.concatenate([np.arange(o[u], o[u] + n[u]) for u in range(len(n))])).to(dev)   # (past P': never written)
        assert torch.equal(s_a[keep], s_b[keep])
    # every list is ascending and is the multiset of the dumped positives' scores
    C = ops.gather_rows([T], [ids])[0]
    _auc, dump = ops.dot_catalog_auc(Q, C, torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev), dump_scores=True)
    d, s = dump.cpu().numpy(), s_a.cpu().numpy()
    for u in range(len(n)):
        assert np.array_equal(s[o[u]:o[u] + n[u]], R.sort_pieces_ref([d[u, idx[o[u]:o[u + 1]]]]))


def test_against_float64(dev):
    """test_gpu_auc_dot.py::test_scale_against_float64's case and bar through the owners: its tables (65 536 x 100 000, dim 64, P = 20,
    the same generator), its 256 sampled users, atol 1e-6.  The bar belongs to that shape: one pair whose order differs between the
    float32 and the float64 scores moves a user's AUC by 1 / (P N) = 5.0e-7 there; with fewer items the step of the statistic itself
    passes 1e-6 (at 20 000 items it is 2.5e-6) and the bound would measure the catalogue's size, not the kernels."""
    ops = _m("ops")
    A = _load("test_gpu_auc_dot")
    U, I, dim, P, W = 65536, 100000, 64, 20, 8
    g = torch.Generator(device=dev).manual_seed(6)
    Q = torch.empty(U, dim, device=dev).uniform_(-0.05, 0.05, generator=g)
    C = torch.empty(I, dim, device=dev).uniform_(-0.05, 0.05, generator=g)
    off, idx = A._truth(np.full(U, P), I, dev, seed=6)
    sample = np.random.default_rng(6).choice(U, 256, replace=False)
    o, x = off.cpu().numpy(), idx.cpu().numpy()
    so = np.r_[0, np.cumsum([o[u + 1] - o[u] for u in sample])].astype(np.int64)
    sx = np.concatenate([x[o[u]:o[u + 1]] for u in sample]).astype(np.int32)
    Qs = Q[torch.from_numpy(sample).to(dev)].contiguous()
    items = np.random.default_rng(6).permutation(I)                  # ids of the rows of C
    rows_of = lambda pos: C[torch.from_numpy(pos).to(dev)].contiguous()
    got = _through_owners(dev, W, items, Qs, rows_of, so, sx)[0]
    assert 1.0 / (P * (I - P)) < 1e-6
    want = A._auc64(Qs.double() @ C.double().T, torch.from_numpy(so), torch.from_numpy(sx))
    print("max |auc - float64| =", np.abs(got.double().cpu().numpy() - want).max())
    np.testing.assert_allclose(got.double().cpu().numpy(), want, rtol=0, atol=1e-6)
    assert _equal(got, ops.dot_catalog_auc(Qs, C, torch.from_numpy(so).to(dev), torch.from_numpy(sx).to(dev)))


# ------------------------------------------------------------------------------------------------------------ 2 ranks, gloo staging
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_truth(rng, n_users, n_items, dev):
    """a truth CSR over a rank's users: random lists, the first user without positives"""
    rows, cols = [], []
    for n in range(n_users):
        c = rng.choice(n_items, int(rng.integers(1, max(2, n_items // 4))), replace=False) if n != 0 else []
        rows += [n] * len(c); cols += list(c)
    return _m("ops").truth_csr(n_users, rows, cols, dev)


def _gathered_single(sh, world, U, I, dim, dev, idt):
    """the single-device engine holding the rows of the sharded engine `sh` as they are now (flushed)"""
    import torch.distributed as dist
    par, bpr = _m("parallel"), _m("bpr")
    shards = [None] * world
    dist.all_gather_object(shards, {k: getattr(sh, k).cpu() for k in ("user", "item")})
    single = bpr.BPREngine(U, I, dim, dev, 256, id_dtype=idt)
    for k, rows in (("user", U), ("item", I)):
        for r in range(world):
            getattr(single, "_" + k)[r::world] = shards[r][k][:par.shard_rows(rows, r, world)].to(dev)
    return single


def _check_engine(rank, world, ctx, dev):
    par, bpr, ops = _m("parallel"), _m("bpr"), _m("ops")
    G = _load("test_gpu_sharded_recommend")
    U, I = 60, 333
    for dim, idt in ((64, torch.int32), (350, torch.int64)):
        g = torch.Generator().manual_seed(dim)
        full = {"user": torch.randn(U, dim, generator=g) * 0.1, "item": torch.randn(I, dim, generator=g) * 0.1}
        full["item"][50:200] = full["item"][torch.arange(50, 200) % 4]          # ties across the two owners
        sh = par.make_sharded_bpr(bpr.BPREngine)(U, I, dim, dev, 256, ctx, full_tables=full, id_dtype=idt)
        # training steps first: the rows lag behind until a flush, which the owner path must do itself
        rng = np.random.default_rng(5 + rank)
        for _ in range(3):
            b = [torch.as_tensor(rng.integers(0, n, 64), dtype=idt, device=dev) for n in (U, I, I)]
            sh.train_step(*b)
        first = None
        for counts, how in (((13, 5), "perm"), ((7, 0), None), ((0, 9), "perm"), ((6, 4), "even"), ((2, 3), "one")):
            rng = np.random.default_rng(23 + len(how or ""))
            users = torch.as_tensor(G._rank_users(rng, rank, U, counts), dtype=idt, device=dev)
            items, n_it = G._items(rng, how, I, idt, dev)
            truth = _rank_truth(np.random.default_rng(200 + rank), counts[rank], n_it, dev)
            got = sh.full_auc(users, truth, items=items, catalog="owners")
            if first is None:
                first = (users, truth, items, got)
                single = _gathered_single(sh, world, U, I, dim, dev, idt)        # (after the first owner-side call: state_dict-like reads flush)
            assert got.shape == (counts[rank],) and got.dtype == torch.float32
            if counts[rank]:
                want = single.full_auc(users, truth, items=items)
                assert _equal(got, want), (dim, counts, how, got, want)
                assert torch.isnan(got[0])
            if min(counts):       # (today's path, unchanged: every candidate row to every rank)
                assert _equal(sh.full_auc(users, truth, items=items), got)
                assert _equal(sh.full_auc(users, truth, items=items, catalog="gather"), got)
        users, truth, items, got = first
        assert _equal(got, single.full_auc(users, truth, items=items))           # the call made on un-flushed tables
        sh.check_ids()
        # differing candidate lists raise on every rank
        bad = torch.arange(40 + rank, dtype=idt, device=dev)
        with pytest.raises(ValueError, match="same items"):
            sh.full_auc(users, _rank_truth(np.random.default_rng(1), users.shape[0], 40, dev), items=bad, catalog="owners")
        with pytest.raises(ValueError):
            sh.full_auc(users, truth, catalog="everywhere")
        with pytest.raises(NotImplementedError):
            sh.full_auc(users, truth, dump_scores=True, catalog="owners")


def _check_model(rank, world, ctx, dev):
    models = _m("models")
    U, I, dim = 50, 300, 64
    m = models.BPRModel(device="cuda:0", max_batch=256)
    m.compileModel(None, U, I, dim)
    assert hasattr(m.model, "ctx") and m.model.ctx.world == world
    m1 = models.BPRModel(device="cuda:0", max_batch=256)
    m1.model = _gathered_single(m.model, world, U, I, dim, dev, m.model.id_dtype)
    rng = np.random.default_rng(8)
    items = rng.permutation(I)[:150].tolist()
    rng = np.random.default_rng(80 + rank)
    gt = [(int(u), [items[j] for j in rng.choice(150, int(rng.integers(0, 30)), replace=False)]) for u in rng.integers(0, U, [9, 4][rank])]
    gt[0] = (gt[0][0], [items[3]])
    want = m1.full_auc(gt, items, method="fused")
    assert m.full_auc(gt, items, method="fused", catalog="owners") == want
    assert m.full_auc(gt, items, method="fused", catalog="gather") == want
    assert m.full_auc(gt, items, method="fused") == want
    with pytest.raises(ValueError):
        m1.full_auc(gt, items, method="fused", catalog="owners")     # a single-device model has no owners


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
def test_sharded_full_auc_two_ranks_one_gpu(dev, kind):
    """2 ranks (3 GPU processes with this one); every child has its own time limit and is never run again"""
    world, port = 2, _free_port()
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
