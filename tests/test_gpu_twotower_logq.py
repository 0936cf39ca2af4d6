"""-m gpu: TwoTower with candidate_sampling_probability (the log-Q correction of tfrs.tasks.Retrieval) through the engine,
the model and the row-sharded engine, against the float64 step of tests/test_gpu_twotower_hard.py with the correction added.

The float64 step: that file's, with the logits q c^T / temperature - b, b = float32(log(clip(p, 1e-6, 1)))[item] (the table the engine
stores), before the mask and the selection (tests/test_softmax_logq_cpu.py::logq_reference's order).  The item tower is applied once per
table row.  p = the item frequency of the test's batches (TwoTowerModel.itemFrequencies); the two reserved rows have p = 1.  Tolerances:
those of test_twotower_step_vs_golden (tests/test_gpu_twotower_bpr.py)."""
import os
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import binrec_oracle as O
from tests.test_gpu_twotower_hard import B, E, I, S, U, _batch, _free_port, _ids, _info, _load, _params
from tests.test_softmax_hard_cpu import hard_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = [(None, None), (5, None), (5, 0.25)]


def _m(name):
    return import_module("binary-recommendation_amd." + name)


def _freq(batches):
    """p of every row of the item table from the batches' item indices: count / total, the reserved rows 1 (as the model forms it)"""
    cnt = np.bincount(np.concatenate([i for _u, i in batches]), minlength=I + 2).astype(np.float64)
    p = cnt / cnt.sum()
    p[:2] = 1.0
    return p


def _logq32(p):
    return np.log(np.clip(np.asarray(p, np.float64), 1e-6, 1.0)).astype(np.float32)


def _loss64(par, u, i, M, tau, bq):
    """-> (loss, dq, dc, eu, ei, q) of one batch in float64; bq: the float32 log-Q table (None: no correction)"""
    f = lambda x: np.asarray(x, np.float64)
    eu, ei = f(par["user_emb"])[u], f(par["item_emb"])[i]
    q = eu @ f(par["Wu"]) + f(par["bu"])
    c_tab = f(par["item_emb"]) @ f(par["Wi"]) + f(par["bi"])
    t = tau if tau is not None else 1.0
    qs = q / t
    tab = qs @ c_tab.T - (0.0 if bq is None else f(bq)[None, :])
    r = hard_reference(qs, c_tab[i], i, i, 0, M, scores=tab[:, i])
    return r["loss"], r["dq"] / t, r["dc"], eu, ei, q


def _step64(par, acc, u, i, M, tau, bq, lr=0.1):
    f = lambda x: np.asarray(x, np.float64)
    loss, dq, dc, eu, ei, q = _loss64(par, u, i, M, tau, bq)
    g = {"Wu": eu.T @ dq, "bu": dq.sum(0), "Wi": ei.T @ dc, "bi": dc.sum(0)}
    rg = {"user_emb": dq @ f(par["Wu"]).T, "item_emb": dc @ f(par["Wi"]).T}
    for k, ids in (("user_emb", u), ("item_emb", i)):
        par[k], acc[k] = O.adagrad_sparse(par[k], acc[k], ids, rg[k], lr)
    for k in ("Wu", "bu", "Wi", "bi"):
        par[k], acc[k] = O.adagrad_dense(f(par[k]), acc[k], g[k], lr)
    return loss, g, rg, q


def _three_batches(seed):
    rng = np.random.default_rng(seed)
    return [_batch(rng, B) for _ in range(3)]


@pytest.mark.parametrize("M,tau", OPTIONS)
def test_engine_steps_vs_float64(dev, M, tau):
    tt = _m("two_tower")
    batches = _three_batches(21)
    p = _freq(batches)
    p32 = _params(5)
    eng = tt.TwoTowerEngine(E, I, U, S, dev, B, lr=0.1, num_hard_negatives=M, temperature=tau, candidate_sampling_probability=p)
    bq = _logq32(p)
    assert np.array_equal(eng.cand_log_q.cpu().numpy(), bq) and bq[0] == 0 and bq[1] == 0
    _load(eng, p32, dev)
    par = {k: v.astype(np.float64) for k, v in p32.items()}
    acc = {k: np.full(v.shape, 0.1) for k, v in par.items()}
    uncorrected_differs = False
    for u, i in batches:
        uncorrected_differs |= abs(_loss64(par, u, i, M, tau, None)[0] - _loss64(par, u, i, M, tau, bq)[0]) > 1e-3
        eng.train_step(_ids(u, dev), _ids(i, dev))
        torch.cuda.synchronize(); eng.check_ids()
        loss, g, rg, q = _step64(par, acc, u, i, M, tau, bq)
        np.testing.assert_allclose(eng.q[:B].cpu().numpy(), q, rtol=1e-5, atol=5e-6 * np.abs(q).max())
        got = eng.pop_loss()
        assert abs(got - loss) <= 1e-5 * abs(loss), (got, loss)
        for tower, (kw, kb) in (("user", ("Wu", "bu")), ("item", ("Wi", "bi"))):
            ref = np.concatenate([g[kw].reshape(-1), g[kb]])
            np.testing.assert_allclose(eng._gW(tower).cpu().numpy(), ref, rtol=1e-4, atol=2e-4 * np.abs(ref).max())
        np.testing.assert_allclose(eng.deu[:B].cpu().numpy(), rg["user_emb"], rtol=1e-4, atol=1e-5 * np.abs(rg["user_emb"]).max())
        np.testing.assert_allclose(eng.dei[:B].cpu().numpy(), rg["item_emb"], rtol=1e-4, atol=1e-5 * np.abs(rg["item_emb"]).max())
        for k in ("item_emb", "user_emb"):
            have = getattr(eng, k).cpu().numpy()
            np.testing.assert_allclose(have, par[k], rtol=1e-5, atol=2e-3 * 0.1)
            assert np.median(np.abs(have - par[k])) <= 1e-7
        np.testing.assert_allclose(eng.W("item")[0].cpu().numpy(), par["Wi"], rtol=1e-5, atol=2e-3 * 0.1)
    assert uncorrected_differs                                    # the correction changes the loss: a step that ignores it would not pass


def _model(dev, **kw):
    return _m("models").TwoTowerModel(E, I, U, "CUSTOMER_ID", "MATERIAL", [f"u{k}" for k in range(U)], [f"m{k}" for k in range(I)], semb=S, max_batch=B,
                                      device=str(dev), **kw)


@pytest.mark.parametrize("M,tau", OPTIONS)
def test_model_losses_use_the_correction(dev, M, tau):
    batches = _three_batches(22)
    infos = [_info(u, i) for u, i in batches]
    plain = _model(dev)
    freq = plain.itemFrequencies(infos)                           # aligned with itemsId
    p = _freq(batches)
    assert np.array_equal(freq, p[2:]) and abs(freq.sum() - 1) < 1e-12
    m = _model(dev, numHardNegatives=M, temperature=tau, candidateSamplingProbability=freq)
    bq = _logq32(p)
    assert np.array_equal(m.engine.cand_log_q.cpu().numpy(), bq)
    by_name = _model(dev, candidateSamplingProbability={f"m{k}": freq[k] for k in range(I)})
    assert torch.equal(by_name.engine.cand_log_q, m.engine.cand_log_q)
    p32 = _params(6)
    _load(m.engine, p32, dev)
    u, i = batches[0]
    info = infos[0]
    par = {k: v.astype(np.float64) for k, v in p32.items()}
    want = _loss64(par, u, i, M, tau, bq)[0]
    assert abs(want - _loss64(par, u, i, M, tau, None)[0]) > 1e-3
    q, c = m.computeEmb(info)
    l_tfrs = float(m.computeLossTfrs(q.clone(), c.clone(), info))
    m.engine.test_step(_ids(u, dev), _ids(i, dev))
    l_engine = m.engine.pop_loss()
    assert abs(l_tfrs - l_engine) <= 1e-6 * abs(l_engine), (l_tfrs, l_engine)      # computeLossTfrs == the engine's test_step loss
    l_step = float(m.train_step(info)["loss"])
    for got in (l_tfrs, l_engine, l_step):
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    m.engine.check_ids()
    with pytest.raises(ValueError):
        _model(dev, rdZero=True, resKey="RATING_TYPE", candidateSamplingProbability=freq)


def test_graph_replay_equals_eager_and_takes_a_new_table_in_place(dev):
    tt = _m("two_tower")
    rng = np.random.default_rng(23)
    batches = [_batch(rng, B) for _ in range(6)]
    p1 = _freq(batches[:3])
    p2 = np.roll(p1[2:], 7)
    p2 = np.concatenate([[1.0, 1.0], p2])
    engs = [tt.TwoTowerEngine(E, I, U, S, dev, B, lr=0.1, init_seed=3, num_hard_negatives=5, temperature=0.25, candidate_sampling_probability=p1) for _ in range(3)]
    engs[1].enable_graph(B)
    engs[2].enable_graph(B)
    losses = [[], [], []]
    for n, (u, i) in enumerate(batches):
        if n == 4:                                                # between two replays: in place, the graph stays
            graph = engs[1]._graph["graph"]
            table = engs[1].cand_log_q.data_ptr()
            for e in engs[:2]:
                e.set_candidate_sampling_probability(p2)
            assert engs[1]._graph is not None and engs[1]._graph["graph"] is graph and engs[1].cand_log_q.data_ptr() == table
        for k, e in enumerate(engs):
            e.train_step(_ids(u, dev), _ids(i, dev))
            torch.cuda.synchronize()
            losses[k].append(e.pop_loss())
    assert engs[1]._graph["graph"] is not None
    assert losses[0] == losses[1]
    assert losses[2][:4] == losses[0][:4] and losses[2][4] != losses[0][4]       # the new table changes the next step
    for name in engs[0]._state_names() + ["dq", "dc", "lse", "thr_score", "thr_pos", "q_t", "logq_b", "cand_log_q"]:
        assert torch.equal(getattr(engs[0], name), getattr(engs[1], name)), name
    engs[1].set_candidate_sampling_probability(None)              # turning the option off drops the graph
    assert engs[1]._graph is None and engs[1].cand_log_q is None
    eng = tt.TwoTowerEngine(E, I, U, S, dev, B)
    eng.enable_graph(B)
    eng.set_candidate_sampling_probability(p1)                    # ... and so does turning it on
    assert eng._graph is None and np.array_equal(eng.cand_log_q.cpu().numpy(), _logq32(p1))


def test_state_dict_round_trip(dev):
    tt = _m("two_tower")
    p = _freq(_three_batches(24))
    off = tt.TwoTowerEngine(E, I, U, S, dev, B, init_seed=4)
    assert "cand_log_q" not in off.state_dict()                  # without the option: the state dict of before
    assert sorted(off.state_dict()) == sorted(["t"] + off._state_names())
    on = tt.TwoTowerEngine(E, I, U, S, dev, B, init_seed=4, candidate_sampling_probability=p)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in on.state_dict().items()}
    assert np.array_equal(sd["cand_log_q"].cpu().numpy(), _logq32(p))
    fresh = tt.TwoTowerEngine(E, I, U, S, dev, B, init_seed=9)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.cand_log_q, on.cand_log_q)
    u, i = _batch(np.random.default_rng(25), B)
    for e in (on, fresh):
        e.test_step(_ids(u, dev), _ids(i, dev))
    assert on.pop_loss() == fresh.pop_loss()
    off.load_state_dict(off.state_dict())
    assert off.cand_log_q is None


def test_out_of_range_item_raises_the_flag_and_faults_nothing(dev):
    tt = _m("two_tower")
    p = _freq(_three_batches(26))
    eng = tt.TwoTowerEngine(E, I, U, S, dev, B, candidate_sampling_probability=p)
    u, i = _batch(np.random.default_rng(27), B)
    i = i.copy()
    i[5] = I + 2 + 1000                                           # past the item table and past the log-Q table
    eng.test_step(_ids(u, dev), _ids(i, dev))
    torch.cuda.synchronize()
    assert eng.logq_b[5].item() == 0.0                            # the gather gives a zero row
    with pytest.raises(IndexError):
        eng.check_ids()
    eng.pop_loss()
    u, i = _batch(np.random.default_rng(28), B)
    eng.test_step(_ids(u, dev), _ids(i, dev))                     # the engine goes on
    torch.cuda.synchronize(); eng.check_ids()
    assert np.isfinite(eng.pop_loss())


def test_serving_is_unchanged_by_the_option(dev):
    tt, ops = _m("two_tower"), _m("ops")
    p = _freq(_three_batches(29))
    a = tt.TwoTowerEngine(E, I, U, S, dev, B, init_seed=6)
    b = tt.TwoTowerEngine(E, I, U, S, dev, B, init_seed=6, candidate_sampling_probability=p)
    for name in a._state_names():
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    users = torch.arange(2, 42, dtype=torch.int32, device=dev)
    ra, rb = a.recommend(users, 10), b.recommend(users, 10)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    rng = np.random.default_rng(30)
    truth = ops.truth_csr(40, np.repeat(np.arange(40), 2), rng.integers(0, I + 2, 80), dev)
    ma, mb = a.rank_metrics(users, truth), b.rank_metrics(users, truth)
    assert sorted(ma) == sorted(mb)
    for k in ma:
        assert torch.equal(ma[k], mb[k]), k


# ------------------------------------------------------------------------------------------------------ two spawned ranks
def _sharded_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from tests import test_gpu_twotower_logq as T
        par_m, tt = T._m("parallel"), T._m("two_tower")
        dev = torch.device("cuda:0")
        ctx = par_m.DistCtx()
        Bl = B // world
        p32 = _params(7)
        u, i = _batch(np.random.default_rng(15), B)
        p = T._freq([(u, i)])
        bq = T._logq32(p)
        sl = slice(rank * Bl, (rank + 1) * Bl)
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        Eng = par_m.make_sharded_two_tower(tt.TwoTowerEngine)
        for M, tau in OPTIONS:
            eng = Eng(E, I, U, S, dev, Bl, ctx, full_tables={k: torch.from_numpy(p32[k]) for k in ("user_emb", "item_emb")}, lr=0.1,
                      num_hard_negatives=M, temperature=tau, candidate_sampling_probability=p)
            assert eng.cand_log_q.shape[0] == I + 2                  # the table is replicated, not sharded
            Wu, bu = eng.W("user"); Wi, bi = eng.W("item")
            Wu.copy_(td(p32["Wu"])); bu.copy_(td(p32["bu"])); Wi.copy_(td(p32["Wi"])); bi.copy_(td(p32["bi"]))
            eng.train_step(_ids(u[sl], dev), _ids(i[sl], dev))
            torch.cuda.synchronize(); eng.check_ids()
            par = {k: v.astype(np.float64) for k, v in p32.items()}
            acc = {k: np.full(v.shape, 0.1) for k, v in par.items()}
            uncorrected = T._loss64(par, u, i, M, tau, None)[0]
            loss, g, rg, q = T._step64(par, acc, u, i, M, tau, bq)      # ONE global batch
            assert abs(uncorrected - loss) > 1e-3
            np.testing.assert_allclose(eng.q[:Bl].cpu().numpy(), q[sl], rtol=1e-5, atol=5e-6 * np.abs(q).max())
            tot = torch.tensor([eng.loss_slots.sum().item()], dtype=torch.float64)
            dist.all_reduce(tot)
            assert abs(tot.item() - loss) <= 1e-5 * abs(loss), (M, tau, tot.item(), loss)
            np.testing.assert_allclose(eng.deu[:Bl].cpu().numpy(), rg["user_emb"][sl], rtol=1e-4, atol=1e-5 * np.abs(rg["user_emb"]).max())
            np.testing.assert_allclose(eng.dei[:Bl].cpu().numpy(), rg["item_emb"][sl], rtol=1e-4, atol=1e-5 * np.abs(rg["item_emb"]).max())
            gref = np.concatenate([g["Wu"].reshape(-1), g["bu"], g["Wi"].reshape(-1), g["bi"]])
            np.testing.assert_allclose(eng.grad.cpu().numpy(), gref, rtol=1e-4, atol=2e-4 * np.abs(gref).max())
            got = eng.item_emb.cpu().numpy()
            ref_t = par["item_emb"][rank::world]
            np.testing.assert_allclose(got[: ref_t.shape[0]], ref_t, rtol=1e-5, atol=2e-3 * 0.1)
        out.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        out.put((rank, "FAIL: " + traceback.format_exc()[-1800:]))
    finally:
        try:
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001
            pass


def test_sharded_engine_on_two_ranks_equals_the_global_float64_step(dev):
    world, port = 2, _free_port()
    ctxm = mp.get_context("spawn")
    out = ctxm.Queue()
    procs = [ctxm.Process(target=_sharded_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [out.get(timeout=240) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
        for p in procs:      # never leave a child behind
            if p.is_alive():
                p.kill()
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}: {r[1]}"
