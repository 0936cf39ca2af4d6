"""-m gpu: the multi-step graph that builds the row index of the whole group in its first step (NeuMFEngine.enable_graph_multi where
brNeumfGroupIndexPlan > 0: the head's lookup launch sorts the chunks of all 2 S id streams, ONE chunk-rank launch ranks them, steps
2..S are the plain lookup with the step-state advance riding in their segment-partials launch) against single-step graph replays of the
same steps.  Same kernels on the same inputs in the same order per step, so everything is compared bit for bit.  Batch 16 400: just
over the 16 384 switch to the fused lookup + index path - three chunks of 8 192 per stream, the last holding 16 keys."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 16400
TAG_INDEX_USER = 10      # include/binrec.h BR_TAG_INDEX_USER: the fused lookup + index call of a step (two launches)


def _m(name):
    return import_module("binary-recommendation_amd." + name)


def _engines(dev, n, dim, idt, dropout, U, I):
    neumf = _m("neumf")
    cfg = neumf.NeuMFConfig(variant="A", dim=dim, optimizer="adam_dense", dense_impl="deferred", dropout=dropout, seed=0xABCDEF12345)
    return [neumf.NeuMFEngine(cfg, U, I, dev, max_batch=B, id_dtype=idt, init_seed=3) for _ in range(n)]


def _group_ids(rng, S, U, I):
    uu, ii = rng.integers(0, U, (S, B)), rng.integers(0, I, (S, B))
    uu[:, :300] = uu[:, :1]                      # a hot row per step, on top of what the id range gives
    yy = (rng.random((S, B)) < 0.3).astype(np.float32)
    return uu, ii, yy


def _feed(dev, idt, one, groups, S, uu, ii, yy):
    """the S steps of a group: single-step graph replays on `one`, one group launch on each engine of `groups`"""
    td = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    if one is not None:
        for k in range(S):
            one.train_step(td(uu[k], idt), td(ii[k], idt), td(yy[k], torch.float32))
    for g in groups:
        g.train_steps(td(uu, idt), td(ii, idt), td(yy, torch.float32))


def _assert_same_state(a, b):
    a.flush(); b.flush()
    for k in ("user", "item"):
        assert torch.equal(a.fused[k], b.fused[k]), "table " + k
        assert torch.equal(a.fused_m[k], b.fused_m[k]) and torch.equal(a.fused_v[k], b.fused_v[k]), "moments " + k
    assert torch.equal(a.theta.buf, b.theta.buf), "dense parameters"
    assert torch.equal(a.adam_m.buf, b.adam_m.buf) and torch.equal(a.adam_v.buf, b.adam_v.buf), "dense moments"
    assert torch.equal(a.moving_buf, b.moving_buf), "moving statistics"
    assert torch.equal(a.msums.sum(0), b.msums.sum(0)), "metric sums"


def _reload(e):
    e.load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in e.state_dict().items()})


def _three_groups(dev, idt, one, groups, S, U, I, seed):
    """three groups, a single step between the first two, a state_dict reload before the last"""
    rng = np.random.default_rng(seed)
    td = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    _feed(dev, idt, one, groups, S, *_group_ids(rng, S, U, I))
    u1, i1, y1 = (a[0] for a in _group_ids(rng, 1, U, I))
    for e in [one] + list(groups):
        e.train_step(td(u1, idt), td(i1, idt), td(y1, torch.float32))
    _feed(dev, idt, one, groups, S, *_group_ids(rng, S, U, I))
    for e in [one] + list(groups):
        _reload(e)
    _feed(dev, idt, one, groups, S, *_group_ids(rng, S, U, I))
    torch.cuda.synchronize()
    for e in [one] + list(groups):
        e.check_ids()
        assert e.t == 3 * S + 1 and int(e.step_state[0].item()) == e.t


@pytest.mark.parametrize("ranges", ["wide", "tiny"])
@pytest.mark.parametrize("dropout", [0.2, 0.0])
@pytest.mark.parametrize("S", [4, 2])
@pytest.mark.parametrize("dim,idt", [(64, torch.int32), (128, torch.int64)])
def test_group_graph_equals_single_step_graphs(dev, dim, idt, S, dropout, ranges):
    """Three group launches (a single step after the first, a reload before the last) against the same 3 S + 1 steps as single-step
    graph replays: tables, moments, dense state, moving statistics and metric sums bit for bit, the device step counter at engine.t,
    no id flagged.  Dropout on: the keep-plane and finalize riders are in every Adam-rows launch.  ranges "tiny": 97 users and 53
    items, so every id sits on a run of hundreds of sorted positions crossing many 64-position blocks - the segment-partials launch
    that carries the later steps' step-state advance has real work beside it."""
    U, I = (3000, 2000) if ranges == "wide" else (97, 53)
    one, grp = _engines(dev, 2, dim, idt, dropout, U, I)
    one.enable_graph(B)
    gm = grp.enable_graph_multi(B, steps=S)
    assert gm["sets"] is not None and len(gm["sets"]) == S      # the capture took the group form
    before = {k: grp.fused[k].clone() for k in ("user", "item")}
    _three_groups(dev, idt, one, [grp], S, U, I, seed=23)
    _assert_same_state(grp, one)
    assert all(bool((grp.fused[k] != before[k]).any(dim=1).all()) for k in before) or ranges == "wide"      # tiny: every row trained
    assert all(not torch.equal(grp.fused[k], before[k]) for k in before) and bool(torch.isfinite(grp.theta.buf).all())


def test_group_head_builds_the_index_of_every_step(dev):
    """After one group launch every step's sorted_ids / sorted_pos are numpy's stable argsort of that step's keys (both streams), with
    an id out of range in the group's second step: it sorts as the key `upper` (= table rows, behind every valid id), raises through
    check_ids() on both engines, and leaves every row as the single-step engine leaves it."""
    S, U, I, idt = 4, 3000, 2000, torch.int32
    one, grp = _engines(dev, 2, 64, idt, 0.2, U, I)
    one.enable_graph(B)
    gm = grp.enable_graph_multi(B, steps=S)
    assert gm["sets"] is not None
    uu, ii, yy = _group_ids(np.random.default_rng(5), S, U, I)
    uu[1, 7777] = U + 5
    ii[1, 12] = -3
    _feed(dev, idt, one, [grp], S, uu, ii, yy)
    torch.cuda.synchronize()
    for k, (ui, xi, _) in enumerate(gm["sets"]):
        for ids, upper, ix in ((uu[k], U, ui), (ii[k], I, xi)):
            keys = np.where((ids >= 0) & (ids < upper), ids, upper)
            order = np.argsort(keys, kind="stable")
            assert np.array_equal(ix.sorted_ids[:B].cpu().numpy(), keys[order]), k
            assert np.array_equal(ix.sorted_pos[:B].cpu().numpy(), order), k
    assert int(gm["sets"][1][0].sorted_ids[B - 1].item()) == U and int(gm["sets"][1][1].sorted_ids[B - 1].item()) == I
    for e in (grp, one):
        with pytest.raises(IndexError):
            e.check_ids()
    assert grp.t == one.t == S and int(grp.step_state[0].item()) == S
    _assert_same_state(grp, one)


def test_group_index_knob_restores_the_per_step_index(dev):
    """BR_GROUP_INDEX=0 at capture: the group's launch list is the per-step one - S fused lookup + index calls (a lookup with its sort
    workgroups and a chunk-rank launch each), counted through the graph probe's record nodes (two around the first launch of every
    such call); the group form has one such call, at the head.  Both captures and the single-step graph compute the same bits."""
    _lib = _m("_lib")
    lib = _lib.load()
    S, U, I, idt = 4, 3000, 2000, torch.int32
    one, grp, per_step = _engines(dev, 3, 64, idt, 0.2, U, I)
    one.enable_graph(B)
    counts = {}
    for name, eng, env in (("group", grp, None), ("per step", per_step, "0")):
        eng.enable_graph(B)
        if env is not None:
            os.environ["BR_GROUP_INDEX"] = env
        try:
            assert lib.brProbeGraphSelect(TAG_INDEX_USER) == 0
            gm = eng.enable_graph_multi(B, steps=S)
        finally:
            lib.brProbeGraphSelect(-1)
            os.environ.pop("BR_GROUP_INDEX", None)
        counts[name] = lib.brProbeGraphNodes()
        assert (gm["sets"] is None) == (env is not None)
    assert counts == {"group": 2, "per step": 2 * S}, counts
    _three_groups(dev, idt, one, [grp, per_step], S, U, I, seed=23)
    _assert_same_state(per_step, one)
    _assert_same_state(grp, one)


def test_two_group_launches_back_to_back(dev):
    """Two group launches with different ids and no synchronisation between them, against the same steps one by one: a per-step
    scratch or index buffer carried over from the previous group (not cleared / rebuilt by the next head) would show here."""
    S, U, I, idt = 4, 97, 2000, torch.int32
    one, grp = _engines(dev, 2, 64, idt, 0.2, U, I)
    one.enable_graph(B)
    assert grp.enable_graph_multi(B, steps=S)["sets"] is not None
    rng = np.random.default_rng(41)
    g1, g2 = _group_ids(rng, S, U, I), _group_ids(rng, S, U, I)
    td = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    dev_groups = [(td(u, idt), td(i, idt), td(y, torch.float32)) for u, i, y in (g1, g2)]
    torch.cuda.synchronize()
    for u, i, y in dev_groups:                    # (staged by a launch on the stream: nothing waits in between)
        grp.train_steps(u, i, y)
    for u, i, y in dev_groups:
        for k in range(S):
            one.train_step(u[k], i[k], y[k])
    torch.cuda.synchronize()
    grp.check_ids(); one.check_ids()
    assert grp.t == one.t == 2 * S and int(grp.step_state[0].item()) == grp.t
    _assert_same_state(grp, one)
