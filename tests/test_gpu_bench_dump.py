"""-m gpu: bench.py --dump-outputs (dump_outputs).  The sampled table rows it writes are brought up to date on copies of those rows
(brAdamFlush on the gathered rows): they must equal the engine's own flushed tables at the same rows, bit for bit, and the engine's
lag state must be left as it was (--full keeps measuring the same run after the dump)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer,impl", [("adam_dense", "deferred"), ("adam_lazy", "sweep")])
def test_dump_outputs_equal_the_engine_state_and_leave_it_untouched(dev, tmp_path, monkeypatch, optimizer, impl):
    neumf = importlib.import_module("binary-recommendation_amd.neumf")
    U, I, B = 3000, 500, 256
    monkeypatch.setattr(bench, "DUMP_ROWS", 1000)              # user rows sampled, item rows all taken
    eng = neumf.NeuMFEngine(neumf.NeuMFConfig(variant="A", dim=16, optimizer=optimizer, dense_impl=impl, seed=5), U, I, dev, B, init_seed=1)
    for u, i, y in bench.make_batches(6, B, U, I, dev, 7, False):
        eng.train_step(u, i, y)
    torch.cuda.synchronize()
    deferred = eng.deferred
    assert deferred == (optimizer == "adam_dense")
    last = {k: eng.last[k].clone() for k in ("user", "item")} if deferred else None
    raw = {k: eng.fused[k].clone() for k in ("user", "item")}
    names = bench.dump_outputs(eng, str(tmp_path / "dump"), B)
    eng.check_ids()
    if deferred:                                               # nothing of the engine moved: rows still lag, tables still raw
        assert eng._stale
        for k in ("user", "item"):
            assert torch.equal(eng.last[k], last[k]) and torch.equal(eng.fused[k], raw[k])
    got = {n: np.load(tmp_path / "dump" / (n + ".npy")) for n in names}
    assert set(os.listdir(tmp_path / "dump")) == {n + ".npy" for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["logit"], eng.logit[:B].cpu().numpy())
    np.testing.assert_array_equal(got["prob"], eng.prob[:B].cpu().numpy())
    np.testing.assert_array_equal(got["dense_params"], eng.theta.buf.cpu().numpy())
    np.testing.assert_array_equal(got["metric_sums"], eng.msums.sum(dim=0).cpu().numpy())
    tabs, ms, vs = eng.tables, eng.tab_m, eng.tab_v                # (flushes a deferred engine)
    for k, rows in (("user", U), ("item", I)):
        ids = got[k + "_row_ids"]
        assert len(ids) == min(rows, 1000) and np.all(np.diff(ids) > 0) and ids[-1] < rows
        ids = torch.from_numpy(ids.astype(np.int64)).to(dev)
        for suffix, src in (("", tabs), ("_m", ms), ("_v", vs)):
            want = torch.cat([src[k + "_mlp"][ids], src[k + "_mf"][ids]], dim=1)
            np.testing.assert_array_equal(got[k + "_rows" + suffix], want.cpu().numpy())
