"""-m gpu: the full-catalogue AUC of the row-sharded BPR engine counted at the owners (parallel.py auc_at_owners) through RCCL: a
1-rank "nccl" group with every collective really issued (force_collectives, the pattern of test_gpu_sharded_recommend_nccl.py) - the
meta all-gather, the id -> owner exchange, the all-gathers of the queries, the truth lists, the per-user counts and the raw scores, and
the all-to-all of the uint64 partials take device tensors straight into the RCCL calls.  One rank owns every row, so the values must
equal the single-device engine's bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from importlib import import_module
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        par, bpr, ops = (import_module("binary-recommendation_amd." + m) for m in ("parallel", "bpr", "ops"))
        ctx = par.DistCtx(force_collectives=True)
        assert ctx.backend == "nccl" and not ctx.local
        same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])
        U, I = 90, 400
        rng = np.random.default_rng(1)
        users = torch.as_tensor(rng.integers(0, U, 33), dtype=torch.int32, device=dev)
        items = torch.as_tensor(rng.permutation(I)[:250], dtype=torch.int32, device=dev)
        rows = np.repeat(np.arange(1, 33), 20)                                   # (the first user has no positives)
        for dim in (64, 350):
            eb = par.make_sharded_bpr(bpr.BPREngine)(U, I, dim, dev, 256, ctx)
            es = bpr.BPREngine(U, I, dim, dev, 256)
            es.user.copy_(eb.user[:U]); es.item.copy_(eb.item[:I])
            for it, n_it in ((None, I), (items, 250)):
                truth = ops.truth_csr(33, rows, rng.integers(0, n_it, rows.size), dev)
                got = eb.full_auc(users, truth, items=it, catalog="owners")
                assert torch.isnan(got[0]) and not torch.isnan(got[1:]).any()
                assert same(got, es.full_auc(users, truth, items=it)), ("bpr", dim)
            torch.cuda.synchronize()
            eb.check_ids()
        q.put("ok")
    except Exception:  # noqa: BLE001
        import traceback
        q.put("FAIL: " + traceback.format_exc()[-2500:])
    finally:
        # leave as test_gpu_nccl_world1.py does: without the process group's teardown; the result is already in the queue
        q.close(); q.join_thread()
        os._exit(0)


def test_sharded_full_auc_rccl_one_rank_group(dev):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    p = ctxm.Process(target=_worker, args=(port, q))
    p.start()
    try:
        res = q.get(timeout=300)
    finally:
        p.join(timeout=60)
        if p.is_alive():        # never leave a child behind: the interpreter would wait for it at exit
            p.kill()
            p.join(timeout=30)
    assert res.startswith("ok"), res
