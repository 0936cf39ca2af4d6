"""NeuMF full-catalogue AUC: the fused path (NeuMFEngine.full_auc method="fused": csrc/auc_neumf.hip) against (a) the pair path it
replaces (method="pairs": every pair through predict, the U x I matrix, brFullAuc) and (b) the catalogue top-k at the same shape
(NeuMFEngine.recommend(k=10): csrc/recommend.hip, the same scoring loop with a selection instead of a count), in one process,
alternating, device events around synchronised work.

Variant A, dim 64, random tables with nonzero BatchNorm moving statistics (tools/recommend_bench.py's model).  (a): 4 096 users x
100 000 items, P = 20 positives per user on both paths (the pair path is capped there: its matrix is 1.6 GB at that size and the rate
is per pair).  (b): 65 536 users x 100 000 items, P = 20 and P = 150.  Prints one JSON line; --out FILE writes it too.

    python tools/neumf_auc_bench.py [--users 65536] [--pair-users 4096] [--items 100000] [--repeats 3] [--out FILE]
    python tools/neumf_auc_bench.py --once fused|recommend|pairs [--positives 20]     # one call, for a kernel trace
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def truth(ops, n_users, n_items, p, dev, seed):
    """p distinct random positions per user, ascending (ops.truth_csr's form), drawn on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.rand(n_users, n_items, device=dev, generator=g).topk(p, dim=1).indices.sort(dim=1).values.to(torch.int32).reshape(-1)
    off = torch.arange(n_users + 1, dtype=torch.int64, device=dev) * p
    return off, idx.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--pair-users", type=int, default=4096)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--positives", type=int, nargs="+", default=[20, 150])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", choices=["fused", "recommend", "pairs"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neumf_auc_bench: no GPU")
    import __graft_entry__ as g
    g.build()
    from importlib import import_module
    neumf, ops = import_module("binary-recommendation_amd.neumf"), import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    cfg = neumf.NeuMFConfig("A", dim=64)
    eng = neumf.NeuMFEngine(cfg, a.users, a.items, dev, max_batch=65536)
    gen = torch.Generator(device=dev).manual_seed(7)
    for k in ("user", "item"):
        eng.fused[k].uniform_(-0.5, 0.5, generator=gen)
    for k in ("mm1", "mm2"):
        eng.moving[k].uniform_(0.1, 0.6, generator=gen)
    for k in ("mv1", "mv2"):
        eng.moving[k].uniform_(0.05, 0.5, generator=gen)
    for k in ("g1", "g2"):
        eng.theta.view(k).uniform_(0.5, 1.5, generator=gen)
    for k in ("be1", "be2", "b1", "b2", "b3"):
        eng.theta.view(k).uniform_(-0.2, 0.2, generator=gen)
    users = torch.arange(a.users, dtype=torch.int32, device=dev)
    # in chunks of users: the draw's own U x I scratch stays small
    truths = {}
    for p in a.positives:
        parts = [truth(ops, min(4096, a.users - u0), a.items, p, dev, seed=p + u0)[1] for u0 in range(0, a.users, 4096)]
        truths[p] = (torch.arange(a.users + 1, dtype=torch.int64, device=dev) * p, torch.cat(parts))
    p0 = a.positives[0]
    small = (truths[p0][0][:a.pair_users + 1].contiguous(), truths[p0][1][:a.pair_users * p0].contiguous())

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3, out

    fused = {p: (lambda p=p: eng.full_auc(users, truths[p])) for p in a.positives}
    fused_small = lambda: eng.full_auc(users[:a.pair_users], small)
    pairs = lambda: eng.full_auc(users[:a.pair_users], small, method="pairs")
    rec = lambda: eng.recommend(users, a.k)
    if a.once:
        t, _ = timed({"fused": fused[p0], "recommend": rec, "pairs": pairs}[a.once])
        print(json.dumps({"metric": "neumf_catalog_auc_once", "what": a.once, "positives": p0, "seconds": t}))
        return
    for f in (pairs, fused_small, rec, *fused.values()):     # warm-up: code objects, allocator
        timed(f)
    tp, ts, tr, tf = [], [], [], {p: [] for p in a.positives}
    for _ in range(a.repeats):                                # alternating
        tp.append(timed(pairs)[0]); ts.append(timed(fused_small)[0]); tr.append(timed(rec)[0])
        for p in a.positives:
            tf[p].append(timed(fused[p])[0])
    _, auc_p = timed(pairs)
    _, auc_f = timed(fused_small)
    eng.check_ids()
    ok = ~torch.isnan(auc_p)
    med = lambda v: float(np.median(v))
    n_big, n_small = a.users * a.items, a.pair_users * a.items
    res = {"metric": "neumf_catalog_auc", "variant": "A", "dim": 64, "items": a.items,
           "pairs_users": a.pair_users, "pairs_positives": p0, "pairs_s": med(tp), "pairs_s_all": tp, "pairs_pairs_per_s": n_small / med(tp),
           "fused_at_pairs_shape_s": med(ts), "fused_at_pairs_shape_s_all": ts, "fused_over_pairs_speedup": med(tp) / med(ts),
           "max_abs_auc_diff_fused_pairs": float((auc_f[ok] - auc_p[ok]).abs().max()),
           "users": a.users, "recommend_k": a.k, "recommend_s": med(tr), "recommend_s_all": tr, "recommend_pairs_per_s": n_big / med(tr),
           "fused": {str(p): {"s": med(tf[p]), "s_all": tf[p], "pairs_per_s": n_big / med(tf[p]), "over_recommend": med(tf[p]) / med(tr)}
                     for p in a.positives}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
