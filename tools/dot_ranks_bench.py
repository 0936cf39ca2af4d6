"""Exact full-catalogue ranks for dot-product models (ops.dot_catalog_ranks, csrc/ranks_dot.hip) against the AUC pass that streams the
same tiles (ops.dot_catalog_auc / dot_catalog_auc_wide), and against the only other route to the same integers: ops.score_matrix plus
torch counting on the stored U x I matrix.  One process, the legs alternating, device events around synchronised work.

Leg "same tiles": 65 536 users x 100 000 items, random U(-0.05, 0.05) tables (BPR's init), 20 random positives per user, at dim 64
(whole-row kernel) and dim 350 (block kernel): ranks against AUC, and ranks + ops.rank_metrics.  Leg "matrix route": 4 096 users x
100 000 items, dim 64: score_matrix, then per chunk of positives `>` / `==` against the stored rows; its counts are compared with the
fused ones (the two score the pairs with different instruction sequences, so they can differ where two scores are one rounding
apart: reported, not asserted).  Prints one JSON line; --out FILE writes it too.

    python tools/dot_ranks_bench.py [--users 65536] [--items 100000] [--dims 64,350] [--p 20] [--matrix-users 4096] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_FLOPS = 155e12     # MI355X fp32-MFMA peak (v_mfma_f32_16x16x4_f32), not measured here


def truth(ops, U, I, P, dev, seed):
    """P random positions per user (duplicates dropped by truth_csr), on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    cols = torch.randint(0, I, (U * P,), generator=g, device=dev).cpu().numpy()
    return ops.truth_csr(U, np.repeat(np.arange(U), P), cols, dev)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, out


def matrix_counts(ops, Q, C, off, idx, users_per_chunk=64):
    """(above, tied) from the stored matrix: the user's other positives are candidates, the entry itself is not"""
    S = ops.score_matrix(Q, C)
    U = Q.shape[0]
    cnt = off[1:] - off[:-1]
    rows = torch.repeat_interleave(torch.arange(U, device=Q.device), cnt)
    s = S[rows, idx.long()]
    above = torch.empty_like(idx)
    tied = torch.empty_like(idx)
    offc = off.cpu()
    for u0 in range(0, U, users_per_chunk):
        u1 = min(U, u0 + users_per_chunk)
        e0, e1 = int(offc[u0]), int(offc[u1])
        r = S[rows[e0:e1]]                                               # (entries, I): index plumbing for the compare
        se = s[e0:e1, None]
        above[e0:e1] = (r > se).sum(1).int()
        tied[e0:e1] = ((r == se).sum(1) - 1).int()
    return above, tied


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--dims", default="64,350")
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--matrix-users", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dot_ranks_bench: no GPU")
    from importlib import import_module
    ops = import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    res = {"metric": "dot_catalog_ranks", "users": a.users, "items": a.items, "P": a.p, "legs": []}
    off, idx = truth(ops, a.users, a.items, a.p, dev, seed=a.p)
    for dim in [int(x) for x in a.dims.split(",")]:
        Q = torch.empty(a.users, dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        C = torch.empty(a.items, dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        auc = lambda: ops.dot_auc_for(dim)(Q, C, off, idx)
        ranks = lambda: ops.dot_catalog_ranks(Q, C, off, idx)
        both = lambda: ops.rank_metrics(*ops.dot_catalog_ranks(Q, C, off, idx), off, (1, 5, 10, 20, 50, 100, 500, 1000))
        for f in (auc, ranks, both):                   # warm-up: code objects, allocator
            timed(f)
        ta, tr, tb = [], [], []
        for _ in range(a.repeats):                      # alternating
            ta.append(timed(auc)[0]); tr.append(timed(ranks)[0]); tb.append(timed(both)[0])
        ma, mr, mb = float(np.median(ta)), float(np.median(tr)), float(np.median(tb))
        pairs = a.users * a.items
        floor_s = 2 * dim * pairs / MFMA_F32_FLOPS
        m = both()
        res["legs"].append({"dim": dim, "truth_entries": int(idx.numel()), "auc_s": ma, "auc_s_all": ta, "ranks_s": mr, "ranks_s_all": tr,
                            "ranks_and_metrics_s": mb, "ranks_over_auc": mr / ma, "floor_s": floor_s, "ranks_fraction_of_floor": floor_s / mr,
                            "auc_fraction_of_floor": floor_s / ma, "mean_mrr": float(m["mrr"].double().nanmean()),
                            "mean_ndcg@10": float(m["ndcg@10"].double().nanmean())})
        del Q, C
    if a.matrix_users:
        Um, dim = a.matrix_users, 64
        Q = torch.empty(Um, dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        C = torch.empty(a.items, dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        offm, idxm = truth(ops, Um, a.items, a.p, dev, seed=1)
        fused = lambda: ops.dot_catalog_ranks(Q, C, offm, idxm)
        mat = lambda: matrix_counts(ops, Q, C, offm, idxm)
        for f in (fused, mat):
            timed(f)
        tf, tm = [], []
        for _ in range(a.repeats):
            tf.append(timed(fused)[0]); tm.append(timed(mat)[0])
        (fa, ft), (xa, xt) = fused(), mat()
        mf, mm = float(np.median(tf)), float(np.median(tm))
        res["matrix_route"] = {"users": Um, "dim": dim, "truth_entries": int(idxm.numel()), "fused_s": mf, "fused_s_all": tf, "matrix_s": mm,
                               "matrix_s_all": tm, "speedup": mm / mf, "matrix_bytes": 4 * Um * a.items,
                               "entries_with_other_counts": int(((fa != xa) | (ft != xt)).sum()),
                               "max_rank_difference": int(((fa + ft).long() - (xa + xt).long()).abs().max())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
