"""Dot-product catalogue AUC (BPR tables): the matrix path (ops.score_matrix + ops.full_auc, users chunked so that the score matrix
stays at or below --matrix-gb) against the fused path (ops.dot_catalog_auc, csrc/auc_dot.hip) in one process, alternating, device
events around synchronised work.

65 536 users x 100 000 items, dim 64, random U(-0.05, 0.05) tables (BPR's init), random truth sets of P = 20 and P = 150 per user;
also the fused path alone at config-3 size (1 M users x 100 000 items, P = 20), where the matrix would take 400 GB.  The floor is
2 * dim FLOP per pair at the 155 TF fp32-MFMA rate.  Prints one JSON line; --out FILE writes it too.

    python tools/dot_auc_bench.py [--users 65536] [--items 100000] [--dim 64] [--ps 20,150] [--big-users 1048576] [--repeats 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--ps", default="20,150")
    ap.add_argument("--big-users", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--matrix-gb", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dot_auc_bench: no GPU")
    from importlib import import_module
    ops = import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    Q = torch.empty(a.users, a.dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
    C = torch.empty(a.items, a.dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
    chunk = max(1, min(a.users, int(a.matrix_gb * 1e9 // (4 * a.items))))

    def matrix(off, idx):
        out = torch.empty(a.users, device=dev)
        offc = off.cpu()
        for s in range(0, a.users, chunk):
            e = min(a.users, s + chunk)
            o0, o1 = int(offc[s]), int(offc[e])
            out[s:e] = ops.full_auc(ops.score_matrix(Q[s:e], C), off[s:e + 1] - o0, idx[o0:o1])
        return out

    pairs = a.users * a.items
    floor_s = 2 * a.dim * pairs / MFMA_F32_FLOPS
    res = {"metric": "dot_catalog_auc", "users": a.users, "items": a.items, "dim": a.dim, "matrix_users_per_chunk": chunk,
           "floor_s": floor_s, "legs": []}
    for P in [int(x) for x in a.ps.split(",")]:
        off, idx = truth(ops, a.users, a.items, P, dev, seed=P)
        fused = lambda: ops.dot_catalog_auc(Q, C, off, idx)
        mat = lambda: matrix(off, idx)
        for f in (fused, mat):                         # warm-up: code objects, allocator
            timed(f)
        tf, tm = [], []
        for _ in range(a.repeats):                      # alternating
            tf.append(timed(fused)[0]); tm.append(timed(mat)[0])
        _, af = timed(fused)
        _, am = timed(mat)
        ok = ~torch.isnan(am)
        diff = float((af[ok].double() - am[ok].double()).abs().max())
        mf, mm = float(np.median(tf)), float(np.median(tm))
        res["legs"].append({"P": P, "truth_entries": int(idx.numel()), "fused_s": mf, "fused_s_all": tf, "fused_pairs_per_s": pairs / mf,
                            "matrix_s": mm, "matrix_s_all": tm, "matrix_pairs_per_s": pairs / mm, "speedup": mm / mf,
                            "fraction_of_floor": floor_s / mf, "max_abs_auc_diff": diff, "nan_same": bool(torch.equal(af.isnan(), am.isnan()))})
        del off, idx
    if a.big_users:
        del Q
        torch.cuda.empty_cache()
        Qb = torch.empty(a.big_users, a.dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        off, idx = truth(ops, a.big_users, a.items, 20, dev, seed=1)
        fused = lambda: ops.dot_catalog_auc(Qb, C, off, idx)
        timed(fused)
        tb = [timed(fused)[0] for _ in range(a.repeats)]
        _, ab = timed(fused)
        pb = a.big_users * a.items
        fb = 2 * a.dim * pb / MFMA_F32_FLOPS
        mb = float(np.median(tb))
        res["big"] = {"users": a.big_users, "P": 20, "fused_s": mb, "fused_s_all": tb, "fused_pairs_per_s": pb / mb, "floor_s": fb,
                      "fraction_of_floor": fb / mb, "matrix_bytes": 4 * pb, "mean_auc": float(ab.double().mean()),
                      "nan_users": int(ab.isnan().sum())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
