"""Dot-product catalogue top-k (BPR tables): the matrix path (ops.score_matrix + ops.topk_rows, users chunked so that the score matrix
stays at or below --matrix-gb) against the fused path (ops.dot_catalog_topk, csrc/recommend_dot.hip) in one process, alternating,
device events around synchronised work.

65 536 users x 100 000 items, dim 64, random U(-0.05, 0.05) tables (BPR's init), k = 10 and k = 100; also the fused path for one user
against the catalogue (predictForUser's latency).  The floor is 2 * dim FLOP per pair at the 155 TF fp32-MFMA rate.
Prints one JSON line; --out FILE writes it too.

    python tools/dot_recommend_bench.py [--users 65536] [--items 100000] [--dim 64] [--ks 10,100] [--repeats 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--matrix-gb", type=float, default=4.0)
    ap.add_argument("--overlap-users", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dot_recommend_bench: no GPU")
    from importlib import import_module
    ops = import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    Q = torch.empty(a.users, a.dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
    C = torch.empty(a.items, a.dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
    chunk = max(1, min(a.users, int(a.matrix_gb * 1e9 // (4 * a.items))))

    def matrix(k, n_users=a.users):
        out_s = torch.empty(n_users, k, device=dev)
        out_i = torch.empty(n_users, k, dtype=torch.int32, device=dev)
        for s in range(0, n_users, chunk):
            e = min(n_users, s + chunk)
            out_s[s:e], out_i[s:e] = ops.topk_rows(ops.score_matrix(Q[s:e], C), k)
        return out_s, out_i

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3, out

    pairs = a.users * a.items
    floor_s = 2 * a.dim * pairs / MFMA_F32_FLOPS
    res = {"metric": "dot_catalog_topk", "users": a.users, "items": a.items, "dim": a.dim, "matrix_users_per_chunk": chunk,
           "floor_s": floor_s, "legs": []}
    for k in [int(x) for x in a.ks.split(",")]:
        fused = lambda: ops.dot_catalog_topk(Q, C, k)
        mat = lambda: matrix(k)
        one = lambda: ops.dot_catalog_topk(Q[:1], C, k)
        for f in (fused, mat, one):                    # warm-up: code objects, allocator
            timed(f)
        tf, tm, t1 = [], [], []
        for _ in range(a.repeats):                      # alternating
            tf.append(timed(fused)[0]); tm.append(timed(mat)[0]); t1.append(timed(one)[0])
        _, (fs, fi) = timed(fused)
        n = min(a.overlap_users, a.users)
        _, (ms, mi) = timed(lambda: matrix(k, n))
        fi, mi = fi[:n].cpu().numpy(), mi.cpu().numpy()
        overlap = float(np.mean([len(set(fi[r]) & set(mi[r])) / k for r in range(n)]))
        top1_rel = float(((fs[:n, 0] - ms[:, 0]).abs() / ms[:, 0].abs()).max())
        mf, mm = float(np.median(tf)), float(np.median(tm))
        res["legs"].append({"k": k, "fused_s": mf, "fused_s_all": tf, "fused_pairs_per_s": pairs / mf, "matrix_s": mm, "matrix_s_all": tm,
                            "matrix_pairs_per_s": pairs / mm, "speedup": mm / mf, "fraction_of_floor": floor_s / mf,
                            "one_user_ms": float(np.median(t1)) * 1e3, "topk_overlap": overlap, "top1_max_rel_diff": top1_rel})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
