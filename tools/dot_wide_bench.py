"""Dot-product catalogue top-k and AUC for rows wider than 128 features (ops.dot_catalog_topk_wide / dot_catalog_auc_wide,
csrc/recommend_dot_wide.hip, csrc/auc_dot.hip) against a matrix path at the same width, in one process, alternating, device
events around synchronised work.

brScoreMatrix stops at 128 features, so the project has no matrix path of its own at these widths.  The matrix leg here is the vendor
fp32 GEMM (torch.matmul, users chunked so that the score matrix stays at or below --matrix-gb) followed by ops.topk_rows or
ops.full_auc: the best two-pass form available, and it is named "gemm" in the record so that nobody takes it for brScoreMatrix.  Its
scores are not the fused path's bit for bit (another summation order), so the record gives the top-k overlap and the largest AUC
difference, not equality.

65 536 users x 100 000 items, dims 256, 350 and 512, random U(-0.05, 0.05) tables (BPR's init), k = 10 and k = 100, and the AUC at
P = 20 positives per user.  The floor is 2 * (padded width) FLOP per pair at the 155 TF fp32-MFMA rate, the padded width being the
128-feature blocks the kernel runs (256, 384, 512).  Prints one JSON line; --out FILE writes it too.

    python tools/dot_wide_bench.py [--users 65536] [--items 100000] [--dims 256,350,512] [--ks 10,100] [--positives 20] [--out FILE]
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
    ap.add_argument("--dims", default="256,350,512")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--positives", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--matrix-gb", type=float, default=4.0)
    ap.add_argument("--overlap-users", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dot_wide_bench: no GPU")
    from importlib import import_module
    ops = import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    gen = torch.Generator(device=dev).manual_seed(7)
    chunk = max(1, min(a.users, int(a.matrix_gb * 1e9 // (4 * a.items))))
    pairs = a.users * a.items

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3, out

    def alternate(fused, mat):
        for f in (fused, mat):                          # warm-up: code objects, allocator, GEMM heuristics
            timed(f)
        tf, tm = [], []
        for _ in range(a.repeats):
            tf.append(timed(fused)[0]); tm.append(timed(mat)[0])
        return tf, tm

    res = {"metric": "dot_catalog_wide", "users": a.users, "items": a.items, "matrix_users_per_chunk": chunk,
           "matrix_path": "torch.matmul (vendor fp32 GEMM) + ops.topk_rows / ops.full_auc; brScoreMatrix stops at dim 128", "legs": []}
    rng = np.random.default_rng(7)
    cols = np.sort(rng.integers(0, a.items, (a.users, a.positives)), axis=1)           # (truth_csr drops the rare duplicate)
    off, idx = ops.truth_csr(a.users, np.repeat(np.arange(a.users), a.positives), cols.reshape(-1), dev)
    for dim in [int(x) for x in a.dims.split(",")]:
        Q = torch.empty(a.users, dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        C = torch.empty(a.items, dim, device=dev).uniform_(-0.05, 0.05, generator=gen)
        padded = max(256, (dim + 127) // 128 * 128)
        floor_s = 2 * padded * pairs / MFMA_F32_FLOPS

        def leg(name, tf, tm, **more):
            mf, mm = float(np.median(tf)), float(np.median(tm))
            res["legs"].append({"leg": name, "dim": dim, "padded_width": padded, "floor_s": floor_s, "fused_s": mf, "fused_s_all": tf,
                                "fused_pairs_per_s": pairs / mf, "gemm_matrix_s": mm, "gemm_matrix_s_all": tm, "speedup": mm / mf,
                                "fraction_of_floor": floor_s / mf, **more})

        for k in [int(x) for x in a.ks.split(",") if x]:      # (--ks "": the AUC legs alone)
            def matrix(n_users=a.users):
                out_s = torch.empty(n_users, k, device=dev)
                out_i = torch.empty(n_users, k, dtype=torch.int32, device=dev)
                for s in range(0, n_users, chunk):
                    e = min(n_users, s + chunk)
                    out_s[s:e], out_i[s:e] = ops.topk_rows(torch.matmul(Q[s:e], C.T), k)
                return out_s, out_i
            fused = lambda: ops.dot_catalog_topk_wide(Q, C, k)
            tf, tm = alternate(fused, matrix)
            n = min(a.overlap_users, a.users)
            fi = fused()[1][:n].cpu().numpy()
            mi = matrix(n)[1].cpu().numpy()
            overlap = float(np.mean([len(set(fi[r]) & set(mi[r])) / k for r in range(n)]))
            leg(f"topk_k{k}", tf, tm, k=k, topk_overlap=overlap)

        def matrix_auc():
            out = torch.empty(a.users, device=dev)
            for s in range(0, a.users, chunk):
                e = min(a.users, s + chunk)
                lo, hi = int(off[s]), int(off[e])
                out[s:e] = ops.full_auc(torch.matmul(Q[s:e], C.T), (off[s:e + 1] - lo).contiguous(), idx[lo:hi].contiguous())
            return out
        fused_auc = lambda: ops.dot_catalog_auc_wide(Q, C, off, idx)
        tf, tm = alternate(fused_auc, matrix_auc)
        diff = float((fused_auc() - matrix_auc()).abs().max())
        leg(f"auc_p{a.positives}", tf, tm, positives=a.positives, max_auc_diff=diff)
        del Q, C
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
