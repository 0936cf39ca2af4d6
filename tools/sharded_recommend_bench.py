"""What scoring the catalogue at its owners costs beside scoring it in one launch, on ONE device with W virtual ranks (the item table
dealt r::W, as tests/test_gpu_sharded_recommend.py does): per k the times of

  (a) merge   : brTopKListsMerge over the W lists of every user
  (b) split   : brCsrSplitByOwner of the exclusion CSR (--seen positions per user), summed over the W owners
  (c) parts   : the W brDotCatalogTopK launches over all users x one owner's candidates, summed
  whole       : the one brDotCatalogTopK launch over all users x all candidates (csrc/recommend_dot.hip, the kernel the single-device
                engines run; the owner path launches it unchanged)

medians of --repeats alternating repeats, device events around synchronised work (the ops wrappers as a caller uses them: (a) and (b)
include their output / workspace allocations, so they bound the kernels from above), and the merged lists are compared bit for bit with
the whole launch.  On W real devices (c) runs in parallel, one part per device: parts / W is the per-device scoring time there.  The
bytes each design moves per rank are derived from the sizes, not timed (one device here).  Prints one JSON line; --out FILE writes it.

    python tools/sharded_recommend_bench.py [--users 65536] [--items 100000] [--dim 64] [--world 8] [--ks 10,100] [--seen 20] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--seen", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sharded_recommend_bench: no GPU")
    from importlib import import_module
    ops = import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    U, I, D, W = a.users, a.items, a.dim, a.world
    gen = torch.Generator(device=dev).manual_seed(7)
    Q = torch.empty(U, D, device=dev).uniform_(-0.05, 0.05, generator=gen)
    C = torch.empty(I, D, device=dev).uniform_(-0.05, 0.05, generator=gen)
    cols = torch.randint(0, I, (U * a.seen,), generator=gen, device=dev).cpu().numpy()
    ex = ops.truth_csr(U, np.repeat(np.arange(U), a.seen), cols, dev)
    parts = [C[r::W].contiguous() for r in range(W)]                         # owner r holds the rows r, r + W, ..
    maps = [torch.arange(r, I, W, dtype=torch.int32, device=dev) for r in range(W)]
    g2l = []
    for r in range(W):
        g = torch.full((I,), -1, dtype=torch.int32, device=dev)
        g[maps[r].long()] = torch.arange(maps[r].numel(), dtype=torch.int32, device=dev)
        g2l.append(g)
    l2g = torch.cat(maps)
    l2g_off = torch.zeros(W + 1, dtype=torch.int64, device=dev)
    l2g_off[1:] = torch.tensor([m.numel() for m in maps], device=dev).cumsum(0)
    res = {"metric": "sharded_recommend_virtual_ranks", "users": U, "items": I, "dim": D, "world": W, "seen_per_user": a.seen,
           "exclusion_entries": int(ex[1].numel()), "legs": []}
    for k in [int(x) for x in a.ks.split(",")]:
        split = lambda: [ops.csr_split_by_owner(ex[0], ex[1], g2l[r]) for r in range(W)]
        _, exl = timed(split)
        S = torch.empty(W, U, k, dtype=torch.float32, device=dev)
        P = torch.empty(W, U, k, dtype=torch.int32, device=dev)

        def score_parts():
            for r in range(W):
                s, p = ops.dot_catalog_topk(Q, parts[r], k, exclude=exl[r])
                S[r], P[r] = s, p

        def score_parts_only():
            for r in range(W):
                ops.dot_catalog_topk(Q, parts[r], k, exclude=exl[r])
        whole = lambda: ops.dot_catalog_topk(Q, C, k, exclude=ex)
        merge = lambda: ops.topk_lists_merge(S, P, W, U, k, l2g, l2g_off)
        score_parts()
        for f in (whole, score_parts_only, merge, split):                     # warm-up: code objects, allocator
            timed(f)
        t = {"whole": [], "parts": [], "merge": [], "split": []}
        for _ in range(a.repeats):                                            # alternating
            t["whole"].append(timed(whole)[0]); t["parts"].append(timed(score_parts_only)[0])
            t["merge"].append(timed(merge)[0]); t["split"].append(timed(split)[0])
        _, (ws, wp) = timed(whole)
        _, (ms, mp) = timed(merge)
        med = {n: float(np.median(v)) for n, v in t.items()}
        res["legs"].append({
            "k": k, "whole_s": med["whole"], "parts_sum_s": med["parts"], "merge_s": med["merge"], "split_sum_s": med["split"],
            "all": t, "parts_over_whole": med["parts"] / med["whole"], "merge_plus_split_over_parts": (med["merge"] + med["split"]) / med["parts"],
            "merge_plus_split_over_parts_per_device": (med["merge"] + med["split"] / W) / (med["parts"] / W),
            "bit_equal_scores": bool(torch.equal(ms.view(torch.int32), ws.view(torch.int32))), "bit_equal_index": bool(torch.equal(mp, wp)),
            # per rank and call, derived from the sizes (each rank asking for users / W of the users)
            "bytes_gather_design_per_rank": I * D * 4 * (W - 1) // W,         # catalog="gather": every candidate row another rank owns
            "bytes_owners_design_per_rank": (U // W) * (W - 1) * D * 4 + (U // W) * (W - 1) * 2 * k * 4})      # user rows out + lists back
        del S, P
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
