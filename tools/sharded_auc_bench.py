"""What counting the full-catalogue AUC at the item owners costs beside counting it in one launch, on ONE device with W virtual ranks
(the item table dealt r::W, as tests/test_gpu_sharded_auc.py does): per row width the times of

  whole       : the one brDotCatalogAuc[Wide] call over all users x all candidates (csrc/auc_dot.hip: the kernels the
                single-device engines run), its three launches together
  (c) counts  : the W brDotAucOwnerCount calls over all users x one owner's candidates, summed
  (a) around  : the W brDotAucOwnerPositives calls + brAucSortPieces over the W pieces of every user + brAucFinalizeLists
  (b) split   : brCsrSplitByOwner of the truth CSR, summed over the W owners

medians of --repeats alternating repeats, device events around synchronised work (the ops wrappers as a caller uses them: they include
their output / workspace allocations, so they bound the kernels from above), and the values through the owners are compared bit for bit
with the whole call.  On W real devices (c) and the positives run in parallel, one part per device: counts / W is the per-device
counting time there, while the sort runs over ALL users on every device.  The bytes each design moves per rank are derived from the
sizes, not timed: one device here, no exchange.  Prints one JSON line; --out FILE writes it.

    python tools/sharded_auc_bench.py [--users 65536] [--items 100000] [--dims 64,350] [--world 8] [--pos 20] [--repeats 3] [--out FILE]
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
    ap.add_argument("--dims", default="64,350")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--pos", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sharded_auc_bench: no GPU")
    from importlib import import_module
    ops = import_module("binary-recommendation_amd.ops")
    dev = torch.device("cuda:0")
    U, I, W = a.users, a.items, a.world
    res = {"metric": "sharded_auc_virtual_ranks", "users": U, "items": I, "world": W, "pos_per_user": a.pos, "legs": []}
    for D in [int(x) for x in a.dims.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(7)
        Q = torch.empty(U, D, device=dev).uniform_(-0.05, 0.05, generator=gen)
        C = torch.empty(I, D, device=dev).uniform_(-0.05, 0.05, generator=gen)
        cols = torch.randint(0, I, (U * a.pos,), generator=gen, device=dev).cpu().numpy()
        off, idx = ops.truth_csr(U, np.repeat(np.arange(U), a.pos), cols, dev)
        T = int(idx.numel())
        parts = [C[r::W].contiguous() for r in range(W)]                         # owner r holds the rows r, r + W, ..
        g2l = []
        for r in range(W):
            m = torch.arange(r, I, W, device=dev)
            g = torch.full((I,), -1, dtype=torch.int32, device=dev)
            g[m] = torch.arange(m.numel(), dtype=torch.int32, device=dev)
            g2l.append(g)
        whole = lambda: ops.dot_auc_for(D)(Q, C, off, idx)
        split = lambda: [ops.csr_split_by_owner(off, idx, g2l[r]) for r in range(W)]
        _, loc = timed(split)
        lens = torch.stack([po[1:] - po[:-1] for po, _pi in loc])
        m = int(lens.sum(1).max().item())
        buf = torch.zeros(W, m, dtype=torch.float32, device=dev)                  # the all-gather's receive buffer
        piece_off = torch.zeros(W, U + 1, dtype=torch.int64, device=dev)
        piece_off[:, 1:] = lens.cumsum(1)
        piece_off += (torch.arange(W, dtype=torch.int64, device=dev) * m).view(W, 1)
        w2 = torch.zeros(W * U, dtype=torch.int64, device=dev)                    # the all-to-all's receive buffer
        state = {}

        def around():
            for r in range(W):
                ops.dot_auc_owner_positives(Q, parts[r], loc[r][0], loc[r][1], out=buf[r])
            state["sorted"], state["pcnt"] = ops.auc_sort_pieces(buf, piece_off, off, T)
            return ops.auc_finalize_lists(w2, W, U, off, state["pcnt"], I)

        def counts(keep=False):
            for r in range(W):
                c = ops.dot_auc_owner_count(Q, parts[r], loc[r][0], loc[r][1], off, state["sorted"], state["pcnt"])
                if keep:
                    w2[r * U:(r + 1) * U] = c
        around()
        counts(keep=True)
        for f in (whole, counts, around, split):                                  # warm-up: code objects, allocator
            timed(f)
        t = {"whole": [], "counts": [], "around": [], "split": []}
        for _ in range(a.repeats):                                                # alternating
            t["whole"].append(timed(whole)[0]); t["counts"].append(timed(counts)[0])
            t["around"].append(timed(around)[0]); t["split"].append(timed(split)[0])
        _, want = timed(whole)
        _, got = timed(around)
        med = {n: float(np.median(v)) for n, v in t.items()}
        nan_w, nan_g = torch.isnan(want), torch.isnan(got)
        res["legs"].append({
            "dim": D, "truth_entries": T, "whole_s": med["whole"], "counts_sum_s": med["counts"], "around_s": med["around"],
            "split_sum_s": med["split"], "all": t, "counts_over_whole": med["counts"] / med["whole"],
            "around_plus_split_over_counts": (med["around"] + med["split"]) / med["counts"],
            "bit_equal": bool(torch.equal(nan_w, nan_g) and torch.equal(want[~nan_w], got[~nan_g])),
            # per rank and call, derived from the sizes (each rank asking for users / W of the users)
            "bytes_gather_design_per_rank": I * D * 4 * (W - 1) // W,             # catalog="gather": every candidate row another rank owns
            "bytes_owners_design_per_rank": (U * (W - 1) // W) * 4 * D + 8 * T * (W - 1) // W + 4 * U * (W - 1) + 16 * U * (W - 1) // W})   # + the owners' per-user counts, the truth lengths, the partials
        del Q, C, parts, buf, w2
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
