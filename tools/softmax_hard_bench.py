"""Hard negatives and temperature of the TwoTower in-batch softmax: what the threshold sweep and the hard forms cost, and
what the options buy on data.ml1m_shaped.  Record: profiles/softmax_hard/softmax_hard_bench.json.

Timing, all in ONE process, device events around a window of back-to-back calls - as many as fill about `window_ms` (30 ms; counted
from a first probe of 10 calls, at least 10), so that a window is long against the clock's resolution and the launch queue -
`rounds` rounds in which the variants alternate, median / min / max over the rounds (every launch is warmed up first; the workspace
is allocated by then):
  * the threshold sweep (ops.inbatch_softmax_hard_threshold) against ops.inbatch_softmax_lse of the same operands;
  * lse + dQ in one sweep, hard against plain;  * dC, hard against plain;
    at 8 192 x 8 192 x 64 and the stripe of config 4, 1 024 x 65 536 x 64, each with M = 8 and M = 64;
  * the dC sweep of a row-sharded rank at config 4: its 1 024 candidates against the 65 536 gathered queries, plain against hard
    (ops.inbatch_softmax_grad(thr_slice=): the thresholds' arithmetic, bf16x6 here, where the plain rule runs 1 024 candidates on fp32);
  * the eager TwoTower step (batch 8 192, embedDim 64, semb 64, 1 M users x 100 K items), plain against M = 8 / M = 64 / temperature.
Quality: 10 epochs on the first 90 % of data.ml1m_shaped, NDCG@10 / MRR of the held-out tenth through TwoTowerEngine.rank_metrics
(training positives excluded): plain, M = 8 and M = 64, each at temperature 1 and 0.1."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from importlib import import_module

tt, ops, data = (import_module("binary-recommendation_amd." + m) for m in ("two_tower", "ops", "data"))


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip() or None
    except Exception:  # noqa: BLE001
        return None


def dirty():
    try:
        return bool(subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip())
    except Exception:  # noqa: BLE001
        return False


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def stats(xs):
    xs = sorted(xs)
    return {"median_us": round(xs[len(xs) // 2], 2), "min_us": round(xs[0], 2), "max_us": round(xs[-1], 2), "rounds": len(xs)}


def alternate(variants, rounds, window_ms):
    """variants: {name: fn} -> {name: stats + calls per window}; every round runs every variant once, the order rotating"""
    names = list(variants)
    iters = {}
    for n in names:
        for _ in range(3):
            variants[n]()
        torch.cuda.synchronize()
        iters[n] = max(10, int(window_ms * 1e3 / max(timed(variants[n], 10), 1.0)))
    got = {n: [] for n in names}
    for r in range(rounds):
        for k in range(len(names)):
            n = names[(k + r) % len(names)]
            got[n].append(timed(variants[n], iters[n]))
    return {n: dict(stats(v), calls_per_window=iters[n]) for n, v in got.items()}


def kernels(args, dev):
    out = {}
    for Bq, Bc, S in ((8192, 8192, 64), (1024, 65536, 64)):
        g = torch.Generator(device=dev).manual_seed(3)
        q, c = torch.randn(Bq, S, device=dev, generator=g) * 0.3, torch.randn(Bc, S, device=dev, generator=g) * 0.3
        ids_c = torch.randint(0, 100000, (Bc,), device=dev, dtype=torch.int32, generator=g)
        ids_q = ids_c[:Bq].contiguous()
        lse, slots = torch.empty(Bq, device=dev), torch.zeros(64, dtype=torch.float64, device=dev)
        dq, dc = torch.empty_like(q), torch.empty_like(c)
        thr = {M: (torch.empty(Bq, device=dev), torch.empty(Bq, dtype=torch.int32, device=dev)) for M in (8, 64)}
        for M in (8, 64):
            ops.inbatch_softmax_hard_threshold(q, c, ids_q, ids_c, 0, M, *thr[M])
        ops.inbatch_softmax_lse(q, c, ids_q, ids_c, 0, lse, slots)
        v = {"lse plain": lambda: ops.inbatch_softmax_lse(q, c, ids_q, ids_c, 0, lse, slots),
             "lse+dQ plain": lambda: ops.inbatch_softmax_lse_grad_q(q, c, ids_q, ids_c, 0, lse, slots, dq),
             "dC plain": lambda: ops.inbatch_softmax_grad(q, c, ids_q, ids_c, 0, lse, None, dc)}
        for M in (8, 64):
            v[f"threshold M={M}"] = lambda M=M: ops.inbatch_softmax_hard_threshold(q, c, ids_q, ids_c, 0, M, *thr[M])
            v[f"lse+dQ hard M={M}"] = lambda M=M: ops.inbatch_softmax_lse_grad_q(q, c, ids_q, ids_c, 0, lse, slots, dq, thr=thr[M])
            v[f"dC hard M={M}"] = lambda M=M: ops.inbatch_softmax_grad(q, c, ids_q, ids_c, 0, lse, None, dc, thr=thr[M])
        res = alternate(v, args.rounds, args.window_ms)
        med = lambda n: res[n]["median_us"]
        res["ratios"] = {f"threshold M={M} / lse plain": round(med(f"threshold M={M}") / med("lse plain"), 3) for M in (8, 64)}
        res["ratios"].update({f"lse+dQ hard M={M} / plain": round(med(f"lse+dQ hard M={M}") / med("lse+dQ plain"), 3) for M in (8, 64)})
        res["ratios"].update({f"dC hard M={M} / plain": round(med(f"dC hard M={M}") / med("dC plain"), 3) for M in (8, 64)})
        res["workspace_bytes"] = {f"M={M}": int(ops._lib.load().brInBatchSoftmaxHardWorkspaceBytes(Bq, Bc, S, M)) for M in (8, 64)}
        out[f"{Bq}x{Bc}x{S}"] = res
    # the dC sweep of one rank of config 4: 65 536 gathered queries stream past the rank's 1 024 candidates (rows [c0, c0 + 1 024) of the gathered)
    Bq, Bl, S, c0 = 65536, 1024, 64, 3 * 1024
    g = torch.Generator(device=dev).manual_seed(5)
    q, c = torch.randn(Bq, S, device=dev, generator=g) * 0.3, torch.randn(Bq, S, device=dev, generator=g) * 0.3
    ids = torch.randint(0, 100000, (Bq,), device=dev, dtype=torch.int32, generator=g)
    cl, idl = c[c0:c0 + Bl].contiguous(), ids[c0:c0 + Bl].contiguous()
    lse, dcl = torch.full((Bq,), 10.0, device=dev), torch.empty(Bl, S, device=dev)      # any finite lse: the sweep's time does not depend on it
    v = {"dC plain": lambda: ops.inbatch_softmax_grad(q, cl, ids, idl, -c0, lse, None, dcl)}
    for M in (8, 64):
        thr = (torch.empty(Bq, device=dev), torch.empty(Bq, dtype=torch.int32, device=dev))
        for r0 in range(0, Bq, 8192):      # the thresholds of all queries, a stripe at a time as the ranks form them
            ops.inbatch_softmax_hard_threshold(q[r0:r0 + 8192], c, ids[r0:r0 + 8192].contiguous(), ids, r0, M, thr[0][r0:r0 + 8192], thr[1][r0:r0 + 8192])
        v[f"dC hard M={M}"] = lambda thr=thr: ops.inbatch_softmax_grad(q, cl, ids, idl, -c0, lse, None, dcl, thr=thr, thr_slice=(c0, Bq))
    res = alternate(v, args.rounds, args.window_ms)
    res["ratios"] = {f"dC hard M={M} / plain": round(res[f"dC hard M={M}"]["median_us"] / res["dC plain"]["median_us"], 3) for M in (8, 64)}
    res["note"] = "65 536 gathered queries against one rank's 1 024 candidates; plain: fp32 MFMA by the plain rule, hard: bf16x6 as the thresholds' sweep"
    out["rank dC 65536x1024x64"] = res
    return out


def step(args, dev):
    U, I, E, S, B = 1_000_000, 100_000, 64, 64, 8192
    g = torch.Generator(device=dev).manual_seed(4)
    users = torch.randint(2, U + 2, (B,), device=dev, dtype=torch.int32, generator=g)
    items = torch.randint(2, I + 2, (B,), device=dev, dtype=torch.int32, generator=g)
    v = {}
    for name, kw in (("plain", {}), ("M=8", dict(num_hard_negatives=8)), ("M=64", dict(num_hard_negatives=64)), ("temperature 0.1", dict(temperature=0.1)),
                     ("M=8 temperature 0.1", dict(num_hard_negatives=8, temperature=0.1))):
        e = tt.TwoTowerEngine(E, I, U, S, dev, B, **kw)
        v[name] = lambda e=e: e.train_step(users, items)
    res = alternate(v, args.rounds, args.window_ms)
    res["note"] = "eager step from the Python host, batch 8 192, embedDim 64, semb 64, 1 M users x 100 K items, uniform ids"
    return res


def quality(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    # StringLookup indices: vocabulary entry k is row k + 2 of the tables; the candidates of rank_metrics are the table's rows
    truth, seen = ops.truth_csr(nU, hu, hi + 2, dev), ops.truth_csr(nU, tu, ti + 2, dev)
    all_users = torch.arange(2, nU + 2, dtype=torch.int32, device=dev)
    B, out = args.quality_batch, {}
    U_, I_ = torch.from_numpy(tu + 2).to(dev).int(), torch.from_numpy(ti + 2).to(dev).int()
    for M in (None, 8, 64):
        for tau in (None, 0.1):
            e = tt.TwoTowerEngine(64, nI, nU, 64, dev, B, init_seed=args.seed, num_hard_negatives=M, temperature=tau)
            g = torch.Generator(device=dev).manual_seed(args.seed)
            losses = []
            for _ in range(args.quality_epochs):
                perm = torch.randperm(U_.shape[0], device=dev, generator=g)
                uu, pp = U_[perm], I_[perm]
                for lo in range(0, uu.shape[0], B):
                    e.train_step(uu[lo:lo + B], pp[lo:lo + B])
                losses.append(round(e.pop_loss(), 3))
            e.check_ids()
            rm = e.rank_metrics(all_users, truth, ks=(10,), exclude=seen)
            out[f"{'plain' if M is None else f'M={M}'}, temperature {1 if tau is None else tau}"] = {
                "ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5), "mrr": round(float(torch.nanmean(rm["mrr"]).item()), 5),
                "loss_per_epoch": losses}
            del e
    return {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "embedDim": 64, "semb": 64, "batch": B,
            "epochs": args.quality_epochs, "optimizer": "Adagrad 0.1",
            "note": "the losses of different rows are over different column sets and temperatures: not comparable across rows", "runs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0, help="length of one timing window (the calls per window follow from a probe)")
    ap.add_argument("--quality-epochs", type=int, default=10)
    ap.add_argument("--quality-batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit of the tree that is measured (default: git rev-parse HEAD; for a tree without its .git)")
    ap.add_argument("--uncommitted", action="store_true", help="the tree holds changes on top of that commit (default: asked of git status)")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("softmax_hard_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/softmax_hard_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
           "device": torch.cuda.get_device_name(0)}
    if not args.skip_timing:
        res["kernels"] = kernels(args, dev)
        res["step"] = step(args, dev)
    if not args.skip_quality:
        res["quality"] = quality(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
