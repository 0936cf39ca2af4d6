"""The log-Q correction of the TwoTower in-batch softmax (candidate_sampling_probability): what the corrected sweeps cost
against their twins and against the extra-column route, and what the correction buys on data.ml1m_shaped.
Record: profiles/softmax_logq/softmax_logq_bench.json.

Timing: the method of tools/softmax_hard_bench.py (one process, device events around windows of back-to-back calls, the variants
alternating over `rounds` rounds, median / min / max).  At 8 192 x 8 192 x 64 and x 24, plain and M = 8, every sweep three ways:
  * "logq": the log-Q entry (logq=);
  * "twin": the same entry without the correction;
  * "column": the extra-column route - the entries without the correction on [q, 1], [c, -b] at dim + 1 (65: past the one-sweep
    lse + dQ and past the bf16x6 gradient bodies; 25: the width class of 24).  The widened copies are made outside the timed calls.
`spread` of a variant = (max - min) / median of its windows; a ratio is called outside the spread when it differs from 1 by more
than the sum of the two spreads.
Step: the eager TwoTower step at batch 8 192 (embedDim 64, semb 64, 1 M users x 100 K items), with and without the option.
Quality: the protocol of tools/softmax_hard_bench.py (10 epochs on the first 90 % of data.ml1m_shaped, NDCG@10 / MRR of the held-out
tenth through rank_metrics, training positives excluded): {plain, M = 8} x {temperature 1, 0.1} x {uncorrected, corrected with the item
frequencies of the training part}."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from importlib import import_module

from tools.softmax_hard_bench import alternate, commit, dirty

tt, ops, data = (import_module("binary-recommendation_amd." + m) for m in ("two_tower", "ops", "data"))


def _spread(r):
    return (r["max_us"] - r["min_us"]) / r["median_us"]


def _ratio(res, a, b):
    r = res[a]["median_us"] / res[b]["median_us"]
    s = _spread(res[a]) + _spread(res[b])
    return {"ratio": round(r, 3), "spread": round(s, 3), "outside_spread": bool(abs(r - 1) > s)}


def kernels(args, dev):
    out = {}
    for B, S in ((8192, 64), (8192, 24)):
        g = torch.Generator(device=dev).manual_seed(3)
        q, c = torch.randn(B, S, device=dev, generator=g) * 0.3, torch.randn(B, S, device=dev, generator=g) * 0.3
        ids = torch.randint(0, 100000, (B,), device=dev, dtype=torch.int32, generator=g)
        b = torch.log(torch.rand(B, device=dev, generator=g).clamp(1e-6, 1.0))
        q1 = torch.cat([q, torch.ones(B, 1, device=dev)], 1).contiguous()
        c1 = torch.cat([c, -b[:, None]], 1).contiguous()
        lse, slots = torch.empty(B, device=dev), torch.zeros(64, dtype=torch.float64, device=dev)
        dq, dc, dq1, dc1 = torch.empty_like(q), torch.empty_like(c), torch.empty_like(q1), torch.empty_like(c1)
        M = 8
        mk = lambda: (torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        thr = {"logq": mk(), "twin": mk(), "column": mk()}
        ops.inbatch_softmax_hard_threshold(q, c, ids, ids, 0, M, *thr["logq"], logq=b)
        ops.inbatch_softmax_hard_threshold(q, c, ids, ids, 0, M, *thr["twin"])
        ops.inbatch_softmax_hard_threshold(q1, c1, ids, ids, 0, M, *thr["column"])
        ops.inbatch_softmax_lse(q, c, ids, ids, 0, lse, slots, logq=b)
        v = {}
        for way, (Q, C, DQ, DC, lq) in (("logq", (q, c, dq, dc, b)), ("twin", (q, c, dq, dc, None)), ("column", (q1, c1, dq1, dc1, None))):
            v[f"threshold M={M} {way}"] = lambda Q=Q, C=C, lq=lq, way=way: ops.inbatch_softmax_hard_threshold(Q, C, ids, ids, 0, M, *thr[way], logq=lq)
            for name, t in (("plain", None), (f"M={M}", thr[way])):
                v[f"lse {name} {way}"] = lambda Q=Q, C=C, lq=lq, t=t: ops.inbatch_softmax_lse(Q, C, ids, ids, 0, lse, slots, thr=t, logq=lq)
                v[f"lse+dQ {name} {way}"] = lambda Q=Q, C=C, DQ=DQ, lq=lq, t=t: ops.inbatch_softmax_lse_grad_q(Q, C, ids, ids, 0, lse, slots, DQ, thr=t, logq=lq)
                v[f"dC {name} {way}"] = lambda Q=Q, C=C, DC=DC, lq=lq, t=t: ops.inbatch_softmax_grad(Q, C, ids, ids, 0, lse, None, DC, thr=t, logq=lq)
        res = alternate(v, args.rounds, args.window_ms)
        ratios = {}
        for n in list(v):
            if n.endswith(" logq"):
                stem = n[:-len(" logq")]
                ratios[f"{stem}: logq / twin"] = _ratio(res, n, stem + " twin")
                ratios[f"{stem}: logq / column"] = _ratio(res, n, stem + " column")
        res["ratios"] = ratios
        out[f"{B}x{B}x{S}"] = res
    return out


def step(args, dev):
    U, I, E, S, B = 1_000_000, 100_000, 64, 64, 8192
    g = torch.Generator(device=dev).manual_seed(4)
    users = torch.randint(2, U + 2, (B,), device=dev, dtype=torch.int32, generator=g)
    items = torch.randint(2, I + 2, (B,), device=dev, dtype=torch.int32, generator=g)
    p = torch.rand(I + 2, generator=torch.Generator().manual_seed(5)) / I
    v = {}
    for name, kw in (("plain", {}), ("plain logq", dict(candidate_sampling_probability=p)), ("M=8", dict(num_hard_negatives=8)),
                     ("M=8 logq", dict(num_hard_negatives=8, candidate_sampling_probability=p))):
        e = tt.TwoTowerEngine(E, I, U, S, dev, B, **kw)
        v[name] = lambda e=e: e.train_step(users, items)
    res = alternate(v, args.rounds, args.window_ms)
    res["ratios"] = {"plain: logq / uncorrected": _ratio(res, "plain logq", "plain"), "M=8: logq / uncorrected": _ratio(res, "M=8 logq", "M=8")}
    res["note"] = "eager step from the Python host, batch 8 192, embedDim 64, semb 64, 1 M users x 100 K items, uniform ids"
    return res


def quality(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    truth, seen = ops.truth_csr(nU, hu, hi + 2, dev), ops.truth_csr(nU, tu, ti + 2, dev)
    all_users = torch.arange(2, nU + 2, dtype=torch.int32, device=dev)
    B, out = args.quality_batch, {}
    U_, I_ = torch.from_numpy(tu + 2).to(dev).int(), torch.from_numpy(ti + 2).to(dev).int()
    # the item frequencies of the training part (what TwoTowerModel.itemFrequencies gives), the reserved rows p = 1
    p = np.concatenate([np.ones(2), np.bincount(ti, minlength=nI) / len(ti)])
    for M in (None, 8):
        for tau in (None, 0.1):
            for corrected in (False, True):
                e = tt.TwoTowerEngine(64, nI, nU, 64, dev, B, init_seed=args.seed, num_hard_negatives=M, temperature=tau,
                                      candidate_sampling_probability=p if corrected else None)
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
                out[f"{'plain' if M is None else f'M={M}'}, temperature {1 if tau is None else tau}, {'corrected' if corrected else 'uncorrected'}"] = {
                    "ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5), "mrr": round(float(torch.nanmean(rm["mrr"]).item()), 5),
                    "loss_per_epoch": losses}
                del e
    return {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "embedDim": 64, "semb": 64, "batch": B,
            "epochs": args.quality_epochs, "optimizer": "Adagrad 0.1", "p": "item frequency of the training part; items never seen there: clip at 1e-6",
            "note": "the losses of different rows are over different logits: not comparable across rows", "runs": out}


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
        sys.exit("softmax_logq_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/softmax_logq_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
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
