"""The per-step NeuMF batch sampler (NeuMFEngine.sample_batch, csrc/sampling_epoch.hip) at the benchmark's shape (1 M users x 100 K items,
dim 64, batch 65 536, adam_dense deferred, the step replayed as one hipGraph), and what it buys on data.ml1m_shaped.

Timing (device events, one process, the variants alternated round after round; the spread = the rounds of one variant):
  the sampler launch alone (uniform, popularity; row0 walks through the epoch), BPR's one-candidate launch of the same batch in the same
  run (its record: profiles/sampling/bpr_sampler_bench.json), the step alone, step + sampler (the batch formed into the graph's own
  inputs), and the path it replaces: per epoch one torch.randperm and three index-selects over all n (1 + r) stored rows, divided by the
  steps of an epoch.  Records, not bars; the step alone is the step nobody touched.
Quality: static negatives (bootstrap_dataset, drawn once, no collision check), per-step uniform and per-step popularity, the same config
  and epochs each, no tuning: NDCG@10 / MRR (NeuMFEngine.rank_metrics, the training positives excluded) and full AUC over the held-out
  tenth.

    python tools/neumf_sampler_bench.py --out profiles/sampling/neumf_sampler_bench.json
"""
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

neumf, bpr, ops, data, models = (import_module("binary-recommendation_amd." + m) for m in ("neumf", "bpr", "ops", "data", "models"))
BPR_ONE_CANDIDATE_US = 8.4          # profiles/sampling/bpr_sampler_bench.json, "sampler uniform M=1"


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


def timing(args, dev):
    U, I, B, r = args.users, args.items, args.batch, args.neg_per_pos
    e = neumf.NeuMFEngine(neumf.NeuMFConfig("A", dim=64, optimizer="adam_dense"), U, I, dev, B, init_seed=1)
    e.enable_graph(B)
    rng = np.random.default_rng(6)
    w = 1.0 / np.arange(1, I + 1) ** 0.9
    pu, pi = rng.integers(0, U, args.positives).astype(np.int32), rng.choice(I, size=args.positives, p=w / w.sum()).astype(np.int32)
    mk = lambda mode: neumf.BatchSampler(pu, pi, U, neg_per_pos=r, mode=mode, seed=1, n_items=I, device=dev)
    samplers = {"uniform": mk("uniform"), "popularity": mk("popularity")}
    N = samplers["uniform"].rows_per_epoch
    steps_per_epoch = -(-N // B)
    bs = bpr.NegativeSampler(pu, pi, U, mode="uniform", candidates=1, seed=1, device=dev, n_items=I)
    be = bpr.BPREngine(U, I, 64, dev, B, optimizer="adam_dense")
    pool = [e.sample_batch(samplers["uniform"], 0, k * B, B) for k in range(16)]          # 16 batches of the epoch, for the step alone
    out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev))
    out_neg = torch.empty(B, dtype=torch.int32, device=dev)
    k = [0]

    def row0():
        k[0] += 1
        return (k[0] % (steps_per_epoch - 1)) * B          # full batches of the epoch, one after the other

    def sampler_alone(s):
        return lambda: e.sample_batch(s, 1, row0(), B, out=out)

    def bpr_alone():
        k[0] += 1
        be.sample_negatives(pool[k[0] % 16][0], None, bs, pos0=0, out=out_neg)

    def step_alone():
        k[0] += 1
        e.train_step(*pool[k[0] % 16])

    def step_with(s):
        ins = (e.in_users, e.in_items, e.in_labels)
        return lambda: e.train_step(*e.sample_batch(s, 1, row0(), B, out=ins))
    # the path this replaces: the stored epoch shuffled on the host's say-so, per epoch
    su, si, sy = ops.bootstrap_dataset(samplers["uniform"].users, samplers["uniform"].items, N - args.positives, 1)
    g = torch.Generator(device=dev).manual_seed(1)

    def shuffle_epoch():
        perm = torch.randperm(N, device=dev, generator=g)
        return su[perm], si[perm], sy[perm]
    for _ in range(args.prime):
        step_alone()
    variants = {"sampler uniform": (sampler_alone(samplers["uniform"]), args.iters), "sampler popularity": (sampler_alone(samplers["popularity"]), args.iters),
                "bpr sampler uniform M=1 (same run)": (bpr_alone, args.iters), "step alone": (step_alone, args.step_iters),
                "step + sampler uniform": (step_with(samplers["uniform"]), args.step_iters),
                "step + sampler popularity": (step_with(samplers["popularity"]), args.step_iters),
                "epoch shuffle of the stored rows (randperm + 3 index-selects)": (shuffle_epoch, 2)}
    for fn, _ in variants.values():          # warm every shape
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, (fn, iters) in variants.items():
            times[n].append(timed(fn, iters))
    e.check_ids(); be.check_ids()
    res = {n: stats(v) for n, v in times.items()}
    sh = res["epoch shuffle of the stored rows (randperm + 3 index-selects)"]
    sh["per_step_us"] = round(sh["median_us"] / steps_per_epoch, 2)
    sh["stored_MB"] = round(N * 12 / 1e6, 1)
    for n in ("sampler uniform", "sampler popularity"):
        res[n]["bpr_one_candidate_recorded_us"] = BPR_ONE_CANDIDATE_US
    st = res["step alone"]
    for n in ("step + sampler uniform", "step + sampler popularity"):
        res[n]["over_step_alone_us"] = round(res[n]["median_us"] - st["median_us"], 2)
    return {"config": {"users": U, "items": I, "dim": 64, "batch": B, "positives": args.positives, "neg_per_pos": r, "rows_per_epoch": N,
                       "steps_per_epoch": steps_per_epoch, "optimizer": "adam_dense deferred", "step": "one hipGraph replay", "prime_steps": args.prime,
                       "steps_run": e.t}, "launches": res}


def quality(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    truth, seen = ops.truth_csr(nU, hu, hi, dev), ops.truth_csr(nU, tu, ti, dev)
    all_users = torch.arange(nU, dtype=torch.int32, device=dev)
    B, r, out = args.quality_batch, args.neg_per_pos, {}
    for name in ("static", "uniform per step", "popularity per step"):
        e = neumf.NeuMFEngine(neumf.NeuMFConfig("A", dim=args.quality_dim, optimizer="adam_dense", seed=args.seed), nU, nI, dev, B, init_seed=args.seed)
        e.enable_graph(B)
        model = models.KerasLikeNeuMF(e)
        if name == "static":
            su, si, sy = data.bootstrap_dataset(tu, ti, neg_ratio=float(r), seed=args.seed, device=dev)
            h = model.fit([su, si], sy, epochs=args.quality_epochs, batch_size=B, shuffle=True, seed=args.seed)
            neg = sy == 0
            collisions = float(torch.isin(su[neg].long() * nI + si[neg].long(), torch.from_numpy(tu.astype(np.int64) * nI + ti).to(dev)).float().mean().item())
        else:
            s = neumf.BatchSampler(tu, ti, nU, neg_per_pos=r, mode=name.split()[0], seed=args.seed, n_items=nI, device=dev)
            h = model.fit(sampler=s, epochs=args.quality_epochs, batch_size=B)
            collisions = 0.0
        e.check_ids()
        rm = e.rank_metrics(all_users, truth, ks=(10,), exclude=seen)
        auc = e.full_auc(all_users, truth)
        e.check_ids()
        out[name] = {"ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5), "mrr": round(float(torch.nanmean(rm["mrr"]).item()), 5),
                     "full_auc": round(float(torch.nanmean(auc).item()), 5), "negatives_that_are_training_positives": round(collisions, 4),
                     "loss_per_epoch": [round(x, 5) for x in h.history["loss"]]}
        del e, model
    return {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "variant": "A", "dim": args.quality_dim, "batch": B,
            "neg_per_pos": r, "epochs": args.quality_epochs,
            "note": "one config for all three, no tuning; the training losses are over different negatives: not comparable across rows", "runs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--positives", type=int, default=4_000_000)
    ap.add_argument("--neg-per-pos", type=int, default=3)
    ap.add_argument("--prime", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--quality-epochs", type=int, default=10)
    ap.add_argument("--quality-batch", type=int, default=4096)
    ap.add_argument("--quality-dim", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit of the tree that is measured (default: git rev-parse HEAD)")
    ap.add_argument("--uncommitted", action="store_true", help="the tree holds changes on top of that commit (default: asked of git status)")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neumf_sampler_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/neumf_sampler_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
           "device": torch.cuda.get_device_name(0)}
    if not args.skip_timing:
        res["timing"] = timing(args, dev)
    if not args.skip_quality:
        res["quality"] = quality(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
