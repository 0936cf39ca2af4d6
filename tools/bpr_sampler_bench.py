"""The per-step BPR negative sampler (BPREngine.sample_negatives, csrc/sampling_step.hip) at config 3 of tools/other_models_bench.py
(1 M users x 100 K items, dim 64, batch 65 536, adam_dense deferred), and what it buys on data.ml1m_shaped.

Timing (device events, one process, the variants alternated round after round; the spread = the rounds of one variant):
  the sampler launch alone (uniform M = 1, popularity M = 1, hardest of M = 4 / 8 / 16), ops.gather_rows_deferred of the same B x M
  candidate ids (existing code that reads the same rows and WRITES them out: the yardstick of the fused launch) and of the B customer
  rows (which the fused launch replays too), the step alone, and step + sampler.  The tables are primed by steps first so that the
  rows lag as they do in a run, and every variant rotates through 16 batches, so the customer rows come from HBM as in a run.  The
  algorithmic bytes of a launch come from the shapes and the measured share of lagging rows; their share of the 8 TB/s HBM peak is
  nominal for the candidate rows: the item table (25.6 MB, 77 MB with its moments) stays in the 256 MB Infinity Cache.
Quality: static negatives (drawn once), per-step uniform and hardest-of-8, the same epochs each: NDCG@10 (BPREngine.rank_metrics, the
  training positives excluded) and full AUC over the held-out tenth.

    python tools/bpr_sampler_bench.py --out profiles/sampling/bpr_sampler_bench.json
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

bpr, ops, data = (import_module("binary-recommendation_amd." + m) for m in ("bpr", "ops", "data"))
HBM_PEAK = 8.0e12


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
    U, I, F, B = args.users, args.items, 64, args.batch
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda n, N: torch.randint(0, N, (n,), generator=g, device=dev, dtype=torch.int32)
    e = bpr.BPREngine(U, I, F, dev, B, optimizer="adam_dense")
    # a training set for the CSR and the popularity weights: 4 M positives, Zipf items
    rng = np.random.default_rng(6)
    w = 1.0 / np.arange(1, I + 1) ** 0.9
    pu, pi = rng.integers(0, U, args.positives).astype(np.int32), rng.choice(I, size=args.positives, p=w / w.sum()).astype(np.int32)
    mk = lambda mode, M: bpr.NegativeSampler(pu, pi, U, mode=mode, candidates=M, seed=1, device=dev, n_items=I)
    samplers = {"uniform M=1": mk("uniform", 1), "popularity M=1": mk("popularity", 1), **{f"hard M={M}": mk("uniform", M) for M in (4, 8, 16)}}
    pool = [(rnd(B, U), rnd(B, I)) for _ in range(16)]
    neg0 = rnd(B, I)
    k = [0]

    def batch():
        k[0] += 1
        return pool[k[0] % len(pool)]

    def step_alone():
        u, p = batch()
        e.train_step(u, p, neg0)

    def step_with(s):
        def f():
            u, p = batch()
            e.train_step(u, p, e.sample_negatives(u, p, s, pos0=k[0] * B))
        return f
    for _ in range(args.prime):
        step_alone()
    # every launch-alone variant rotates through the 16 batches (their customer rows with moments: 16 x 50 MB, more than the 256 MB
    # Infinity Cache holds beside the item table), as the steps do: a launch repeated on ONE batch would find its rows cached
    variants, cand_ids = {}, {}
    outs = {M: torch.empty(B * M, F, device=dev) for M in (4, 8, 16)}
    hp = (e.BETA1, e.BETA2, e.EPS)
    out_neg = torch.empty(B, dtype=torch.int32, device=dev)

    def sampler_alone(s):
        def f():
            u, p = batch()
            e.sample_negatives(u, p, s, pos0=0, out=out_neg)
        return f

    def gather_cands(M):
        def f():
            k[0] += 1
            ops.gather_rows_deferred(e._item, e.item_m, e.item_v, e.last["item"], cand_ids[M][k[0] % len(pool)], e.step_state, *hp, out=outs[M], err_flag=e.err)
        return f
    for name, s in samplers.items():
        M = s.candidates
        variants["sampler " + name] = (sampler_alone(s), args.iters)
        if M > 1:          # the ids that launch draws for each batch (at this step), for the gather of the same rows
            cand_ids[M] = [e.sample_negatives(u, p, s, pos0=0, dump=True)[1].reshape(-1).contiguous() for u, p in pool]
            variants[f"gather_rows_deferred B*M rows, M={M}"] = (gather_cands(M), args.iters)
    out_u = torch.empty(B, F, device=dev)

    def gather_users():
        u, _ = batch()
        ops.gather_rows_deferred(e._user, e.user_m, e.user_v, e.last["user"], u, e.step_state, *hp, out=out_u, err_flag=e.err)
    variants["gather_rows_deferred B user rows"] = (gather_users, args.iters)
    variants["step alone"] = (step_alone, args.step_iters)
    variants["step + sampler uniform M=1"] = (step_with(samplers["uniform M=1"]), args.step_iters)
    variants["step + sampler hard M=8"] = (step_with(samplers["hard M=8"]), args.step_iters)
    for fn, _ in variants.values():          # warm every shape
        fn()
    torch.cuda.synchronize()
    # the share of lagging rows at sampling time (what the launch's m / v reads depend on), before the timed steps move on
    t = e.t
    lag_user = float(torch.stack([(e.last["user"][u.long()] < t).float().mean() for u, _ in pool]).mean().item())
    lag_cand = {M: float(torch.stack([(e.last["item"][c.long()] < t).float().mean() for c in cs]).mean().item()) for M, cs in cand_ids.items()}
    times = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, (fn, iters) in variants.items():
            times[n].append(timed(fn, iters))
    e.check_ids()
    res = {n: stats(v) for n, v in times.items()}
    row = F * 4
    for M in (4, 8, 16):
        # theta of B user rows and B*M candidate rows, m and v of the lagging ones, last[] and ids, B x (M ids in, 1 id out)
        fused = B * row * (1 + 2 * lag_user) + B * M * row * (1 + 2 * lag_cand[M]) + 4 * B * (M + 1) + 4 * B * 2
        gathered = B * M * row * (1 + 2 * lag_cand[M]) + 4 * B * M * 2 + B * M * row         # the same candidate rows, and written out
        for name, nbytes in ((f"sampler hard M={M}", fused), (f"gather_rows_deferred B*M rows, M={M}", gathered)):
            r = res[name]
            r["algorithmic_MB"] = round(nbytes / 1e6, 2)
            r["TB_per_s"] = round(nbytes / (r["median_us"] * 1e-6) / 1e12, 3)
            r["share_of_hbm_peak"] = round(nbytes / (r["median_us"] * 1e-6) / HBM_PEAK, 3)
        res[f"sampler hard M={M}"]["lagging_candidate_rows"] = round(lag_cand[M], 3)
        f_, g_ = res[f"sampler hard M={M}"], res[f"gather_rows_deferred B*M rows, M={M}"]
        spread = max(g_["max_us"] - g_["min_us"], f_["max_us"] - f_["min_us"])
        both = g_["median_us"] + res["gather_rows_deferred B user rows"]["median_us"]          # the rows the fused launch reads: candidates AND customers
        f_["vs_gather"] = {"ratio_of_medians": round(f_["median_us"] / g_["median_us"], 3), "within_gather_plus_spread": bool(f_["median_us"] <= g_["median_us"] + spread),
                           "gathers_of_candidates_and_users_us": round(both, 2), "ratio_to_both_gathers": round(f_["median_us"] / both, 3)}
    return {"config": {"users": U, "items": I, "dim": F, "batch": B, "optimizer": "adam_dense deferred", "replay": e.replay, "prime_steps": args.prime,
                       "lagging_user_rows": round(lag_user, 3), "steps_run": e.t}, "launches": res}


def quality(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    truth, seen = ops.truth_csr(nU, hu, hi, dev), ops.truth_csr(nU, tu, ti, dev)
    all_users = torch.arange(nU, dtype=torch.int32, device=dev)
    B, out = args.quality_batch, {}
    U_, P_ = torch.from_numpy(tu).to(dev), torch.from_numpy(ti).to(dev)
    for name in ("static", "uniform per step", "hard M=8 per step"):
        e = bpr.BPREngine(nU, nI, 64, dev, B, optimizer="adam_dense", init_seed=args.seed)
        g = torch.Generator(device=dev).manual_seed(args.seed)
        if name == "static":
            u, p, n = data.sample_bpr_triplets(tu, ti, nU, nI, 1, args.seed, device=dev)
            s = None
        else:
            u, p, n = U_, P_, None
            s = bpr.NegativeSampler(tu, ti, nU, mode="uniform", candidates=8 if "hard" in name else 1, seed=args.seed, device=dev, n_items=nI)
        off, losses = 0, []
        for _ in range(args.quality_epochs):
            perm = torch.randperm(u.shape[0], device=dev, generator=g)
            uu, pp, nn = u[perm], p[perm], (n[perm] if s is None else None)
            for lo in range(0, u.shape[0], B):
                hi_ = min(lo + B, u.shape[0])
                neg = nn[lo:hi_] if s is None else e.sample_negatives(uu[lo:hi_], pp[lo:hi_], s, pos0=off + lo)
                e.train_step(uu[lo:hi_], pp[lo:hi_], neg)
            off += u.shape[0]
            losses.append(round(e.pop_loss(), 5))
        e.check_ids()
        rm = e.rank_metrics(all_users, truth, ks=(10,), exclude=seen)
        auc = e.full_auc(all_users, truth)
        out[name] = {"ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5), "mrr": round(float(torch.nanmean(rm["mrr"]).item()), 5),
                     "full_auc": round(float(torch.nanmean(auc).item()), 5), "loss_per_epoch": losses}
        del e
    return {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "dim": 64, "batch": B, "epochs": args.quality_epochs,
            "note": "the loss of the per-step hard run is on harder triplets: not comparable across rows", "runs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--positives", type=int, default=4_000_000)
    ap.add_argument("--prime", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--quality-epochs", type=int, default=10)
    ap.add_argument("--quality-batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit of the tree that is measured (default: git rev-parse HEAD)")
    ap.add_argument("--uncommitted", action="store_true", help="the tree holds changes on top of that commit (default: asked of git status)")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bpr_sampler_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/bpr_sampler_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
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
