"""Implicit-feedback ALS (csrc/als.hip, als.ALSEngine) on the device: the two kernels against their bounds, the torch route they
replace, and what the model reaches on data.ml1m_shaped.

Timing (device events, one process, warm-up first, `rounds` rounds of `iters` calls each; the spread = the rounds):
  brGram at 100 000 x 64, 1 000 000 x 64 and 100 000 x 128, rotating through enough copies of the table that no call finds it in the
    256 MB Infinity Cache; in us and as a share of the HBM read of Y (it reads Y once: that is its bound).
  brAlsSolveRows for both half-steps at 1 M users x 100 K items, 16 M pairs (users uniform, items Zipf 0.9 as tools/bpr_sampler_bench.py
    draws them; duplicates merged), dim 64 and 128; in us and against the flop count sum_u 2 P_u dim^2 + n_rows dim^3 / 3 at the 157.3 TF
    fp32 peak (MFMA and VALU alike).
  The same half-step with torch on the same card: per chunk of 4 096 rows, index_add_ of the entries' outer products into a
    (chunk, dim, dim) tensor (the entries taken 65 536 at a time so that the outer products fit), torch.linalg.cholesky + cholesky_solve.
Quality: data.ml1m_shaped, 10 epochs, dim 64, reg 0.01, alpha 40: NDCG@10 (rank_metrics, the training positives excluded) and full
  AUC over the held-out tenth - the split and the metrics of tools/bpr_sampler_bench.py's quality leg - and the same at four other
  settings of (reg, alpha).

    python tools/als_bench.py --out profiles/als/als_bench.json
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

als, ops, data = (import_module("binary-recommendation_amd." + m) for m in ("als", "ops", "data"))
HBM_PEAK = 8.0e12
FP32_PEAK = 157.3e12


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


def measure(fn, rounds, iters):
    fn()
    fn()
    torch.cuda.synchronize()
    return stats([timed(fn, iters) for _ in range(rounds)])


def gram_timing(args, dev):
    out = {}
    for rows, dim in ((100_000, 64), (1_000_000, 64), (100_000, 128)):
        nbytes = rows * dim * 4
        copies = max(2, -(-3 * 256 * 2 ** 20 // nbytes))                    # >= 3 x the Infinity Cache between two reads of one copy
        tabs = [torch.randn(rows, dim, device=dev) for _ in range(copies)]
        G = torch.empty(dim, dim, device=dev)
        k = [0]

        def f():
            k[0] += 1
            ops.gram(tabs[k[0] % copies], out=G)
        r = measure(f, args.rounds, max(args.iters, copies))
        r.update({"read_MB": round(nbytes / 1e6, 1), "copies_rotated": copies, "share_of_hbm_peak": round(nbytes / (r["median_us"] * 1e-6) / HBM_PEAK, 3),
                  "mfma_TFLOP_s": round(2 * rows * dim * dim * (0.75 if dim == 64 else 0.625) / (r["median_us"] * 1e-6) / 1e12, 1),
                  "workspace_MB": round(int(import_module("binary-recommendation_amd._lib").load().brGramWorkspaceBytes(rows, dim)) / 1e6, 2)})
        out[f"{rows} x {dim}"] = r
        del tabs
    return out


def torch_half_step(Y, G, off, idx, reg, alpha, X, chunk=4096, entries=65536):
    """the route the fused kernel replaces: the entries' outer products added into (chunk, dim, dim), then batched Cholesky"""
    dim = Y.shape[1]
    eye = reg * torch.eye(dim, device=Y.device)
    for r0 in range(0, X.shape[0], chunk):
        r1 = min(r0 + chunk, X.shape[0])
        e0, e1 = int(off[r0]), int(off[r1])
        A = (G + eye).expand(r1 - r0, dim, dim).contiguous()
        b = torch.zeros(r1 - r0, dim, device=Y.device)
        rows = torch.repeat_interleave(torch.arange(r1 - r0, device=Y.device), off[r0 + 1:r1 + 1] - off[r0:r1])
        for s in range(e0, e1, entries):
            t = min(s + entries, e1)
            y = Y[idx[s:t].long()]
            rr = rows[s - e0:t - e0]
            A.index_add_(0, rr, alpha * y[:, :, None] * y[:, None, :])
            b.index_add_(0, rr, (1 + alpha) * y)
        L = torch.linalg.cholesky(A)
        x = torch.cholesky_solve(b[:, :, None], L)[:, :, 0]
        x[off[r0 + 1:r1 + 1] == off[r0:r1]] = 0
        X[r0:r1] = x


def solve_timing(args, dev):
    U, I, N = args.users, args.items, args.pairs
    rng = np.random.default_rng(6)
    w = 1.0 / np.arange(1, I + 1) ** 0.9
    pu, pi = rng.integers(0, U, N).astype(np.int32), rng.choice(I, size=N, p=w / w.sum()).astype(np.int32)
    ucsr, icsr = als.csr_pair(torch.from_numpy(pu), torch.from_numpy(pi), U, I, dev)
    n_pairs = int(ucsr[1].numel())
    cnt_i = (icsr[0][1:] - icsr[0][:-1])
    cnt_u = (ucsr[0][1:] - ucsr[0][:-1])
    out = {"config": {"users": U, "items": I, "pairs_drawn": N, "distinct_pairs": n_pairs, "reg": 0.01, "alpha": 40.0,
                      "entries_per_user_row": {"mean": round(n_pairs / U, 1), "max": int(cnt_u.max())},
                      "entries_per_item_row": {"mean": round(n_pairs / I, 1), "max": int(cnt_i.max())}}}
    for dim in (64, 128):
        eng = als.ALSEngine(U, I, dim, dev)
        res = {}
        for side, csr, Y, X in (("user", ucsr, eng.item, eng.user), ("item", icsr, eng.user, eng.item)):
            n_rows = X.shape[0]
            flop = 2.0 * n_pairs * dim * dim + n_rows * dim ** 3 / 3.0
            G = ops.gram(Y)
            Xo = torch.empty_like(X)

            def fused():
                ops.als_solve_rows(Y, G, csr[0], csr[1], 0.01, 40.0, out=Xo, err_flag=eng.err)
            r = measure(fused, args.rounds, args.solve_iters)
            r.update({"rows": n_rows, "GFLOP": round(flop / 1e9, 1), "TFLOP_s": round(flop / (r["median_us"] * 1e-6) / 1e12, 2),
                      "share_of_fp32_peak": round(flop / (r["median_us"] * 1e-6) / FP32_PEAK, 4)})
            res[f"{side} half-step, fused"] = r
            if not args.skip_torch:
                Xt = torch.empty_like(X)

                def base():
                    torch_half_step(Y, G, csr[0], csr[1], 0.01, 40.0, Xt)
                rt = measure(base, max(2, args.rounds // 2), 1)
                res[f"{side} half-step, torch"] = rt
                r["speedup_over_torch"] = round(rt["median_us"] / r["median_us"], 1)
                nz = Xt.abs().sum(1) > 0
                r["max_rel_row_diff_to_torch"] = float(((Xo[nz] - Xt[nz]).norm(dim=1) / Xt[nz].norm(dim=1)).max().item())
            eng.half_step(side, csr)                 # the next side's Y: solved rows, as in a run
        eng.check_ids()
        out[f"dim {dim}"] = res
        del eng
    return out


def quality(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    truth, seen = ops.truth_csr(nU, hu, hi, dev), ops.truth_csr(nU, tu, ti, dev)
    all_users = torch.arange(nU, dtype=torch.int32, device=dev)
    ucsr, icsr = als.csr_pair(tu, ti, nU, nI, dev)

    def run(reg, alpha):
        e = als.ALSEngine(nU, nI, 64, dev, reg=reg, alpha=alpha, init_seed=args.seed)
        obj = []
        for _ in range(args.quality_epochs):
            e.epoch(ucsr, icsr)
            obj.append(round(e.objective(ucsr), 2))
        e.check_ids()
        rm = e.rank_metrics(all_users, truth, ks=(10,), exclude=seen)
        auc = e.full_auc(all_users, truth)
        return {"reg": reg, "alpha": alpha, "ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5),
                "mrr": round(float(torch.nanmean(rm["mrr"]).item()), 5), "full_auc": round(float(torch.nanmean(auc).item()), 5), "objective_per_epoch": obj}
    out = {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "dim": 64, "epochs": args.quality_epochs}
    out.update(run(0.01, 40.0))
    # the same data at other settings of the two hyper-parameters (reg 0.01 leaves 64 factors per row almost unregularised)
    out["other_settings"] = [{k: v for k, v in run(reg, alpha).items() if k != "objective_per_epoch"} for reg, alpha in ((10.0, 40.0), (100.0, 40.0), (30.0, 10.0), (30.0, 1.0))]
    out["bpr_ndcg@10_for_comparison"] = {"static": 0.311, "uniform per step": 0.318}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=16_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--solve-iters", type=int, default=3)
    ap.add_argument("--quality-epochs", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit of the tree that is measured (default: git rev-parse HEAD)")
    ap.add_argument("--uncommitted", action="store_true", help="the tree holds changes on top of that commit (default: asked of git status)")
    ap.add_argument("--skip-gram", action="store_true")
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("als_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/als_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
           "device": torch.cuda.get_device_name(0)}
    if not args.skip_gram:
        res["gram"] = gram_timing(args, dev)
    if not args.skip_solve:
        res["solve"] = solve_timing(args, dev)
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
