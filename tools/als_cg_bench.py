"""The conjugate-gradient ALS half-step and the wide Gram (csrc/als_wide.hip) on the device: brAlsSolveRowsCg against brAlsSolveRows
where both exist, against a torch batched-CG route above 128 features, brGramWide against the HBM read of Y, and what the model
reaches on data.ml1m_shaped with 2, 3 and 5 steps.

Timing (device events, one process, 2 warm-up calls, `rounds` rounds of `iters` calls each; the spread = the rounds):
  both half-steps at 1 M users x 100 K items, 16 M pairs drawn (users uniform, items Zipf 0.9; duplicates merged) - tools/als_bench.py's
    workload.  dim 64 and 128: brAlsSolveRowsCg with 3 steps and brAlsSolveRows, the ratio stated.  dim 256, 350 and 512:
    brAlsSolveRowsCg with 3 steps and the same schedule with torch on the same card (the search directions of all rows as one matrix:
    P @ G, and the sparse term by a gather of the entries' rows, a row-wise dot and index_add_, the entries taken 2 M at a time).
    Every call starts from the same vectors: a device copy of the table inside the timed region, whose own time is reported beside it.
  brGramWide at 100 000 x 350 and 1 000 000 x 512, rotating through copies of the table so that no call finds it in the Infinity Cache;
    in us, as a share of the HBM read of Y and in TFLOP/s of the fp32 MFMA.
Quality: data.ml1m_shaped, 10 epochs, dim 64, reg 30, alpha 1 (tools/als_bench.py's best setting: Cholesky reached NDCG@10 0.277, full
  AUC 0.749): solver "cg" with 2, 3 and 5 steps, "cholesky" in the same process, and one "cg" run at dim 350.

    python tools/als_cg_bench.py --out profiles/als/als_cg_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from importlib import import_module

from tools.als_bench import FP32_PEAK, HBM_PEAK, commit, dirty, measure

als, ops, data = (import_module("binary-recommendation_amd." + m) for m in ("als", "ops", "data"))
REG, ALPHA, STEPS = 0.01, 40.0, 3


def workload(args, dev):
    U, I, N = args.users, args.items, args.pairs
    rng = np.random.default_rng(6)
    w = 1.0 / np.arange(1, I + 1) ** 0.9
    pu, pi = rng.integers(0, U, N).astype(np.int32), rng.choice(I, size=N, p=w / w.sum()).astype(np.int32)
    ucsr, icsr = als.csr_pair(torch.from_numpy(pu), torch.from_numpy(pi), U, I, dev)
    n_pairs = int(ucsr[1].numel())
    cnt_u, cnt_i = ucsr[0][1:] - ucsr[0][:-1], icsr[0][1:] - icsr[0][:-1]
    cfg = {"users": U, "items": I, "pairs_drawn": N, "distinct_pairs": n_pairs, "reg": REG, "alpha": ALPHA, "cg_steps": STEPS,
           "entries_per_user_row": {"mean": round(n_pairs / U, 1), "max": int(cnt_u.max())},
           "entries_per_item_row": {"mean": round(n_pairs / I, 1), "max": int(cnt_i.max())}}
    return ucsr, icsr, n_pairs, cfg


def torch_cg_half_step(Y, G, off, idx, reg, alpha, X, steps, entries=2_000_000):
    """the same schedule with torch: every row's vectors as the rows of one matrix; no row is ever frozen (a timing route)"""
    n_rows = X.shape[0]
    cnt = off[1:] - off[:-1]
    rows = torch.repeat_interleave(torch.arange(n_rows, device=Y.device), cnt)
    idl = idx.long()

    def sparse(P, with_b):
        q = torch.zeros_like(P)
        b = torch.zeros_like(P) if with_b else None
        for s in range(0, idl.numel(), entries):
            y, rr = Y[idl[s:s + entries]], rows[s:s + entries]
            t = (y * P[rr]).sum(1, keepdim=True)
            q.index_add_(0, rr, alpha * t * y)
            if with_b:
                b.index_add_(0, rr, (1 + alpha) * y)
        return q, b

    def A(P):
        return P @ G + reg * P + sparse(P, False)[0]
    q, b = sparse(X, True)
    r = b - (X @ G + reg * X + q)
    p, rs = r.clone(), (r * r).sum(1, keepdim=True)
    for _ in range(steps):
        q = A(p)
        a = rs / (p * q).sum(1, keepdim=True).clamp_min(1e-30)
        X += a * p
        r -= a * q
        rn = (r * r).sum(1, keepdim=True)
        p = r + (rn / rs.clamp_min(1e-30)) * p
        rs = rn
    X[cnt == 0] = 0
    return X


def solve_timing(args, dev, ucsr, icsr, n_pairs, dims):
    out = {}
    for dim in dims:
        eng = als.ALSEngine(args.users, args.items, dim, dev, reg=REG, alpha=ALPHA, solver="cg", cg_steps=STEPS)
        res = {}
        for side, csr, Y, X in (("user", ucsr, eng.item, eng.user), ("item", icsr, eng.user, eng.item)):
            n_rows = X.shape[0]
            G = ops.gram(Y)
            X0, Xc = X.clone(), torch.empty_like(X)
            copy = measure(lambda: Xc.copy_(X0), args.rounds, args.solve_iters)

            def cg():
                Xc.copy_(X0)
                ops.als_solve_rows_cg(Y, G, csr[0], csr[1], REG, ALPHA, Xc, steps=STEPS, err_flag=eng.err)
            r = measure(cg, args.rounds, args.solve_iters)
            # (1 + steps) applications of A: 2 dim^2 for G p and 4 dim per entry, and the entries' sum for b once
            flop = (1 + STEPS) * (2.0 * n_rows * dim * dim + 4.0 * n_pairs * dim) + 2.0 * n_pairs * dim
            r.update({"rows": n_rows, "copy_of_the_start_vectors_us": copy["median_us"], "GFLOP": round(flop / 1e9, 1),
                      "share_of_fp32_peak": round(flop / (r["median_us"] * 1e-6) / FP32_PEAK, 4),
                      "gathered_GB": round((1 + STEPS) * n_pairs * dim * 4 / 1e9, 2),
                      "gather_TB_s": round((1 + STEPS) * n_pairs * dim * 4 / (r["median_us"] * 1e-6) / 1e12, 3)})
            res[f"{side} half-step, cg {STEPS} steps"] = r
            if dim <= ops.ALS_MAX_DIM:
                Xo = torch.empty_like(X)
                rc = measure(lambda: ops.als_solve_rows(Y, G, csr[0], csr[1], REG, ALPHA, out=Xo, err_flag=eng.err), args.rounds, args.solve_iters)
                res[f"{side} half-step, cholesky"] = rc
                r["cholesky_over_cg"] = round(rc["median_us"] / r["median_us"], 2)
                nz = Xo.abs().sum(1) > 0
                r["median_rel_row_distance_to_the_exact_solve"] = float(((Xc[nz] - Xo[nz]).norm(dim=1) / Xo[nz].norm(dim=1)).median().item())
            elif not args.skip_torch:
                Xt = torch.empty_like(X)

                def base():
                    Xt.copy_(X0)
                    torch_cg_half_step(Y, G, csr[0], csr[1], REG, ALPHA, Xt, STEPS)
                rt = measure(base, max(2, args.rounds // 2), 1)
                res[f"{side} half-step, torch batched cg"] = rt
                r["torch_over_cg"] = round(rt["median_us"] / r["median_us"], 1)
                nz = Xt.abs().sum(1) > 0
                r["median_rel_row_diff_to_torch"] = float(((Xc[nz] - Xt[nz]).norm(dim=1) / Xt[nz].norm(dim=1)).median().item())
            eng.half_step(side, csr)                 # the next side's Y: solved rows, as in a run
        eng.check_ids()
        out[f"dim {dim}"] = res
        del eng
    return out


def gram_timing(args, dev):
    lib = import_module("binary-recommendation_amd._lib").load()
    out = {}
    for rows, dim in ((100_000, 350), (1_000_000, 512)):
        nbytes = rows * dim * 4
        copies = max(2, -(-3 * 256 * 2 ** 20 // nbytes))                    # >= 3 x the Infinity Cache between two reads of one copy
        tabs = [torch.randn(rows, dim, device=dev) for _ in range(copies)]
        G = torch.empty(dim, dim, device=dev)
        k = [0]

        def f():
            k[0] += 1
            ops.gram(tabs[k[0] % copies], out=G)
        r = measure(f, args.rounds, max(args.iters, copies))
        nb = -(-dim // 128)
        r.update({"read_MB": round(nbytes / 1e6, 1), "copies_rotated": copies, "share_of_hbm_peak": round(nbytes / (r["median_us"] * 1e-6) / HBM_PEAK, 3),
                  "column_block_pairs": nb * (nb + 1) // 2, "column_blocks_read_per_row": nb * (nb + 1) - nb,
                  "mfma_TFLOP_s_issued": round(2.0 * rows * 128 * 128 * (nb * (nb + 1) // 2) / (r["median_us"] * 1e-6) / 1e12, 1),
                  "workspace_MB": round(int(lib.brGramWideWorkspaceBytes(rows, dim)) / 1e6, 2)})
        out[f"{rows} x {dim}"] = r
        del tabs
    return out


def quality(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    truth, seen = ops.truth_csr(nU, hu, hi, dev), ops.truth_csr(nU, tu, ti, dev)
    all_users = torch.arange(nU, dtype=torch.int32, device=dev)
    ucsr, icsr = als.csr_pair(tu, ti, nU, nI, dev)
    reg, alpha = 30.0, 1.0

    def run(dim, solver, steps):
        e = als.ALSEngine(nU, nI, dim, dev, reg=reg, alpha=alpha, init_seed=args.seed, solver=solver, cg_steps=steps)
        obj = []
        for _ in range(args.quality_epochs):
            e.epoch(ucsr, icsr)
            obj.append(round(e.objective(ucsr), 2))
        e.check_ids()
        rm = e.rank_metrics(all_users, truth, ks=(10,), exclude=seen)
        auc = e.full_auc(all_users, truth)
        return {"dim": dim, "solver": solver, "cg_steps": steps if solver == "cg" else None, "ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5),
                "mrr": round(float(torch.nanmean(rm["mrr"]).item()), 5), "full_auc": round(float(torch.nanmean(auc).item()), 5), "objective_per_epoch": obj}
    out = {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "epochs": args.quality_epochs,
           "reg": reg, "alpha": alpha, "cholesky_recorded_by_tools/als_bench.py": {"ndcg@10": 0.277, "full_auc": 0.749}}
    out["runs"] = [run(64, "cholesky", 3)] + [run(64, "cg", s) for s in (2, 3, 5)] + [run(350, "cg", 3)]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=16_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--solve-iters", type=int, default=1)
    ap.add_argument("--quality-epochs", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit of the tree that is measured (default: git rev-parse HEAD)")
    ap.add_argument("--uncommitted", action="store_true", help="the tree holds changes on top of that commit (default: asked of git status)")
    ap.add_argument("--skip-gram", action="store_true")
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--skip-wide", action="store_true", help="no half-steps above 128 features")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("als_cg_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {"tool": "tools/als_cg_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
           "device": torch.cuda.get_device_name(0)}
    if not args.skip_gram:
        res["gram_wide"] = gram_timing(args, dev)
    if not (args.skip_solve and args.skip_wide):
        ucsr, icsr, n_pairs, cfg = workload(args, dev)
        res["solve"] = {"config": cfg}
        if not args.skip_solve:
            res["solve"].update(solve_timing(args, dev, ucsr, icsr, n_pairs, (64, 128)))
        if not args.skip_wide:
            res["solve"].update(solve_timing(args, dev, ucsr, icsr, n_pairs, (256, 350, 512)))
        del ucsr, icsr
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
