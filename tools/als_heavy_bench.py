"""The heavy rows of the conjugate-gradient ALS (csrc/als_heavy.hip, ALSEngine(heavy_rows=)) on the device, at tools/als_cg_bench.py's
workload: 1 M users x 100 K items, 16 M pairs drawn (users uniform, items Zipf 0.9; duplicates merged), reg 0.01, alpha 40, 3 steps.

Timing (tools/als_bench.py's scheme: device events, one process, 2 warm-up calls, `rounds` rounds of one call; the spread = the rounds;
every call starts from the same vectors, a device copy of the table inside the timed region).  Legs, each a run of its own (--leg):
  solve    dim 64 and 128: the item half-step through the engine with and without heavy_rows (without = the unchanged
           ops.als_solve_rows_cg), the Cholesky half-step beside them, the user half-step (no row above 37 entries) both ways,
           ops.als_normal_rows and ops.als_solve_rows_dense_cg alone on the heavy rows, and the item half-step at every heavy_rows of the
           sweep.  "faster" asks for spreads that do not overlap.
  wide     dim 256, 350 and 512, 3 rounds: the item and user half-steps with heavy_rows; the plain item half-step once, without warm-up.
  quality  data.ml1m_shaped, 10 epochs, dim 64, reg 30, alpha 1, 3 steps: NDCG@10, full AUC and the objective with and without heavy_rows.
A leg adds its key to the record at --out and keeps the others.

    python tools/als_heavy_bench.py --leg solve --out profiles/als/als_heavy_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from importlib import import_module

from tools.als_bench import FP32_PEAK, HBM_PEAK, commit, dirty, measure, stats, timed
from tools.als_cg_bench import ALPHA, REG, STEPS, workload

als, ops, data = (import_module("binary-recommendation_amd." + m) for m in ("als", "ops", "data"))
SWEEP = (256, 1024, 4096, 16384, 65536)


def apart(fast, slow):
    """the spreads do not overlap: every round of `fast` below every round of `slow`"""
    return fast["max_us"] < slow["min_us"]


def half_step_timer(eng, side, csr, X0):
    X = eng.user if side == "user" else eng.item

    def f():
        X.copy_(X0)
        eng.half_step(side, csr)
    return f


def heavy_parts(eng, Y, hc, rounds):
    """ops.als_normal_rows and ops.als_solve_rows_dense_cg alone, over the batches of hc"""
    off, idx, conf = hc.csr
    G = ops.gram(Y)
    x0 = torch.zeros(hc.rows.numel(), eng.dim, device=Y.device)
    entries = int((off[hc.rows.long() + 1] - off[hc.rows.long()]).sum().item())

    def normal():
        for bt in hc.batches:
            ops.als_normal_rows(Y, off, idx, ALPHA, bt.rows, conf=conf, slice=hc.slice, plan=(bt.slice_off, bt.n_slices))
    rn = measure(normal, rounds, 1)
    dim, nb = eng.dim, -(-eng.dim // 128)
    tiles = sum(1 for bi in range(nb) for bj in range(bi + 1) for w in range(4) for t in range(4)
                if 32 * w < min(128, dim - 128 * bi) and 32 * t < min(128, dim - 128 * bj) and not (bi == bj and t > w))
    blocks_read = nb * nb                                                     # a diagonal pair gathers one column block, the others two
    rn.update({"heavy_rows": int(hc.rows.numel()), "entries": entries, "slices": sum(b.n_slices for b in hc.batches), "batches": len(hc.batches),
               "ns_per_entry": round(rn["median_us"] * 1e3 / max(entries, 1), 3),
               "gathered_GB": round(entries * min(dim, 128) * 4 * blocks_read / 1e9, 3),
               "gather_share_of_hbm_peak": round(entries * min(dim, 128) * 4 * blocks_read / (rn["median_us"] * 1e-6) / HBM_PEAK, 4),
               "mfma_share_of_fp32_peak": round(2.0 * entries * tiles * 1024 / (rn["median_us"] * 1e-6) / FP32_PEAK, 4)})
    Hb = [ops.als_normal_rows(Y, off, idx, ALPHA, bt.rows, conf=conf, slice=hc.slice, plan=(bt.slice_off, bt.n_slices)) for bt in hc.batches[:1]]

    def dense():
        for (H, b), bt in zip(Hb, hc.batches[:1]):
            ops.als_solve_rows_dense_cg(G, H, b, REG, x0[bt.lo:bt.hi], steps=STEPS)
    rd = measure(dense, rounds, 1) if Hb else None
    if rd:
        rd["rows_of_the_first_batch"] = hc.batches[0].hi - hc.batches[0].lo
    return rn, rd


def solve_leg(args, dev, ucsr, icsr, n_pairs):
    out = {}
    for dim in (64, 128):
        eng = als.ALSEngine(args.users, args.items, dim, dev, reg=REG, alpha=ALPHA, solver="cg", cg_steps=STEPS, heavy_rows=args.heavy_rows)
        res = {}
        U0, I0 = eng.user.clone(), eng.item.clone()
        uh, ih = eng.prepare(ucsr), eng.prepare(icsr)
        # the user side first (the item table as initialised), then the item side against the solved users, as in a run
        res["user half-step, plain"] = ru = measure(half_step_timer(eng, "user", ucsr, U0), args.rounds, 1)
        res["user half-step, heavy_rows"] = ruh = measure(half_step_timer(eng, "user", uh, U0), args.rounds, 1)
        ruh.update({"heavy_rows": int(uh.rows.numel()), "inside_the_plain_spread": ru["min_us"] <= ruh["median_us"] <= ru["max_us"]})
        res["item half-step, plain"] = rp = measure(half_step_timer(eng, "item", icsr, I0), args.rounds, 1)
        res["item half-step, heavy_rows"] = rh = measure(half_step_timer(eng, "item", ih, I0), args.rounds, 1)
        with_heavy = eng.item.clone()
        half_step_timer(eng, "item", icsr, I0)()
        nz = eng.item.abs().sum(1) > 0
        rh.update({"threshold": args.heavy_rows, "heavy_rows": int(ih.rows.numel()), "faster_than_plain_spreads_apart": apart(rh, rp),
                   "plain_over_heavy": round(rp["median_us"] / rh["median_us"], 1),
                   "max_rel_row_diff_to_plain": float(((with_heavy[nz] - eng.item[nz]).norm(dim=1) / eng.item[nz].norm(dim=1)).max().item()),
                   "ns_per_entry": round(rh["median_us"] * 1e3 / n_pairs, 3), "user_side_ns_per_entry": round(ru["median_us"] * 1e3 / n_pairs, 3),
                   "item_over_user_per_entry": round(rh["median_us"] / ru["median_us"], 2)})
        if dim <= ops.ALS_MAX_DIM:
            Xo, G = torch.empty_like(eng.item), ops.gram(eng.user)
            res["item half-step, cholesky"] = measure(lambda: ops.als_solve_rows(eng.user, G, icsr[0], icsr[1], REG, ALPHA, out=Xo, err_flag=eng.err),
                                                      args.rounds, 1)
        res["als_normal_rows alone"], res["als_solve_rows_dense_cg alone"] = heavy_parts(eng, eng.user, ih, args.rounds)
        sweep = {}
        for thr in SWEEP:
            hc = als.split_heavy(icsr, thr, dim=dim, heavy_ws_bytes=eng.heavy_ws_bytes)
            r = measure(half_step_timer(eng, "item", hc, I0), args.rounds, 1)
            r.update({"heavy_rows": int(hc.rows.numel()), "batches": len(hc.batches)})
            sweep[str(thr)] = r
            del hc
        res["item half-step by heavy_rows"] = sweep
        res["best heavy_rows"] = int(min(sweep, key=lambda k: sweep[k]["median_us"]))
        eng.check_ids()
        out[f"dim {dim}"] = res
        del eng
    return out


def wide_leg(args, dev, ucsr, icsr, n_pairs):
    out = {}
    for dim in (256, 350, 512):
        eng = als.ALSEngine(args.users, args.items, dim, dev, reg=REG, alpha=ALPHA, solver="cg", cg_steps=STEPS, heavy_rows=args.heavy_rows)
        U0, I0 = eng.user.clone(), eng.item.clone()
        uh, ih = eng.prepare(ucsr), eng.prepare(icsr)
        res = {"user half-step, heavy_rows": measure(half_step_timer(eng, "user", uh, U0), args.wide_rounds, 1)}
        res["item half-step, heavy_rows"] = rh = measure(half_step_timer(eng, "item", ih, I0), args.wide_rounds, 1)
        rh.update({"threshold": args.heavy_rows, "heavy_rows": int(ih.rows.numel()), "batches": len(ih.batches),
                   "ns_per_entry": round(rh["median_us"] * 1e3 / n_pairs, 3)})
        res["als_normal_rows alone"], res["als_solve_rows_dense_cg alone"] = heavy_parts(eng, eng.user, ih, args.wide_rounds)
        if not args.skip_plain_wide:
            torch.cuda.synchronize()
            rp = stats([timed(half_step_timer(eng, "item", icsr, I0), 1)])      # once, no warm-up: seconds per call
            rp["plain_over_heavy"] = round(rp["median_us"] / rh["median_us"], 1)
            res["item half-step, plain, one call without warm-up"] = rp
        eng.check_ids()
        out[f"dim {dim}"] = res
        del eng
    return out


def quality_leg(args, dev):
    users, items = data.ml1m_shaped(args.seed)
    nU, nI = int(users.max()) + 1, int(items.max()) + 1
    cut = int(len(users) * 0.9)          # the order is time-like: the last tenth is held out
    tu, ti, hu, hi = users[:cut], items[:cut], users[cut:], items[cut:]
    truth, seen = ops.truth_csr(nU, hu, hi, dev), ops.truth_csr(nU, tu, ti, dev)
    all_users = torch.arange(nU, dtype=torch.int32, device=dev)
    ucsr, icsr = als.csr_pair(tu, ti, nU, nI, dev)

    def run(heavy_rows):
        e = als.ALSEngine(nU, nI, 64, dev, reg=30.0, alpha=1.0, init_seed=args.seed, solver="cg", cg_steps=STEPS, heavy_rows=heavy_rows)
        uc, ic = e.prepare(ucsr), e.prepare(icsr)
        obj = []
        for _ in range(args.quality_epochs):
            e.epoch(uc, ic)
            obj.append(round(e.objective(ucsr), 2))
        e.check_ids()
        rm = e.rank_metrics(all_users, truth, ks=(10,), exclude=seen)
        auc = e.full_auc(all_users, truth)
        return {"heavy_rows": heavy_rows, "rows_taken": None if heavy_rows is None else [int(uc.rows.numel()), int(ic.rows.numel())],
                "ndcg@10": round(float(torch.nanmean(rm["ndcg@10"]).item()), 5), "full_auc": round(float(torch.nanmean(auc).item()), 5),
                "objective_per_epoch": obj}
    return {"data": f"data.ml1m_shaped({args.seed}): {cut} training positives, {len(users) - cut} held out", "epochs": args.quality_epochs, "dim": 64,
            "reg": 30.0, "alpha": 1.0, "cg_steps": STEPS, "runs": [run(None), run(256), run(4096)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("solve", "wide", "quality"), required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=16_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--wide-rounds", type=int, default=3)
    ap.add_argument("--heavy-rows", type=int, default=ops.ALS_HEAVY_ROWS, help="the threshold of the legs that are not the sweep")
    ap.add_argument("--skip-plain-wide", action="store_true", help="no plain item half-step above 128 features (8 - 15 s per call)")
    ap.add_argument("--quality-epochs", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit of the tree that is measured (default: git rev-parse HEAD)")
    ap.add_argument("--uncommitted", action="store_true", help="the tree holds changes on top of that commit (default: asked of git status)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("als_heavy_bench: no GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update({"tool": "tools/als_heavy_bench.py", "commit": args.commit or commit(), "uncommitted_changes_on_top": args.uncommitted or dirty(),
                "device": torch.cuda.get_device_name(0), "heavy_slice": ops.ALS_HEAVY_SLICE})
    if args.leg == "quality":
        res["quality"] = quality_leg(args, dev)
    else:
        ucsr, icsr, n_pairs, cfg = workload(args, dev)
        res.setdefault("config", cfg)
        res[args.leg] = (solve_leg if args.leg == "solve" else wide_leg)(args, dev, ucsr, icsr, n_pairs)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
