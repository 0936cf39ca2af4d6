"""-m gpu: the BatchNorm backward that brDenseBackward folds into the producer layer, and the BatchNorm helper kernels, against float64.

The tower is Dense -> activation -> BatchNorm -> dropout, twice.  The producer layer's backward turns gy into
    da = gamma rstd (gy - S1/Bt - (y - mean) rstd S2/Bt),   dz = da act'(y)
from (mean, rstd, gamma, bn_sums, batch_total); S1, S2 are the consumer's column sums in BR_STAT_REPLICAS replicas of doubles.  The
arithmetic exists twice, written differently (csrc/dense_bwd.hip: fused launch, fp32-MFMA and bf16x6 body; csrc/mlp.hip dense_dx_kernel:
two-kernel path), and was reached only end to end through NeuMFEngine.train_step.  Here:
  1. one brDenseBackward with an out-BN per dispatch path (CASES), float64 numpy on the kernel's own inputs and its own fp32 y, every
     output element within BOUND x (the same expression with every term replaced by its absolute value); rows past `batch` and padding
     columns hold NaN;
  2. the same cases in a child process with BR_MLP_MATH=f32 (the switch is read once per process): the fp32-MFMA fused body;
  3. brBnFinalize, brBnInference, brBnParamGrads and brBnParamGradsPair alone;
  4. layer 1 -> finalize -> layer 2 -> loss -> backward 2 -> param grads -> backward 1 with the real kernels against torch float64
     autograd on the CPU, whole and as two shards of one global batch: what the consumer's sums mean to the producer.
The measured maxima of part 1 / 2 go to dense_bn_errors.json in the directory that BR_TEST_REPORT_DIR names, when it is set and exists.

BOUND = 2.5e-6: 1.5e-6 is what test_gpu_mlp_math.py holds the products to in both math modes; dz is formed in about 8 fp32 roundings
(gamma rstd, S1/Bt, S2/Bt, its product with rstd, y - mean, the product with c3, two subtractions, the product with c1, act', the product
with it: each relative to a term of the magnitude expression, half an ulp = 6e-8 each, 5e-7), tx in about 3 (x scale + shift, 1/(1-p),
the product with it: 2e-7).  The bound is derived, not fitted: the largest figure measured on an MI355X is 3.0e-7 (gx of the 200 x 64
layer, either math mode).
"""
import functools
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import binrec_oracle as O
from tests.test_gpu_neumf import _close

pytestmark = pytest.mark.gpu

BOUND = 2.5e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
EXTRA = 3           # rows every buffer has beyond `batch`


def _ops():
    return import_module("binary-recommendation_amd.ops")


def _td(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np64(t):
    return t.cpu().numpy().astype(np.float64)


# (K, N, B, act, padded rows, gx wanted, batch_total = 3B + 5 instead of B).  Which kernel runs (brDenseBackward, csrc/mlp.hip): the fused
# launch needs every row stride a multiple of 4 floats and dense_bwd_fused_lds(n-tiles, k-tiles) <= 160 KiB; inside it the bf16x6 body runs
# where its piece image fits (every fused shape below) unless BR_MLP_MATH=f32, which selects the fp32-MFMA body.  Everything else runs
# dense_dx_kernel + dense_dw_kernel, the same in both math modes.
CASES = [
    (128, 100, 200, "sigmoid", True, True, False),   # fused (157 KiB image); the benchmarked layer, last 64-row tile holds 8 rows
    (100, 50, 129, "relu", True, True, True),        # fused; rows of 52 floats: the last 16-B group of gy / y straddles N
    (64, 112, 65, "linear", True, True, False),      # fused; 7 n-tiles: the bf16x6 dx product ends in a half block
    (16, 16, 64, "sigmoid", True, True, True),       # fused; one n-tile, one k-tile, exactly one row tile
    (128, 128, 130, "relu", True, True, True),       # aligned rows, but the fused image is 173 KiB: two-kernel path, 16-B loads
    (37, 23, 13, "sigmoid", False, True, False),     # row strides 37 and 23: two-kernel path, scalar loads, less than one 16-row tile
    (96, 33, 77, "relu", False, True, True),         # gy stride 33: two-kernel path; x (stride 96) still loads 16 B at a time in dW
    (200, 64, 150, "sigmoid", True, True, False),    # K > 128, aligned: two fused launches (columns 0..127 and 128..199), dz formed twice
    (200, 64, 150, "sigmoid", True, False, True),    #   ... without gx
    (130, 17, 77, "linear", False, True, True),      # K > 128, stride 130: two dx launches (96 + 34 columns), then two dW launches
    (130, 17, 77, "linear", False, False, False),    #   ... without gx: one dx launch only forms dz for the two dW launches
]
CASE_IDS = ["{}x{}x{}-{}-{}-{}-{}".format(K, N, B, act, "padded" if pad else "contiguous", "gx" if gx else "nogx", "Bt3" if bt3 else "Bt1")
            for K, N, B, act, pad, gx, bt3 in CASES]
SEED, STEP, SITE, DROP_P, ROW0 = 987654321, 3, 1, 0.2, 64


def _measure(dev, case):
    """One case on the GPU and in float64 -> {"ratios": {output: max |got - ref| / mag}, "problems": [...]} (JSON-able: the child
    process of the fp32 mode reports the same)."""
    K, N, B, act, padded, want_gx, bt3 = case
    ops = _ops()
    rng = np.random.default_rng(K * 977 + N * 31 + B + (0 if want_gx else 7))
    f = np.float32
    ldk, ldn = ((K + 3) & ~3, (N + 3) & ~3) if padded else (K, N)
    wide = K > 128                                   # two K-halves: a tower's first layer, no BatchNorm on the input side
    Bt = 3 * B + 5 if bt3 else B
    x = rng.normal(size=(B, K)).astype(f)
    W = rng.normal(scale=0.2, size=(K, N)).astype(f)
    b = rng.normal(size=N).astype(f)
    sc, sh = rng.uniform(0.5, 1.5, K).astype(f), rng.normal(size=K).astype(f)
    mean_in, rstd_in = rng.normal(size=K).astype(f), rng.uniform(0.5, 2, K).astype(f)
    # the out-BN vectors are arbitrary per column (the kernel does not need them consistent with y): a misplaced factor shows
    mean, rstd = rng.normal(0.2, 0.5, N).astype(f), rng.uniform(0.5, 2, N).astype(f)
    gamma = (rng.choice([-1.0, 1.0], N) * rng.uniform(0.5, 1.5, N)).astype(f)
    # gy ~ 1e-2 and every replica of the sums a distinct non-zero value of order B 1e-3: the three terms of da are of one size
    gy = rng.normal(scale=1e-2, size=(B, N)).astype(f)
    sums = rng.choice([-1.0, 1.0], (8, 2 * N)) * rng.uniform(0.5, 1.5, (8, 2 * N)) * B * 1e-3
    assert len(np.unique(sums)) == sums.size and np.all(sums != 0)

    def rows(a, ld):     # (B + EXTRA) x ld, NaN outside a's block
        buf = torch.full((B + EXTRA, ld), NAN, device=dev)
        buf[:B, :a.shape[1]] = _td(dev, a)
        return buf

    xb, gyb = rows(x, ldk), rows(gy, ldn)
    yb = torch.full((B + EXTRA, ldn), NAN, device=dev)
    Wd = _td(dev, W)
    ops.dense_forward(xb[:, :K], Wd, _td(dev, b), yb[:, :N], act, _td(dev, sc), _td(dev, sh), DROP_P, SEED, STEP, SITE, ROW0, batch=B)
    yk = _np64(yb[:B, :N])                           # the kernel's own fp32 y: act' and xhat of the reference come from it
    yb[B:, :] = NAN
    yb[:, N:] = NAN
    ns = ops.dense_backward_slabs(B, K, N)
    slabs = torch.full((ns * (K * N + N),), NAN, device=dev)
    gxb = torch.full((B + EXTRA, ldk), NAN, device=dev) if want_gx else None
    insum = None if wide else torch.zeros(8, 2 * K, dtype=torch.float64, device=dev)
    ops.dense_backward(gyb[:, :N], yb[:, :N], xb[:, :K], Wd, act, slabs, ns, gx=gxb[:, :K] if want_gx else None,
                       out_bn=(_td(dev, mean), _td(dev, rstd), _td(dev, gamma)), bn_sums=_td(dev, sums), batch_total=Bt,
                       in_scale=_td(dev, sc), in_shift=_td(dev, sh), in_bn=None if wide else (_td(dev, mean_in), _td(dev, rstd_in)),
                       in_drop_p=DROP_P, in_site=SITE, seed=SEED, step=STEP, row0=ROW0, in_bn_sums=insum, batch=B)
    red = torch.full((K * N + N,), NAN, device=dev)
    ops.reduce_slabs(slabs, ns, K * N + N, red)
    torch.cuda.synchronize()

    # ---- float64 on the same inputs
    d = lambda a: np.asarray(a, dtype=np.float64)
    keep = O.dropout_mask(SEED, STEP, SITE, B, K, DROP_P, ROW0) / (1.0 - float(f(DROP_P)))
    S = d(sums).sum(0)
    t1, t2 = S[:N] / Bt, (yk - d(mean)) * d(rstd) * S[N:] / Bt
    actp = O.act_bwd_from_out(yk, act)
    dz = d(gamma) * d(rstd) * (d(gy) - t1 - t2) * actp
    dzmag = np.abs(d(gamma) * d(rstd)) * (np.abs(d(gy)) + np.abs(t1) + np.abs(t2)) * np.abs(actp)
    tx = (d(x) * d(sc) + d(sh)) * keep
    txmag = (np.abs(d(x) * d(sc)) + np.abs(d(sh))) * keep
    ref = {"dW": tx.T @ dz, "db": dz.sum(0), "gx": (dz @ d(W).T) * keep}
    mag = {"dW": txmag.T @ dzmag, "db": dzmag.sum(0), "gx": (dzmag @ np.abs(d(W)).T) * keep}
    r = _np64(red)
    got = {"dW": r[:K * N].reshape(K, N), "db": r[K * N:]}
    problems = []
    if want_gx:
        got["gx"] = _np64(gxb[:B, :K])
        if not bool(torch.isnan(gxb[B:, :]).all()):
            problems.append("gx rows past the batch were written")
        if not bool(torch.isnan(gxb[:, K:]).all()):
            problems.append("gx padding columns were written")
    else:
        del ref["gx"], mag["gx"]
    if not wide:
        xhat_in = (d(x) - d(mean_in)) * d(rstd_in)
        ins = _np64(insum).sum(0)
        got["sum_dh"], got["sum_dh_xhat"] = ins[:K], ins[K:]
        ref["sum_dh"], ref["sum_dh_xhat"] = ref["gx"].sum(0), (ref["gx"] * xhat_in).sum(0)
        mag["sum_dh"], mag["sum_dh_xhat"] = mag["gx"].sum(0), (mag["gx"] * np.abs(xhat_in)).sum(0)
    if not bool(torch.isfinite(slabs).all()):
        problems.append("a slab was left unwritten or is not finite")
    ratios = {}
    for k in ref:
        if not np.all(np.isfinite(got[k])):
            problems.append(k + " is not finite")
            continue
        err = np.abs(got[k] - ref[k])
        if np.any(err[mag[k] == 0] != 0):
            problems.append(k + " is non-zero where every term is zero")
        live = mag[k] > 0
        ratios[k] = float(np.max(err[live] / mag[k][live])) if live.any() else 0.0
    return {"ratios": ratios, "problems": problems}


_REPORT = {}


def _record(mode, case_id, res):
    _REPORT.setdefault(case_id, {})[mode] = res["ratios"]
    out = os.environ.get("BR_TEST_REPORT_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "dense_bn_errors.json"), "w") as fh:
            json.dump({"note": "brDenseBackward with an out-BatchNorm: max |got - float64| / (the same expression on |terms|) per output, by math mode",
                       "bound": BOUND, "cases": _REPORT}, fh, indent=1)


def _assert_case(case_id, res):
    print(case_id, json.dumps(res))
    assert not res["problems"], (case_id, res["problems"])
    for k, e in res["ratios"].items():
        assert e <= BOUND, (case_id, k, e)


def _this_mode():
    return "f32" if os.environ.get("BR_MLP_MATH", "")[:1] == "f" else "bf16x6"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_out_bn_backward_against_float64(dev, case):
    cid = CASE_IDS[CASES.index(case)]
    res = _measure(dev, case)
    _record(_this_mode(), cid, res)
    _assert_case(cid, res)


CHILD = "from tests import test_gpu_dense_bn as t; t._child_main()"


def _child_main():
    dev = torch.device("cuda:0")
    print("RESULT " + json.dumps({cid: _measure(dev, case) for cid, case in zip(CASE_IDS, CASES)}))


def test_out_bn_backward_on_the_fp32_mfma_bodies(dev):
    """The same cases and assertions in one fresh process with BR_MLP_MATH=f32: the fused shapes run the fp32-MFMA body (its out-BN
    staging, dropout epilogue and producer sums), which no other test reaches where a bf16 piece image fits."""
    env = dict(os.environ)
    env["BR_MLP_MATH"] = "f32"
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    got = json.loads(line[len("RESULT "):])
    assert sorted(got) == sorted(CASE_IDS)
    for cid in CASE_IDS:
        _record("f32", cid, got[cid])
    for cid in CASE_IDS:
        _assert_case(cid, got[cid])


# ------------------------------------------------------------------------------------------------ 3. the BatchNorm helper kernels
BN_BT = 613          # rows behind the sums: no buffer in this file has that many
MOMENTUM = float(np.float32(0.99))      # the kernels receive fp32 momentum and eps; the reference computes on those values


def _bn_stats(N, rng):
    """Column sums of BN_BT rows spread unevenly over the 8 replicas (two replicas get nothing).  From N = 3 up column 0 is constant 0.5
    (every sum exact: variance exactly 0), column 1 all zero, column 2 constant 1 with its sum of squares 2^-40 short, as sums rounded
    in another order can come out: raw variance -9e-13, which without the clamp is most of eps = 1e-12 and beyond it NaN."""
    X = rng.normal(0.3, 1.0, (BN_BT, N)).astype(np.float32).astype(np.float64)
    if N >= 3:
        X[:, 0], X[:, 1], X[:, 2] = 0.5, 0.0, 1.0
    rep = rng.choice(8, BN_BT, p=[0.4, 0.25, 0.15, 0.1, 0.05, 0.05, 0.0, 0.0])
    stats = np.zeros((8, 2 * N))
    for r in range(8):
        stats[r, :N], stats[r, N:] = X[rep == r].sum(0), (X[rep == r] ** 2).sum(0)
    if N >= 3:
        stats[:, N + 2] *= 1.0 - 2.0 ** -40
    return stats


@pytest.mark.parametrize("eps", [1e-3, 1e-12])
@pytest.mark.parametrize("N", [1, 100, 257])
def test_bn_finalize_against_float64(dev, N, eps):
    """Inputs are double sums, outputs a few fp32 operations (1/sqrtf, one product, one fma-like expression): rtol 1e-6 (about 16 ulp
    against about 6 roundings in the longest expression, shift), shift with the absolute floor 1e-6 (|beta| + |mean scale|) for its
    cancellation."""
    ops = _ops()
    rng = np.random.default_rng(N)
    f = np.float32
    eps = float(f(eps))
    stats = _bn_stats(N, rng)
    gamma, beta = (1 + rng.normal(0, 0.3, N)).astype(f), rng.normal(0, 0.5, N).astype(f)
    mm, mv = rng.uniform(0.3, 0.6, N).astype(f), rng.uniform(0.05, 0.3, N).astype(f)
    S = stats.sum(0)
    mu = S[:N] / BN_BT
    raw = S[N:] / BN_BT - mu * mu
    var = np.maximum(raw, 0.0)
    if N >= 3:
        assert raw[0] == 0 and raw[1] == 0 and -1e-12 < raw[2] < -8e-13
    rs = 1.0 / np.sqrt(var + eps)
    d = lambda a: a.astype(np.float64)
    ref = {"scale": d(gamma) * rs, "mean": mu, "rstd": rs, "mm": d(mm) * MOMENTUM + mu * (1 - MOMENTUM), "mv": d(mv) * MOMENTUM + var * (1 - MOMENTUM)}
    ref["shift"] = d(beta) - mu * ref["scale"]
    out = lambda: {k: torch.full((N,), NAN, device=dev) for k in ("scale", "shift", "mean", "rstd")}
    a, b = out(), out()
    mmd, mvd = _td(dev, mm), _td(dev, mv)
    ops.bn_finalize(_td(dev, stats), BN_BT, _td(dev, gamma), _td(dev, beta), eps, MOMENTUM, mmd, mvd, a["scale"], a["shift"], a["mean"], a["rstd"])
    ops.bn_finalize(_td(dev, stats), BN_BT, _td(dev, gamma), _td(dev, beta), eps, MOMENTUM, None, None, b["scale"], b["shift"], b["mean"], b["rstd"])
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k + " differs between the forms with and without moving statistics"
    got = {k: _np64(v) for k, v in a.items()}
    got["mm"], got["mv"] = _np64(mmd), _np64(mvd)
    for k, g in got.items():
        assert np.all(np.isfinite(g)), k
        floor = 1e-6 * (np.abs(d(beta)) + np.abs(mu * ref["scale"])) if k == "shift" else 0.0
        assert np.all(np.abs(g - ref[k]) <= np.maximum(1e-6 * np.abs(ref[k]), floor)), (k, g, ref[k])
    if N >= 3:      # zero variance, clamped: rstd = 1 / sqrt(eps)
        assert np.all(np.abs(got["rstd"][:3] * np.sqrt(eps) - 1.0) <= 1e-6), got["rstd"][:3]


@pytest.mark.parametrize("N", [1, 100, 257])
def test_bn_inference_against_float64(dev, N):
    ops = _ops()
    rng = np.random.default_rng(N + 1000)
    f = np.float32
    eps = float(f(1e-3))
    gamma, beta = (1 + rng.normal(0, 0.3, N)).astype(f), rng.normal(0, 0.5, N).astype(f)
    mm, mv = rng.normal(0.4, 0.3, N).astype(f), rng.uniform(0.0, 0.3, N).astype(f)
    mv[0] = 0.0
    d = lambda a: a.astype(np.float64)
    scale_ref = d(gamma) / np.sqrt(d(mv) + eps)
    shift_ref = d(beta) - d(mm) * scale_ref
    scale, shift = torch.full((N,), NAN, device=dev), torch.full((N,), NAN, device=dev)
    ops.bn_inference(_td(dev, gamma), _td(dev, beta), _td(dev, mm), _td(dev, mv), eps, scale, shift)
    torch.cuda.synchronize()
    gs, gh = _np64(scale), _np64(shift)
    assert np.all(np.abs(gs - scale_ref) <= 1e-6 * np.abs(scale_ref)), (gs, scale_ref)
    assert np.all(np.abs(gh - shift_ref) <= np.maximum(1e-6 * np.abs(shift_ref), 1e-6 * (np.abs(d(beta)) + np.abs(d(mm) * scale_ref)))), (gh, shift_ref)


@pytest.mark.parametrize("Na,Nb", [(100, 33), (33, 257)])
def test_bn_param_grads_single_and_pair(dev, Na, Nb):
    """dbeta / dgamma are the fp32 rounding of the float64 replica totals, exactly; the two-layer launch is bit-equal to two single ones.
    The replica values are multiples of 2^-16 below 2^20: every partial sum is exact in double whatever the order, and 36 bits need the
    rounding to fp32."""
    ops = _ops()
    rng = np.random.default_rng(Na * 1000 + Nb)
    res = {}
    for tag, N in (("a", Na), ("b", Nb)):
        sums = rng.integers(-2 ** 36, 2 ** 36, (8, 2 * N)).astype(np.float64) * 2.0 ** -16
        sd = _td(dev, sums)
        dg, db = torch.full((N,), NAN, device=dev), torch.full((N,), NAN, device=dev)
        ops.bn_param_grads(sd, dg, db)
        tot = sums.sum(0)
        assert np.array_equal(db.cpu().numpy(), tot[:N].astype(np.float32)), "dbeta " + tag
        assert np.array_equal(dg.cpu().numpy(), tot[N:].astype(np.float32)), "dgamma " + tag
        res[tag] = (sd, dg, db, torch.full((N,), NAN, device=dev), torch.full((N,), NAN, device=dev))
    (sa, dga, dba, pga, pba), (sb, dgb, dbb, pgb, pbb) = res["a"], res["b"]
    ops.bn_param_grads_pair(sa, pga, pba, sb, pgb, pbb)
    torch.cuda.synchronize()
    assert torch.equal(pga, dga) and torch.equal(pba, dba) and torch.equal(pgb, dgb) and torch.equal(pbb, dbb)


# ------------------------------------------------------------------------------------------------ 4. the chain of a tower, in miniature
CH_B, CH_K, CH_N1, CH_N2, CH_DEAD = 300, 40, 100, 48, 7      # every row is a multiple of 4 floats: the padded layout, fused launches
CH_SEED, CH_STEP, CH_P, CH_EPS = 0xABCDEF12345, 5, 0.2, float(np.float32(1e-3))


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """Inputs and torch float64 autograd of: dropout(site 0) -> Dense(40, 100) sigmoid -> BatchNorm -> dropout(site 1) -> Dense(100, 48)
    relu -> sum(a2 G).  Column CH_DEAD of layer 1 has zero weights and bias -100: the same output in every row, zero batch variance."""
    rng = np.random.default_rng(2024)
    f = np.float32
    inp = {"x0": rng.normal(size=(CH_B, CH_K)).astype(f), "W1": rng.normal(scale=0.3, size=(CH_K, CH_N1)).astype(f),
           "b1": rng.normal(scale=0.3, size=CH_N1).astype(f), "gamma": (1 + rng.normal(0, 0.2, CH_N1)).astype(f),
           "beta": rng.normal(0, 0.3, CH_N1).astype(f), "W2": rng.normal(scale=0.2, size=(CH_N1, CH_N2)).astype(f),
           "b2": rng.normal(scale=0.3, size=CH_N2).astype(f), "G": rng.normal(size=(CH_B, CH_N2)).astype(f)}
    inp["W1"][:, CH_DEAD] = 0.0
    inp["b1"][CH_DEAD] = -100.0
    inv_keep = 1.0 / (1.0 - float(f(CH_P)))
    m0 = torch.from_numpy(O.dropout_mask(CH_SEED, CH_STEP, 0, CH_B, CH_K, CH_P).astype(np.float64) * inv_keep)
    m1 = torch.from_numpy(O.dropout_mask(CH_SEED, CH_STEP, 1, CH_B, CH_N1, CH_P).astype(np.float64) * inv_keep)
    t = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(k != "G") for k, v in inp.items()}
    a1 = torch.sigmoid((t["x0"] * m0) @ t["W1"] + t["b1"])
    mean, var = a1.mean(0), a1.var(0, unbiased=False)
    h = (a1 - mean) / torch.sqrt(var + CH_EPS) * t["gamma"] + t["beta"]
    z2 = (h * m1) @ t["W2"] + t["b2"]
    (torch.relu(z2) * t["G"]).sum().backward()
    # input condition: no ReLU unit close enough to 0 to come out on the other side in fp32
    assert float(z2.detach().abs().min()) >= 1e-5, float(z2.detach().abs().min())
    assert float(var.detach()[CH_DEAD]) < 1e-80
    ref = {"dW1": t["W1"].grad, "db1": t["b1"].grad, "dx": t["x0"].grad, "dgamma": t["gamma"].grad, "dbeta": t["beta"].grad,
           "dW2": t["W2"].grad, "db2": t["b2"].grad}
    return inp, {k: v.numpy() for k, v in ref.items()}


@pytest.mark.parametrize("shards", [((0, 300),), ((0, 177), (177, 123))], ids=["whole", "two-shards"])
def test_tower_chain_against_float64_autograd(dev, shards):
    """The kernels' conventions against each other (a wrong one is off by O(1); the tight bounds are in part 1), with the bars of the
    direct dense tests: rtol 1e-4, atol 1e-5 max |ref|.  As shards of one global batch (row0, batch_total = 300): the statistics and the
    backward sums are added across the shards before use, the slabs, sums and dx rows after."""
    ops = _ops()
    inp, ref = _chain_reference()
    K, N1, N2, Bt = CH_K, CH_N1, CH_N2, CH_B
    td = lambda a: _td(dev, a)
    W1, b1, W2, b2, gamma, beta = (td(inp[k]) for k in ("W1", "b1", "W2", "b2", "gamma", "beta"))
    nan = lambda *s: torch.full(s, NAN, device=dev)
    zsum = lambda n: torch.zeros(8, 2 * n, dtype=torch.float64, device=dev)
    sh = [{"r0": r0, "B": B, "x0": td(inp["x0"][r0:r0 + B]), "G": td(inp["G"][r0:r0 + B]), "a1": nan(B, N1), "a2": nan(B, N2), "gh1": nan(B, N1),
           "dx": nan(B, K), "stats": zsum(N1), "bsum": zsum(N1)} for r0, B in shards]
    drop = lambda s: dict(seed=CH_SEED, step=CH_STEP, row0=s["r0"])
    for s in sh:
        ops.dense_forward(s["x0"], W1, b1, s["a1"], "sigmoid", None, None, CH_P, CH_SEED, CH_STEP, 0, s["r0"], s["stats"])
    stats = torch.stack([s["stats"] for s in sh]).sum(0)
    scale, shift, mean, rstd = nan(N1), nan(N1), nan(N1), nan(N1)
    ops.bn_finalize(stats, Bt, gamma, beta, CH_EPS, MOMENTUM, None, None, scale, shift, mean, rstd)
    grads = {k: np.zeros(v.shape) for k, v in ref.items() if k not in ("dx", "dgamma", "dbeta")}
    for s in sh:
        ops.dense_forward(s["a1"], W2, b2, s["a2"], "relu", scale, shift, CH_P, CH_SEED, CH_STEP, 1, s["r0"])
        ns = ops.dense_backward_slabs(s["B"], N1, N2)
        slabs, red = nan(ns * (N1 * N2 + N2)), nan(N1 * N2 + N2)
        # d sum(a2 G) / d a2 = G
        ops.dense_backward(s["G"], s["a2"], s["a1"], W2, "relu", slabs, ns, gx=s["gh1"], in_scale=scale, in_shift=shift, in_bn=(mean, rstd),
                           in_drop_p=CH_P, in_site=1, in_bn_sums=s["bsum"], **drop(s))
        ops.reduce_slabs(slabs, ns, N1 * N2 + N2, red)
        grads["dW2"] += _np64(red)[:N1 * N2].reshape(N1, N2)
        grads["db2"] += _np64(red)[N1 * N2:]
    bsum = torch.stack([s["bsum"] for s in sh]).sum(0)
    dgamma, dbeta = nan(N1), nan(N1)
    ops.bn_param_grads(bsum, dgamma, dbeta)
    for s in sh:
        ns = ops.dense_backward_slabs(s["B"], K, N1)
        slabs, red = nan(ns * (K * N1 + N1)), nan(K * N1 + N1)
        ops.dense_backward(s["gh1"], s["a1"], s["x0"], W1, "sigmoid", slabs, ns, gx=s["dx"], out_bn=(mean, rstd, gamma), bn_sums=bsum, batch_total=Bt,
                           in_drop_p=CH_P, in_site=0, **drop(s))
        ops.reduce_slabs(slabs, ns, K * N1 + N1, red)
        grads["dW1"] += _np64(red)[:K * N1].reshape(K, N1)
        grads["db1"] += _np64(red)[K * N1:]
    torch.cuda.synchronize()
    grads["dx"] = np.concatenate([_np64(s["dx"]) for s in sh])
    grads["dgamma"], grads["dbeta"] = _np64(dgamma), _np64(dbeta)
    assert abs(float(rstd[CH_DEAD]) * np.sqrt(CH_EPS) - 1.0) <= 1e-6        # zero batch variance
    for k in ("dW1", "db1", "dx", "dgamma", "dbeta", "dW2", "db2"):
        assert np.all(np.isfinite(grads[k])), k
        _close(grads[k], ref[k], k, rtol=1e-4, atol_frac=1e-5)
        assert np.all(grads[k][ref[k] == 0] == 0), k + ": non-zero where the reference is exactly 0"
