"""-m gpu: brNeumfTailFused called directly (ops.neumf_tail_fused) against a float64 reference of the whole tail.

The tail of the NeuMF step (trainers/NFC_plain.py:143-155, src/models/NeuMFModel.py:75-93): BatchNorm-2 affine + dropout -> Dense(n3) ->
concat [dot | a3] -> Dense(1) -> sigmoid -> loss, and the backward of all of it.  The engines only ever reach it through brNeumfStepRun at
the shapes they produce; here both forms (MFMA: csrc/tail_mfma.hip, VALU: csrc/tail.hip) run at the shapes where they can go wrong: one
keep word per row (n2 <= 32), full and ragged 16-row tiles, a batch behind the 256-workgroup grid cap (a second tile per wave, slabs nobody
owns), every activation x loss x concat order, explicit BatchNorm vectors and the in-launch fold, no dropout, optional outputs left out,
the largest widths the VALU form's 128-row LDS tiles hold, and the widths beyond them, which it walks as two 64-row tiles per workgroup.

Inputs are float32 with fixed seeds; a2 / gh2 live in buffers padded to 4 floats, the a2 padding holds 1e30 (the MFMA form multiplies it
by a zero scale).  Every output that the launch WRITES is pre-filled with NaN (all slabs included) and must come back finite; the two
buffers it ADDS to (sums, bn_sums: double atomics) start at zero.  Rows 0, B/2 and B-1 get |logit| of about 40 and 100 through dot.
Conditions asserted on the reference alone: relu cases keep every |z3| >= 1e-4 (no kink flip between fp32 and fp64; seeds chosen on the
CPU), every |p - 0.5| >= 1e-4 so the counts are well defined (rows whose reference logit lands within 1e-3 of 0 have their dot moved
0.05 away before anything runs), except in the all-zero case, where logit = 0, p = 0.5 exactly and Keras' strict `> 0.5` predicts negative.

The weights are drawn at the scale of a Keras-initialised layer (variance 1 / fan-in).  The kernels form act'(z3) from the stored
activation and dlogit from the stored p, as the whole project does (oracle act_bwd_from_out): the fp32 rounding of a3 is amplified
by 1 / (1 - a3) in a3 (1 - a3), that of p by 1 / (1 - p) in the MSE gradient, so the 1e-5 x sum |summands| bar on the parameter gradients,
made for layers at that scale, cannot hold where most units of a row are saturated.  A first draft drew W3 with a fixed sigma of 0.3: at
n2 >= 100 that is |z3| of 4 and more, and the bar was missed on a one-row batch (102 x 32, sigmoid: db3 at 1.8 x the bar) and on
128 x 32 with MSE (dW3 at 8.5 x the bar where the 1e-12 floor carries it), by the VALU form, with every per-row output inside 0.1 of
its bar.  The rows at |logit| = 40 and 100 stay: p is exactly 0 or 1 there and their gradient terms vanish in both precisions.

Tolerances are the project's own (none measured on these kernels): a3 / logit / prob / ddot: _close of test_gpu_neumf.py; gh2 and the
BatchNorm-backward sums: the gx / "sum dh" bars of test_dense_layer_shapes; parameter gradients: 1e-5 x the sum of |summands| (gabs of
neumf_step_grads) + 1e-12; loss sums 1e-5 relative; counts exact; folded scale / mean / rstd / moving statistics 1e-6 relative to float64
(two or three correctly rounded fp32 operations), shift 1e-6 (|beta| + |mean scale|).  The measured maxima (error / bound) go to
neumf_tail_errors.json in the directory that BR_TEST_REPORT_DIR names, when it is set and exists.
"""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import binrec_oracle as O
from tests.test_gpu_neumf import _close

pytestmark = pytest.mark.gpu

SEED, STEP, SITE, ROW0 = 0x1234ABCD5678, 5, 2, 4099
REPORT = {}


def _ops():
    return import_module("binary-recommendation_amd.ops")


def _lib():
    return import_module("binary-recommendation_amd._lib")


class Case:
    def __init__(self, n2, n3, B, act="sigmoid", loss="bce", mf_first=1, drop_p=0.2, fold=True, padded=True, a3=True, sums=True, bn_sums=True,
                 zero=False, seed=0):
        self.n2, self.n3, self.B, self.act, self.loss, self.mf_first, self.drop_p = n2, n3, B, act, loss, mf_first, drop_p
        self.fold, self.padded, self.a3, self.sums, self.bn_sums, self.zero, self.seed = fold, padded, a3, sums, bn_sums, zero, seed

    @property
    def id(self):
        opt = "".join(c for c, on in (("-noa3", not self.a3), ("-nosums", not self.sums), ("-nobnsums", not self.bn_sums), ("-zero", self.zero),
                                      ("-unpadded", not self.padded)) if on)
        return (f"{self.n2}x{self.n3}-B{self.B}-{self.act}-{self.loss}-mf{self.mf_first}-p{self.drop_p}-" + ("fold" if self.fold else "vectors") + opt)

    @property
    def mfma(self):
        return self.n2 <= 64 and self.n3 <= 16 and self.padded


def make_inputs(c: Case):
    """float32 inputs of a case (numpy), the same on every call."""
    rng = np.random.default_rng(1000003 * c.n2 + 1009 * c.n3 + c.B + 7919 * c.seed)
    n2, n3, B = c.n2, c.n3, c.B
    f = np.float32
    mean = rng.normal(0.4, 0.1, n2); var = rng.uniform(0.05, 0.3, n2)
    a2 = (mean + np.sqrt(var) * rng.standard_normal((B, n2))).astype(f)
    # weights at the scale of a Keras-initialised layer (variance 1 / fan-in), so that z3 and the logit stay of order 1 at every width
    inp = {"a2": a2, "W3": rng.normal(0, n2 ** -0.5, (n2, n3)).astype(f), "b3": rng.normal(0, 0.1, n3).astype(f),
           "w4": rng.normal(0, (n3 + 1) ** -0.5, n3 + 1).astype(f), "b4": rng.normal(0, 0.1, 1).astype(f),
           "dot": rng.normal(0, 1.0, B).astype(f), "labels": (rng.random(B) < 0.3).astype(f),
           "inv_batch": f(1.0 / B), "drop_p": f(c.drop_p)}
    if c.fold:
        bt = 1000.0
        frac = rng.dirichlet(np.ones(8), size=2 * n2).T                            # (8, 2*n2): the sums spread over the replicas
        inp.update(stats=frac * np.concatenate([bt * mean, bt * (var + mean ** 2)]), batch_total=bt,
                   gamma=(1 + rng.normal(0, 0.1, n2)).astype(f), beta=rng.normal(0, 0.1, n2).astype(f), eps=f(1e-3), momentum=f(0.99),
                   mm=rng.normal(0.4, 0.1, n2).astype(f), mv=rng.uniform(0.05, 0.3, n2).astype(f))
    else:
        inp.update(scale2=rng.uniform(0.5, 1.5, n2).astype(f), shift2=rng.normal(0, 0.3, n2).astype(f),
                   mean2=rng.normal(0.4, 0.1, n2).astype(f), rstd2=rng.uniform(0.5, 2.0, n2).astype(f))
    inp["keep"] = O.dropout_mask(SEED, STEP, SITE, B, n2, float(c.drop_p), ROW0)
    if c.zero:
        for k in ("W3", "b3", "w4", "b4", "dot"):
            inp[k] = np.zeros_like(inp[k])
        return inp
    wdot = float(inp["w4"][0 if c.mf_first else n3])
    if abs(wdot) < 0.1:                                                            # the extreme logits below are made through dot
        wdot = 0.5
        inp["w4"][0 if c.mf_first else n3] = wdot
    lz = tail_reference(c, inp)["logit"]
    near = np.abs(lz) < 1e-3                                                       # counts at the 0.5 threshold must be well defined
    inp["dot"][near] += f(0.05 / wdot)
    if B >= 15:                                                                    # saturated rows, right and wrong: p = 1 - 4e-18, p = 4e-44, ...
        for row, target, y in ((0, 40.0, 1.0), (B // 2, -100.0, 1.0), (B - 1, 100.0, 0.0)):
            inp["dot"][row] += f((target - lz[row]) / wdot)
            inp["labels"][row] = y
    return inp


def tail_reference(c: Case, inp):
    """float64 numpy reference of the whole tail; every reduced quantity comes with the sum of |summands| (gabs)."""
    d = lambda k: np.asarray(inp[k], dtype=np.float64)
    n3, B = c.n3, c.B
    a2, W3, b3, w4, b4, dot, y = d("a2"), d("W3"), d("b3"), d("w4"), d("b4"), d("dot"), d("labels")
    r = {}
    if c.fold:
        st = d("stats").sum(0)
        n2 = c.n2
        mean = st[:n2] / inp["batch_total"]
        var = np.maximum(st[n2:] / inp["batch_total"] - mean * mean, 0.0)           # biased batch variance [TF-sem]
        rstd = 1.0 / np.sqrt(var + float(inp["eps"]))
        scale = d("gamma") * rstd
        shift = d("beta") - mean * scale
        mom = float(inp["momentum"])
        r.update(scale=scale, shift=shift, mean=mean, rstd=rstd, shift_mag=np.abs(d("beta")) + np.abs(mean * scale),
                 mm=d("mm") * mom + mean * (1 - mom), mv=d("mv") * mom + var * (1 - mom))
    else:
        scale, shift, mean, rstd = d("scale2"), d("shift2"), d("mean2"), d("rstd2")
    p_drop = float(inp["drop_p"])
    km = inp["keep"].astype(np.float64) / (1.0 - p_drop)
    x = km * (a2 * scale + shift)
    z3 = x @ W3 + b3
    a3 = O.act_fwd(z3, c.act)
    w4a = w4[1:] if c.mf_first else w4[:n3]
    wdot = w4[0] if c.mf_first else w4[n3]
    comb = np.concatenate([dot[:, None], a3], axis=1) if c.mf_first else np.concatenate([a3, dot[:, None]], axis=1)
    logit = comb @ w4 + b4[0]
    prob = O.sigmoid(logit)
    inv_b = float(inp["inv_batch"])
    bce_mean, dbce = O.bce_from_logits(logit, y)
    bce_rows = np.maximum(logit, 0) - logit * y + np.log1p(np.exp(-np.abs(logit)))
    assert abs(bce_rows.mean() - bce_mean) <= 1e-12 * abs(bce_mean)
    if c.loss == "bce":
        loss_rows, dlogit = bce_rows, dbce * B * inv_b
    else:
        loss_rows, dlogit = (prob - y) ** 2, 2.0 * (prob - y) * prob * (1 - prob) * inv_b
    pp, yp = prob > 0.5, y > 0.5
    km_ = O.keras_metrics(prob, y)
    assert abs(km_["binary_accuracy"] * B - (pp == yp).sum()) < 1e-6
    sums = np.array([loss_rows.sum(), ((prob - y) ** 2).sum(), np.abs(prob - y).sum(), (pp == yp).sum(), bce_rows.sum(),
                     (pp & yp).sum(), (pp & ~yp).sum(), (~pp & yp).sum()], dtype=np.float64)
    dz3 = dlogit[:, None] * w4a[None, :] * O.act_bwd_from_out(a3, c.act)
    gh2 = km * (dz3 @ W3.T)
    xhat = (a2 - mean) * rstd
    A = np.abs
    r.update(z3=z3, a3=a3, logit=logit, prob=prob, sums=sums, ddot=dlogit * wdot, gh2=gh2,
             dW3=x.T @ dz3, db3=dz3.sum(0), dW4=comb.T @ dlogit, db4=np.array([dlogit.sum()]),
             bn_dh=gh2.sum(0), bn_dhx=(gh2 * xhat).sum(0),
             gabs={"dW3": A(x).T @ A(dz3), "db3": A(dz3).sum(0), "dW4": A(comb).T @ A(dlogit), "db4": np.array([A(dlogit).sum()])})
    return r


def check_conditions(c: Case, ref):
    """the conditions on the inputs, on the reference alone"""
    if c.act == "relu":
        assert np.abs(ref["z3"]).min() >= 1e-4, "relu kink: pick another seed"
    if c.zero:
        assert np.all(ref["logit"] == 0.0) and np.all(ref["prob"] == 0.5)
    else:
        assert np.abs(ref["prob"] - 0.5).min() >= 1e-4


class Run:
    """device buffers of one launch: outputs NaN-filled, accumulators zero"""

    def __init__(self, c: Case, inp, dev, explicit=None):
        ops = _ops()
        n2, n3, B = c.n2, c.n3, c.B
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        ld = (n2 + 3) & ~3 if c.padded else n2
        a2buf = torch.full((B, ld), 1e30, device=dev)
        a2buf[:, :n2] = td(inp["a2"])
        self.ghbuf = nan(B, ld)
        self.a3, self.logit, self.prob, self.ddot = (nan(B, n3) if c.a3 else None), nan(B), nan(B), nan(B)
        self.sums = torch.zeros(ops.SUM_SLOTS, ops.METRIC_SUMS, dtype=torch.float64, device=dev) if c.sums else None
        self.bn_sums = torch.zeros(ops.STAT_REPLICAS, 2 * n2, dtype=torch.float64, device=dev) if c.bn_sums else None
        self.n_slabs, self.elems = ops.neumf_tail_slabs(B), ops.neumf_tail_slab_elems(n2, n3)
        self.slabs = nan(self.n_slabs * self.elems)
        keep = None
        if c.drop_p > 0:
            keep = ops.dropout_keep_bits(float(inp["drop_p"]), SEED, STEP, ROW0, B, [SITE], [n2])[0]
        kw = {}
        self.fold_out = None
        if explicit is not None:
            kw.update(zip(("scale2", "shift2", "mean2", "rstd2"), explicit))
        elif c.fold:
            self.fold_out = [nan(n2) for _ in range(4)]
            self.mm, self.mv = td(inp["mm"]), td(inp["mv"])
            kw["bn2"] = (td(inp["stats"]), inp["batch_total"], td(inp["gamma"]), td(inp["beta"]), float(inp["eps"]), float(inp["momentum"]),
                         self.mm, self.mv, *self.fold_out)
        else:
            kw.update({k: td(inp[k]) for k in ("scale2", "shift2", "mean2", "rstd2")})
        self.args = (a2buf[:, :n2], td(inp["W3"]), td(inp["b3"]), td(inp["w4"]), td(inp["b4"]), td(inp["dot"]), td(inp["labels"]), c.act, c.mf_first,
                     c.loss, float(inp["inv_batch"]), self.logit, self.prob, self.ddot, self.ghbuf[:, :n2])
        self.kw = dict(kw, drop_p=float(inp["drop_p"]), keep=keep, a3=self.a3, sums=self.sums, bn_sums=self.bn_sums, slabs=self.slabs)
        self.c, self.ld = c, ld

    def launch(self):
        ops = _ops()
        ops.neumf_tail_fused(*self.args, **self.kw)
        self.red = torch.empty(self.elems, device=self.ghbuf.device)
        ops.reduce_slabs(self.slabs, self.n_slabs, self.elems, self.red)
        torch.cuda.synchronize()
        return self

    def outputs(self):
        return [t for t in (self.a3, self.logit, self.prob, self.ddot, self.ghbuf, self.slabs) if t is not None] + list(self.fold_out or [])


def _ratio(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref) + 1e-300)))


def _ratio_close(got, ref, rtol=1e-5, atol_frac=5e-6):
    return _ratio(got, ref, rtol, atol_frac * (np.abs(np.asarray(ref, dtype=np.float64)).max() + 1e-30))


def compare(c: Case, inp, ref, run: Run, tag=""):
    """every output of a launch against the reference; prints and records error / bound per quantity before asserting"""
    n2, n3, B = c.n2, c.n3, c.B
    np_ = lambda t: t.cpu().numpy().astype(np.float64)
    rep = {}
    for t in run.outputs():
        if t is run.ghbuf:
            g = t[:, :n2]
            assert bool(torch.isfinite(g).all()), "gh2 not fully written"
            pad = t[:, n2:]
            assert bool((torch.isnan(pad) | (pad == 0)).all()), "gh2 padding: untouched or zero"
        else:
            assert bool(torch.isfinite(t).all()), "an output was not fully written"
    got = {"logit": np_(run.logit), "prob": np_(run.prob), "ddot": np_(run.ddot), "gh2": np_(run.ghbuf[:, :n2])}
    if c.a3:
        got["a3"] = np_(run.a3)
    red = np_(run.red)
    got.update(dW3=red[:n2 * n3].reshape(n2, n3), db3=red[n2 * n3:n2 * n3 + n3], dW4=red[n2 * n3 + n3:n2 * n3 + 2 * n3 + 1], db4=red[n2 * n3 + 2 * n3 + 1:])
    for k in ("a3", "logit", "prob", "ddot"):
        if k in got:
            rep[k] = _ratio_close(got[k], ref[k])
    rep["gh2"] = _ratio_close(got["gh2"], ref["gh2"], 1e-4, 1e-5)
    for k in ("dW3", "db3", "dW4", "db4"):
        rep[k] = float(np.max(np.abs(got[k] - ref[k]) / (1e-5 * ref["gabs"][k] + 1e-12)))
    if c.bn_sums:
        bs = np_(run.bn_sums).sum(0)
        got["bn_dh"], got["bn_dhx"] = bs[:n2], bs[n2:]
        rep["bn_dh"] = _ratio_close(got["bn_dh"], ref["bn_dh"], 1e-4, 1e-5)
        rep["bn_dhx"] = _ratio_close(got["bn_dhx"], ref["bn_dhx"], 1e-4, 1e-5)
    if c.sums:
        got["sums"] = np_(run.sums).sum(0)
        for j, k in ((0, "loss"), (1, "se"), (2, "ae"), (4, "bce")):
            rep["sum_" + k] = abs(got["sums"][j] - ref["sums"][j]) / (1e-5 * abs(ref["sums"][j]) + 1e-300)
    if run.fold_out is not None:
        fo = [np_(t) for t in run.fold_out]
        for k, g in zip(("scale", "mean", "rstd"), (fo[0], fo[2], fo[3])):
            rep["bn_" + k] = float(np.max(np.abs(g - ref[k]) / (1e-6 * np.abs(ref[k]) + 1e-300)))
        rep["bn_shift"] = float(np.max(np.abs(fo[1] - ref["shift"]) / (1e-6 * ref["shift_mag"])))
        rep["bn_mm"] = float(np.max(np.abs(np_(run.mm) - ref["mm"]) / (1e-6 * np.abs(ref["mm"]))))
        rep["bn_mv"] = float(np.max(np.abs(np_(run.mv) - ref["mv"]) / (1e-6 * np.abs(ref["mv"]))))
    REPORT[c.id + tag] = rep
    print(c.id + tag, json.dumps({k: round(v, 4) for k, v in rep.items()}))
    # the assertions proper
    for k in ("a3", "logit", "prob", "ddot"):
        if k in got:
            _close(got[k], ref[k], k)
    _close(got["gh2"], ref["gh2"], "gh2", rtol=1e-4, atol_frac=1e-5)
    for k in ("dW3", "db3", "dW4", "db4"):
        assert np.all(np.abs(got[k] - ref[k]) <= 1e-5 * ref["gabs"][k] + 1e-12), "grad " + k
    if c.bn_sums:
        _close(got["bn_dh"], ref["bn_dh"], "sum gh2", rtol=1e-4, atol_frac=1e-5)
        _close(got["bn_dhx"], ref["bn_dhx"], "sum gh2*xhat2", rtol=1e-4, atol_frac=1e-5)
    if c.sums:
        for j in (0, 1, 2, 4):
            assert abs(got["sums"][j] - ref["sums"][j]) <= 1e-5 * abs(ref["sums"][j]), ("metric sum", j, got["sums"][j], ref["sums"][j])
        for j in (3, 5, 6, 7):
            assert got["sums"][j] == ref["sums"][j], ("count", j, got["sums"][j], ref["sums"][j])
    for k in [k for k in rep if k.startswith("bn_") and k not in ("bn_dh", "bn_dhx")]:
        assert rep[k] <= 1.0, (k, rep[k])
    return rep


# ---------------------------------------------------------------------------------------------------------------- the cases
# MFMA form: every (n2, n3) with one ragged and one exact batch, every batch size at least once; activation x loss x concat order, drop_p,
# fold / vectors and the optional outputs rotate over them.  relu stays on the small cases (the kink condition; seeds from the CPU).
MFMA = [
    Case(50, 10, 129, "sigmoid", "bce", 1, 0.2, fold=True),
    Case(50, 10, 128, "relu", "mse", 0, 0.2, fold=True),
    Case(64, 16, 300, "sigmoid", "mse", 1, 0.2, fold=False),
    Case(64, 16, 16, "relu", "bce", 0, 0.0, fold=True),
    Case(32, 16, 17, "relu", "bce", 1, 0.2, fold=False),
    Case(32, 16, 128, "sigmoid", "mse", 0, 0.2, fold=True, a3=False),
    Case(33, 5, 127, "relu", "mse", 1, 0.2, fold=True, sums=False),
    Case(33, 5, 16, "sigmoid", "bce", 0, 0.0, fold=False),
    Case(17, 3, 15, "sigmoid", "bce", 0, 0.2, fold=True, bn_sums=False),
    Case(17, 3, 128, "relu", "mse", 1, 0.2, fold=False),
    Case(4, 1, 1, "sigmoid", "mse", 0, 0.2, fold=True),
    Case(4, 1, 16, "relu", "bce", 1, 0.2, fold=False, a3=False, sums=False, bn_sums=False),
    Case(63, 15, 17, "sigmoid", "bce", 1, 0.0, fold=False),
    Case(63, 15, 128, "relu", "bce", 0, 0.2, fold=True),
    Case(50, 10, 129, "sigmoid", "bce", 1, 0.2, fold=True, zero=True),
    # behind the grid cap of 256 workgroups: waves walk a second tile, slab 256 of 257 has no owner and must read as zeros
    Case(64, 16, 32768 + 19, "sigmoid", "bce", 1, 0.2, fold=True),
]
# VALU form: the widest shapes its 128-row LDS tiles hold (include/binrec.h), n3 not a multiple of 4, n2 > 64, the default shape forced
# through it by unpadded strides; then the widths beyond, run as two 64-row passes per workgroup: a last workgroup whose second pass is
# ragged (127 = 64 + 63), empty (300 = 2 * 128 + 44, and B = 1) and one row long (129)
VALU = [
    Case(65, 10, 129, "sigmoid", "bce", 1, 0.2, fold=True),
    Case(50, 17, 1, "sigmoid", "mse", 0, 0.2, fold=False),
    Case(64, 32, 127, "relu", "bce", 1, 0.2, fold=False),
    Case(100, 32, 300, "sigmoid", "mse", 1, 0.0, fold=True, a3=False),
    Case(128, 8, 128, "relu", "mse", 0, 0.2, fold=True),
    Case(128, 12, 300, "sigmoid", "bce", 0, 0.2, fold=True),
    Case(128, 32, 127, "relu", "mse", 1, 0.2, fold=False, seed=2),
    Case(102, 32, 1, "sigmoid", "bce", 1, 0.2, fold=True, sums=False),
    Case(124, 16, 129, "relu", "bce", 0, 0.0, fold=False, a3=False, bn_sums=False),
    Case(50, 10, 129, "sigmoid", "bce", 1, 0.2, fold=True, padded=False),
]


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("BR_TEST_REPORT_DIR", "")
    if out and os.path.isdir(out) and REPORT:
        worst = {}
        for rep in REPORT.values():
            for k, v in rep.items():
                worst[k] = max(worst.get(k, 0.0), v)
        with open(os.path.join(out, "neumf_tail_errors.json"), "w") as fh:
            json.dump({"note": "max |got - float64| / bound per quantity (1.0 = at the bound)", "worst": worst, "cases": REPORT}, fh, indent=1)


@pytest.mark.parametrize("c", MFMA + VALU, ids=lambda c: c.id)
def test_tail_against_float64(dev, c):
    assert c.mfma == (c in MFMA)
    inp = make_inputs(c)
    ref = tail_reference(c, inp)
    check_conditions(c, ref)
    run = Run(c, inp, dev).launch()
    compare(c, inp, ref, run)
    if c.zero:      # logit = 0, p = 0.5 exactly: Keras' strict > 0.5 predicts negative
        y = inp["labels"]
        assert np.all(run.logit.cpu().numpy() == 0.0) and np.all(run.prob.cpu().numpy() == 0.5)
        s = run.sums.sum(0).cpu().numpy()
        assert s[3] == (y <= 0.5).sum() and s[5] == 0 and s[6] == 0 and s[7] == (y > 0.5).sum()
    if c.B > 256 * 128:
        last = run.slabs.view(run.n_slabs, run.elems)[256:]
        assert last.shape[0] == 1 and bool((last == 0).all()), "the slab behind the grid must read as zeros"


def test_fold_equals_its_own_vectors(dev):
    """The in-launch BatchNorm fold writes scale / shift / mean / rstd; the same launch fed those four vectors runs the same instructions
    on the same operands: a3, logit, prob, ddot, gh2 and the slabs are bit-equal (the double atomics of sums / bn_sums are not ordered)."""
    c = MFMA[0]
    inp = make_inputs(c)
    a = Run(c, inp, dev).launch()
    b = Run(c, inp, dev, explicit=a.fold_out).launch()
    for x, y in ((a.a3, b.a3), (a.logit, b.logit), (a.prob, b.prob), (a.ddot, b.ddot), (a.ghbuf[:, :c.n2], b.ghbuf[:, :c.n2]), (a.slabs, b.slabs)):
        assert torch.equal(x, y)


def test_both_forms_agree_with_float64_on_identical_inputs(dev):
    """(50, 10): padded strides take the MFMA form, lda2 = ldgh2 = 50 the VALU form; the same inputs, the same reference."""
    cm, cv = MFMA[0], VALU[-1]
    assert (cm.n2, cm.n3, cm.B, cm.act, cm.loss, cm.mf_first, cm.seed) == (cv.n2, cv.n3, cv.B, cv.act, cv.loss, cv.mf_first, cv.seed) and cm.mfma and not cv.mfma
    inp = make_inputs(cm)
    inp_v = make_inputs(cv)
    for k in inp:
        assert np.array_equal(np.asarray(inp[k]), np.asarray(inp_v[k])), k
    ref = tail_reference(cm, inp)
    rm = Run(cm, inp, dev).launch()
    rv = Run(cv, inp, dev).launch()
    assert rm.ld == 52 and rv.ld == 50
    compare(cm, inp, ref, rm, tag=" (forms: mfma)")
    compare(cv, inp, ref, rv, tag=" (forms: valu)")
    # and with each other, to the sum of the two bounds
    for x, y, rt, af in ((rm.logit, rv.logit, 2e-5, 1e-5), (rm.ghbuf[:, :50], rv.ghbuf[:, :50], 2e-4, 2e-5)):
        _close(x.cpu().numpy(), y.cpu().numpy(), "mfma vs valu", rtol=rt, atol_frac=af)
