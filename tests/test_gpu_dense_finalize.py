"""-m gpu: the dense finalize (csrc/finalize.hip, finalize.h) - the fixed-order reduction of the three dW|db slab regions, the BatchNorm
parameter gradients from the double column sums and Keras-Adam on the flat vector, one launch - against float64 and against the
separate kernels it replaced, and the three places the step driver can run it from (csrc/neumf_step.cpp, BR_KEEP_PREFETCH).

(a) brDenseFinalize alone (ops.dense_finalize) on a synthetic layout in which no boundary is convenient: regions of 130, 65 and 7
    elements, BatchNorm widths 33 and 1, n = 270; the third region lies in front of the first, a dgamma range sits between two slab
    regions, so the first 64-element workgroup spans a slab region, a BatchNorm range and a region with another slab count, and the
    last workgroup is ragged.  Slab counts come from the code: part p of final_part takes the 4-wide loop when p + 48 < n_slabs, a
    second time when p + 112 < n_slabs, and the tail steps by 16 - hence 1, 2, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 127, 128, 129.
      grad, slab regions: |got - float64 sum| <= d 2^-24 sum|terms| 1.01, d = ceil(n_slabs / 16) + 15 (the fp32 additions on the longest
        chain: one part's, then the 15 additions of the parts; 1.01 = the second-order terms).  Derived, not measured.  The inputs are
        first shown (on the CPU, also from tests/test_dense_finalize_cpu.py) to be such that leaving out or doubling ANY one slab moves
        every element of its region by more than 10 x that bound.  Bit for bit against a numpy float32 restatement of the order
        (16 interleaved parts, slabs p, p + 16, .. in that order, parts added 0..15) and against ops.reduce_slabs per region.
      grad, BatchNorm ranges: the bits of np.float32 of a float64 loop over the replicas in replica order (dbeta from the first N
        columns, dgamma from the second N), and of ops.bn_param_grads_pair.
      theta, m, v: the bits of ops.adam_flat on the same start with the kernel's own grad; float64 O.adam_dense fed that fp32 gradient
        within test_adam_flat_and_adagrad's rtol 1e-5 / atol 1e-7 (theta) and test_adam_sparse_tf_form's 2e-6 max|.| floors (m, v).
        The start is two earlier steps' worth of moments, with elements at m = v = 0, elements with sqrt(v) = 1e-10 << eps, and a
        BatchNorm block whose sums are zero (g exactly 0); alpha_t of steps 1 and 1000.
      theta = None (the data-parallel host, fused_final == 2): the same grad bits.
    The largest error / bound per slab-count triple goes to dense_finalize_errors.json in the directory that BR_TEST_REPORT_DIR names,
    when it is set and exists (on an MI355X: 0.04 to 0.11 of the bound; every bit-equality above held as written).

(b) whole steps with BR_KEEP_PREFETCH = 0 (finalize inline behind the Adam rows, dropout planes made at the head of the next step),
    1 (both as launches on the aux stream behind a fork / join) and 2 (default: both ride as extra workgroups of the Adam-rows grid,
    sparse_opt.hip AdamRiders): three engines from the same parameters, 4 eager steps of duplicate-heavy ids, and after EVERY step
    the bits of the metric sums, theta / adam_m / adam_v / grad, both fused tables with m, v and last (deferred) or marks (sweep) and
    the BatchNorm moving statistics must be equal.  The planes cannot be compared buffer to buffer - placement 0 holds THIS step's
    rows [0, B), placements 1 and 2 the NEXT step's rows [0, max_batch) - so each is compared, bit for bit, with brDropoutKeepBits run
    alone for the step it must hold (stronger than equality among the three).  Rider index map of the wave kernel
    (adam_rows_launch, strip 4): rows_x = ceil(B / 16) per table, total = keep blocks(max_batch) + ceil(n_dense / 64),
    grid = 2 rows_x + total, P = grid / total; every P-th workgroup is a rider.  The P each case reaches stands in its id and is
    recomputed and asserted by the test; CASES covers P = 1 (riders outnumber the row workgroups), 2 and 3, grid % total != 0, a ragged
    step, B = 7, both id widths, rows of 64 and 128 floats, and rows of 20 floats (row-group kernel: only the planes ride, keep_x).
    A placement-2 engine is also held to the float64 oracle with test_forward_backward_parity's own assertions for two steps, the
    second of which consumes the planes the riders made - "all three equal" cannot mean "all three wrong".
    The BatchNorm column sums are double atomics over 8 replicas; their order is not fixed, and a sum that lands within 1e-16 of a
    float32 rounding boundary could differ between two runs of the SAME placement.  The bit-equal engine tests of test_gpu_neumf.py
    live with the same one-in-many-millions chance.
"""
import functools
import json
import math
import os
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import binrec_oracle as O

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ (a) the layout
R = 8                                # BR_STAT_REPLICAS
ELEMS = (130, 65, 7)                 # slab regions 0, 1, 2
GRAD_OFF = (40, 204, 0)              # region 2 lies in front of region 0
BN_N = (33, 1)
DGAMMA_OFF = (7, 269)                # BatchNorm 0's dgamma between regions 2 and 0
DBETA_OFF = (171, 170)
N = 270                              # [reg2 7 | dgamma0 33 | reg0 130 | dbeta1 1 | dbeta0 33 | reg1 65 | dgamma1 1]
SLAB_COUNTS = [(1, 65, 128), (2, 113, 16), (15, 129, 48), (17, 64, 127), (49, 63, 112), (129, 2, 63), (128, 17, 1)]
ALL_COUNTS = {1, 2, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 127, 128, 129}
LR = 1e-3
U24 = 2.0 ** -24


def layout_cover():
    """how often each of the N parameters is written by the layout above (must be once each)"""
    cover = np.zeros(N, np.int64)
    for el, off in zip(ELEMS, GRAD_OFF):
        cover[off:off + el] += 1
    for n, og, ob in zip(BN_N, DGAMMA_OFF, DBETA_OFF):
        cover[og:og + n] += 1
        cover[ob:ob + n] += 1
    return cover


def chain_depth(n_slabs):
    return math.ceil(n_slabs / 16) + 15


def slab_bound(S):
    """per element: d 2^-24 sum|terms| 1.01"""
    return chain_depth(S.shape[0]) * U24 * np.abs(S.astype(np.float64)).sum(0) * 1.01


@functools.lru_cache(maxsize=None)
def slab_inputs(counts):
    """three float32 [n_slabs][elems] arrays: mixed sign, magnitudes log-uniform over two decades"""
    rng = np.random.default_rng(1000 * counts[0] + 10 * counts[1] + counts[2])
    out = []
    for ns, el in zip(counts, ELEMS):
        mag = 10.0 ** rng.uniform(-1.0, 1.0, size=(ns, el))
        out.append((mag * np.where(rng.random((ns, el)) < 0.5, -1.0, 1.0)).astype(np.float32))
    return tuple(out)


def omission_margin(S):
    """Leaving slab s out of the sum, or adding it twice, moves element e by |S[s, e]|: the smallest such move over the bound,
    per region (must exceed 10 for the bound to see every single-slab mistake)."""
    return float((np.abs(S.astype(np.float64)).min(0) / slab_bound(S)).min())


def reduce_in_kernel_order(S):
    """float32 restatement of final_part / final_apply: part p = slabs p, p + 16, .. added in that order from 0, parts added 0..15"""
    ns, el = S.shape
    parts = np.zeros((16, el), np.float32)
    for p in range(16):
        for s in range(p, ns, 16):
            parts[p] = parts[p] + S[s]
    g = parts[0].copy()
    for q in range(1, 16):
        g = g + parts[q]
    assert g.dtype == np.float32
    return g


def bn_grads_ref(sums):
    """sums float64 [R][2N] -> (dgamma, dbeta) float32: a float64 loop over the replicas in replica order, rounded once"""
    n = sums.shape[1] // 2
    acc = np.zeros(2 * n, np.float64)
    for r in range(R):
        acc = acc + sums[r]
    return acc[n:].astype(np.float32), acc[:n].astype(np.float32)


@functools.lru_cache(maxsize=None)
def bn_inputs(zero_block):
    rng = np.random.default_rng(77 + zero_block)
    out = []
    for b, n in enumerate(BN_N):
        s = rng.normal(size=(R, 2 * n)) * 10.0 ** rng.uniform(-2.0, 1.0, size=(R, 2 * n))
        out.append(np.zeros_like(s) if b == zero_block else s)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def adam_start():
    """theta, m, v (float32) after two earlier steps' worth of moments, with fresh (m = v = 0) and sqrt(v) << eps elements"""
    rng = np.random.default_rng(5)
    theta = rng.normal(scale=0.1, size=N)
    g1, g2 = rng.normal(scale=8.0, size=N), rng.normal(scale=8.0, size=N)
    m = 0.9 * (0.1 * g1) + 0.1 * g2
    v = 0.999 * (0.001 * g1 * g1) + 0.001 * g2 * g2
    e = np.arange(N)
    fresh = e % 7 == 3
    tiny = (e % 11 == 5) & ~fresh
    m[fresh], v[fresh] = 0.0, 0.0
    m[tiny], v[tiny] = np.where(e[tiny] % 2 == 0, 1e-10, -1e-10), 1e-20
    return theta.astype(np.float32), m.astype(np.float32), v.astype(np.float32), fresh, tiny


def _mods():
    return import_module("binary-recommendation_amd.ops"), import_module("binary-recommendation_amd.neumf")


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _np_same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _guarded(a, dev, guard=64):
    """a copy of `a` on the device with NaN in front of and behind it: a read one slab or one column off the buffer poisons the sum"""
    buf = torch.full((a.size + 2 * guard,), float("nan"), dtype=torch.from_numpy(a).dtype, device=dev)
    view = buf[guard:guard + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    return view


_REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("BR_TEST_REPORT_DIR", "")
    if out and os.path.isdir(out) and _REPORT:
        with open(os.path.join(out, "dense_finalize_errors.json"), "w") as fh:
            json.dump({"note": "brDenseFinalize, slab regions: max |grad - float64 sum| / (d 2^-24 sum|terms| 1.01) per slab-count triple (1.0 = at the bound)",
                       "triples": _REPORT}, fh, indent=1)


def test_slab_counts_cover_the_loop_thresholds():
    assert {c for t in SLAB_COUNTS for c in t} == ALL_COUNTS
    assert any(min(t) < 16 and max(t) > 64 for t in SLAB_COUNTS)
    assert np.array_equal(layout_cover(), np.ones(N, np.int64)) and N % 64 and all(e % 64 for e in ELEMS)


@pytest.mark.parametrize("t,zero_block", [(1, 1), (1000, 0)])
@pytest.mark.parametrize("counts", SLAB_COUNTS, ids=lambda c: "slabs%d-%d-%d" % c)
def test_dense_finalize_alone(dev, counts, t, zero_block):
    ops, _ = _mods()
    slabs, sums = slab_inputs(counts), bn_inputs(zero_block)
    th0, m0, v0, fresh, tiny = adam_start()
    # a property of the inputs alone: no single-slab omission or repeat fits inside the bound
    for S in slabs:
        assert omission_margin(S) > 10.0
    d_slabs = [_guarded(S, dev) for S in slabs]
    d_sums = [_guarded(s, dev) for s in sums]
    regions = [(d_slabs[r], counts[r], ELEMS[r], GRAD_OFF[r]) for r in range(3)]
    blocks = [(d_sums[b], BN_N[b], DGAMMA_OFF[b], DBETA_OFF[b]) for b in range(2)]
    td = lambda a: torch.from_numpy(a.copy()).to(dev)
    nan = lambda: torch.full((N,), float("nan"), device=dev)
    alpha = ops.adam_alpha(LR, t)
    grad, th, m, v = nan(), td(th0), td(m0), td(v0)
    ops.dense_finalize(regions, blocks, grad, th, m, v, alpha)
    grad_only = nan()
    ops.dense_finalize(regions, blocks, grad_only)
    # the kernels it replaced, on the same inputs
    parts = nan()
    for r in range(3):
        ops.reduce_slabs(d_slabs[r], counts[r], ELEMS[r], parts[GRAD_OFF[r]:GRAD_OFF[r] + ELEMS[r]])
    ops.bn_param_grads_pair(d_sums[0], parts[DGAMMA_OFF[0]:DGAMMA_OFF[0] + BN_N[0]], parts[DBETA_OFF[0]:DBETA_OFF[0] + BN_N[0]],
                            d_sums[1], parts[DGAMMA_OFF[1]:DGAMMA_OFF[1] + BN_N[1]], parts[DBETA_OFF[1]:DBETA_OFF[1] + BN_N[1]])
    th2, m2, v2 = td(th0), td(m0), td(v0)
    ops.adam_flat(th2, m2, v2, grad, alpha)
    torch.cuda.synchronize()
    g = grad.cpu().numpy()
    assert np.isfinite(g).all(), "elements not written: %s" % np.flatnonzero(~np.isfinite(g))[:8]

    worst = 0.0
    for r, S in enumerate(slabs):
        got = g[GRAD_OFF[r]:GRAD_OFF[r] + ELEMS[r]]
        ref64 = S.astype(np.float64).sum(0)
        ratio = np.abs(got.astype(np.float64) - ref64) / slab_bound(S)
        print("region %d: %d slabs, max error / bound %.4f" % (r, counts[r], ratio.max()))
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, "region %d (%d slabs): %.3f x the derived bound at element %d" % (r, counts[r], ratio.max(), ratio.argmax())
        assert _np_same_bits(got, reduce_in_kernel_order(S)), "region %d (%d slabs): not the stated summation order" % (r, counts[r])
    _REPORT["%d-%d-%d" % counts] = max(worst, _REPORT.get("%d-%d-%d" % counts, 0.0))
    for b, s in enumerate(sums):
        dgamma, dbeta = bn_grads_ref(s)
        assert _np_same_bits(g[DGAMMA_OFF[b]:DGAMMA_OFF[b] + BN_N[b]], dgamma), "dgamma of BatchNorm %d" % b
        assert _np_same_bits(g[DBETA_OFF[b]:DBETA_OFF[b] + BN_N[b]], dbeta), "dbeta of BatchNorm %d" % b
    zb = np.r_[DGAMMA_OFF[zero_block]:DGAMMA_OFF[zero_block] + BN_N[zero_block], DBETA_OFF[zero_block]:DBETA_OFF[zero_block] + BN_N[zero_block]]
    assert np.all(g[zb] == 0.0)
    assert _same_bits(grad, parts), "grad differs from reduce_slabs x 3 + bn_param_grads_pair at %s" % torch.nonzero(grad != parts).view(-1)[:8].tolist()
    assert _same_bits(grad, grad_only), "the gradients-only form (theta = NULL) writes other grad bits"

    # Adam: the bits of adam_flat fed the kernel's own gradient ...
    for name, a, b in (("theta", th, th2), ("m", m, m2), ("v", v, v2)):
        assert _same_bits(a, b), "%s differs from adam_flat at %s" % (name, torch.nonzero(a != b).view(-1)[:8].tolist())
    # ... and float64 on that fp32 gradient
    r_th, r_m, r_v = O.adam_dense(th0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), g.astype(np.float64), LR, t)
    np.testing.assert_allclose(th.cpu().numpy(), r_th, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(m.cpu().numpy(), r_m, rtol=1e-5, atol=2e-6 * np.abs(r_m).max())
    np.testing.assert_allclose(v.cpu().numpy(), r_v, rtol=1e-5, atol=2e-6 * np.abs(r_v).max())
    # the edge elements were really there: untouched parameters under g = 0 with m = v = 0, and denominators dominated by eps
    idle = np.zeros(N, bool); idle[zb] = True
    assert (idle & fresh).any() and np.array_equal(th.cpu().numpy()[idle & fresh], th0[idle & fresh])
    assert (idle & tiny).any() and (~idle & tiny).any() and (~idle & fresh).any()
    assert np.all(np.sqrt(r_v[idle & tiny]) < 1e-2 * 1e-7)


# ------------------------------------------------------------------------------------------------- (b) the three placements in whole steps
HIDDEN = (100, 50, 10)


def rider_map(dim, B, max_batch):
    """(P, grid, total) of adam_rows_launch's one-wave-per-row launch at strip 4 with both kinds of riders"""
    n1, n2, n3 = HIDDEN
    n_dense = 2 * dim * n1 + 3 * n1 + n1 * n2 + 3 * n2 + n2 * n3 + n3 + (n3 + 1) + 1
    keep = sum(-(-(max_batch * ((K + 31) // 32)) // 256) for K in (2 * dim, n1, n2))
    total = keep + -(-n_dense // 64)
    grid = 2 * -(-B // 16) + total
    return grid // total, grid, total


class Case:
    def __init__(self, dim, optimizer, impl, batches, P, idt=torch.int32, rows=(97, 53)):
        self.dim, self.optimizer, self.impl, self.idt, self.rows = dim, optimizer, impl, idt, rows
        self.batches = (batches,) * 4 if isinstance(batches, int) else tuple(batches)
        self.max_batch = max(self.batches)
        self.P = P          # per step; None: rows of 2 dim floats are no wave rows (row-group kernel, the finalize runs alone)

    @property
    def id(self):
        b = "B%d" % self.batches[0] if len(set(self.batches)) == 1 else "B" + "_".join(map(str, self.batches))
        p = "rowgroup" if self.P is None else "P" + "_".join(map(str, sorted(set(self.P)) if len(set(self.batches)) == 1 else self.P))
        return "d%d-%s-%s-%s-%s-%s" % (self.dim, self.optimizer, self.impl, b, "i64" if self.idt == torch.int64 else "i32", p)


BIG = (2999, 1013)     # table rows of the large batches: duplicate-heavy ids, and rows that sit out steps (deferred lags)
CASES = [
    Case(32, "adam_dense", "deferred", 64, (1,) * 4),                                    # grid 205 = 8 row workgroups + 197 riders
    Case(32, "adam_dense", "deferred", 7, (1,) * 4),                                     # grid 199: one row workgroup per table
    Case(32, "adam_dense", "deferred", 4096, (2,) * 4, rows=BIG),                        # grid 834, total 322: 834 % 322 = 190
    Case(32, "adam_dense", "deferred", 8192, (3,) * 4, rows=BIG),                        # grid 1474, total 450: 1474 % 450 = 124
    Case(32, "adam_dense", "deferred", 4096, (2,) * 4, idt=torch.int64, rows=BIG),
    Case(32, "adam_dense", "deferred", (4096, 1000, 4096, 7), (2, 1, 2, 1), rows=BIG),   # ragged: planes for 4096 rows, row workgroups for B
    Case(32, "adam_dense", "sweep", 4096, (2,) * 4, rows=BIG),
    Case(32, "adam_lazy", "sweep", 8192, (3,) * 4, idt=torch.int64, rows=BIG),
    Case(64, "adam_dense", "deferred", 8192, (2,) * 4, rows=BIG),                        # grid 1638, total 614: 1638 % 614 = 410
    Case(64, "adam_dense", "sweep", 64, (1,) * 4),
    Case(64, "adam_lazy", "sweep", (4096, 333, 4096, 4096), (2, 1, 2, 2), rows=BIG),
    Case(10, "adam_dense", "deferred", 300, None),
    Case(10, "adam_dense", "sweep", (300, 7, 300, 300), None),
    Case(10, "adam_lazy", "sweep", 300, None, idt=torch.int64),
]


def test_cases_reach_every_branch_of_the_rider_map():
    """the P in each case's id is what adam_rows_launch's arithmetic gives; together: P = 1, 2 and >= 3, and a grid % total != 0"""
    seen, ragged_grid = set(), False
    for c in CASES:
        if c.P is None:
            assert 2 * c.dim % 64          # no one-wave-per-row shape
            continue
        assert 2 * c.dim in (64, 128)
        for B, P in zip(c.batches, c.P):
            got, grid, total = rider_map(c.dim, B, c.max_batch)
            assert got == P, (c.id, B, got, grid, total)
            seen.add(P)
            ragged_grid = ragged_grid or grid % total != 0
    assert {1, 2, 3} <= seen and ragged_grid
    assert rider_map(32, 64, 64)[:1] == (1,) and rider_map(32, 64, 64)[2] > 2 * 4      # riders outnumber the row workgroups
    assert any(len(set(c.batches)) > 1 for c in CASES) and any(7 in c.batches for c in CASES)
    assert {c.idt for c in CASES if c.dim == 32} == {torch.int32, torch.int64}


def _params(dim, U, I, seed=3):
    """the parameters of test_gpu_neumf._setup: Keras initialisation with the zeros / ones of biases, gammas and moving statistics replaced"""
    spec = O.NeuMFSpec("A", dim=dim)
    p = O.neumf_init(spec, U, I, seed=seed, dt=np.float32)
    rng = np.random.default_rng(seed + 1)
    for k in ("b1", "b2", "b3", "b4", "be1", "be2"):
        p[k] = rng.normal(0, 0.1, p[k].shape).astype(np.float32)
    for k in ("g1", "g2"):
        p[k] = (1 + rng.normal(0, 0.1, p[k].shape)).astype(np.float32)
    for k in ("mm1", "mm2"):
        p[k] = rng.normal(0.4, 0.1, p[k].shape).astype(np.float32)
    for k in ("mv1", "mv2"):
        p[k] = rng.uniform(0.05, 0.3, p[k].shape).astype(np.float32)
    return spec, p


def _engine(dev, p, dim, U, I, max_batch, optimizer="adam_dense", impl="deferred", idt=torch.int32):
    _, neumf = _mods()
    cfg = neumf.NeuMFConfig(variant="A", dim=dim, optimizer=optimizer, seed=0xABCDEF12345, dense_impl=impl)
    assert cfg.hidden == HIDDEN and cfg.dropout > 0          # riders exist only with dropout
    eng = neumf.NeuMFEngine(cfg, U, I, dev, max_batch=max_batch, id_dtype=idt)
    eng.load_numpy_params(p)
    return eng, cfg


def _batch(rng, B, U, I):
    u, i = rng.integers(0, U, B), rng.integers(0, I, B)
    u[: B // 8] = u[0]; i[: B // 6] = i[1]      # long duplicate runs
    return u, i, (rng.random(B) < 0.25).astype(np.float32)


def _state(e):
    """everything a step leaves behind, by name (raw buffers: a deferred table is compared as it lags, with its last[])"""
    s = {"metric sums": e.msums, "theta": e.theta.buf, "adam_m": e.adam_m.buf, "adam_v": e.adam_v.buf, "grad": e.grad.buf, "moving": e.moving_buf}
    for k in ("user", "item"):
        s["table " + k], s["m " + k], s["v " + k] = e.fused[k], e.fused_m[k], e.fused_v[k]
        if e.deferred:
            s["last " + k] = e.last[k]
        elif e._sweep:
            s["mark " + k] = e.mark[k]
    return s


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_three_placements_leave_the_same_bits(dev, monkeypatch, case):
    ops, _ = _mods()
    U, I = case.rows
    spec, p = _params(case.dim, U, I)
    monkeypatch.delenv("BR_AUX_STREAM", raising=False)      # placements 1 and 2 exist only on an engine with its aux stream (the default)
    engines = {}
    for place in ("0", "1", "2"):
        engines[place], cfg = _engine(dev, p, case.dim, U, I, case.max_batch, case.optimizer, case.impl, case.idt)
    widths = (2 * case.dim,) + HIDDEN[:2]
    planes_of = lambda step: torch.cat(ops.dropout_keep_bits(cfg.dropout, cfg.seed, step, 0, case.max_batch, (0, 1, 2), widths))
    td = lambda a, dt: torch.from_numpy(a).to(dev).to(dt)
    rng = np.random.default_rng(41)
    for step, B in enumerate(case.batches, start=1):
        u, i, y = _batch(rng, B, U, I)
        for place, e in engines.items():
            monkeypatch.setenv("BR_KEEP_PREFETCH", place)
            e.train_step(td(u, case.idt), td(i, case.idt), td(y, torch.float32))
            assert e.t == step and e.step_struct.keep_prefetch == int(place)
            assert e.step_struct.keep_ready == (1 if place != "0" and step > 1 else 0)      # prefetched planes are consumed, not remade
        torch.cuda.synchronize()
        want = _state(engines["2"])
        for place in ("0", "1"):
            for name, t in _state(engines[place]).items():
                assert _same_bits(t, want[name]), "step %d: %s of placement %s differs from placement 2 in %d elements" % (
                    step, name, place, int((t != want[name]).sum()))
        # dropout planes: placements 1 and 2 hold the next step's for all max_batch rows, placement 0 this step's rows [0, B)
        nxt, now = planes_of(step + 1), planes_of(step)
        for place in ("1", "2"):
            assert _same_bits(engines[place].keep_bits, nxt), "step %d: planes prefetched by placement %s" % (step, place)
        o = 0
        for K in widths:
            w = ops.dropout_keep_words(B, K)
            assert _same_bits(engines["0"].keep_bits[o:o + w], now[o:o + w]), "step %d: plane of width %d, placement 0" % (step, K)
            o += ops.dropout_keep_words(case.max_batch, K)
    for e in engines.values():
        e.check_ids()


def test_default_placement_against_the_oracle(dev, monkeypatch):
    """Placement 2 for two steps under test_forward_backward_parity's assertions and tolerances, at a batch its headline bound holds for
    (300 rows, dim 32: P = 1, both kinds of riders).  Step 1: eng.grad is written by the riding finalize.  Step 2 starts from the
    engine's own parameters after step 1 (read back, so Adam's amplification of rounding does not enter the comparison) and runs on
    the dropout planes that step 1's riders made: keep_ready, no plane launch of its own."""
    tn = import_module("tests.test_gpu_neumf")
    B, dim, U, I = 300, 32, 97, 53
    assert rider_map(dim, B, B)[0] == 1
    monkeypatch.setenv("BR_KEEP_PREFETCH", "2")
    monkeypatch.delenv("BR_AUX_STREAM", raising=False)
    spec, p = _params(dim, U, I)
    eng, cfg = _engine(dev, p, dim, U, I, B)
    td = lambda a, dt: torch.from_numpy(a).to(dev).to(dt)
    rng = np.random.default_rng(43)
    for step in (1, 2):
        u, i, y = _batch(rng, B, U, I)
        eng.train_step(td(u, torch.int32), td(i, torch.int32), td(y, torch.float32))
        torch.cuda.synchronize()
        assert eng.step_struct.keep_prefetch == 2 and eng.step_struct.keep_ready == (1 if step == 2 else 0)
        tn._assert_step_parity(eng, spec, cfg, p, u, i, y, step=step)
        back = {k: eng.tables[k] for k in ("user_mlp", "item_mlp", "user_mf", "item_mf")}
        back.update({k: eng.theta.view(k) for k in O.DENSE_ORDER})
        back.update(eng.moving)
        p = {k: t.cpu().numpy().reshape(p[k].shape).copy() for k, t in back.items()}
