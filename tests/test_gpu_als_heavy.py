"""-m gpu: the heavy rows of the conjugate-gradient ALS on the device (csrc/als_heavy.hip: brAlsNormalRows, brAlsSolveRowsDenseCg;
als.split_heavy; als.ALSEngine(heavy_rows=); models.ALSModel.train(heavyRows=)) against the numpy restatements of
tests/test_als_heavy_cpu.py.  Determinism and independence are bit equality.  Accuracy of the rows: the bar of test_als_heavy_cpu.py,
max(4 x the float32 numpy restatement's figure, 4 x the figure of float32(X64) itself) against the float64 cg_half_step; of H: the
yardstick of the Gram tests, 4 x the error of the float32 CPU product on the same inputs.  Every case is printed before the test asserts.

Shapes: slice = 64, so that a row of 130 entries already has three slices; row lengths around the 64-entry chunk and slice; every count
of 128-column blocks with a full and a partial last block; both load paths; n_y = 500."""
from importlib import import_module

import numpy as np
import pytest
import torch

from tests.test_als_cg_cpu import cg_half_step
from tests.test_als_cpu import half_step_f64, objective
from tests.test_als_heavy_cpu import bar, heavy_rows_of, normal_rows_f64, references, solve_cases, solve_inputs
from tests.test_gpu_als import N_Y, _bits, _csv, _dev_rows, _engine_case, _row_errs, _solve_case
from tests.test_gpu_als_cg import CG_DIMS, _cholesky_allowance, _g32

pytestmark = pytest.mark.gpu

NORMAL_DIMS = [1, 20, 33, 64, 128, 129, 350, 512]
NORMAL_LENS = [1, 63, 64, 65, 128, 129, 200]


def _m(name):
    return import_module("binary-recommendation_amd." + name)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rows_t(rows, dev):
    return torch.tensor(list(rows), dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------ the normal matrix
def _h_err(H, H64, Yu, c):
    """the Gram tests' figure (tests/test_gpu_als.py::_gram_err) for the weighted product: max |H - H64| over the outer product of the
    weighted column norms"""
    nrm = np.sqrt((c[:, None] * Yu * Yu).sum(0))
    den = np.outer(nrm, nrm)
    den[den == 0] = 1.0
    return float((np.abs(np.asarray(H, np.float64) - H64) / den).max())


def _h_cpu32(Yu, c32):
    """the float32 CPU product, formed as normal_equations (tests/test_als_cpu.py) forms it"""
    Yt = torch.from_numpy(np.ascontiguousarray(Yu, np.float32))
    return ((Yt * torch.from_numpy(c32)[:, None]).T @ Yt).numpy()


@pytest.mark.parametrize("dim", NORMAL_DIMS)
def test_normal_rows_symmetric_deterministic_independent_and_as_accurate_as_float32(dev, dim):
    ops = _m("ops")
    missed = []
    for with_conf in (False, True):
        alpha = 40.0 if with_conf else 0.1                                   # (0.1 is no float32: b is held to the value the kernel is given)
        Y, off, idx, conf = _solve_case(dim, 600 + 2 * dim + with_conf, with_conf, counts=NORMAL_LENS)
        rows = list(range(len(NORMAL_LENS)))
        H64, b64 = normal_rows_f64(Y, off, idx, conf, alpha, rows)
        offd, idxd, confd, rowsd = _t(off, dev), _t(idx, dev), _t(conf, dev), _rows_t(rows, dev)
        outs = {}
        for slice in (64, 128):
            for ld in (dim, dim + 5):                                        # dim + 5: the scalar loads
                if slice == 128 and ld != dim:
                    continue
                Yd, _ = _dev_rows(Y, ld, dev)
                err = ops.new_err_flag(dev)
                H, b = ops.als_normal_rows(Yd, offd, idxd, alpha, rowsd, conf=confd, slice=slice, err_flag=err)
                H2, b2 = ops.als_normal_rows(Yd, offd, idxd, alpha, rowsd, conf=confd, slice=slice, err_flag=err)
                assert int(err.item()) == 0
                assert H.shape == (len(rows), dim, dim) and H.dtype == torch.float32 and b.shape == (len(rows), dim) and b.dtype == torch.float64
                assert torch.equal(_bits(H), _bits(H2)) and torch.equal(b, b2), (slice, ld)             # a second call
                assert torch.equal(_bits(H), _bits(H.transpose(1, 2))), (slice, ld)
                outs[(slice, ld)] = (H, b)
                Hn, bn = H.cpu().numpy(), b.cpu().numpy()
                a32 = np.float64(np.float32(alpha))
                for h, u in enumerate(rows):
                    e = np.arange(off[u], off[u + 1])
                    Yu = Y[idx[e]].astype(np.float64)
                    c = a32 * (conf[e].astype(np.float64) if conf is not None else np.ones(e.size))
                    c32 = np.float32(alpha) * (conf[e] if conf is not None else np.ones(e.size, np.float32))
                    e_k, e_cpu = _h_err(Hn[h], H64[h], Yu, c), _h_err(_h_cpu32(Y[idx[e]], c32.astype(np.float32)), H64[h], Yu, c)
                    b_k = float((np.abs(bn[h] - b64[h]) / np.maximum(((1 + c)[:, None] * np.abs(Yu)).sum(0), 1e-300)).max())
                    print(f"normal rows dim {dim} conf {with_conf} slice {slice} ld {ld} len {e.size}: H kernel {e_k:.3e} float32 CPU {e_cpu:.3e}"
                          f"  b {b_k:.3e}")
                    if not (e_k <= 4 * e_cpu and b_k <= 1e-12):
                        missed.append((with_conf, slice, ld, e.size, e_k, e_cpu, b_k))
        Hd, bd = outs[(64, dim)]
        assert torch.equal(_bits(Hd), _bits(outs[(64, dim + 5)][0])) and torch.equal(bd, outs[(64, dim + 5)][1])   # the two strides
        Yd = _t(Y, dev)
        for h in (0, 3, 4, 6):                                               # a row listed alone, and in another batch
            H1, b1 = ops.als_normal_rows(Yd, offd, idxd, alpha, _rows_t([h], dev), conf=confd, slice=64)
            assert torch.equal(_bits(H1[0]), _bits(Hd[h])) and torch.equal(b1[0], bd[h]), h
        H3, b3 = ops.als_normal_rows(Yd, offd, idxd, alpha, _rows_t([1, 4, 6], dev), conf=confd, slice=64)
        assert torch.equal(_bits(H3), _bits(Hd[[1, 4, 6]])) and torch.equal(b3, bd[[1, 4, 6]])
    assert not missed, missed


def test_normal_rows_of_no_rows_and_of_an_empty_row(dev):
    ops = _m("ops")
    Y, off, idx, conf = _solve_case(20, 5, True, counts=[0, 70])
    Yd, offd, idxd, confd = _t(Y, dev), _t(off, dev), _t(idx, dev), _t(conf, dev)
    H, b = ops.als_normal_rows(Yd, offd, idxd, 1.0, _rows_t([], dev), conf=confd, slice=64)
    assert H.shape == (0, 20, 20) and b.shape == (0, 20)
    H, b = ops.als_normal_rows(Yd, offd, idxd, 1.0, _rows_t([0, 1], dev), conf=confd, slice=64)
    assert not H[0].any() and not b[0].any() and H[1].any() and b[1].any()


def test_normal_rows_ids_out_of_range_are_flagged_and_never_used(dev):
    """An index of -1 and one of n_y, in two rows: the flag is set, the entry counts as absent (compared, never an address), every other
    row keeps its bits; a listed row outside the CSR is flagged too and gives zeros."""
    ops = _m("ops")
    dim = 20
    lens = [70, 130, 65, 200, 90]
    Y, off, idx, _c = _solve_case(dim, 11, False, counts=lens)
    Yd = _t(Y, dev)
    rows = _rows_t(range(5), dev)
    good_H, good_b = ops.als_normal_rows(Yd, _t(off, dev), _t(idx, dev), 10.0, rows, slice=64)
    bad = idx.copy()
    bad[off[1] + 64] = -1                                                    # the second slice of row 1
    bad[off[3] + 199] = N_Y                                                  # the last entry of row 3
    err = ops.new_err_flag(dev)
    H, b = ops.als_normal_rows(Yd, _t(off, dev), _t(bad, dev), 10.0, rows, slice=64, err_flag=err)
    assert int(err.item()) == _m("_lib").parse_enums()["BR_ERRFLAG_RANGE"]
    with pytest.raises(IndexError):
        ops.raise_if_flag(err)
    assert torch.isfinite(H).all() and torch.isfinite(b).all()
    for h in (0, 2, 4):
        assert torch.equal(_bits(H[h]), _bits(good_H[h])) and torch.equal(b[h], good_b[h]), h
    # "absent": the row without that entry
    for h, drop in ((1, off[1] + 64), (3, off[3] + 199)):
        keep = np.ones(len(idx), bool)
        keep[drop] = False
        off2 = off.copy()
        off2[h + 1:] -= 1
        H64, b64 = normal_rows_f64(Y, off2, idx[keep], None, 10.0, [h])
        assert np.abs(H[h].cpu().numpy() - H64[0]).max() <= 1e-5 * np.abs(H64[0]).max()
        assert np.abs(b[h].cpu().numpy() - b64[0]).max() <= 1e-12 * np.abs(b64[0]).max() + 1e-12
        assert not torch.equal(_bits(H[h]), _bits(good_H[h]))
    err = ops.new_err_flag(dev)
    pre = torch.tensor([0, 2, 3], dtype=torch.int64, device=dev)
    H, b = ops.als_normal_rows(Yd, _t(off, dev), _t(idx, dev), 10.0, _rows_t([0, 5], dev), slice=64, err_flag=err, plan=(pre, 3))
    assert int(err.item()) == _m("_lib").parse_enums()["BR_ERRFLAG_RANGE"]
    assert torch.equal(_bits(H[0]), _bits(good_H[0])) and not H[1].any() and not b[1].any()


def test_python_surface_argument_checks(dev):
    ops = _m("ops")
    Y = torch.zeros(10, 8, device=dev)
    off, idx = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    rows = _rows_t([0], dev)
    for slice in (0, 65, 32):
        with pytest.raises(ValueError):
            ops.als_normal_rows(Y, off, idx, 1.0, rows, slice=slice)
    with pytest.raises(TypeError):
        ops.als_normal_rows(Y, off, idx, 1.0, rows.long(), slice=64)
    G, H, b, x0 = ops.gram(Y), torch.zeros(1, 8, 8, device=dev), torch.zeros(1, 8, dtype=torch.float64, device=dev), torch.zeros(1, 8, device=dev)
    for steps in (0, 65):
        with pytest.raises(ValueError):
            ops.als_solve_rows_dense_cg(G, H, b, 0.1, x0, steps=steps)
    with pytest.raises(TypeError):
        ops.als_solve_rows_dense_cg(G, H, b.float(), 0.1, x0)
    with pytest.raises(ValueError):
        ops.als_solve_rows_dense_cg(G, H, b, 0.1, torch.zeros(2, 8, device=dev))
    with pytest.raises(ValueError):
        ops.als_solve_rows_dense_cg(G, H[:, :4, :4].contiguous(), b, 0.1, x0)


# ------------------------------------------------------------------------------ the dense CG
def _dense_dev(ops, dev, Yd, G, off, idx, conf, alpha, rows, X0, reg, steps, slice=64, ld_out=None):
    dim = X0.shape[1]
    H, b = ops.als_normal_rows(Yd, _t(off, dev), _t(idx, dev), alpha, _rows_t(rows, dev), conf=_t(conf, dev), slice=slice)
    out, buf = _dev_rows(np.zeros((len(rows), dim), np.float32), dim if ld_out is None else ld_out, dev, fill=-7.5)
    got = ops.als_solve_rows_dense_cg(G, H, b, reg, _t(X0[rows], dev), steps=steps, out=out)
    assert got is out
    return out, buf, (H, b)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("dim", CG_DIMS)
def test_dense_cg_holds_the_accuracy_bar(dev, dim, steps):
    """12 cases per (dim, steps): the rows with entries of a solve case through als_normal_rows + als_solve_rows_dense_cg against the
    float64 cg_half_step.  The ratios kernel / bar are printed; DESIGN.md section 4t has the worst and the median."""
    ops = _m("ops")
    missed, ratios = [], []
    for n, (reg, alpha, with_conf, warm, seed) in enumerate(solve_cases(dim, steps)):
        Y, off, idx, conf, rows, X0 = solve_inputs(dim, seed, with_conf, warm)
        X64, X32 = references(Y, off, idx, conf, reg, alpha, X0, steps)
        assert np.isfinite(X32).all() and _row_errs(X32, X64)[1] < 1e-3
        ok_rms, ok_max = bar(X32[rows], X64[rows])
        wide = n % 2 == 1
        Yd, _ = _dev_rows(Y, dim + 5 if wide else dim, dev)
        out, buf, _hb = _dense_dev(ops, dev, Yd, ops.gram(Yd), off, idx, conf, alpha, rows, X0, reg, steps, ld_out=dim + 5 if wide else None)
        if wide:
            assert bool((buf[:, dim:] == -7.5).all())                        # the columns past dim keep the sentinel
        X = out.cpu().numpy()
        assert np.isfinite(X).all()
        rms, mx = _row_errs(X, X64[rows])
        rms32, max32 = _row_errs(X32[rows], X64[rows])
        ratios += [rms / rms32, mx / max32]
        print(f"dense cg dim {dim} steps {steps} reg {reg} alpha {alpha} conf {with_conf} warm {warm} wide {wide}: kernel rms {rms:.3e} max {mx:.3e}"
              f"  float32 CPU rms {rms32:.3e} max {max32:.3e}  bar rms {ok_rms:.3e} max {ok_max:.3e}")
        if not (rms <= ok_rms and mx <= ok_max):
            missed.append((reg, alpha, with_conf, warm, rms, ok_rms, mx, ok_max))
    print(f"dense cg dim {dim} steps {steps}: kernel / float32 CPU worst {max(ratios):.3f} median {float(np.median(ratios)):.3f}")
    assert not missed, missed


@pytest.mark.parametrize("dim", [4, 20, 33, 64])
def test_dense_cg_converges_to_the_exact_solve(dev, dim):
    ops = _m("ops")
    steps = min(2 * dim, 64)
    missed = []
    for reg, alpha in ((1.0, 1.0), (30.0, 1.0)):
        for with_conf in (False, True):
            Y, off, idx, conf = _solve_case(dim, 7000 * dim + int(reg) + with_conf, with_conf)
            rows = heavy_rows_of(off)
            X0 = np.zeros((len(off) - 1, dim), np.float32)
            X64 = half_step_f64(Y, off, idx, conf, reg, alpha)[rows]
            X32 = cg_half_step(Y, _g32(Y), off, idx, conf, reg, alpha, X0, steps, dt=np.float32)[rows]
            rms32, max32 = _row_errs(X32, X64)
            assert max32 < 1e-3
            Yd = _t(Y, dev)
            out, _buf, _hb = _dense_dev(ops, dev, Yd, ops.gram(Yd), off, idx, conf, alpha, rows, X0, reg, steps)
            rms, mx = _row_errs(out.cpu().numpy(), X64)
            print(f"dense cg convergence dim {dim} steps {steps} reg {reg} alpha {alpha} conf {with_conf}: kernel rms {rms:.3e} max {mx:.3e}"
                  f"  float32 CPU CG rms {rms32:.3e} max {max32:.3e}")
            if not (rms <= 4 * rms32 and mx <= 4 * max32):
                missed.append((reg, alpha, with_conf, rms, rms32, mx, max32))
    assert not missed, missed


def test_dense_cg_rows_are_independent_and_calls_repeat_bit_for_bit(dev):
    ops = _m("ops")
    dim = 129
    Y, off, idx, conf, rows, X0 = solve_inputs(dim, 3, True, True)
    Yd = _t(Y, dev)
    G = ops.gram(Yd)
    out, _b, (H, b) = _dense_dev(ops, dev, Yd, G, off, idx, conf, 10.0, rows, X0, 0.1, 3)
    x0 = _t(X0[rows], dev)
    assert torch.equal(_bits(out), _bits(ops.als_solve_rows_dense_cg(G, H, b, 0.1, x0, steps=3)))
    for h in (0, 3, len(rows) - 1):
        one = ops.als_solve_rows_dense_cg(G, H[h:h + 1].contiguous(), b[h:h + 1].contiguous(), 0.1, x0[h:h + 1].contiguous(), steps=3)
        assert torch.equal(_bits(one[0]), _bits(out[h])), h


# ------------------------------------------------------------------------------ the engine
MIXED = [0, 5, 64, 65, 130, 0, 33, 200, 64, 300, 1, 66]                      # empty, light (<= 64) and heavy rows


def _mixed_case(dev, dim, seed, with_conf, **kw):
    als = _m("als")
    Y, off, idx, conf = _solve_case(dim, seed, with_conf, counts=MIXED)
    eng = als.ALSEngine(len(MIXED), N_Y, dim, dev, reg=0.1, alpha=10.0, init_seed=seed, solver="cg", cg_steps=3, **kw)
    X0 = (np.random.default_rng(seed + 1).normal(size=(len(MIXED), dim)) * 0.1).astype(np.float32)
    eng.load_state_dict({"user": torch.from_numpy(X0), "item": torch.from_numpy(Y)})
    return eng, (_t(off, dev), _t(idx, dev), _t(conf, dev)), (Y, off, idx, conf, X0)


@pytest.mark.parametrize("dim,with_conf", [(20, True), (129, False)])
def test_engine_half_step_with_heavy_rows(dev, dim, with_conf):
    ops, als = _m("ops"), _m("als")
    eng, csr, (Y, off, idx, conf, X0) = _mixed_case(dev, dim, 50 + dim, with_conf, heavy_rows=64)
    hc = eng.prepare(csr)
    heavy = [u for u, c in enumerate(MIXED) if c > 64]
    assert isinstance(hc, als.HeavyCSR) and hc.rows.tolist() == heavy and hc.slice == ops.ALS_HEAVY_SLICE
    hc = als.split_heavy(csr, 64, dim=dim, slice=64)                          # (slice 64: rows of two to five slices)
    plain = ops.als_solve_rows_cg(eng.item, ops.gram(eng.item), csr[0], csr[1], eng.reg, eng.alpha, _t(X0, dev), steps=3, conf=csr[2])
    eng.half_step("user", hc)
    eng.check_ids()
    X = eng.user.clone()
    for u, c in enumerate(MIXED):
        if c == 0:
            assert not _bits(X[u]).any(), u                                  # empty rows: bit-zero
        elif c <= 64:
            assert torch.equal(_bits(X[u]), _bits(plain[u])), u              # light rows: the bits of the plain kernel on the full CSR
    X64, X32 = references(Y, off, idx, conf, eng.reg, eng.alpha, X0, 3)
    ok_rms, ok_max = bar(X32[heavy], X64[heavy])
    rms, mx = _row_errs(X[heavy].cpu().numpy(), X64[heavy])
    print(f"engine half-step dim {dim}: heavy rows rms {rms:.3e} max {mx:.3e}  bar rms {ok_rms:.3e} max {ok_max:.3e}")
    assert rms <= ok_rms and mx <= ok_max
    assert all(bool(X[u].any()) for u in heavy)                              # not the zeros the light pass left
    # a second run from the same tables
    eng.load_state_dict({"user": torch.from_numpy(X0), "item": torch.from_numpy(Y)})
    eng.half_step("user", hc)
    assert torch.equal(_bits(eng.user), _bits(X))
    # a threshold above every row: the plain tuple path, bit for bit
    for form in (als.split_heavy(csr, 300, dim=dim, slice=64), csr):
        eng.load_state_dict({"user": torch.from_numpy(X0), "item": torch.from_numpy(Y)})
        eng.half_step("user", form)
        assert torch.equal(_bits(eng.user), _bits(plain))
    with pytest.raises(ValueError):
        als.ALSEngine(len(MIXED), N_Y, 8, dev).half_step("user", hc)         # the Cholesky engine takes no HeavyCSR


def test_engine_batches_give_the_bits_of_one_batch(dev):
    als = _m("als")
    dim = 33
    eng, csr, (Y, _o, _i, _c, X0) = _mixed_case(dev, dim, 9, True, heavy_rows=64)
    one = als.split_heavy(csr, 64, dim=dim, slice=64)
    assert len(one.batches) == 1
    eng.half_step("user", one)
    want = eng.user.clone()
    small = als.ALSEngine(len(MIXED), N_Y, dim, dev, reg=0.1, alpha=10.0, solver="cg", cg_steps=3, heavy_rows=64,
                          heavy_ws_bytes=2 * als.heavy_row_bytes(2, dim))
    small.load_state_dict({"user": torch.from_numpy(X0), "item": torch.from_numpy(Y)})
    many = als.split_heavy(csr, 64, dim=dim, heavy_ws_bytes=small.heavy_ws_bytes, slice=64)
    assert len(many.batches) >= 3
    small.half_step("user", many)
    small.check_ids()
    assert torch.equal(_bits(small.user), _bits(want))


def test_heavy_engine_trajectory_follows_float64_cg(dev):
    U, I, dim, reg, alpha, steps = 200, 150, 16, 0.01, 40.0, 3
    als = _m("als")
    _e, ucsr, icsr, (off, idx), (toff, tidx), _p = _engine_case(dev, U, I, 3000, dim, 21, reg, alpha)
    eng = als.ALSEngine(U, I, dim, dev, reg=reg, alpha=alpha, init_seed=21, solver="cg", cg_steps=steps, heavy_rows=8)
    uh, ih = eng.prepare(ucsr), eng.prepare(icsr)
    assert 0 < uh.rows.numel() < U and 0 < ih.rows.numel() <= I
    X0, Y0 = eng.user.cpu().numpy(), eng.item.cpu().numpy()
    L = lambda X, Y: float(objective(X, Y, off, idx, None, reg, alpha))
    allow = _cholesky_allowance(X0, Y0, off, idx, toff, tidx, reg, alpha, L)
    X, Y, l64 = X0.astype(np.float64), Y0.astype(np.float64), []
    for _ in range(3):
        X = cg_half_step(Y, Y.T @ Y, off, idx, None, reg, alpha, X, steps); l64.append(L(X, Y))
        Y = cg_half_step(X, X.T @ X, toff, tidx, None, reg, alpha, Y, steps); l64.append(L(X, Y))
    got = []
    for _ in range(3):
        for side, csr in (("user", uh), ("item", ih)):
            eng.half_step(side, csr)
            got.append(L(eng.user.cpu().numpy(), eng.item.cpu().numpy()))
    eng.check_ids()
    got, l64 = np.array(got), np.array(l64)
    print(f"heavy cg trajectory: float64 CG {l64}\n  engine {got}\n  rel diff {np.abs(got - l64) / l64}\n  allowance {allow:.3e}")
    assert (np.diff(got) <= allow * got[:-1]).all()
    assert got[0] <= L(X0, Y0)
    assert abs(got[-1] - l64[-1]) <= allow * l64[-1]


def test_heavy_engine_at_350_features_lowers_the_objective(dev):
    als = _m("als")
    U, I, dim = 200, 150, 350
    rng = np.random.default_rng(31)
    u, i = rng.integers(0, U, 3000), rng.integers(0, I, 3000)
    ucsr, icsr = als.csr_pair(u, i, U, I, dev)
    eng = als.ALSEngine(U, I, dim, dev, reg=0.1, alpha=10.0, init_seed=31, solver="cg", heavy_rows=8)
    before = eng.objective(ucsr)
    eng.epoch(eng.prepare(ucsr), eng.prepare(icsr))
    eng.check_ids()
    after = eng.objective(ucsr)
    print(f"heavy rows, dim 350: objective {before:.6e} -> {after:.6e}")
    assert np.isfinite(after) and after < before


def test_als_model_trains_with_heavy_rows(dev, tmp_path):
    models = _m("models")
    m = models.ALSModel(device=dev)
    m.epochs, m.numFactor = 2, 8
    res = m.train(_csv(tmp_path), 300, reg=0.05, alpha=10.0, seed=3, solver="cg", cgSteps=3, heavyRows=4)
    hist = res["history"].history["objective"]
    assert res["result"] == "completed" and len(hist) == 2 and res["metrics"] == [hist[-1]]
    assert m.model.solver == "cg" and m.model.heavy_rows == 4
    assert hist[1] <= hist[0] * (1 + 1e-6)
    with pytest.raises(ValueError):
        models.ALSModel(device=dev).train(_csv(tmp_path), 300, solver="cholesky", heavyRows=4)
