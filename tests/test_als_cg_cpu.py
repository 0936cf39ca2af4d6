"""-m "not gpu": the conjugate-gradient ALS half-step and the wide Gram (csrc/als_wide.hip) without a device - the C-ABI's argument
checks, and the numpy restatement of the CG loop that tests/test_gpu_als_cg.py compares the kernel with (checked here on its own:
float64 CG with 2 dim steps reaches the exact solve, and the quadratic of a row never rises from one step count to the next)."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

from tests.test_als_cpu import P, _case, half_step_f64, normal_equations


# ------------------------------------------------------------------------------ the restatement (numpy; the product never imports it)
def cg_half_step(Y, G, off, idx, conf, reg, alpha, X0, steps, dt=np.float64):
    """`steps` conjugate-gradient steps per row from X0, every operation in dtype dt.  The operator is applied, never formed:
    A p = G p + reg p + sum_e c_e y_e (y_e . p); b = sum_e (1 + c_e) y_e.  A row without entries is zeros."""
    Y, G, reg_, alpha_ = np.asarray(Y, dt), np.asarray(G, dt), dt(reg), dt(alpha)
    X = np.zeros((len(off) - 1, Y.shape[1]), dt)
    for u in range(len(off) - 1):
        e = np.arange(off[u], off[u + 1])
        if e.size == 0:
            continue
        Yu = Y[idx[e]]
        c = alpha_ * (conf[e].astype(dt) if conf is not None else np.ones(e.size, dt))
        A = lambda p: G @ p + reg_ * p + Yu.T @ (c * (Yu @ p))
        b = Yu.T @ (1 + c)
        x = np.asarray(X0[u], dt).copy()
        r = b - A(x)
        p = r.copy()
        rs = r @ r
        for _ in range(steps):
            if not rs >= 1e-20:
                break
            q = A(p)
            d = p @ q
            if not (d > 0 and np.isfinite(d)):
                break
            a = rs / d
            x = x + a * p
            r = r - a * q
            rn = r @ r
            p = r + (rn / rs) * p
            rs = rn
        X[u] = x
    return X


# ------------------------------------------------------------------------------ C-ABI
@pytest.fixture(scope="module")
def lib():
    import_module("binary-recommendation_amd.build").build_library(verbose=False)
    return import_module("binary-recommendation_amd._lib")


def test_header_declares_and_library_exports_the_wide_entries(lib):
    protos = lib.parse_header()
    cdll = ctypes.CDLL(import_module("binary-recommendation_amd.build").LIB_PATH)
    for name, n_args in (("brGramWideWorkspaceBytes", 2), ("brGramWide", 8), ("brAlsSolveRowsCg", 16)):
        assert name in protos and len(protos[name][1]) == n_args, name
        assert hasattr(cdll, name), name
    assert protos["brGramWideWorkspaceBytes"][0] is ctypes.c_int64
    assert protos["brAlsSolveRowsCg"][2][11:14] == ["X", "ld_x", "steps"]


def test_wide_gram_workspace_query(lib):
    h = lib.load()
    assert h.brGramWideWorkspaceBytes(1000, 350) > 0
    assert h.brGramWideWorkspaceBytes(1000, 0) == -1 and h.brGramWideWorkspaceBytes(1000, 513) == -1
    assert h.brGramWideWorkspaceBytes(0, 350) == 0 and h.brGramWideWorkspaceBytes(-1, 350) == -1
    # the 128-column entry keeps its limit
    assert h.brGramWorkspaceBytes(1000, 129) == -1


def test_argument_errors_come_before_any_launch(lib):
    h = lib.load()
    E = lib.parse_enums()
    nan = float("nan")

    def gram(Y=P, ld=350, rows=1000, dim=350, G=P, ws=P, ws_bytes=None):
        need = h.brGramWideWorkspaceBytes(rows, dim if 1 <= dim <= 512 else 350)
        return h.brGramWide(Y, ld, rows, dim, G, ws, need if ws_bytes is None else ws_bytes, None)

    def solve(Y=P, ld_y=350, n_y=100, dim=350, G=P, off=P, idx=P, conf=None, alpha=40.0, reg=0.01, n_rows=10, X=P, ld_x=350, steps=3):
        return h.brAlsSolveRowsCg(Y, ld_y, n_y, dim, G, off, idx, conf, alpha, reg, n_rows, X, ld_x, steps, None, None)

    bad_gram = {"null Y": dict(Y=None), "null G": dict(G=None), "dim 0": dict(dim=0), "dim 513": dict(dim=513, ld=513), "ld < dim": dict(ld=349),
                "rows < 0": dict(rows=-1)}
    for what, kw in bad_gram.items():
        assert gram(**kw) == E["BR_ERR_ARG"], what
        assert h.brGetLastError().startswith(b"brGramWide"), what
    need = h.brGramWideWorkspaceBytes(1000, 350)
    for kw in (dict(ws_bytes=need - 1), dict(ws=None)):
        assert gram(**kw) == E["BR_ERR_WORKSPACE"] and h.brGetLastError().startswith(b"brGramWide")
    bad_solve = {"null Y": dict(Y=None), "null G": dict(G=None), "null off": dict(off=None), "null X": dict(X=None), "dim 0": dict(dim=0),
                 "dim 513": dict(dim=513, ld_y=513, ld_x=513), "ld_y < dim": dict(ld_y=349), "ld_x < dim": dict(ld_x=349), "reg 0": dict(reg=0.0),
                 "reg < 0": dict(reg=-1.0), "reg nan": dict(reg=nan), "reg inf": dict(reg=float("inf")), "alpha < 0": dict(alpha=-1.0),
                 "alpha nan": dict(alpha=nan), "n_y = 2^31": dict(n_y=1 << 31), "steps 0": dict(steps=0), "steps 65": dict(steps=65),
                 "steps < 0": dict(steps=-3), "n_rows < 0": dict(n_rows=-1)}
    for what, kw in bad_solve.items():
        assert solve(**kw) == E["BR_ERR_ARG"], what
        assert h.brGetLastError().startswith(b"brAlsSolveRowsCg"), what
    assert solve(n_rows=0) == E["BR_OK"]                                   # a no-op


# ------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("with_conf", [False, True])
@pytest.mark.parametrize("reg,alpha", [(0.01, 40.0), (1.0, 1.0), (0.1, 0.0)])
@pytest.mark.parametrize("dim", [4, 20])
def test_float64_cg_reaches_the_exact_solve(dim, reg, alpha, with_conf):
    ((off, idx, conf), _t), X0, Y = _case(40, 30, 300, dim, 3, with_conf)
    want = half_step_f64(Y, off, idx, conf, reg, alpha)
    G = Y.T @ Y
    for start in (np.zeros_like(X0), X0):                                    # cold and warm
        got = cg_half_step(Y, G, off, idx, conf, reg, alpha, start, 2 * dim)
        nz = np.abs(want).sum(1) > 0
        assert not got[~nz].any()
        err = np.linalg.norm(got[nz] - want[nz], axis=1) / np.linalg.norm(want[nz], axis=1)
        assert err.max() <= 1e-9, err.max()


def test_float64_quadratic_of_a_row_never_rises_with_the_step_count():
    ((off, idx, conf), _t), X0, Y = _case(40, 30, 300, 8, 4, True)
    reg, alpha = 0.01, 40.0
    G = Y.T @ Y
    last = None
    for steps in range(0, 12):
        X = cg_half_step(Y, G, off, idx, conf, reg, alpha, X0, steps) if steps else np.where(np.diff(off)[:, None] > 0, X0, 0.0)
        phi = np.zeros(len(off) - 1)
        for u in range(len(off) - 1):
            ne = normal_equations(Y, G, off, idx, conf, reg, alpha, u)
            if ne is not None:
                phi[u] = 0.5 * X[u] @ ne[0] @ X[u] - ne[1] @ X[u]
        if last is not None:
            assert (phi <= last + 1e-12 * np.abs(last)).all(), steps
        last = phi
