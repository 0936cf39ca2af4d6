"""-m gpu: csrc/sparse_opt.hip against float64 - the ordered duplicate sum (brSegmentSumRows), the Adam row update in both kernel forms
(brAdamRowsSorted, brAdamRowsSortedPair with hi_scale, brAdamRowsSortedPairReplayed with tables of different lengths), Adagrad rows, the
dense sweep past its grid cap, the flat updates, and the strip widths 2 and 8 of the one-wave-per-row kernel.

Index.  sorted_ids / sorted_pos / n of an ops.RowIndex are filled from numpy (stable order, invalid ids behind the valid ones), so a failure
points at this unit; test_through_the_built_index runs the same data through RowIndex.build and asks for the same bits.

Layouts (test_the_layouts_reach_every_walk, no GPU).  An id stream is built from a list of run lengths: run k of the sorted order has the
k-th smallest id, positions are shuffled (ascending inside a run: the stable order).  A and B have the same n (one pair launch takes both)
and hold, each: for strips of 2 / 4 / 8 sorted positions and every start offset a run that ends inside its strip (no such run starts at
the strip's last position), at its end, 1 and 3 positions into the next strip; own parts of 7, 8, 9, 15, 16, 17 positions behind the head
(both sides of seg_walk's batches of 8); runs that start at 0, 1, 60, 63 of a 64-block, end on a boundary, one past it (a partial of one
row), and span 1, 2, 3, 4, 5, 8, 9 later blocks (the four-at-a-time loop of seg_acc_from once and twice, with and without a remainder;
blocks continued for all 64 positions and for fewer).  A ends in invalid ids - one repeated id above table_rows (7 positions over a
64-boundary), 5 distinct ones, 3 x -1.  B has none: its largest id runs to n, n % 64 = 10, n % 4 = 2.  Small: n = 1, 2, 63, 64, 65 and 300
positions of one id.

Gradients.  Per run a scale 10^U(-12, 3); a third of the runs cancel (|sum| = 1e-3 sum |g|), some even runs are (a, -a) pairs (sum exactly
0), some are all zero.  G = the oracle's ordered fp32 sum (O.ordered_segment_sum; O.dedup_rows_sequential without partials) of the rows as
the kernel reads them; a hi_scale source is the fp32 numpy product rows * scale (the one rounded product of grow()).  index.seg_ws(dim) is
NaN before every launch: a head that reads a partial nobody wrote shows.

Bounds, u = 2^-24 (all derived from the operations in adam_math.h / sparse_opt.hip, none from a kernel's output):
  ordered sum      heads: every bit of the oracle's sum; head_flag = the head mask; non-head rows of `out` still NaN; and
                   |got - S| <= len u sum |g| against the float64 sum S (len - 1 fp32 additions, each within u of a partial sum <= sum |g|)
  Adam m           m = fma(omb1, G, fl(b1 m0)): two roundings, each within u of a term <= |b1 m0| + |omb1 G|
                   |m - (b1f m0 + omb1f G)| <= 2 u (|b1f m0| + |omb1f G|);   m0 = v0 = 0: m = fl(omb1f G) (+0 for G = -0), v = fl(omb2f fl(G G)) in every bit
  Adam v           v = fma(omb2, fl(G G), fl(b2 v0)): fl(G G) and fl(b2 v0) within u of their (non-negative) terms, the fma's rounding within
                   u of v:  |v - (b2f v0 + omb2f G^2)| <= 2 u v_ref + 2^-149 (the last term: a subnormal result has an absolute rounding)
  Adam theta       on the kernel's own m, v:  |theta - (theta0 - upd)| <= 7 u |upd| + u |theta_ref|, upd = alpha m / (sqrt(v) + eps):
                   alpha m, the hardware sqrt, the add and the hardware rcp at one unit each as adam_math.h documents them, one to spare for
                   second order; u |theta_ref|: the rounding of the fma's result
  Adagrad          acc0 = 0: acc = fl(G G) in every bit (with or without contraction); else |acc - (acc0 + G^2)| <= 2 u ref;
                   |theta - (theta0 - upd)| <= 6 u |upd| + u |theta_ref|, upd = lr G / (sqrt(acc) + eps) on the kernel's own acc (product, sqrt,
                   add, divide at up to 1 ulp each)
  rows nobody touched and rows of invalid ids keep every bit (lazy); with `mark`: exactly the valid touched rows are marked, and
  brAdamDenseSweep brings every other row to the float64 g = 0 step within the Adam bounds and clears the marks.
Pair launches: bit-equal to two single launches (hi source premultiplied in fp32; deferred: brAdamRowsSortedDeferredReplayed), and the
Adam bounds.  Strips of 2 and 8: one child process per value (BR_ADAM_STRIP is read once per process), bit-equal to this process.

Observed maxima in units of each bound go to sorted_rows_errors.json in the directory BR_TEST_RECORD_DIR names, when it is set and exists
(profiles/sorted_rows/ holds the file of one run)."""
import functools
import hashlib
import json
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import binrec_oracle as O
from tests.test_gpu_row_kernels import WIDTHS, _geom, _nan, _passes, _same_bits, _td, _vec_width, _written_exactly

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U24, SUB = 2.0 ** -24, 2.0 ** -149
I32, I64 = torch.int32, torch.int64
SUM_WIDTHS = WIDTHS + (48, 128)
WIDE = max(SUM_WIDTHS)
B1, B2, EPS, LR = 0.9, 0.999, 1e-7, 0.005
ALPHA = LR * (1.0 - B2 ** 3) ** 0.5 / (1.0 - B1 ** 3)                    # alpha_3 of Keras Adam
B1F, OMB1F, B2F, OMB2F, EPSF, AF = (f64(f32(x)) for x in (B1, 1.0 - B1, B2, 1.0 - B2, EPS, ALPHA))      # as make_hp rounds them
LR_G, LR_GF = 0.1, f64(f32(0.1))                                           # Adagrad


def _ops():
    return import_module("binary-recommendation_amd.ops")


# ------------------------------------------------------------------------------------------------------------ layouts
class _Layout:
    """runs: lengths of the valid runs in sorted order; tail: (repeats of one id above the table, distinct invalid ids, repeats of -1)"""

    def __init__(self, name, runs, tail=(0, 0, 0), seed=0):
        rng = np.random.default_rng(seed)
        runs = np.asarray(runs, np.int64)
        self.name, self.nvr, self.nv = name, len(runs), int(runs.sum())
        self.rows = len(runs) + len(runs) // 3 + 7
        self.run_row = np.sort(rng.choice(self.rows, len(runs), replace=False)).astype(np.int64)
        bad = [self.rows + 3] * tail[0] + [self.rows + 10 + k for k in range(tail[1])] + [-1] * tail[2]
        self.sid = np.concatenate([np.repeat(self.run_row, runs), np.asarray(bad, np.int64)])
        self.n = n = len(self.sid)
        self.start = np.flatnonzero(np.r_[True, self.sid[1:] != self.sid[:-1]])
        self.length = np.diff(np.r_[self.start, n])
        key = np.repeat(np.arange(len(self.start)), self.length)
        perm = rng.permutation(n)
        self.spos = perm[np.lexsort((perm, key))].astype(np.int32)          # shuffled positions, ascending inside every run
        self.ids = np.empty(n, np.int64); self.ids[self.spos] = self.sid      # the stream by position
        self.key = np.empty(n, np.int64); self.key[self.spos] = key           # run number by position: the oracle's sort key
        valid = (self.ids >= 0) & (self.ids < self.rows)
        order = np.argsort(np.where(valid, self.ids, self.rows), kind="stable")
        assert np.array_equal(order[:self.nv], self.spos[:self.nv]) and np.array_equal(np.argsort(self.key, kind="stable"), self.spos)
        self.touched = np.zeros(self.rows, bool); self.touched[self.run_row] = True
        self._idx = {}

    def index(self, dev, idt):
        if idt not in self._idx:
            ix = _ops().RowIndex(self.n, idt, dev)
            ix.sorted_ids.copy_(torch.from_numpy(self.sid).to(idt)); ix.sorted_pos.copy_(torch.from_numpy(self.spos)); ix.n = self.n
            self._idx[idt] = ix
        return self._idx[idt]


def _core_specs():
    """(modulus, start offset, run length) of every designed run"""
    sp = [(S, o, S - o + x) for S in (2, 4, 8) for o in range(S) for x in (-1, 0, 1, 3) if S - o + x >= 1]
    sp += [(32, o, w + 1) for w in (7, 8, 9, 15, 16, 17) for o in (0, 5)]
    sp += [(64, 60, 4 + 64), (64, 63, 2), (64, 0, 64 * 2 + 5), (64, 1, 63 + 64 * 3 - 10), (64, 60, 4 + 64 * 3 + 1), (64, 63, 1 + 64 * 4 + 20),
           (64, 0, 64 + 64 * 8), (64, 1, 63 + 64 * 8 + 33), (64, 0, 64), (64, 1, 64), (64, 60, 3), (64, 63, 1)]
    return sp


def _compose(specs, rng, fill_max):
    runs, pos = [], 0
    for mod, off, ln in specs:
        while pos % mod != off:
            f = min(int(rng.integers(1, fill_max + 1)), (off - pos) % mod)
            runs.append(f); pos += f
        runs.append(ln); pos += ln
    return runs, pos


@functools.lru_cache(None)
def _layouts():
    rng = np.random.default_rng(2024)
    sp = _core_specs()
    ra, na = _compose(sp, rng, 2)
    rb, nb = _compose([sp[k] for k in rng.permutation(len(sp))], rng, 3)
    T = -(-(max(na, nb) + 70) // 64) * 64
    ra += [1] * (T + 59 - na)                                   # A: the invalid tail starts at 59 of a 64-block
    rb += [1] * (T - 4 - nb) + [4 + 64 + 10]                    # B: the largest id starts at 60, fills a block and is cut by n
    A, B = _Layout("A", ra, (7, 5, 3), 11), _Layout("B", rb, (0, 0, 0), 12)
    assert A.n == B.n == T + 74
    return {"A": A, "B": B}


@functools.lru_cache(None)
def _small_layouts():
    return tuple(_Layout(f"one id x {n}", [n], (0, 0, 0), 30 + n) for n in (1, 2, 63, 64, 65, 300))


def _reach(L):
    seen = set()
    for s, ln in zip(L.start.tolist(), L.length.tolist()):
        e = s + ln
        for S in (2, 4, 8):
            E = s - s % S + S
            seen.add(("strip", S, s % S, "inside" if e < E else "at the end" if e == E else "one over" if e == E + 1 else "several over"))
        seen.add(("own part behind the head", min(e, (s // 64 + 1) * 64) - s - 1))
        seen.add(("start", s % 64))
        later = (e - 1) // 64 - s // 64                          # block starts inside (s, e)
        if e % 64 == 0:
            seen.add(("ends on a boundary", "crossed" if later else "own part"))
        if later:
            last = e - (e - 1) // 64 * 64
            seen.add(("later blocks", later))
            if last == 1:
                seen.add("a partial of one row")
            if later > 1 or last == 64:
                seen.add(("continued for", 64))
            if last < 64:
                seen.add(("continued for", "fewer"))
    return seen


def test_the_layouts_reach_every_walk():
    want = {("strip", S, o, c) for S in (2, 4, 8) for o in range(S) for c in ("inside", "at the end", "one over", "several over")
            if not (c == "inside" and o == S - 1)}            # (a run at the strip's last position ends at the strip's end at the earliest)
    want |= {("own part behind the head", w) for w in (7, 8, 9, 15, 16, 17)} | {("start", s) for s in (0, 1, 60, 63)}
    want |= {("later blocks", k) for k in (1, 2, 3, 4, 5, 8, 9)} | {("ends on a boundary", "crossed"), ("ends on a boundary", "own part")}
    want |= {"a partial of one row", ("continued for", 64), ("continued for", "fewer")}
    for L in _layouts().values():
        assert not want - _reach(L), (L.name, sorted(map(str, want - _reach(L))))
        assert 2000 < L.n < 6000 and L.touched.sum() < L.rows - 100
    A, B = _layouts()["A"], _layouts()["B"]
    # A: the tail of invalid ids crosses a 64-boundary and strip boundaries; its repeated id is one run over the 64-boundary
    assert A.n - A.nv == 15 and A.nv % 64 == 59 and A.nv // 64 < (A.n - 1) // 64 and A.nv // 8 < (A.n - 1) // 8
    t = A.sid[A.nv:]
    assert (t[:7] == A.rows + 3).all() and len(set(t[7:12].tolist())) == 5 and (t[7:12] > A.rows).all() and (t[12:] == -1).all()
    assert (A.sid[:A.nv] < A.rows).all() and (A.sid[:A.nv] >= 0).all() and (np.diff(A.sid[:A.nv]) >= 0).all()
    # B: no invalid id; the largest id reaches n through a whole block, the last partial block and the last strip are cut by n
    assert B.nv == B.n and B.n % 4 and B.n % 64 and B.sid[-1] == B.sid.max() and B.start[-1] + 64 < B.n // 64 * 64 + 1 and B.start[-1] % 64 == 60
    assert [L.n for L in _small_layouts()] == [1, 2, 63, 64, 65, 300] and all(len(L.start) == 1 for L in _small_layouts())
    # the forms of the Adam launch the widths reach (rows.h wave_row_vec / vec_width / row_geom_ld)
    assert {d for d in SUM_WIDTHS if d in (64, 128, 256)} == {64, 128, 256}
    assert _geom(128, _vec_width([128, 65, 63])) == (1, 128, 6) and _passes(128, 1) == 2 and _geom(256, _vec_width([130, 126, 130]))[0] == 2
    for d in SUM_WIDTHS:
        s4, s2, odd = _splits(d)
        assert (s4 is None or (s4 % 4 == 0 and 0 < s4 < d)) and (s2 is None or (s2 % 4 == 2 and 0 < s2 < d)) and (odd is None or (odd % 2 and 0 < odd < d))
    assert all(None not in _splits(d) for d in SUM_WIDTHS if d > 4)


# ------------------------------------------------------------------------------------------------------------ gradients and sums
class _Data:
    """gradient rows by position for one layout (WIDE columns; a test takes the first `dim`) and their sums per run of the sorted order"""

    def __init__(self, L, seed, width=WIDE, designed=True):
        rng = np.random.default_rng(seed)
        self.L, nr = L, len(L.start)
        r = np.arange(nr)
        even = (L.length % 2 == 0) & (L.length <= 8)
        self.zero = (r % 11 == 5) & designed
        self.pairs = even & (np.cumsum(even) % 3 == 1) & ~self.zero
        multi = (L.length >= 2) & ~self.zero & ~self.pairs
        self.cancel = multi & (np.cumsum(multi) % 3 == 1)             # a third of the runs that have something to add
        self.scale = 10.0 ** rng.uniform(-12, 3, nr)
        self.scale[:4] = (1e-12, 1e3, 1.0, 1e-6)[:min(nr, 4)] if designed else 1.0
        gs = rng.uniform(0.25, 1.0, (L.n, width)) * rng.choice([-1.0, 1.0], (L.n, width))
        for k in np.flatnonzero(self.cancel):
            s, e = L.start[k], L.start[k] + L.length[k]
            gs[e - 1] = -gs[s:e - 1].sum(0) + 1e-3 * np.abs(gs[s:e - 1]).sum(0)
        gs = (gs * np.repeat(self.scale, L.length)[:, None]).astype(f32)
        for k in np.flatnonzero(self.pairs):
            s, e = L.start[k], L.start[k] + L.length[k]
            gs[s + 1:e:2] = -gs[s:e:2]
        gs[np.repeat(self.zero, L.length)] = 0.0
        self.g = np.empty_like(gs); self.g[L.spos] = gs
        g64 = gs.astype(f64)
        self.S64, self.A64 = np.add.reduceat(g64, L.start, axis=0), np.add.reduceat(np.abs(g64), L.start, axis=0)
        self.G_two, self.G_seq = self.sums(self.g)
        if not designed:
            return
        c = self.cancel
        assert c.sum() >= multi.sum() // 3 and c.sum() >= 15 and (np.abs(self.S64[c]) <= 2e-3 * self.A64[c]).all()          # (the test's own inputs)
        assert self.pairs.sum() >= 3 and (self.G_two[self.pairs] == 0).all() and (self.A64[self.pairs] > 0).all()
        a = np.abs(self.G_two[:L.nvr])
        assert a[a > 0].min() < 1e-11 and a.max() > 1e2

    def sums(self, g):
        uniq, two = O.ordered_segment_sum(self.L.key, g, dt=f32)
        _, seq = O.dedup_rows_sequential(self.L.key, g, dt=f32)
        assert np.array_equal(uniq, np.arange(len(self.L.start)))
        return two, seq


@functools.lru_cache(None)
def _data(name):
    if name in _layouts():
        return _Data(_layouts()[name], 100 + ord(name))
    return {L.name: _Data(L, 200 + L.n, 256, designed=False) for L in _small_layouts()}[name]


@functools.lru_cache(None)
def _hi(name):
    """a second source for the pair launch: raw rows H (128 columns), a per-position factor, their fp32 product and its ordered sum"""
    D = _data(name)
    rng = np.random.default_rng(300 + ord(name))
    hs = (rng.uniform(0.25, 1.0, (D.L.n, 128)) * rng.choice([-1.0, 1.0], (D.L.n, 128)) * np.repeat(D.scale, D.L.length)[:, None]).astype(f32)
    hs[np.repeat(D.zero, D.L.length)] = 0.0
    H = np.empty_like(hs); H[D.L.spos] = hs
    rs = np.random.default_rng(299)                          # ONE factor per position for both tables of a launch, as a NeuMF step has it (ddot)
    sc = (rs.uniform(0.5, 2.0, D.L.n) * rs.choice([-1.0, 1.0], D.L.n)).astype(f32)
    E = H * sc[:, None]                                         # fp32 product: one rounding
    assert E.dtype == f32
    return H, sc, E, D.sums(E)[0]


_REC = {}


def _record(group, key, value):
    _REC.setdefault(group, {})[key] = value
    out = os.environ.get("BR_TEST_RECORD_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "sorted_rows_errors.json"), "w") as fh:
            json.dump({"note": "max |got - float64| / bound per entry, width and form (<= 1 passes; bounds in tests/test_gpu_sorted_rows.py)", **_REC},
                      fh, indent=1, sort_keys=True)


def _ratio(what, got, ref, bound, ctx=""):
    """max |got - ref| / bound; a zero bound asks for equality.  Fails with the element when the bound is exceeded."""
    err = np.abs(got.astype(f64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound == 0, np.where(err == 0, 0.0, np.inf), err / bound)
    if r.size == 0:
        return 0.0
    r = np.where(np.isnan(r), np.inf, r)
    k = np.unravel_index(int(r.argmax()), r.shape)
    assert r[k] <= 1.0, f"{what}: |got - float64| = {err[k]:.6g} is {r[k]:.3f} of the bound {np.asarray(bound)[k]:.6g} at {k}: got {got[k]!r}, ref {ref[k]!r} {ctx}"
    return float(r[k])


def _source(dev, g, ld, off=0):
    """the (n, dim) rows in a NaN-filled buffer with row stride ld, starting `off` floats into an aligned allocation"""
    n, dim = g.shape
    flat = np.full(off + n * ld + 8, np.nan, f32)
    flat[off:off + n * ld].reshape(n, ld)[:, :dim] = g
    t = _td(dev, flat)
    assert t.data_ptr() % 16 == 0
    return t[off:]


# ------------------------------------------------------------------------------------------------------------ 2. the ordered sum
def _sum_case(dev, D, idt, dim, two_level, ld=None, off=0, index=None):
    ops, L = _ops(), D.L
    ld = dim if ld is None else ld
    src = _source(dev, D.g[:, :dim], ld, off)
    idx = L.index(dev, idt) if index is None else index
    idx.seg_ws(dim).fill_(float("nan"))
    out, head = _nan(dev, L.n, dim), torch.full((L.n,), -7, dtype=torch.int32, device=dev)
    ops.segment_sum_rows(idx, src, dim=dim, ldg=ld, out=out, head_flag=head, two_level=two_level)
    o, h = out.cpu().numpy(), head.cpu().numpy()
    what = f"segment sum {L.name} dim {dim} ld {ld} off {off} {'two-level' if two_level else 'one by one'} {idt}"
    mask = np.zeros(L.n, np.int32); mask[L.start] = 1
    assert np.array_equal(h, mask), what + ": head_flag"
    G = (D.G_two if two_level else D.G_seq)[:, :dim]
    assert _written_exactly(o, [(L.start, 0, G)]), what + ": heads differ from the ordered sum, or a non-head row was written"
    return _ratio(what, o[L.start], D.S64[:, :dim], L.length[:, None] * U24 * D.A64[:, :dim])


@pytest.mark.parametrize("dim", SUM_WIDTHS)
def test_segment_sum_every_geometry(dev, dim):
    worst = {}
    for name in ("A", "B"):
        D = _data(name)
        for idt in (I32, I64):
            for two in (True, False):
                r = _sum_case(dev, D, idt, dim, two)
                worst["aligned"] = max(worst.get("aligned", 0.0), r)
        idt = I32 if name == "A" else I64
        for ld, off in ((dim + 4, 0), (dim + 2, 0), (dim + 1, 0), (dim, 1), (dim, 2), (dim + 4, 1), (dim + 2, 2)):
            key = f"ld+{ld - dim} off {off}"
            worst[key] = max(worst.get(key, 0.0), _sum_case(dev, D, idt, dim, True, ld, off), _sum_case(dev, D, idt, dim, False, ld, off))
    for k, v in worst.items():
        _record("brSegmentSumRows", f"{dim} {k}", v)
    if dim in (64, 48, 10, 256):
        for L in _small_layouts():
            for two in (True, False):
                _sum_case(dev, _data(L.name), I32 if two else I64, dim, two)


# ------------------------------------------------------------------------------------------------------------ 3. Adam rows
class _AdamState:
    """theta0, m0, v0 of a table for one layout and the float64 step they expect, given the ordered sums G (valid runs, dim) of its rows"""

    def __init__(self, D, G, seed):
        L, rng = D.L, np.random.default_rng(seed)
        nvr, dim, rows = L.nvr, G.shape[1], L.rows
        G = np.ascontiguousarray(G[:nvr])
        self.L, self.G, self.dim = L, G, dim
        self.th0 = rng.uniform(-0.05, 0.05, (rows, dim)).astype(f32)
        m0 = 10.0 ** rng.uniform(-9, -2, (rows, dim)) * rng.choice([-1.0, 1.0], (rows, dim))
        v0 = 10.0 ** rng.uniform(-16, -4, (rows, dim))
        r, sc = np.arange(nvr), D.scale[:nvr, None]
        mt = rng.uniform(0.1, 10.0, (nvr, dim)) * rng.choice([-1.0, 1.0], (nvr, dim)) * OMB1F * sc
        vt = OMB2F * sc * sc * rng.uniform(0.05, 1.0, (nvr, dim))
        zero, pairs = D.zero[:nvr] & (G == 0).all(1), D.pairs[:nvr]
        assert zero.sum() >= 3 and zero.sum() == D.zero[:nvr].sum()
        self.cancel = (r % 3 == 1) & ~pairs & ~zero
        mt[self.cancel] = -(OMB1F * G[self.cancel].astype(f64)) * (1 - 1e-3) / B1F          # b1f m0 ~ -omb1f G: m = 1e-3 of the terms
        self.first = (r % 4 == 0) | zero                                              # first touch: m0 = v0 = 0
        mt[self.first] = 0.0; vt[self.first] = 0.0
        m0[L.run_row], v0[L.run_row] = mt, vt
        self.m0, self.v0 = m0.astype(f32), v0.astype(f32)
        self.sub = (int(L.run_row[np.flatnonzero(pairs & ~self.first)[0]]), 0)       # one subnormal v (G = 0 there: it stays subnormal)
        self.v0[self.sub] = f32(1e-40)
        assert 0 < self.v0[self.sub] < 2.0 ** -126 and self.first.sum() >= nvr // 4 and self.cancel.sum() >= nvr // 5
        self.zero_rows = L.run_row[zero]
        Gf = np.zeros((rows, dim), f64); Gf[L.run_row] = G
        m64, v64 = self.m0.astype(f64), self.v0.astype(f64)
        self.Gf = Gf
        self.m_ref, self.bm = B1F * m64 + OMB1F * Gf, 2 * U24 * (np.abs(B1F * m64) + np.abs(OMB1F * Gf))
        self.v_ref = B2F * v64 + OMB2F * Gf * Gf
        self.bv = 2 * U24 * self.v_ref + SUB

    def check(self, what, th, m, v, rows, th_in=None):
        """the Adam bounds on `rows` (a mask) of the outputs against the step from (th_in or theta0, m0, v0) with the gradient G (0 on
        rows without one); -> the maxima in units of the bounds"""
        th_in = self.th0 if th_in is None else th_in
        finite = all(bool(np.isfinite(a[rows]).all()) for a in (th, m, v))
        assert finite, what + ": theta, m or v is not finite"
        rm = _ratio(what + " m", m[rows], self.m_ref[rows], self.bm[rows])
        rv = _ratio(what + " v", v[rows], self.v_ref[rows], self.bv[rows])
        upd = AF * m[rows].astype(f64) / (np.sqrt(v[rows].astype(f64)) + EPSF)
        ref = th_in[rows].astype(f64) - upd
        rt = _ratio(what + " theta", th[rows], ref, 7 * U24 * np.abs(upd) + U24 * np.abs(ref))
        return rm, rv, rt

    def check_rows_step(self, what, th, m, v, mark=None):
        """after the rows launch: bounds on the touched rows, the bit-exact probes, and everything else untouched"""
        L, t = self.L, self.L.touched
        worst = self.check(what, th, m, v, t)
        fr = L.run_row[self.first]
        G = self.G[self.first]
        assert _same_bits(m[fr], f32(OMB1F) * G + f32(0.0)), what + ": first-touch rows: m is not the single product omb1f * G (the ordered sum inside the optimizer)"
        assert _same_bits(v[fr], f32(OMB2F) * (G * G)), what + ": first-touch rows: v is not omb2f * (G * G)"
        assert _same_bits(th[self.zero_rows], self.th0[self.zero_rows]), what + ": theta moved on rows with m0 = v0 = G = 0"
        for got, was, name in ((th, self.th0, "theta"), (m, self.m0, "m"), (v, self.v0, "v")):
            assert _same_bits(got[~t], was[~t]), f"{what}: {name} of a row nobody touched (or of an invalid id) changed"
        if mark is not None:
            assert np.array_equal(mark.astype(bool), t), what + ": marks are not exactly the valid touched rows"
        return worst


def _splits(dim):
    """split points of a two-source launch: a multiple of 4, 2 mod 4, odd (None where the width has none)"""
    s4 = 4 * max(1, dim // 8) if dim > 4 else None
    s2 = s4 + 2 if s4 and s4 + 2 < dim else 2 if dim > 2 else None
    odd = s4 - 1 if s4 else 1 if dim >= 2 else None
    return s4, s2, odd


def _forms(dim):
    s4, s2, odd = _splits(dim)
    return [("one source", None), ("odd stride", None)] + [(n, s) for n, s in (("split % 4 == 0", s4), ("split % 4 == 2", s2), ("odd split", odd)) if s]


def _rows_launch(dev, L, idt, g, st, form, split, with_mark, index=None):
    ops, dim = _ops(), st.dim
    th, m, v = _td(dev, st.th0), _td(dev, st.m0), _td(dev, st.v0)
    mark = torch.zeros(L.rows, dtype=torch.uint8, device=dev) if with_mark else None
    idx = L.index(dev, idt) if index is None else index
    idx.seg_ws(dim).fill_(float("nan"))
    if split:
        lo, hi = _source(dev, g[:, :split], split), _source(dev, g[:, split:dim], dim - split)
        ops.adam_rows_sorted(th, m, v, idx, lo, split, ALPHA, B1, B2, EPS, mark=mark, row_grads_hi=hi, ldg_hi=dim - split, split=split)
    else:
        ld = dim + 1 if form == "odd stride" else dim
        ops.adam_rows_sorted(th, m, v, idx, _source(dev, g[:, :dim], ld), ld, ALPHA, B1, B2, EPS, mark=mark)
    return th, m, v, mark


def _np(*ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _sweep_and_check(what, dev, st, th, m, v, mark):
    """brAdamDenseSweep behind a marked rows launch: marked rows keep their bits, every other row takes the float64 g = 0 step"""
    t = st.L.touched
    th1, m1, v1 = _np(th, m, v)
    _ops().adam_dense_sweep(th, m, v, ALPHA, B1, B2, EPS, mark=mark)
    th2, m2, v2, mk = _np(th, m, v, mark)
    assert not mk.any(), what + ": marks left behind the sweep"
    for a, b, name in ((th2, th1, "theta"), (m2, m1, "m"), (v2, v1, "v")):
        assert _same_bits(a[t], b[t]), f"{what}: the sweep changed {name} of a marked row"
    return st.check(what + " sweep", th2, m2, v2, ~t)


@functools.lru_cache(None)
def _state(name, dim):
    D = _data(name)
    return _AdamState(D, D.G_two[:, :dim], 1000 * dim + len(name) + ord(name[0]))


@pytest.mark.parametrize("dim", SUM_WIDTHS)
def test_adam_rows_both_forms(dev, dim):
    worst = {}
    for name in ("A", "B"):
        D, st = _data(name), _state(name, dim)
        for idt in (I32, I64):
            for k, (form, split) in enumerate(_forms(dim)):
                for with_mark in ((False, True) if form == "one source" else ((k + (idt == I64)) % 2 == 0,)):
                    what = f"adam rows {name} dim {dim} {form} {'mark' if with_mark else 'lazy'} {idt}"
                    th, m, v, mark = _rows_launch(dev, D.L, idt, D.g, st, form, split, with_mark)
                    w = st.check_rows_step(what, *_np(th, m, v, mark))
                    if with_mark:
                        for q, val in zip(("m", "v", "theta"), _sweep_and_check(what, dev, st, th, m, v, mark)):
                            worst[("brAdamRowsSorted + brAdamDenseSweep " + q, form)] = max(worst.get(("brAdamRowsSorted + brAdamDenseSweep " + q, form), 0.0), val)
                    for q, val in zip(("m", "v", "theta"), w):
                        worst[("brAdamRowsSorted " + q, form)] = max(worst.get(("brAdamRowsSorted " + q, form), 0.0), val)
    for (group, form), val in worst.items():
        _record(group, f"{dim} {form}", val)
    if dim in (64, 128, 48, 10):
        for L in _small_layouts():
            D = _data(L.name)
            st = _AdamStateSmall(D, dim)
            for idt, with_mark in ((I32, True), (I64, False)):
                th, m, v, mark = _rows_launch(dev, L, idt, D.g, st, "one source", None, with_mark)
                st.check_rows_step(f"adam rows {L.name} dim {dim} {idt}", *_np(th, m, v, mark))


class _AdamStateSmall(_AdamState):
    """the small layouts: one run; no first-touch / cancel designations to satisfy"""

    def __init__(self, D, dim):
        L, rng = D.L, np.random.default_rng(dim)
        G = np.ascontiguousarray(D.G_two[:1, :dim])
        self.L, self.G, self.dim = L, G, dim
        rows = L.rows
        self.th0 = rng.uniform(-0.05, 0.05, (rows, dim)).astype(f32)
        self.m0 = (10.0 ** rng.uniform(-9, -2, (rows, dim)) * rng.choice([-1.0, 1.0], (rows, dim))).astype(f32)
        self.v0 = (10.0 ** rng.uniform(-16, -4, (rows, dim))).astype(f32)
        self.first = np.array([dim % 3 == 0])
        if self.first[0]:
            self.m0[L.run_row] = 0.0; self.v0[L.run_row] = 0.0
        self.zero_rows = np.zeros(0, np.int64)
        Gf = np.zeros((rows, dim), f64); Gf[L.run_row] = G
        m64, v64 = self.m0.astype(f64), self.v0.astype(f64)
        self.m_ref, self.bm = B1F * m64 + OMB1F * Gf, 2 * U24 * (np.abs(B1F * m64) + np.abs(OMB1F * Gf))
        self.v_ref = B2F * v64 + OMB2F * Gf * Gf
        self.bv = 2 * U24 * self.v_ref + SUB


# ------------------------------------------------------------------------------------------------------------ the built index
@pytest.mark.parametrize("idt", [I32, I64])
def test_through_the_built_index(dev, idt):
    """RowIndex.build on the same streams: the same order of the valid positions, and then the same bits"""
    ops = _ops()
    for name in ("A", "B"):
        D = _data(name); L = D.L
        built = ops.RowIndex(L.n, idt, dev).build(torch.from_numpy(L.ids).to(dev).to(idt), L.rows)
        sid, spos = built.sorted_ids.cpu().numpy().astype(np.int64), built.sorted_pos.cpu().numpy()
        assert np.array_equal(sid[:L.nv], L.sid[:L.nv]) and np.array_equal(spos[:L.nv], L.spos[:L.nv])
        assert sorted(spos[L.nv:].tolist()) == sorted(L.spos[L.nv:].tolist())
        for dim in (64, 48):
            out = _nan(dev, L.n, dim)
            built.seg_ws(dim).fill_(float("nan"))
            ops.segment_sum_rows(built, _source(dev, D.g[:, :dim], dim), dim=dim, ldg=dim, out=out, two_level=True)
            heads = L.start[:L.nvr]
            assert _same_bits(out.cpu().numpy()[heads], D.G_two[:L.nvr, :dim])
            st = _state(name, dim)
            a = _np(*_rows_launch(dev, L, idt, D.g, st, "one source", None, True))
            b = _np(*_rows_launch(dev, L, idt, D.g, st, "one source", None, True, index=built))
            for x, y in zip(a[:3], b[:3]):
                assert _same_bits(x, y)
            assert np.array_equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------------------ 4. the pair launches
PAIR_WIDTHS = (64, 128, 256, 48, 20, 75)


@functools.lru_cache(None)
def _pair_state(name, dim):
    D, split = _data(name), dim // 2
    G = np.concatenate([D.G_two[:, :split], _hi(name)[3][:, :dim - split]], axis=1)
    return _AdamState(D, G, 5000 + dim + ord(name))


def _run_pair(dev, idt, dim, paired):
    ops, split = _ops(), dim // 2
    sc = _hi("A")[1]
    assert np.array_equal(sc, _hi("B")[1])
    out = []
    tabs = []
    for name in ("A", "B"):
        D, st = _data(name), _pair_state(name, dim)
        idx = D.L.index(dev, idt)
        idx.seg_ws(dim).fill_(float("nan"))
        tabs.append((D, [_td(dev, st.th0), _td(dev, st.m0), _td(dev, st.v0), torch.zeros(D.L.rows, dtype=torch.uint8, device=dev)], idx))
    lo = [_source(dev, D.g[:, :split], split) for D, _, _ in tabs]
    if paired:
        hi = [_source(dev, _hi(name)[0][:, :dim - split], dim - split) for name in ("A", "B")]
        (Da, ta, ia), (Db, tb, ib) = tabs
        ops.adam_rows_sorted_pair(ta[0], ta[1], ta[2], ia, lo[0], split, hi[0], dim - split, tb[0], tb[1], tb[2], ib, lo[1], split, hi[1], dim - split,
                                  split, ALPHA, B1, B2, EPS, hi_scale=_td(dev, sc), mark_a=ta[3], mark_b=tb[3])
    else:
        for k, name in enumerate(("A", "B")):
            D, tt, idx = tabs[k]
            hi = _source(dev, _hi(name)[2][:, :dim - split], dim - split)
            ops.adam_rows_sorted(tt[0], tt[1], tt[2], idx, lo[k], split, ALPHA, B1, B2, EPS, mark=tt[3], row_grads_hi=hi, ldg_hi=dim - split, split=split)
    return [_np(*tt) for _, tt, _ in tabs]


@pytest.mark.parametrize("dim", PAIR_WIDTHS)
def test_adam_rows_pair_with_hi_scale(dev, dim):
    for idt in (I32, I64):
        one = _run_pair(dev, idt, dim, True)
        two = _run_pair(dev, idt, dim, False)
        for name, p, s in zip(("A", "B"), one, two):
            what = f"adam pair table {name} dim {dim} {idt}"
            for x, y, q in zip(p, s, ("theta", "m", "v", "mark")):
                assert _same_bits(x, y) if q != "mark" else np.array_equal(x, y), f"{what}: {q} differs from the single launch on the premultiplied source"
            w = _pair_state(name, dim).check_rows_step(what, *p)
            for q, val in zip(("m", "v", "theta"), w):
                _record("brAdamRowsSortedPair " + q, f"{dim} table {name} {'i32' if idt == I32 else 'i64'}", val)


REPLAYED_WIDTHS = (64, 128, 256)


def _random_layout(n, seed):
    rng = np.random.default_rng(seed)
    runs = []
    while sum(runs) < n:
        runs.append(int(min(n - sum(runs), rng.choice([1, 1, 2, 3, 5, 9, 40, 70, 150, 300]))))
    rng.shuffle(runs)
    return _Layout(f"random {n}", runs, (0, 0, 0), seed)


@functools.lru_cache(None)
def _replay_jobs():
    A = _layouts()["A"]
    long, short = _random_layout(2 * A.n, 71), _random_layout(A.n - 100, 72)
    assert short.n % 64 and short.n // 64 < A.n // 64          # the shorter job ends inside a 64-block of the longer one
    return A, long, short


def _deferred_tables(dev, L, dim, seed, T):
    rng = np.random.default_rng(seed)
    th = rng.uniform(-0.05, 0.05, (L.rows, dim)).astype(f32)
    g = 10.0 ** rng.uniform(-6, -2, (L.rows, dim)) * rng.choice([-1.0, 1.0], (L.rows, dim))
    m, v = ((1 - B1) * g).astype(f32), ((1 - B2) * g * g).astype(f32)
    m[::7] = 0.0; v[::7] = 0.0                                   # rows nobody has touched
    last = (T - 1 - rng.choice([0, 1, 3, 8], L.rows)).astype(np.int32)
    return [th, m, v, last]


@pytest.mark.parametrize("replay", ["exact", "fast"])
@pytest.mark.parametrize("dim", REPLAYED_WIDTHS)
def test_adam_rows_pair_replayed_with_two_lengths(dev, dim, replay):
    ops = _ops()
    _lib = import_module("binary-recommendation_amd._lib")
    lib = _lib.load()
    T = 12
    ss = ops.new_step_state(dev, B1, B2, EPS, replay)
    for _ in range(T):
        _lib.check(lib.brStepStateAdvance(ss.data_ptr(), LR, B1, B2, None, 0, ops._stream()), "brStepStateAdvance")
    A, long, short = _replay_jobs()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for other, idt, split in ((long, I32, 0), (short, I64, dim // 2), (short, I32, 0), (long, I64, dim // 2)):
        jobs = []
        for k, L in enumerate((A, other)):
            rng = np.random.default_rng(dim + 10 * k + L.n)
            g = _td(dev, (rng.normal(size=(L.n, dim)) * 1e-2).astype(f32))
            host = _deferred_tables(dev, L, dim, 900 + k + dim, T)
            ids = torch.from_numpy(L.ids).to(dev).to(idt)
            sets = [[_td(dev, x) for x in host] for _ in range(2)]
            rep = ops.gather_rows_deferred(*sets[0], ids, ss, B1, B2, EPS, err_flag=err)
            idx = L.index(dev, idt)
            idx.seg_ws(dim).fill_(float("nan"))
            jobs.append((L, g, sets, rep, idx, host))
        (La, ga, sa, ra, ia, ha), (Lb, gb, sb, rb, ib, hb) = jobs
        ops.adam_rows_sorted_deferred_pair_replayed(*sa[0], ia, ga, ra, *sb[0], ib, gb, rb, split, ss, B1, B2, EPS)
        pair = [_np(*sa[0]), _np(*sb[0])]
        for L, g, sets, rep, idx, host in jobs:
            idx.seg_ws(dim).fill_(float("nan"))
            kw = dict(row_grads_hi=g[:, split:], ldg_hi=dim, split=split) if split else {}
            ops.adam_rows_sorted_deferred(*sets[1], idx, g, dim, ss, B1, B2, EPS, replayed=rep, **kw)
        for k, (L, g, sets, rep, idx, host) in enumerate(jobs):
            single = _np(*sets[1])
            for x, y, q in zip(pair[k], single, ("theta", "m", "v", "last")):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"pair replayed dim {dim} {replay} n {La.n} / {Lb.n} table {k}: {q} differs"
            assert (single[3][L.touched] == T).all() and np.array_equal(single[3][~L.touched], host[3][~L.touched])
            assert not np.array_equal(single[0][L.touched].view(np.uint32), host[0][L.touched].view(np.uint32))


def test_pair_replayed_refuses_two_lengths_off_the_wave_shapes(dev):
    ops = _ops()
    _lib = import_module("binary-recommendation_amd._lib")
    lib = _lib.load()
    dim, T = 48, 12
    ss = ops.new_step_state(dev, B1, B2, EPS, "exact")
    for _ in range(T):
        _lib.check(lib.brStepStateAdvance(ss.data_ptr(), LR, B1, B2, None, 0, ops._stream()), "brStepStateAdvance")
    A, long, short = _replay_jobs()
    for other in (long, short):
        args, keep = [], []
        for k, L in enumerate((A, other)):
            host = _deferred_tables(dev, L, dim, 40 + k, T)
            tabs = [_td(dev, x) for x in host]
            g, rep = _td(dev, np.ones((L.n, dim), f32)), _td(dev, np.ones((L.n, dim), f32))
            idx = L.index(dev, I32)
            idx.seg_ws(dim).fill_(float("nan"))
            args += [*tabs, idx, g, rep]
            keep.append((host, tabs, idx))
        with pytest.raises(_lib.BinrecError, match="tables of different lengths in one launch need the one-wave-per-row shapes"):
            ops.adam_rows_sorted_deferred_pair_replayed(*args, 0, ss, B1, B2, EPS)
        torch.cuda.synchronize()
        for host, tabs, idx in keep:
            for x, y in zip(host, _np(*tabs)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "a refused call wrote to a table"
            assert bool(torch.isnan(idx.seg_ws(dim)).all()), "a refused call wrote partials"


# ------------------------------------------------------------------------------------------------------------ 5. Adagrad, sweep, flat
def _adagrad_check(what, th, acc, th0, acc0, G, fresh=None):
    """Adagrad bounds of the elements given (float32 arrays of one shape); fresh: mask of elements with acc0 = 0 (acc = fl(G G) exactly)"""
    G64 = G.astype(f64)
    ref = acc0.astype(f64) + G64 * G64
    ra = _ratio(what + " acc", acc, ref, 2 * U24 * ref)
    if fresh is not None:
        assert _same_bits(acc[fresh], G[fresh] * G[fresh]), what + ": acc0 = 0: acc is not the single product G * G"
    upd = LR_GF * G64 / (np.sqrt(acc.astype(f64)) + EPSF)
    tref = th0.astype(f64) - upd
    return ra, _ratio(what + " theta", th, tref, 6 * U24 * np.abs(upd) + U24 * np.abs(tref))


@pytest.mark.parametrize("dim", SUM_WIDTHS)
def test_adagrad_rows(dev, dim):
    ops = _ops()
    for name in ("A", "B"):
        D = _data(name); L = D.L
        rng = np.random.default_rng(7000 + dim + ord(name))
        G = np.ascontiguousarray(D.G_two[:L.nvr, :dim])
        th0 = rng.uniform(-0.05, 0.05, (L.rows, dim)).astype(f32)
        acc0 = np.full((L.rows, dim), 0.1, f32)
        at = (D.scale[:L.nvr, None] ** 2 * rng.uniform(0.05, 1.0, (L.nvr, dim)))
        fresh = (np.arange(L.nvr) % 4 == 0)
        at[fresh] = 0.0
        acc0[L.run_row] = at.astype(f32)
        for idt in (I32, I64):
            for ld, off in ((dim, 0), (dim, 1), (dim, 2), (dim + 1, 0)):
                what = f"adagrad rows {name} dim {dim} ld {ld} off {off} {idt}"
                th, acc = _td(dev, th0), _td(dev, acc0)
                idx = L.index(dev, idt)
                idx.seg_ws(dim).fill_(float("nan"))
                ops.adagrad_rows_sorted(th, acc, idx, _source(dev, D.g[:, :dim], ld, off), ld, LR_G, EPS)
                t, a = _np(th, acc)
                r = L.run_row
                fm = np.repeat(fresh[:, None], dim, axis=1)
                ra, rt = _adagrad_check(what, t[r], a[r], th0[r], acc0[r], G, fm)
                assert np.isfinite(t).all() and _same_bits(t[~L.touched], th0[~L.touched]) and _same_bits(a[~L.touched], acc0[~L.touched]), what + ": untouched rows"
                _record("brAdagradRowsSorted acc", f"{dim} ld+{ld - dim} off {off}", ra)
                _record("brAdagradRowsSorted theta", f"{dim} ld+{ld - dim} off {off}", rt)


@pytest.mark.parametrize("rows,dim", [(70_000, 64), (1001, 75)])
def test_dense_sweep_past_the_grid_cap_and_at_75_columns(dev, rows, dim):
    vec, chunks, _ = _geom(dim)
    assert (rows * chunks > 256 * 16 * 256) == (dim == 64) and (dim == 64 or (vec, chunks) == (1, 75))
    ops = _ops()
    rng = np.random.default_rng(rows)
    th0 = rng.uniform(-0.05, 0.05, (rows, dim)).astype(f32)
    m0 = (10.0 ** rng.uniform(-9, -2, (rows, dim)) * rng.choice([-1.0, 1.0], (rows, dim))).astype(f32)
    v0 = (10.0 ** rng.uniform(-16, -4, (rows, dim))).astype(f32)
    m0[5] = 0.0; v0[5] = 0.0
    mk = rng.random(rows) < 0.1
    mk[[0, rows - 1, rows // 2]] = True; mk[[1, rows - 2]] = False
    th, m, v, mark = _td(dev, th0), _td(dev, m0), _td(dev, v0), _td(dev, mk.astype(np.uint8))
    ops.adam_dense_sweep(th, m, v, ALPHA, B1, B2, EPS, mark=mark)
    t, mm, vv, k = _np(th, m, v, mark)
    assert not k.any(), "marks left behind the sweep"
    for a, b, name in ((t, th0, "theta"), (mm, m0, "m"), (vv, v0, "v")):
        assert _same_bits(a[mk], b[mk]), f"the sweep changed {name} of a marked row"
    fr = ~mk
    m64, v64 = m0[fr].astype(f64), v0[fr].astype(f64)
    what = f"dense sweep {rows} x {dim}"
    rm = _ratio(what + " m", mm[fr], B1F * m64, 2 * U24 * np.abs(B1F * m64))
    rv = _ratio(what + " v", vv[fr], B2F * v64, 2 * U24 * B2F * v64 + SUB)
    upd = AF * mm[fr].astype(f64) / (np.sqrt(vv[fr].astype(f64)) + EPSF)
    ref = th0[fr].astype(f64) - upd
    rt = _ratio(what + " theta", t[fr], ref, 7 * U24 * np.abs(upd) + U24 * np.abs(ref))
    assert _same_bits(t[5], th0[5])
    for q, val in (("m", rm), ("v", rv), ("theta", rt)):
        _record("brAdamDenseSweep " + q, f"{rows} x {dim}", val)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_flat_updates(dev, n):
    ops = _ops()
    rng = np.random.default_rng(n)
    g = (10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    th0 = rng.uniform(-0.05, 0.05, n).astype(f32)
    m0 = (rng.uniform(0.1, 10.0, n) * rng.choice([-1.0, 1.0], n) * OMB1F * np.abs(g)).astype(f32)
    v0 = (OMB2F * g.astype(f64) ** 2 * rng.uniform(0.05, 1.0, n)).astype(f32)
    m0[::3] = (-(OMB1F * g[::3].astype(f64)) * (1 - 1e-3) / B1F).astype(f32)
    m0[::4] = 0.0; v0[::4] = 0.0
    pad = lambda a: _td(dev, np.r_[a, np.full(3, np.nan, f32)])
    th, m, v, gd = pad(th0), pad(m0), pad(v0), pad(g)
    ops.adam_flat(th[:n], m[:n], v[:n], gd[:n], ALPHA, B1, B2, EPS)
    t, mm, vv = _np(th, m, v)
    assert np.isnan(t[n:]).all() and np.isnan(mm[n:]).all() and np.isnan(vv[n:]).all(), "brAdamFlat wrote past n"
    t, mm, vv = t[:n], mm[:n], vv[:n]
    g64, m64, v64 = g.astype(f64), m0.astype(f64), v0.astype(f64)
    what = f"adam flat n {n}"
    rm = _ratio(what + " m", mm, B1F * m64 + OMB1F * g64, 2 * U24 * (np.abs(B1F * m64) + np.abs(OMB1F * g64)))
    vref = B2F * v64 + OMB2F * g64 * g64
    rv = _ratio(what + " v", vv, vref, 2 * U24 * vref + SUB)
    assert _same_bits(mm[::4], f32(OMB1F) * g[::4]) and _same_bits(vv[::4], f32(OMB2F) * (g[::4] * g[::4]))
    upd = AF * mm.astype(f64) / (np.sqrt(vv.astype(f64)) + EPSF)
    ref = th0.astype(f64) - upd
    rt = _ratio(what + " theta", t, ref, 7 * U24 * np.abs(upd) + U24 * np.abs(ref))
    for q, val in (("m", rm), ("v", rv), ("theta", rt)):
        _record("brAdamFlat " + q, str(n), val)
    acc0 = (g.astype(f64) ** 2 * rng.uniform(0.05, 1.0, n)).astype(f32)
    acc0[::4] = 0.0
    th, acc = pad(th0), pad(acc0)
    ops.adagrad_flat(th[:n], acc[:n], gd[:n], LR_G, EPS)
    t, a = _np(th, acc)
    assert np.isnan(t[n:]).all() and np.isnan(a[n:]).all(), "brAdagradFlat wrote past n"
    fresh = np.zeros(n, bool); fresh[::4] = True
    ra, rt = _adagrad_check(f"adagrad flat n {n}", t[:n], a[:n], th0, acc0, g, fresh)
    _record("brAdagradFlat acc", str(n), ra)
    _record("brAdagradFlat theta", str(n), rt)


# ------------------------------------------------------------------------------------------------------------ 6. strips of 2 and 8
def _strip_digests(dev):
    """the wave cases of sections 3 and 4 at 64 and 128 floats -> {case: sha256 of theta, m, v, marks}"""
    out = {}
    dig = lambda arrs: hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrs)).hexdigest()
    for dim in (64, 128):
        for name in ("A", "B"):
            D, st = _data(name), _state(name, dim)
            for idt in (I32, I64):
                for form, split in _forms(dim):
                    if _vec_width([split or 0, dim + 1 if form == "odd stride" else dim, dim - (split or 0)]) < {64: 1, 128: 2}[dim]:
                        continue                                  # not a wave launch at this width
                    out[f"rows {name} {dim} {form} {idt}"] = dig(_np(*_rows_launch(dev, D.L, idt, D.g, st, form, split, True)))
        for idt in (I32, I64):
            for name, r in zip(("A", "B"), _run_pair(dev, idt, dim, True)):
                out[f"pair {name} {dim} {idt}"] = dig(r)
    return out


_HERE = {}
CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd())
import torch
from tests import test_gpu_sorted_rows as T
print("RESULT " + json.dumps(T._strip_digests(torch.device("cuda:0"))))
"""


@pytest.mark.parametrize("strip", [2, 8])
def test_strips_of_2_and_8_give_the_same_bits(dev, strip):
    assert os.environ.get("BR_ADAM_STRIP", "4") == "4"          # this process runs the default strip
    if not _HERE:
        _HERE.update(_strip_digests(dev))
    here = _HERE
    assert len(here) >= 2 * (2 * 2 * 3 + 2 * 2)
    env = dict(os.environ)
    env["BR_ADAM_STRIP"] = str(strip)
    env.pop("BR_TEST_RECORD_DIR", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    there = json.loads(line[len("RESULT "):])
    assert there.keys() == here.keys()
    assert not [k for k in here if here[k] != there[k]], [k for k in here if here[k] != there[k]]
