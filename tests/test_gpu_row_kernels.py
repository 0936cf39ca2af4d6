"""-m gpu: the row-group kernels of csrc/gather.hip against float64 - row_dot / row_dot_bwd, neumf_embed_fwd (with and without the stashes),
neumf_embed_bwd (by position and by id), mf_grad_inplace, bpr_fwd_bwd - and the out-of-range flag of every kernel that stores it.

A row group of 1 - 64 lanes owns one embedding row (rows.h): row_geom / row_geom_ld pick VEC in {4, 2, 1} floats per lane and
lpr = min(64, pow2ceil(dim / VEC)) lanes per row, and a kernel loops when dim / VEC > 64.  WIDTHS reaches every such geometry (asserted in
test_the_widths_reach_every_geometry): one lane, idle lanes, 64 lanes in one pass, one chunk in a second pass, several chunks behind the
first pass, at every VEC.  Batches: 1 (every other lane of the workgroup clamps to row batch - 1), one row past a workgroup, 1001.  Both id types.

References are float64 numpy on the float32 inputs as given; every output is filled with NaN before the launch, and whatever a launch
has no business writing (rows past the batch, columns past dim of a strided output, rows of invalid ids) must still be NaN behind it.

  dot products (row_dot, `dot` of the embed forward)   |got - ref| <= (depth + 1) 2^-24 sum_k |a_k b_k|,
        depth = VEC + ceil(chunks / lpr) + log2(lpr): the roundings a term passes through in vdot (one product, VEC - 1 fused adds),
        the per-lane accumulation over the passes and the shuffle tree.  A third of the rows cancel (sum = 1e-3 sum |terms|).
  single products (dA / dB of row_dot_backward, the MF gradients of neumf_embed_backward, mf_grad_inplace)    bit-equal to the one
        fp32 multiply np.float32(g) * np.float32(row); inputs are drawn from +-[2^-6, 1) (no subnormal product)
  copies (x0 in both concat orders, both stashes, g_*_mlp)    bit-equal

BPR on hard scores (test_bpr_on_hard_margins): every triplet has rows of its own, rescaled so that the float64 margin x = u.p - u.n lands near
0, +-1e-3, +-1, +-5, +-10, +-14, +-16.5, +-17, +-20, +-40, +-88, +-100 in turn.  l = sigmoid(-x), dx = -sigmoid(x) l inv_batch (the two scores are
not outputs: they are judged through l).  With E_x = (depth + 1) 2^-24 (sum |u p| + sum |u n|) + 2^-24 |x| - what the rounding of the two dot
products and of their difference can move the margin by -
  |l - l_ref| <= l_ref (expm1(E_x) + 8 2^-24) + 2^-126        (|d ln l / dx| = sigmoid(x) <= 1; exp, add, divide, product: 4 roundings, x 2)
  |g - g_ref| <= |g_ref| (2 expm1(E_x) + 17 2^-24) + 2^-126    per gradient element (|d ln(s l) / dx| <= 1; 8 roundings x 2, + the row product)
2^-126 is the smallest normal float: subnormal results at |x| >= 88 are neither demanded nor forbidden.  loss_sum: the 64 slots enter holding
known non-zero doubles; what the launch added must match sum l_ref to the largest per-row relative bound (+ the double roundings of the adds).

Observed maxima in units of each bound, per width (and per margin for BPR), go to row_kernels_errors.json in the directory that
BR_TEST_RECORD_DIR names, when it is set and exists (profiles/row_kernels/ holds the file of one run)."""
import itertools
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

from oracle import binrec_oracle as O

pytestmark = pytest.mark.gpu
U24, TINY = 2.0 ** -24, 2.0 ** -126
RANGE, CAPACITY = 1, 2                     # BR_ERRFLAG_RANGE, BR_ERRFLAG_CAPACITY
I32, I64 = torch.int32, torch.int64
WIDTHS = (4, 12, 64, 256, 260, 1024, 2, 10, 126, 130, 350, 1, 3, 63, 65, 75)
MARGINS = (0.0,) + tuple(s * t for t in (1e-3, 1.0, 5.0, 10.0, 14.0, 16.5, 17.0, 20.0, 40.0, 88.0, 100.0) for s in (1.0, -1.0))
f64 = np.float64


def _ops():
    return import_module("binary-recommendation_amd.ops")


# ------------------------------------------------------------------------------------------------------------ geometry (rows.h)
def _vec_width(strides, ptrs=()):
    """rows.h vec_width: the widest vector that divides every stride (floats) and that every pointer (bytes) is aligned to"""
    st = 0
    for s in strides:
        st |= int(s)
    al = 0
    for p in ptrs:
        al |= int(p)
    return 4 if (st & 3) == 0 and (al & 15) == 0 else 2 if (st & 1) == 0 and (al & 7) == 0 else 1


def _geom(dim, also=4):
    """rows.h row_geom_ld: (VEC, chunks, log2 lanes per row); `also` = the widest vector the call's strides and pointers allow"""
    vec = 4 if dim % 4 == 0 and also >= 4 else 2 if dim % 2 == 0 and also >= 2 else 1
    chunks = dim // vec
    l = 0
    while (1 << l) < chunks and l < 6:
        l += 1
    return vec, chunks, l


def _passes(dim, also=4):
    _, chunks, l = _geom(dim, also)
    return -(-chunks // (1 << l))


def _depth(dim, also=4):
    vec, _, l = _geom(dim, also)
    return vec + _passes(dim, also) + l


def _rows_per_block(dim, also=4):
    return 256 >> _geom(dim, also)[2]


def _batches(dim, also=4):
    return (1, _rows_per_block(dim, also) + 1, 1001)


def test_the_widths_reach_every_geometry():
    seen = set()
    for dim in WIDTHS:
        vec, chunks, l = _geom(dim)
        lpr, passes = 1 << l, _passes(dim)
        assert vec * chunks == dim and lpr <= 64 and (lpr >= chunks or lpr == 64)
        if lpr == 1:
            seen.add((vec, "one lane"))
        if chunks < lpr:
            seen.add((vec, "idle lanes"))
        if lpr == 64 and passes == 1:
            seen.add((vec, "64 lanes, one pass"))
        if chunks == 64:
            seen.add((vec, "last single pass"))
        if chunks == 65:
            seen.add((vec, "one chunk in a second pass"))
        if chunks > 65:
            seen.add((vec, "several chunks behind the first pass"))
        if passes >= 3 and chunks % lpr == 0:
            seen.add((vec, "full passes"))
        b = _batches(dim)
        assert b[0] == 1 and 1 < b[1] <= 257 and b[1] % _rows_per_block(dim) == 1 and b[2] > 3 * _rows_per_block(dim) and b[2] % _rows_per_block(dim)
    want = {(v, w) for v in (4, 2, 1) for w in ("one lane", "idle lanes", "64 lanes, one pass", "one chunk in a second pass", "several chunks behind the first pass")}
    want |= {(4, "last single pass"), (4, "full passes")}
    assert seen >= want, want - seen
    # a stride or a pointer that forces a narrower vector than dim allows (row_geom_ld): the single-pass boundary of VEC 2 and 1
    assert _geom(64, 2) == (2, 32, 5) and _geom(64, 1) == (1, 64, 6) and _passes(256, 2) == 2 and _passes(128, 1) == 2
    assert _vec_width([68], [8]) == 2 and _vec_width([68], [4]) == 1 and _vec_width([66], [0]) == 2 and _vec_width([65, 0], [0]) == 1
    assert len(MARGINS) == 23


# ------------------------------------------------------------------------------------------------------------ inputs, checks, record
def _vals(rng, shape):
    """float32 in +-[2^-6, 1): no product of two or three of them is subnormal"""
    return (rng.uniform(2.0 ** -6, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _dot_rows(rng, batch, dim):
    """two (batch, dim) operands; in rows 0, 3, 6, .. the terms alternate in sign and sum to 1e-3 of the sum of their magnitudes"""
    a, b = _vals(rng, (batch, dim)), _vals(rng, (batch, dim))
    if dim >= 2:
        rows = np.arange(batch) % 3 == 0
        sgn = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)
        bb = np.abs(b[rows]).astype(f64) * np.sign(a[rows]) * sgn
        t = a[rows].astype(f64) * bb
        bb[:, 0::2] *= (-t[:, 1::2].sum(1) * (1 + 2e-3) / t[:, 0::2].sum(1))[:, None]
        b[rows] = bb.astype(np.float32)
        t = a[rows].astype(f64) * b[rows].astype(f64)
        assert (np.abs(t.sum(1)) <= 2e-3 * np.abs(t).sum(1)).all()      # (the test's own inputs)
    return a, b


def _td(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _flag(dev, v=0):
    return torch.full((1,), v, dtype=torch.int32, device=dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, ref):
    return got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


def _written_exactly(full, regions):
    """full: a NaN-prefilled 2-d output as read back; regions: [(row index array or None = rows 0 .. len - 1, first column, expected float32
    (n, w))].  The regions hold the expected bits and every other element is still NaN."""
    exp = np.full(full.shape, np.nan, dtype=np.float32)
    for rows, c0, val in regions:
        r = np.arange(val.shape[0]) if rows is None else rows
        exp[r, c0:c0 + val.shape[1]] = val
    mask = ~np.isnan(exp)
    return np.array_equal(_bits(full)[mask], _bits(exp)[mask]) and bool(np.isnan(full[~mask]).all())


_REC = {}


def _record(group, key, value):
    _REC.setdefault(group, {})[key] = value
    out = os.environ.get("BR_TEST_RECORD_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "row_kernels_errors.json"), "w") as fh:
            json.dump({"note": "max |got - float64| / bound (<= 1 passes; bounds in tests/test_gpu_row_kernels.py).  dot: per kernel and width; "
                               "bpr: per width and margin [loss, gradients]", **_REC}, fh, indent=1, sort_keys=True)


def _dot_ratio(got, a, b, depth):
    t = a.astype(f64) * b.astype(f64)
    bound = (depth + 1) * U24 * np.abs(t).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got.astype(f64) - t.sum(1)) / bound
    r = np.where((bound == 0) & (got == 0), 0.0, r)          # a row of zeros (an invalid id): exactly 0 is asked for
    return float(r.max()) if not np.isnan(r).any() else float("nan")


def _check_dot(group, key, ratios):
    worst = max(ratios, key=lambda r: (np.isnan(r), r))
    _record(group, key, worst)
    assert worst <= 1.0, f"{group} {key}: |got - float64| reaches {worst} of (depth + 1) 2^-24 sum |terms|"


# ------------------------------------------------------------------------------------------------------------ row_dot
@pytest.mark.parametrize("dim", WIDTHS)
def test_row_dot_and_backward(dev, dim):
    ops = _ops()
    rng = np.random.default_rng(100 + dim)
    ratios = []
    for batch in _batches(dim):
        a, b = _dot_rows(rng, batch, dim)
        ad, bd = _td(dev, a), _td(dev, b)
        out = _nan(dev, batch + 3)
        ops.row_dot(ad, bd, out=out[:batch])
        o = out.cpu().numpy()
        assert np.isnan(o[batch:]).all()
        ratios.append(_dot_ratio(o[:batch], a, b, _depth(dim)))
        g = _vals(rng, batch)
        da, db = _nan(dev, batch + 1, dim), _nan(dev, batch + 1, dim)
        ops.row_dot_backward(ad, bd, _td(dev, g), da=da[:batch], db=db[:batch])
        assert _written_exactly(da.cpu().numpy(), [(None, 0, g[:, None] * b)]), (dim, batch)
        assert _written_exactly(db.cpu().numpy(), [(None, 0, g[:, None] * a)]), (dim, batch)
    _check_dot("dot row_dot", str(dim), ratios)


# ------------------------------------------------------------------------------------------------------------ NeuMF embed block
ROWS = 1001      # rows of every table of the embed tests


class _Tables:
    """the four tables of the embed block.  layout: separate (ld = dim), fused ([mlp | mf], ld = 2 dim), in130 / in129 (the first 2 dim
    columns of a 130- / 129-wide allocation).  Row r of user_mf cancels against row r of item_mf for r % 3 == 0 (_dot_rows)."""

    def __init__(self, rng, dim, layout, dev):
        self.dim, self.layout = dim, layout
        self.um, self.im = _vals(rng, (ROWS, dim)), _vals(rng, (ROWS, dim))
        self.uf, self.vf = _dot_rows(rng, ROWS, dim)
        self.width = {"separate": dim, "fused": 2 * dim, "in130": 130, "in129": 129}[layout]
        if layout == "separate":
            self.d = [_td(dev, t) for t in (self.um, self.im, self.uf, self.vf)]
        else:
            assert self.width >= 2 * dim
            dev_t = []
            for mlp, mf in ((self.um, self.uf), (self.im, self.vf)):
                alloc = np.full((ROWS, self.width), 7.0, dtype=np.float32)
                alloc[:, :dim], alloc[:, dim:2 * dim] = mlp, mf
                dev_t.append(_td(dev, alloc))
            self.d = [dev_t[0][:, :dim], dev_t[1][:, :dim], dev_t[0][:, dim:2 * dim], dev_t[1][:, dim:2 * dim]]

    def ids(self, rng, batch):
        u = rng.integers(0, ROWS, batch)
        u[:7] = u[0]                                                  # duplicates
        i = np.where(u % 3 == 0, u, rng.integers(0, ROWS, batch))     # a third of the pairs cancel
        return u, i


def _strided(dev, rows, dim, ld, off):
    """a NaN-filled flat buffer and its (rows, dim) view of row stride ld that starts `off` floats into it"""
    flat = _nan(dev, off + rows * ld + 5)
    return flat, flat[off:off + rows * ld].view(rows, ld)[:, :dim]


def _flat_regions(flat, rows, ld, off, val):
    """_written_exactly on the flat buffer of _strided: rows 0 .. len(val) - 1 hold val, everything else is NaN"""
    f = flat.cpu().numpy()
    body = f[off:off + rows * ld].reshape(rows, ld)
    return bool(np.isnan(f[:off]).all() and np.isnan(f[off + rows * ld:]).all()) and _written_exactly(body, [(None, 0, val)])


def _embed_forward(ops, dev, T, u, i, idt, item_first, stash=None, flag=None, zero_user=(), zero_item=()):
    """one forward launch, checked: x0 and the stashes bit for bit, NaN wherever nothing belongs; -> the ratio of `dot` to its bound.
    stash = (ld, off); zero_user / zero_item: batch positions whose id is invalid (their rows read as zeros)."""
    dim, batch = T.dim, len(u)
    x0, dot = _nan(dev, batch + 1, 2 * dim), _nan(dev, batch + 2)
    ud, idd = _td(dev, u).to(idt), _td(dev, i).to(idt)
    st = None
    if stash is not None:
        ld, off = stash
        fu, su = _strided(dev, batch + 1, dim, ld, off)
        fi, si = _strided(dev, batch + 1, dim, ld, off)
        st = (su[:batch], si[:batch])
    ops.neumf_embed_forward(T.d[0], T.d[1], T.d[2], T.d[3], ud, idd, item_first, x0[:batch], dot[:batch], err_flag=flag, stash=st)
    also = _vec_width([T.d[0].stride(0), T.d[1].stride(0), stash[0] if stash else 0], [t.data_ptr() for t in st] if st else [])
    uu, ii = np.clip(u, 0, ROWS - 1), np.clip(i, 0, ROWS - 1)
    um, im, uf, vf = T.um[uu], T.im[ii], T.uf[uu], T.vf[ii]
    for rows, z in ((list(zero_user), (um, uf)), (list(zero_item), (im, vf))):
        for a in z:
            a[rows] = 0.0
    first, second = (im, um) if item_first else (um, im)
    assert _written_exactly(x0.cpu().numpy(), [(None, 0, first), (None, dim, second)]), "x0"
    if stash is not None:
        assert _flat_regions(fu, batch + 1, ld, off, uf), "stash_user"
        assert _flat_regions(fi, batch + 1, ld, off, vf), "stash_item"
    d = dot.cpu().numpy()
    assert np.isnan(d[batch:]).all()
    return _dot_ratio(d[:batch], uf, vf, _depth(dim, also)), also


def _embed_backward(ops, dev, T, rng, u, i, idt, item_first, with_mlp):
    """one backward launch by batch position into outputs laid out like the tables, checked bit for bit"""
    dim, batch, W = T.dim, len(u), T.width
    dx0, g = _vals(rng, (batch, 2 * dim)), _vals(rng, batch)
    ud, idd = _td(dev, u).to(idt), _td(dev, i).to(idt)
    if T.layout == "separate":
        bufs = [_nan(dev, batch + 1, dim) for _ in range(4)]
        views = [b[:batch] for b in bufs]                        # user mlp, item mlp, user mf, item mf
    else:
        gu, gi = _nan(dev, batch + 1, W), _nan(dev, batch + 1, W)
        bufs = [gu, gi]
        views = [gu[:batch, :dim], gi[:batch, :dim], gu[:batch, dim:2 * dim], gi[:batch, dim:2 * dim]]
    ops.neumf_embed_backward(T.d[2], T.d[3], ud, idd, item_first, _td(dev, dx0) if with_mlp else None, _td(dev, g), views[2], views[3],
                             views[0] if with_mlp else None, views[1] if with_mlp else None)
    uo, io = (dim, 0) if item_first else (0, dim)
    exp = [dx0[:, uo:uo + dim], dx0[:, io:io + dim], g[:, None] * T.vf[i], g[:, None] * T.uf[u]]
    if T.layout == "separate":
        for k in range(4):
            assert _written_exactly(bufs[k].cpu().numpy(), [(None, 0, exp[k])] if (with_mlp or k >= 2) else []), k
    else:
        for k, b in enumerate(bufs):
            assert _written_exactly(b.cpu().numpy(), ([(None, 0, exp[k])] if with_mlp else []) + [(None, dim, exp[2 + k])]), k


def _embed_cases():
    for k, (layout, idt, item_first) in enumerate(itertools.product(("separate", "fused"), (I32, I64), (1, 0))):
        yield layout, idt, item_first, bin(k).count("1") % 2 == 1       # stashes / g_*_mlp: with every layout, id type and order, on and off


@pytest.mark.parametrize("dim", WIDTHS)
def test_embed_block(dev, dim):
    ops = _ops()
    rng = np.random.default_rng(200 + dim)
    tabs = {layout: _Tables(rng, dim, layout, dev) for layout in ("separate", "fused")}
    ratios = []
    for batch in _batches(dim):
        for layout, idt, item_first, extra in _embed_cases():
            T = tabs[layout]
            u, i = T.ids(rng, batch)
            flag = _flag(dev)
            r, also = _embed_forward(ops, dev, T, u, i, idt, item_first, stash=(dim, 0) if extra else None, flag=flag)
            assert also >= _geom(dim)[0] and int(flag.item()) == 0
            ratios.append(r)
            _embed_backward(ops, dev, T, rng, u, i, idt, item_first, with_mlp=extra)
    _check_dot("dot neumf_embed_fwd", str(dim), ratios)


@pytest.mark.parametrize("layout,vec", [("in130", 2), ("in129", 1)])
def test_embed_block_on_views_that_force_a_narrower_vector(dev, layout, vec):
    """dim 64 allows float4; a row stride of 130 / 129 floats allows float2 / float (row_geom_ld): 32 lanes, and 64 lanes = the last
    single pass of VEC 1"""
    ops = _ops()
    dim = 64
    rng = np.random.default_rng(300 + vec)
    T = _Tables(rng, dim, layout, dev)
    ratios = []
    for batch in _batches(dim, vec):
        for k, (idt, item_first) in enumerate(itertools.product((I32, I64), (1, 0))):
            u, i = T.ids(rng, batch)
            r, also = _embed_forward(ops, dev, T, u, i, idt, item_first, stash=(dim, 0) if k % 3 else None)
            assert also == vec
            ratios.append(r)
            _embed_backward(ops, dev, T, rng, u, i, idt, item_first, with_mlp=k % 3 != 1)
    _check_dot("dot neumf_embed_fwd", f"64 in {T.width}", ratios)


#           dim, ld, off, VEC: the stashes' row stride, then their base alignment, force the narrower vector on aligned tables
STASHES = [(64, 68, 0, 4), (64, 66, 0, 2), (64, 65, 0, 1), (64, 68, 2, 2), (64, 68, 1, 1), (64, 66, 1, 1), (256, 258, 0, 2), (128, 129, 0, 1), (128, 132, 3, 1)]


@pytest.mark.parametrize("dim,ld,off,vec", STASHES)
def test_embed_forward_stashes_that_force_a_narrower_vector(dev, dim, ld, off, vec):
    """(256 at VEC 2 and 128 at VEC 1 are 128 chunks: two full passes where float4 has one)"""
    ops = _ops()
    rng = np.random.default_rng(400 + ld + off)
    T = _Tables(rng, dim, "separate", dev)
    ratios = []
    for batch in _batches(dim, vec):
        for idt, item_first in ((I32, 1), (I64, 0)):
            u, i = T.ids(rng, batch)
            r, also = _embed_forward(ops, dev, T, u, i, idt, item_first, stash=(ld, off))
            assert also == vec
            ratios.append(r)
    _check_dot("dot neumf_embed_fwd", f"{dim} stash ld {ld} + {off}", ratios)


@pytest.mark.parametrize("dim", [64, 10, 75, 260])
@pytest.mark.parametrize("idt", [I32, I64])
def test_embed_backward_rows_by_id(dev, dim, idt):
    """out_rows_by_id: the gradient of pair b goes to row users[b] / items[b] of the outputs.  The ids are a permutation with two
    invalid ones per stream: nothing is written for those, and the rows no id names stay NaN."""
    ops = _ops()
    rng = np.random.default_rng(500 + dim)
    batch = R = 300
    uf, vf = _vals(rng, (R, dim)), _vals(rng, (R, dim))
    u, i = rng.permutation(R), rng.permutation(R)
    u[5], u[77], i[9], i[200] = -1, R + 3, R + 3, -1
    if idt == I64:
        u[78] = 2 ** 32 + 5
    uok, iok = (u >= 0) & (u < R), (i >= 0) & (i < R)
    dx0, g = _vals(rng, (batch, 2 * dim)), _vals(rng, batch)
    for item_first, ldg in ((1, dim), (0, dim + 3)):
        outs = [_nan(dev, R + 1, ldg) for _ in range(4)]         # user mlp, item mlp, user mf, item mf
        v = [o[:, :dim] for o in outs]
        ops.neumf_embed_backward(_td(dev, uf), _td(dev, vf), _td(dev, u).to(idt), _td(dev, i).to(idt), item_first, _td(dev, dx0), _td(dev, g),
                                 v[2], v[3], v[0], v[1], out_rows_by_id=True)
        uo, io = (dim, 0) if item_first else (0, dim)
        ufz, vfz = np.where(uok[:, None], uf[np.clip(u, 0, R - 1)], np.float32(0)), np.where(iok[:, None], vf[np.clip(i, 0, R - 1)], np.float32(0))
        exp = [(u[uok], dx0[uok, uo:uo + dim]), (i[iok], dx0[iok, io:io + dim]), (u[uok], (g[:, None] * vfz)[uok]), (i[iok], (g[:, None] * ufz)[iok])]
        for k in range(4):
            assert _written_exactly(outs[k].cpu().numpy(), [(exp[k][0], 0, exp[k][1])]), (k, item_first)


@pytest.mark.parametrize("dim", WIDTHS)
def test_mf_grad_inplace(dev, dim):
    """(u, i) -> (ddot * i, ddot * u) in place on the stashed MF rows, at every vector width the stashes' stride and base allow"""
    ops = _ops()
    rng = np.random.default_rng(600 + dim)
    for batch in _batches(dim):
        for ld, off in ((dim, 0), (dim + 4, 0), (dim + 2, 0), (dim + 1, 0), (dim + 4, 2), (dim + 4, 1)):
            uf, vf, g = _vals(rng, (batch, dim)), _vals(rng, (batch, dim)), _vals(rng, batch)
            fu, su = _strided(dev, batch + 1, dim, ld, off)
            fi, si = _strided(dev, batch + 1, dim, ld, off)
            su[:batch] = _td(dev, uf)
            si[:batch] = _td(dev, vf)
            ops.mf_grad_inplace(su[:batch], si[:batch], _td(dev, g))
            assert _flat_regions(fu, batch + 1, ld, off, g[:, None] * vf), (batch, ld, off)
            assert _flat_regions(fi, batch + 1, ld, off, g[:, None] * uf), (batch, ld, off)


# ------------------------------------------------------------------------------------------------------------ BPR
def _bpr_ref(eu, ep, en, inv_batch, depth):
    """float64 loss and gradients of the gathered float32 rows, and the relative bounds of the module docstring"""
    eu, ep, en = eu.astype(f64), ep.astype(f64), en.astype(f64)
    x = (eu * ep).sum(1) - (eu * en).sum(1)
    l = O.sigmoid(-x)
    dx = -O.sigmoid(x) * l * f64(inv_batch)
    ex = (depth + 1) * U24 * (np.abs(eu * ep).sum(1) + np.abs(eu * en).sum(1)) + U24 * np.abs(x)
    return dict(x=x, l=l, gu=dx[:, None] * (ep - en), gp=dx[:, None] * eu, gn=-dx[:, None] * eu,
                rel_l=np.expm1(ex) + 8 * U24, rel_g=2 * np.expm1(ex) + 17 * U24)


def _bpr_ratios(R, per, gu, gp, gn):
    """per-row |got - ref| in units of its bound: (loss, worst gradient element)"""
    rl = np.abs(per.astype(f64) - R["l"]) / (R["l"] * R["rel_l"] + TINY)
    rg = np.zeros_like(rl)
    for got, ref in ((gu, R["gu"]), (gp, R["gp"]), (gn, R["gn"])):
        rg = np.fmax(rg, (np.abs(got.astype(f64) - ref) / (np.abs(ref) * R["rel_g"][:, None] + TINY)).max(1))      # (NaN in got: checked by the caller)
    return rl, rg


PREFILL = 0.25 * (np.arange(64) + 1)        # BR_SUM_SLOTS known non-zero doubles


def _bpr_launch(ops, dev, ut, it, u, p, n, idt, inv_batch, flag=None):
    """-> per_triplet, g_user, g_pos, g_neg, what the launch added to each loss slot; rows and elements past the batch are still NaN"""
    batch, dim = len(u), ut.shape[1]
    loss = _td(dev, PREFILL.copy())
    gu, gi, per = _nan(dev, batch + 1, dim), _nan(dev, 2 * batch + 1, dim), _nan(dev, batch + 2)
    ops.bpr_forward_backward(_td(dev, ut), _td(dev, it), _td(dev, u).to(idt), _td(dev, p).to(idt), _td(dev, n).to(idt), inv_batch, loss,
                             gu[:batch], gi[:2 * batch], per_triplet=per[:batch], err_flag=flag)
    gu, gi, per = gu.cpu().numpy(), gi.cpu().numpy(), per.cpu().numpy()
    assert np.isnan(gu[batch:]).all() and np.isnan(gi[2 * batch:]).all() and np.isnan(per[batch:]).all()
    assert not (np.isnan(gu[:batch]).any() or np.isnan(gi[:2 * batch]).any() or np.isnan(per[:batch]).any())
    return per[:batch], gu[:batch], gi[:batch], gi[batch:2 * batch], loss.cpu().numpy() - PREFILL


def _loss_sum_ok(added, R, batch, dim):
    blocks = -(-batch // _rows_per_block(dim))
    want = R["l"].sum()
    bound = R["rel_l"].max() * want + batch * TINY + (blocks + batch) * 2.0 ** -52 * (PREFILL.max() + batch)      # (the double adds)
    untouched = blocks >= 64 or not added[blocks:].any()          # slot = workgroup & 63
    return untouched and abs(added.sum() - want) <= bound, (added.sum(), want, bound)


def _hard_triplets(rng, batch, dim):
    """tables in which every triplet has three rows of its own, the item rows rescaled so that the float64 margin is MARGINS[b % 23] with
    the two scores on either side of a common offset; -> float32 tables, ids, the margins asked for"""
    u = _vals(rng, (batch, dim)).astype(f64)
    rows = []
    for _ in range(2):
        e = np.abs(_vals(rng, (batch, dim))).astype(f64) * np.sign(u) * rng.choice([1.0, 1.0, 1.0, -1.0], (batch, dim))
        weak = np.abs((u * e).sum(1)) < 0.25 * np.abs(u * e).sum(1)
        e[weak] = np.abs(e[weak]) * np.sign(u[weak])              # a score too close to 0 to be rescaled: all terms positive
        rows.append(e)
    want = np.array([MARGINS[b % len(MARGINS)] for b in range(batch)])
    mid = rng.normal(0.0, 1.0, batch)
    for e, s in zip(rows, (mid + want / 2, mid - want / 2)):
        e *= (s / (u * e).sum(1))[:, None]
    uid, iid = rng.permutation(batch), rng.permutation(2 * batch)
    ut, it = np.empty((batch, dim), np.float32), np.empty((2 * batch, dim), np.float32)
    ut[uid], it[iid[:batch]], it[iid[batch:]] = u, rows[0], rows[1]
    return ut, it, uid, iid[:batch], iid[batch:], want


@pytest.mark.parametrize("dim", WIDTHS)
def test_bpr_on_hard_margins(dev, dim):
    """The kernel this test was written against formed l = 1 - s and dx = -s (1 - s) inv_batch and failed here at every width, from
    margin +5 (narrow rows, 1.2 - 2.3 of the loss bound) or +10 (27 - 160) on: 150 - 930 at +14, 2.7e4 - 2.2e5 at +16.5 .. +20 (1 - s is
    exactly 0 from 16.64 on: the error is the whole value).  With l = e r the worst case over all widths and margins is 0.23 of the loss
    bound and 0.20 of the gradient bound (profiles/row_kernels/row_kernels_errors.json)."""
    ops = _ops()
    rng = np.random.default_rng(700 + dim)
    worst, fails = {}, []
    for batch in _batches(dim):
        ut, it, u, p, n, want = _hard_triplets(rng, batch, dim)
        inv_batch = float(np.float32(1.0 / batch))
        R = _bpr_ref(ut[u], it[p], it[n], inv_batch, _depth(dim))
        assert (np.abs(R["x"] - want) <= 1e-4 * (1 + np.abs(want))).all()          # (the test's own inputs: the rounded tables keep the margins)
        for idt in (I32, I64):
            per, gu, gp, gn, added = _bpr_launch(ops, dev, ut, it, u, p, n, idt, inv_batch)
            rl, rg = _bpr_ratios(R, per, gu, gp, gn)
            for m in MARGINS[:batch]:
                sel = want == m
                w = worst.setdefault(f"{m:+g}", [0.0, 0.0])
                w[0], w[1] = max(w[0], float(rl[sel].max())), max(w[1], float(rg[sel].max()))
            ok, figures = _loss_sum_ok(added, R, batch, dim)
            if not ok:
                fails.append(f"loss_sum at batch {batch}: got, want, bound = {figures}")
    _record("bpr", str(dim), worst)
    fails += [f"margin {m}: loss {w[0]:.3g}, gradients {w[1]:.3g} of the bound" for m, w in worst.items() if not max(w) <= 1.0]
    assert not fails, f"dim {dim}: " + "; ".join(fails)


# ------------------------------------------------------------------------------------------------------------ ids out of range, the flag
def _bad_ids(rows, idt):
    return [rows + 3, -1] + ([2 ** 32 + 5] if idt == I64 else [])      # (the last must be flagged, not wrapped to row 5)


def _flag_cases(rows, idt):
    """(the id to plant or None, the flag on entry, the flag on exit): a capacity bit raised earlier stays"""
    for bad in [None] + _bad_ids(rows, idt):
        for before in (0, CAPACITY):
            yield bad, before, before | (RANGE if bad is not None else 0)


@pytest.mark.parametrize("idt", [I32, I64])
def test_ids_gather_rows(dev, idt):
    ops = _ops()
    rng = np.random.default_rng(800)
    dim, batch = 48, 300
    tabs = [_vals(rng, (97, dim)), _vals(rng, (53, dim))]
    for bad, before, after in _flag_cases(53, idt):
        ids = [rng.integers(0, t.shape[0], batch) for t in tabs]
        ref = [t[i].copy() for t, i in zip(tabs, ids)]
        if bad is not None:
            ids[1][123] = bad
            ref[1][123] = 0.0
        outs, flag = [_nan(dev, batch + 1, dim) for _ in tabs], _flag(dev, before)
        ops.gather_rows([_td(dev, t) for t in tabs], [_td(dev, i).to(idt) for i in ids], outs=[o[:batch] for o in outs], err_flag=flag)
        assert int(flag.item()) == after, (bad, before)
        for o, r in zip(outs, ref):
            assert _written_exactly(o.cpu().numpy(), [(None, 0, r)]), (bad, before)
    out, flag = _nan(dev, 4, dim), _flag(dev)
    ops.gather_rows([_td(dev, tabs[0])], [torch.empty(0, dtype=idt, device=dev)], outs=[out], err_flag=flag)      # batch 0
    assert int(flag.item()) == 0 and bool(torch.isnan(out).all())


@pytest.mark.parametrize("idt", [I32, I64])
def test_ids_embed_forward(dev, idt):
    ops = _ops()
    rng = np.random.default_rng(810)
    dim, batch = 48, 300
    T = _Tables(rng, dim, "fused", dev)
    for stream in (0, 1):
        for bad, before, after in _flag_cases(ROWS, idt):
            u, i = T.ids(rng, batch)
            if bad is not None:
                (u, i)[stream][211] = bad
            zero = [211] if bad is not None else []
            flag = _flag(dev, before)
            r, _ = _embed_forward(ops, dev, T, u, i, idt, stream, stash=(dim, 0), flag=flag, zero_user=zero if stream == 0 else (),
                                  zero_item=zero if stream == 1 else ())
            assert int(flag.item()) == after, (stream, bad, before)
            assert r <= 1.0, (stream, bad, r)
    # batch 0 through the C-ABI (the wrapper takes the batch from x0): nothing written, the flag stays 0
    lib = import_module("binary-recommendation_amd._lib").load()
    x0, dot, su, si, flag = _nan(dev, 4, 2 * dim), _nan(dev, 4), _nan(dev, 4, dim), _nan(dev, 4, dim), _flag(dev)
    ids = torch.zeros(4, dtype=idt, device=dev)
    P = lambda t: t.data_ptr()
    rc = lib.brNeumfEmbedForwardStash(P(T.d[0]), P(T.d[1]), P(T.d[2]), P(T.d[3]), 2 * dim, 2 * dim, ROWS, ROWS, P(ids), P(ids), 1 if idt == I64 else 0, dim, 0, 1,
                                      P(x0), P(dot), P(su), P(si), dim, P(flag), ops._stream())
    assert rc == 0 and int(flag.item()) == 0
    assert all(bool(torch.isnan(t).all()) for t in (x0, dot, su, si))


@pytest.mark.parametrize("dim", [48, 260])
@pytest.mark.parametrize("idt", [I32, I64])
def test_ids_bpr(dev, dim, idt):
    """each of the three id streams on its own: the bad row reads as zeros (in both passes of the two-pass form, dim 260)"""
    ops = _ops()
    rng = np.random.default_rng(820 + dim)
    batch, U, I = 300, 97, 53
    ut, it = (0.3 * _vals(rng, (U, dim))).astype(np.float32), (0.3 * _vals(rng, (I, dim))).astype(np.float32)
    inv_batch = float(np.float32(1.0 / batch))
    for stream in range(3):
        for bad, before, after in _flag_cases((U, I, I)[stream], idt):
            ids = [rng.integers(0, U, batch), rng.integers(0, I, batch), rng.integers(0, I, batch)]
            rows = [ut[ids[0]].copy(), it[ids[1]].copy(), it[ids[2]].copy()]
            if bad is not None:
                ids[stream][187] = bad
                rows[stream][187] = 0.0
            flag = _flag(dev, before)
            per, gu, gp, gn, added = _bpr_launch(ops, dev, ut, it, *ids, idt, inv_batch, flag=flag)
            assert int(flag.item()) == after, (stream, bad, before)
            R = _bpr_ref(*rows, inv_batch, _depth(dim))
            rl, rg = _bpr_ratios(R, per, gu, gp, gn)
            assert rl.max() <= 1.0 and rg.max() <= 1.0, (stream, bad, rl.max(), rg.max())
            ok, figures = _loss_sum_ok(added, R, batch, dim)
            assert ok, (stream, bad, figures)
    # batch 0 through the C-ABI (the wrapper takes the batch from the ids): nothing written, the flag stays 0
    lib = import_module("binary-recommendation_amd._lib").load()
    P = lambda t: t.data_ptr()
    ids = torch.zeros(4, dtype=idt, device=dev)
    per, gu, gi, loss, flag = _nan(dev, 4), _nan(dev, 4, dim), _nan(dev, 8, dim), _td(dev, PREFILL.copy()), _flag(dev)
    rc = lib.brBprForwardBackward(P(_td(dev, ut)), P(_td(dev, it)), U, I, P(ids), P(ids), P(ids), 1 if idt == I64 else 0, dim, 0, 1.0, P(per), P(loss), P(gu), P(gi),
                                  P(flag), ops._stream())
    assert rc == 0 and int(flag.item()) == 0 and np.array_equal(loss.cpu().numpy(), PREFILL)
    assert all(bool(torch.isnan(t).all()) for t in (per, gu, gi))


@pytest.mark.parametrize("idt", [I32, I64])
def test_ids_gather_rows_pair_seg(dev, idt):
    """the owner side of the row-sharded exchange: ids and rows in [peer][stream][cap] order, table a serves stream 0 and table b stream 1.
    It runs on the flag brShardDedupPlanPair raises the capacity bit on."""
    ops = _ops()
    rng = np.random.default_rng(830)
    dim, ld, W, cap = 48, 48, 3, 40
    tabs = [_vals(rng, (97, dim)), _vals(rng, (53, dim))]
    slots = W * 2 * cap
    stream = (np.arange(slots) // cap) % 2
    for bad, before, after in _flag_cases(53, idt):
        ids = np.where(stream == 0, rng.integers(0, 97, slots), rng.integers(0, 53, slots))
        ref = np.where((stream == 0)[:, None], tabs[0][np.clip(ids, 0, 96)], tabs[1][np.clip(ids, 0, 52)])
        if bad is not None:
            at = 3 * cap + 7                                        # peer 1, stream 1
            ids[at], ref[at] = bad, 0.0
        out, flag = _nan(dev, slots + 1, ld), _flag(dev, before)
        ops.gather_rows_pair_seg(_td(dev, tabs[0]), _td(dev, tabs[1]), _td(dev, ids).to(idt), out[:, :dim], W * cap, (cap, 2 * cap, 0, cap), err_flag=flag)
        assert int(flag.item()) == after, (bad, before)
        assert _written_exactly(out.cpu().numpy(), [(None, 0, ref.astype(np.float32))]), (bad, before)
    out, flag = _nan(dev, slots + 1, ld), _flag(dev)
    ops.gather_rows_pair_seg(_td(dev, tabs[0]), _td(dev, tabs[1]), _td(dev, ids).to(idt), out[:, :dim], 0, (cap, 2 * cap, 0, cap), err_flag=flag)
    assert int(flag.item()) == 0 and bool(torch.isnan(out).all())


@pytest.mark.parametrize("idt", [I32, I64])
def test_ids_gather_rows_deferred_row_group(dev, idt):
    """width 48 has no wave-per-row form.  A fresh step state (step 0) and last = 0: no row lags, the lookup returns the stored rows."""
    ops = _ops()
    rng = np.random.default_rng(840)
    dim, rows, batch = 48, 97, 300
    tab = _vals(rng, (rows, dim))
    th, m, v = _td(dev, tab), torch.zeros(rows, dim, device=dev), torch.zeros(rows, dim, device=dev)
    last, ss = torch.zeros(rows, dtype=torch.int32, device=dev), ops.new_step_state(dev)
    for bad, before, after in _flag_cases(rows, idt):
        ids = rng.integers(0, rows, batch)
        ref = tab[ids].copy()
        if bad is not None:
            ids[55], ref[55] = bad, 0.0
        out, flag = _nan(dev, batch + 1, dim), _flag(dev, before)
        ops.gather_rows_deferred(th, m, v, last, _td(dev, ids).to(idt), ss, out=out[:batch], err_flag=flag)
        assert int(flag.item()) == after, (bad, before)
        assert _written_exactly(out.cpu().numpy(), [(None, 0, ref)]), (bad, before)
    out, flag = _nan(dev, 4, dim), _flag(dev)
    ops.gather_rows_deferred(th, m, v, last, torch.empty(0, dtype=idt, device=dev), ss, out=out, err_flag=flag)
    assert int(flag.item()) == 0 and bool(torch.isnan(out).all())


@pytest.mark.parametrize("idt", [I32, I64])
def test_ids_scatter_add_rows(dev, idt):
    """distinct ids onto a table of ones: every touched element is the one fp32 sum 1 + x, bit for bit; the bad row is skipped"""
    ops = _ops()
    rng = np.random.default_rng(850)
    dim, rows, batch = 48, 97, 60
    one = np.ones((rows, dim), np.float32)
    for bad, before, after in _flag_cases(rows, idt):
        ids, x = rng.permutation(rows)[:batch], _vals(rng, (batch, dim))
        ref = one.copy()
        ref[ids] += x
        if bad is not None:
            ref[ids[31]] = 1.0
            ids[31] = bad
        g, flag = _td(dev, one), _flag(dev, before)
        ops.scatter_add_rows(g, _td(dev, ids).to(idt), _td(dev, x), err_flag=flag)
        assert int(flag.item()) == after, (bad, before)
        assert _same_bits(g.cpu().numpy(), ref), (bad, before)
    g, flag = _td(dev, one), _flag(dev)
    ops.scatter_add_rows(g, torch.empty(0, dtype=idt, device=dev), torch.empty(0, dim, device=dev), err_flag=flag)
    assert int(flag.item()) == 0 and _same_bits(g.cpu().numpy(), one)
