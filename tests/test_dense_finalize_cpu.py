"""-m "not gpu": what tests/test_gpu_dense_finalize.py takes for granted about its own inputs and arithmetic, checked without a GPU - the
synthetic layout is a partition, no single-slab omission fits inside the derived bound, the float32 restatement of the summation
order itself meets that bound, and the P written into each whole-step case is what the launch arithmetic gives."""
from importlib import import_module

import numpy as np

F = import_module("tests.test_gpu_dense_finalize")


def test_layout_is_an_inconvenient_partition():
    assert np.array_equal(F.layout_cover(), np.ones(F.N, np.int64))
    assert F.N % 64 and all(e % 64 for e in F.ELEMS) and F.BN_N == (33, 1)
    assert F.GRAD_OFF[2] < F.GRAD_OFF[0]                                              # offsets are not monotonic
    assert F.GRAD_OFF[2] + F.ELEMS[2] <= F.DGAMMA_OFF[0] < F.GRAD_OFF[0] < 64         # workgroup 0: region 2, a BatchNorm range, region 0
    assert {c for t in F.SLAB_COUNTS for c in t} == F.ALL_COUNTS
    assert any(min(t) < 16 and max(t) > 64 for t in F.SLAB_COUNTS)
    assert all(t[2] != t[0] for t in F.SLAB_COUNTS)                                   # ... with different slab counts


def test_no_single_slab_mistake_fits_inside_the_bound():
    for counts in F.SLAB_COUNTS:
        for S in F.slab_inputs(counts):
            a = np.abs(S)
            assert S.dtype == np.float32 and (S > 0).any() and (S < 0).any() and a.max() / a.min() <= 100.0
            assert F.omission_margin(S) > 10.0, counts
            # said once more without the helper: drop / repeat slab s, every element moves by more than 10 bounds
            full, bound = S.astype(np.float64).sum(0), F.slab_bound(S)
            for s in {0, S.shape[0] // 2, S.shape[0] - 1}:
                without = np.delete(S, s, axis=0).astype(np.float64).sum(0)
                assert np.all(np.abs(full - without) > 10 * bound) and np.all(np.abs(full + S[s] - full) > 10 * bound)


def test_stated_order_meets_the_derived_bound():
    """the bound is on the order, not on the GPU: its float32 restatement on the CPU stays inside it (and is not the float64 sum)"""
    exact = 0
    for counts in F.SLAB_COUNTS:
        for S in F.slab_inputs(counts):
            got, ref = F.reduce_in_kernel_order(S), S.astype(np.float64).sum(0)
            assert np.all(np.abs(got - ref) <= F.slab_bound(S))
            exact += int(np.all(got == ref.astype(np.float32)))
    assert exact < 3 * len(F.SLAB_COUNTS)      # long sums round differently from float64: the bit comparison says something
    assert F.chain_depth(1) == 16 and F.chain_depth(16) == 16 and F.chain_depth(17) == 17 and F.chain_depth(129) == 24


def test_bn_reference_rounds_once():
    s = F.bn_inputs(1)[0]
    dgamma, dbeta = F.bn_grads_ref(s)
    n = F.BN_N[0]
    assert dgamma.dtype == dbeta.dtype == np.float32 and dgamma.shape == dbeta.shape == (n,)
    np.testing.assert_allclose(dbeta, s[:, :n].sum(0), rtol=1e-7)
    np.testing.assert_allclose(dgamma, s[:, n:].sum(0), rtol=1e-7)
    assert not F.bn_inputs(1)[1].any() and not F.bn_inputs(0)[0].any()


def test_rider_map_of_the_cases():
    F.test_cases_reach_every_branch_of_the_rider_map()
    assert [F.rider_map(32, B, B)[0] for B in (64, 4096, 8192)] == [1, 2, 3]
    assert len({c.id for c in F.CASES}) == len(F.CASES) and all(max(c.batches) <= 8192 for c in F.CASES)
