"""The float64 references of tests/pointops_refs.py against the CPU oracle (no GPU): on
in-range indices the forward references, rounded to fp32, equal the oracle bit for bit, and
the oracle's sequential fp32 scatter-adds lie within the references' own bound
(n + 1) * 2^-24 * S -- one summation order among those the bound covers.  The out-of-range
rule and the (n, S) bookkeeping are checked on hand-made cases."""
import numpy as np
import pytest

import pointops_refs as R
from oracle import oracle as O

I32_MIN = np.iinfo(np.int32).min


def _idx(rng, shape, n):
    """Random in-range indices with an all-equal row and a sorted row per batch element."""
    idx = rng.integers(0, n, shape).astype(np.int32)
    flat = idx.reshape(shape[0], -1)
    flat[0, :] = flat[0, 0]
    if shape[0] > 1:
        flat[1].sort()
    return idx


@pytest.mark.parametrize("B,C,N,M", [(3, 5, 37, 41), (1, 1, 1, 7), (2, 3, 9, 3001), (2, 4, 64, 64)])
def test_gather_refs_match_oracle(B, C, N, M):
    rng = np.random.default_rng(B * 100 + M)
    f = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = _idx(rng, (B, M), N)
    np.testing.assert_array_equal(R.gather(f, idx).astype(np.float32), O.gather_operation(f, idx))
    go = rng.standard_normal((B, C, M)).astype(np.float32)
    ref, n, S = R.gather_grad(go, idx, N)
    R.assert_grad(O.gather_operation_grad(go, idx, N), ref, n, S, "gather_grad")
    assert n.sum() == B * C * M


@pytest.mark.parametrize("B,C,N,S,K", [(3, 5, 37, 41, 3), (1, 1, 1, 7, 1), (2, 3, 9, 273, 11), (1, 2, 50, 625, 16)])
def test_group_refs_match_oracle(B, C, N, S, K):
    rng = np.random.default_rng(B * 100 + S + K)
    f = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = _idx(rng, (B, S, K), N)
    np.testing.assert_array_equal(R.group(f, idx).astype(np.float32), O.grouping_operation(f, idx))
    go = rng.standard_normal((B, C, S, K)).astype(np.float32)
    ref, n, Sm = R.group_grad(go, idx, N)
    R.assert_grad(O.grouping_operation_grad(go, idx, N), ref, n, Sm, "group_grad")


@pytest.mark.parametrize("B,C,M,N", [(2, 5, 37, 41), (1, 1, 1, 7), (2, 3, 9, 3001), (2, 7, 300, 255)])
def test_three_interpolate_refs_match_oracle(B, C, M, N):
    rng = np.random.default_rng(B * 100 + M + N)
    f = rng.standard_normal((B, C, M)).astype(np.float32)
    idx = _idx(rng, (B, N, 3), M)
    w = rng.random((B, N, 3)).astype(np.float32)
    np.testing.assert_array_equal(R.three_interpolate(f, idx, w).astype(np.float32), O.three_interpolate(f, idx, w))
    go = rng.standard_normal((B, C, N)).astype(np.float32)
    ref, n, S = R.three_interpolate_grad(go, idx, w, M)
    R.assert_grad(O.three_interpolate_grad(go, idx, w, M), ref, n, S, "three_interpolate_grad")
    assert n.sum() == B * C * N * 3


def test_out_of_range_counts_as_zero():
    f = np.array([[[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]]], np.float32)            # (1,2,3)
    idx = np.array([[2, -1, 3, I32_MIN, 0, 2]], np.int32)
    np.testing.assert_array_equal(R.gather(f, idx), [[[4, 0, 0, 0, 1, 4], [32, 0, 0, 0, 8, 32]]])
    np.testing.assert_array_equal(R.group(f, idx.reshape(1, 2, 3)).reshape(1, 2, 6), R.gather(f, idx))
    go = np.array([[[1, 10, 100, 1000, -3, 0.5], [2, 20, 200, 2000, 7, -7]]], np.float32)
    ref, n, S = R.gather_grad(go, idx, 3)
    np.testing.assert_array_equal(ref, [[[-3, 0, 1.5], [7, 0, -5]]])
    np.testing.assert_array_equal(n, [[[1, 0, 2], [1, 0, 2]]])
    np.testing.assert_array_equal(S, [[[3, 0, 1.5], [7, 0, 9]]])
    # three_interpolate: the out-of-range neighbour drops out of the sum and of the gradient
    i3 = np.array([[[0, 5, 2], [-1, I32_MIN, 3]]], np.int32)                     # (1,2,3), M = 3
    w = np.array([[[0.5, 0.25, 2.0], [1.0, 1.0, 1.0]]], np.float32)
    np.testing.assert_array_equal(R.three_interpolate(f, i3, w), [[[8.5, 0], [68, 0]]])
    g = np.array([[[2.0, 9.0], [4.0, 9.0]]], np.float32)
    ref, n, S = R.three_interpolate_grad(g, i3, w, 3)
    np.testing.assert_array_equal(ref, [[[1, 0, 4], [2, 0, 8]]])
    np.testing.assert_array_equal(n, [[[1, 0, 1], [1, 0, 1]]])
    # an empty source (n = 0): every index is out of range
    assert not R.gather(np.zeros((1, 2, 0), np.float32), idx).any()


def test_bound_is_tight_enough_to_catch_a_dropped_term():
    """One dropped or doubled term of a many-term sum must exceed the bound (the terms are
    O(1), the bound O(n * 2^-24)), and exact zeros are demanded where nothing was added."""
    rng = np.random.default_rng(9)
    go = (rng.random((1, 1, 1000)) + 0.5).astype(np.float32)
    idx = np.zeros((1, 1000), np.int32)
    ref, n, S = R.gather_grad(go, idx, 2)
    good = np.array([[[np.float32(ref[0, 0, 0]), 0.0]]], np.float32)
    R.assert_grad(good, ref, n, S)
    for bad in (good - np.float32([go[0, 0, 17], 0]), good + np.float32([go[0, 0, 3], 0]), good + np.float32([0, 1e-30])):
        with pytest.raises(AssertionError):
            R.assert_grad(bad.astype(np.float32), ref, n, S)
