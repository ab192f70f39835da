"""Counted Chamfer (clouds of unequal size in one padded batch) without a GPU:

  * the float64 restatements of tests/chamfer_counts_refs.py (oracle Chamfer per slice, then the
    reference's loss / metric formulas) against tests/golden/chamfer_counts.npz -- the reference's own
    code at B = 1 on every truncated pair -- at tests/test_loss_golden.py's bar, atol 1e-5 / rtol 0;
  * the new C-ABI symbols: declared in include/pcops.h, bound in _lib.py, exported by libpcops.so;
  * their status codes, which are decided before any device call: B == 0 is ok, a negative size is
    invalid, both counts NULL is invalid (as pcops_furthest_point_sampling_counts).
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_counts_refs as R  # noqa: E402

ATOL = 1e-5
NEW_SYMBOLS = ("pcops_chamfer_forward_counts", "pcops_chamfer_backward_counts", "pcops_chamfer_counts_means",
               "pcops_chamfer_counts_mean_grad", "pcops_completion_metrics_counts")


@pytest.fixture(scope="module")
def restated():
    a, b = R.golden_case()
    c1, c2 = R.GOLDEN_COUNTS1, R.GOLDEN_COUNTS2
    fwd = R.forward_counts(a, b, c1, c2)
    return a, b, c1, c2, fwd


def test_golden_case_shape():
    a, b = R.golden_case()
    assert a.shape == (4, 600, 3) and b.shape == (4, 520, 3)
    assert R.GOLDEN_COUNTS1 == (600, 257, 33, 1) and R.GOLDEN_COUNTS2 == (1, 520, 512, 100)


def test_forward_restatement_pads_with_zeros(restated):
    a, b, c1, c2, (d1, d2, i1, i2) = restated
    for k in range(4):
        assert not d1[k, c1[k]:].any() and not i1[k, c1[k]:].any()
        assert not d2[k, c2[k]:].any() and not i2[k, c2[k]:].any()
        assert i1[k, :c1[k]].max() < c2[k] and i2[k, :c2[k]].max() < c1[k]
    # truncation changes the answer: the full-size search is not the counted one
    from oracle import oracle as O

    full = O.chamfer_forward(a, b)
    assert not np.array_equal(full[0][1, :c1[1]], d1[1, :c1[1]]) or not np.array_equal(full[1][1], d2[1])


@pytest.mark.parametrize("key,root,both", [("sqrt", True, True), ("l2", False, True), ("ss_sqrt", True, False),
                                           ("ss_l2", False, False)])
def test_loss_restatement_meets_golden(restated, key, root, both):
    _, _, c1, c2, (d1, d2, _, _) = restated
    got = R.loss_counts(d1, d2, c1, c2, root=root, both=both)
    np.testing.assert_allclose(got, golden("chamfer_counts.npz")[key], rtol=0, atol=ATOL, err_msg=key)


def test_partial_matching_restatement_meets_golden(restated):
    """get_loss_PM's term: the counted first cloud against the FULL second cloud."""
    a, b, c1, _, _ = restated
    d1, d2, _, _ = R.forward_counts(a, b, c1, None)
    ref = golden("chamfer_counts.npz")
    np.testing.assert_allclose(R.loss_counts(d1, d2, c1, None, True, False), ref["pm_sqrt"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(R.loss_counts(d1, d2, c1, None, False, False), ref["pm_l2"], rtol=0, atol=ATOL)


def test_metrics_restatement_meets_golden(restated):
    _, _, c1, c2, (d1, d2, i1, i2) = restated
    ref = golden("chamfer_counts.npz")
    r = R.metrics_counts(d1, d2, i1, i2, c1, c2)
    for key in ("cd_p", "cd_t", "f1"):
        np.testing.assert_allclose(r[key], ref[key], rtol=0, atol=ATOL, err_msg=key)
    for row, key in enumerate(("dcd", "cd_p", "cd_t")):
        np.testing.assert_allclose(r[key], ref["dcd"][row], rtol=0, atol=ATOL, err_msg=f"dcd {key}")
    rn = R.metrics_counts(d1, d2, i1, i2, c1, c2, non_reg=True)
    for row, key in enumerate(("dcd", "cd_p", "cd_t")):
        np.testing.assert_allclose(rn[key], ref["dcd_nonreg"][row], rtol=0, atol=ATOL, err_msg=f"dcd_nonreg {key}")


def test_restatements_empty_side():
    a, b = R.golden_case()
    c1, c2 = [600, 0, 5, 7], [0, 520, 9, 3]
    d1, d2, i1, i2 = R.forward_counts(a, b, c1, c2)
    assert not d1[:2].any() and not d2[:2].any() and not i1[:2].any() and not i2[:2].any()
    r = R.metrics_counts(d1, d2, i1, i2, c1, c2)
    assert all(np.isnan(r[k][:2]).all() and np.isfinite(r[k][2:]).all() for k in R.FIELDS)
    assert not R.loss_counts(d1, d2, c1, c2)[:2].any()
    g1, g2 = R.backward_counts(a, b, c1, c2, np.full_like(d1, np.nan), np.full_like(d2, np.nan), i1, i2)
    assert not g1[:2].any() and not g2[:2].any() and not g1[2, 5:].any() and not g2[3, 3:].any()


def test_new_symbols_declared_bound_and_exported():
    from svdformer_pointsea_amd import _lib

    src = open(os.path.join(ROOT, "include", "pcops.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pcops_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(L, name), name
    assert _lib.lib().pcops_abi_version() == 2


def test_cpu_tensors_with_counts_raise():
    import torch

    from svdformer_pointsea_amd import metrics as M
    from svdformer_pointsea_amd.chamfer3D import chamfer_3DDist, chamfer_forward_raw

    a, b, c = torch.zeros(2, 8, 3), torch.ones(2, 5, 3), torch.tensor([8, 3], dtype=torch.int32)
    for call in (lambda: chamfer_forward_raw(a, b, c, None), lambda: chamfer_3DDist()(a, b, counts2=c),
                 lambda: M.chamfer(a, b, c), lambda: M.chamfer_sqrt(a, b, counts2=c),
                 lambda: M.chamfer_single_side(a, b, c), lambda: M.chamfer_single_side_sqrt(a, b, c),
                 lambda: M.completion_metrics(b, a, gt_counts=c),
                 lambda: M.get_loss_PM((b, b, b), a, a, partial_counts=c)):
        with pytest.raises(RuntimeError):
            call()


def test_status_codes_without_gpu():
    from svdformer_pointsea_amd import _lib

    L = _lib.lib()
    n, one = ctypes.c_void_p(0), ctypes.c_void_p(8)   # `one`: a non-null pointer that is never dereferenced
    OK, INVALID = 0, 1
    fwd = lambda c1, c2, B, N, M: L.pcops_chamfer_forward_counts(one, one, c1, c2, B, N, M, one, one, one, one, n)
    bwd = lambda c1, c2, B, N, M: L.pcops_chamfer_backward_counts(one, one, c1, c2, B, N, M, one, one, one, one, one,
                                                                  one, n)
    means = lambda c1, c2, B, N, M: L.pcops_chamfer_counts_means(one, one, c1, c2, B, N, M, one, n)
    grad = lambda c1, c2, B, N, M: L.pcops_chamfer_counts_mean_grad(one, 0.5, one, one, c1, c2, B, N, M, 1, 1, one,
                                                                    one, n)
    met = lambda c1, c2, B, N, M: L.pcops_completion_metrics_counts(one, one, one, one, c1, c2, B, N, M, 1e-4, 1000.0,
                                                                    0, one, n, 0, n)
    for name, fn in (("forward", fwd), ("backward", bwd), ("means", means), ("mean_grad", grad), ("metrics", met)):
        assert fn(one, one, 0, 16, 16) == OK, name
        assert fn(n, n, 0, 16, 16) == OK, name              # B == 0 comes first
        assert fn(one, one, -1, 16, 16) == INVALID, name
        assert fn(one, one, 2, -1, 16) == INVALID, name
        assert fn(one, one, 2, 16, -3) == INVALID, name
        assert fn(n, n, 2, 16, 16) == INVALID, name         # both counts NULL
