"""Counted Chamfer on the GPU: clouds of unequal size in one padded batch (csrc/chamfer.hip
pcops_chamfer_forward_counts / _backward_counts / _counts_means / _counts_mean_grad, csrc/metrics.hip
pcops_completion_metrics_counts) and the Python layers above them.

References: the CPU oracle per slice (bit-equal forward; backward at rtol 1e-5 / atol 1e-6, the bar of
tests/test_gpu_pointops.py), tests/golden/chamfer_counts.npz (the reference's loss code at B = 1 on every
truncated pair, atol 1e-5), the *_counts_chain functions (a loop of B = 1 calls of the uniform path) and the
float64 restatements of tests/chamfer_counts_refs.py.  Absent rows are filled with NaN in half the cases
and with zeros in the other half; the zero-padded cases hold valid points next to the origin, which a
search that read the padding would hand to the zero rows.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_counts_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

ATOL_GOLDEN = 1e-5


def _M():
    from svdformer_pointsea_amd import metrics as M

    return M


def _raw(a, b, c1, c2):
    from svdformer_pointsea_amd.chamfer3D import chamfer_forward_raw

    return chamfer_forward_raw(a, b, c1, c2)


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def C(counts, dev):
    return None if counts is None else torch.tensor(list(counts), dtype=torch.int32, device=dev)


def _pad(x, counts, pad):
    """rows k >= counts[b] of x[b] overwritten: NaN or zeros."""
    x = x.copy()
    for k, c in enumerate(R.clamp_counts(counts, x.shape[0], x.shape[1])):
        x[k, c:] = np.nan if pad == "nan" else 0.0
    return x


def _clouds(rng, B, N, M, c1, c2, pad):
    """Two random clouds; a handful of valid points of each lie within 1e-3 of the origin (the zero
    rows' position); then the padding; then, past each count, a copy of the cloud's last valid point
    (a duplicate straddling the boundary) and a copy of the other cloud's first point (distance 0 to
    a valid query, if it were read)."""
    a = (rng.random((B, N, 3)) - 0.5).astype(np.float32)
    b = (rng.random((B, M, 3)) - 0.5).astype(np.float32)
    a[:, :3] = (1e-3 * rng.standard_normal((B, 3, 3))).astype(np.float32)
    b[:, 1:3] = (1e-3 * rng.standard_normal((B, 2, 3))).astype(np.float32)
    a0, b0 = a[:, 0].copy(), b[:, 0].copy()
    a, b = _pad(a, c1, pad), _pad(b, c2, pad)
    for x, cs, other in ((a, R.clamp_counts(c1, B, N), b0), (b, R.clamp_counts(c2, B, M), a0)):
        for k, c in enumerate(cs):
            if 0 < c < x.shape[1]:
                x[k, c] = x[k, c - 1]
            if c + 1 < x.shape[1]:
                x[k, c + 1] = other[k]
    return a, b


def _assert_forward(got, a, b, c1, c2):
    ref = R.forward_counts(a, b, c1, c2)
    for name, x, y in zip(("dist1", "dist2", "idx1", "idx2"), got, ref):
        np.testing.assert_array_equal(x.cpu().numpy(), y, err_msg=name)   # padding: exactly (0, 0)


SIZES = [31, 32, 33, 511, 512, 513, 1023, 1024, 1025]


@pytest.mark.parametrize("pad", ["nan", "zero"])
def test_forward_boundaries_bitexact(dev, pad):
    """Counts across the 32-target sub-tile, the 512 reference chunk, the 1024-point LDS tile and the
    256-thread block, in opposite orders on the two sides."""
    B, N, M = 9, 1100, 1056
    c1, c2 = SIZES, [min(c, M) for c in reversed(SIZES)]
    a, b = _clouds(np.random.default_rng(3), B, N, M, c1, c2, pad)
    _assert_forward(_raw(T(a, dev), T(b, dev), C(c1, dev), C(c2, dev)), a, b, c1, c2)


@pytest.mark.parametrize("pad", ["nan", "zero"])
def test_forward_full_single_and_empty(dev, pad):
    B, N, M = 3, 300, 200
    c1, c2 = [N, 1, 0], [0, M, 1]
    a, b = _clouds(np.random.default_rng(4), B, N, M, c1, c2, pad)
    got = _raw(T(a, dev), T(b, dev), C(c1, dev), C(c2, dev))
    _assert_forward(got, a, b, c1, c2)
    assert not got[0][0].any() and not got[1][0].any() and not got[0][2].any() and not got[1][2].any()


VARIANTS = [{"PCOPS_CHAMFER_Q": "1"}, {"PCOPS_CHAMFER_Q": "2"}, {"PCOPS_CHAMFER_Q": "4"},
            {"PCOPS_CHAMFER_SCREEN": "0"}, {"PCOPS_CHAMFER_SCREEN": "0", "PCOPS_CHAMFER_Q": "2"},
            {"PCOPS_CHAMFER_SCREEN": "0", "PCOPS_CHAMFER_Q": "4"}, {"PCOPS_CHAMFER_SCREEN": "0", "PCOPS_CHAMFER_Q": "8"}]


@pytest.mark.parametrize("n", range(len(VARIANTS)))
def test_forward_every_variant_bitexact(dev, monkeypatch, n):
    """The screened kernel at 1 / 2 / 4 queries per lane and the direct kernel at 1 / 2 / 4 / 8: every
    search the counted entry can dispatch to (it has no MFMA and no culled form)."""
    for k, v in VARIANTS[n].items():
        monkeypatch.setenv(k, v)
    B, N, M = 3, 2500, 1300
    c1, c2 = [2500, 1025, 700], [1300, 33, 1290]
    pad = "nan" if n % 2 else "zero"
    a, b = _clouds(np.random.default_rng(10 + n), B, N, M, c1, c2, pad)
    a[0, 100:400] = a[0, 1100:1400]   # exact ties across sub-tiles and tiles
    b[2, 600:700] = b[2, 0:100]
    _assert_forward(_raw(T(a, dev), T(b, dev), C(c1, dev), C(c2, dev)), a, b, c1, c2)


@pytest.mark.parametrize("kernel", [{}, {"PCOPS_CHAMFER_Q": "4"}, {"PCOPS_CHAMFER_SCREEN": "0"}])
def test_forward_nonfinite_scan_order(dev, monkeypatch, kernel):
    """A VALID NaN coordinate on a chunk-start target (index 512c below the count) pins (NaN, 0) for c = 0
    and hides chunk c otherwise, as tests/test_gpu_pointops.py::test_chamfer_nonfinite_scan_order requires
    of the uniform entry; the same values past the count do nothing."""
    for k, v in kernel.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(23)
    B, N, M = 3, 700, 1100
    c1, c2 = [700, 650, 600], [1100, 600, 500]
    a = _pad((rng.random((B, N, 3)) - 0.5).astype(np.float32), c1, "zero")
    b = _pad((rng.random((B, M, 3)) - 0.5).astype(np.float32), c2, "zero")
    b[0, 512, 0] = np.nan           # valid chunk start, c = 1
    b[0, 1024, 2] = np.inf
    a[0, 3] = [np.inf, 0.0, 0.0]
    b[1, 0, 1] = np.nan             # valid chunk start, c = 0
    a[1, 512, 2] = np.nan           # valid (512 < 650)
    b[2, 512, 1] = np.nan           # absent (512 >= 500): no effect
    a[2, 5, 1] = np.nan
    got = _raw(T(a, dev), T(b, dev), C(c1, dev), C(c2, dev))
    _assert_forward(got, a, b, c1, c2)
    assert torch.isnan(got[0][1, :650]).all() and torch.isfinite(got[1][2, :500]).all()


def test_forward_padding_content_and_full_counts(dev):
    B, N, M = 4, 1300, 900
    c1, c2 = [1300, 513, 40, 1024], [900, 900, 257, 31]
    rng = np.random.default_rng(6)
    a, b = _clouds(rng, B, N, M, c1, c2, "nan")
    outs = [_raw(T(x, dev), T(y, dev), C(c1, dev), C(c2, dev))
            for x, y in ((a, b), (_pad(a, c1, "zero"), _pad(b, c2, "zero")),
                         (np.where(np.isnan(a), np.float32(np.inf), a), np.where(np.isnan(b), np.float32(7.0), b)))]
    for other in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(outs[0], other))
    # one side counted, the other full (a null counts pointer)
    _assert_forward(_raw(T(a, dev), T(_pad(b, None, "nan"), dev), C(c1, dev), None), a, b, c1, None)
    # full counts: the uniform call's outputs
    fa, fb = T(_pad(a, c1, "zero"), dev), T(_pad(b, c2, "zero"), dev)
    full = _raw(fa, fb, C([N] * B, dev), C([M + 5] * B, dev))   # a count above M clamps to M
    assert all(torch.equal(x, y) for x, y in zip(full, _raw(fa, fb, None, None)))


# ------------------------------------------------------------------ backward
@pytest.fixture(scope="module")
def bwd_case(dev):
    B, N, M = 3, 2100, 600   # 2100 targets: more than one 2048-target block
    c1, c2 = [2100, 2049, 5], [600, 1, 513]
    rng = np.random.default_rng(8)
    a, b = _clouds(rng, B, N, M, c1, c2, "nan")
    gd1, gd2 = rng.standard_normal((B, N)).astype(np.float32), rng.standard_normal((B, M)).astype(np.float32)
    d1, d2, i1, i2 = R.forward_counts(a, b, c1, c2)
    ref = R.backward_counts(a, b, c1, c2, gd1, gd2, i1, i2)
    return a, b, c1, c2, _pad(gd1, c1, "nan"), _pad(gd2, c2, "nan"), ref   # NaN gradient on absent rows


def _run_bwd(dev, a, b, c1, c2, gd1, gd2):
    from svdformer_pointsea_amd.chamfer3D import chamfer_3DDist

    at, bt = T(a, dev).requires_grad_(True), T(b, dev).requires_grad_(True)
    d1, d2, _, _ = chamfer_3DDist()(at, bt, C(c1, dev), C(c2, dev))
    return torch.autograd.grad((d1, d2), (at, bt), (T(gd1, dev), T(gd2, dev)))


def test_backward_against_oracle(dev, bwd_case):
    a, b, c1, c2, gd1, gd2, ref = bwd_case
    g1, g2 = _run_bwd(dev, a, b, c1, c2, gd1, gd2)
    for got, want, cs in ((g1, ref[0], c1), (g2, ref[1], c2)):
        got = got.cpu().numpy()
        err = np.abs(got - want)
        print("max abs err", float(err.max()))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
        for k, c in enumerate(cs):
            assert not got[k, c:].any()   # absent rows: exactly zero


def test_backward_reproducible_and_padding_independent(dev, bwd_case):
    a, b, c1, c2, gd1, gd2, _ = bwd_case
    first = _run_bwd(dev, a, b, c1, c2, gd1, gd2)
    again = _run_bwd(dev, a, b, c1, c2, gd1, gd2)
    zeros = _run_bwd(dev, _pad(a, c1, "zero"), _pad(b, c2, "zero"), c1, c2, _pad(gd1, c1, "zero") + 0,
                     np.where(np.isnan(gd2), np.float32(np.inf), gd2))
    for x, y, z in zip(first, again, zeros):
        assert torch.equal(x, y) and torch.equal(x, z)


# ------------------------------------------------------------------ losses
@pytest.fixture(scope="module")
def gcase(dev):
    a, b = R.golden_case()
    c1, c2 = R.GOLDEN_COUNTS1, R.GOLDEN_COUNTS2
    return T(_pad(a, c1, "nan"), dev), T(_pad(b, c2, "zero"), dev), C(c1, dev), C(c2, dev)


LOSSES = [("chamfer_sqrt", "sqrt"), ("chamfer", "l2"), ("chamfer_single_side_sqrt", "ss_sqrt"),
          ("chamfer_single_side", "ss_l2")]


@pytest.mark.parametrize("fn,key", LOSSES)
def test_loss_golden_and_chain(dev, gcase, fn, key):
    """Value: the reference's own code per truncated pair (golden); value and both gradients: the
    *_counts_chain of B = 1 uniform calls.  Gradients taken on the first cloud only and on the second only."""
    M = _M()
    a, b, c1, c2 = gcase
    at, bt = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss = getattr(M, fn)(at, bt, c1, c2)
    want = float(golden("chamfer_counts.npz")[key].mean())
    print(fn, "loss", float(loss.detach()), "golden", want)
    assert abs(float(loss.detach()) - want) <= ATOL_GOLDEN
    ac = torch.nan_to_num(a).requires_grad_(True)   # the chain multiplies sliced-away rows by 0: keep them finite
    bc = b.clone().requires_grad_(True)
    chain = getattr(M, fn + "_counts_chain")(ac, bc, c1, c2)
    torch.testing.assert_close(loss.detach(), chain.detach(), rtol=1e-5, atol=1e-6)
    (g1,) = torch.autograd.grad(loss, at, retain_graph=True)
    (h1,) = torch.autograd.grad(chain, ac, retain_graph=True)
    torch.testing.assert_close(g1, h1, rtol=1e-5, atol=1e-6)
    if "single_side" in fn:
        (g2,) = torch.autograd.grad(loss, bt)
        (h2,) = torch.autograd.grad(chain, bc)
        torch.testing.assert_close(g2, h2, rtol=1e-5, atol=1e-6)
    else:
        (g2,) = torch.autograd.grad(getattr(M, fn)(a, bt, c1, c2), bt)   # second cloud only: a takes no gradient
        (h2,) = torch.autograd.grad(chain, bc)
        torch.testing.assert_close(g2, h2, rtol=1e-5, atol=1e-6)
    for g, c in ((g1, R.GOLDEN_COUNTS1), (g2, R.GOLDEN_COUNTS2)):
        assert all(not g[k, n:].any() for k, n in enumerate(c))
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()


def test_loss_switch_runs_the_chain(dev, gcase, monkeypatch):
    M = _M()
    a, b, c1, c2 = gcase
    a = torch.nan_to_num(a)
    on = M.chamfer_sqrt(a, b, c1, c2)
    monkeypatch.setenv("PCOPS_LOSS_FUSED", "0")
    off = M.chamfer_sqrt(a, b, c1, c2)
    assert torch.equal(off, M.chamfer_sqrt_counts_chain(a, b, c1, c2))
    torch.testing.assert_close(on, off, rtol=1e-5, atol=1e-6)


def test_loss_empty_side_and_one_sided_counts(dev):
    M = _M()
    a, b = R.golden_case()
    c1 = [600, 0, 17, 600]
    at, bt = T(_pad(a, c1, "nan"), dev).requires_grad_(True), T(b, dev).requires_grad_(True)
    loss = M.chamfer_sqrt(at, bt, counts1=C(c1, dev))
    d1, d2, _, _ = R.forward_counts(a, b, c1, None)
    want = R.loss_counts(d1, d2, c1, None).mean()
    assert abs(float(loss) - want) <= ATOL_GOLDEN
    g1, g2 = torch.autograd.grad(loss, (at, bt))
    assert not g1[1].any() and not g2[1].any() and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    assert g2[0].any() and g1[2, :17].any() and not g1[2, 17:].any()


@pytest.mark.parametrize("sqrt", [True, False])
def test_get_loss_pm_partial_counts(dev, gcase, sqrt):
    """The partial-matching term against the counted partial: get_loss_PM - get_loss is the mean over b of the
    reference's single-sided loss of partial[b, :c] against the whole fine2 cloud."""
    M = _M()
    partial, _, c1, _ = gcase
    fine2 = T(R.golden_case()[1], dev)   # the prediction is not counted: all 520 rows
    pred =(fine2[:, :64].contiguous(), fine2[:, :256].contiguous(), fine2)
    gt = torch.nan_to_num(partial) * 0.5 + 0.1
    tot_pm, parts_pm = M.get_loss_PM(pred, partial, gt, sqrt=sqrt, partial_counts=c1)
    tot, parts = M.get_loss(pred, gt, sqrt=sqrt)
    want = float(golden("chamfer_counts.npz")["pm_sqrt" if sqrt else "pm_l2"].mean())
    print("pm", float(tot_pm - tot), "golden", want)
    assert abs(float(tot_pm - tot) - want) <= ATOL_GOLDEN
    assert all(torch.equal(x, y) for x, y in zip(parts_pm, parts))


# ------------------------------------------------------------------ metrics
def _check_metrics(dev, gt, x, cg, cx, non_reg=False):
    """Counted rows against the float64 restatement per slice (rtol 1e-5, atol 1e-6 on t1 / t2 / dcd, as
    tests/test_gpu_completion_metrics.py::_check_raw); p1 / p2 / f1 bitwise equal to metrics.fscore on the slice."""
    M = _M()
    d1, d2, i1, i2 = _raw(gt, x, C(cg, dev), C(cx, dev))
    res = M.completion_metrics_raw(d1, d2, i1, i2, non_reg=non_reg, counts1=C(cg, dev), counts2=C(cx, dev))
    ref = R.metrics_counts(d1.cpu().numpy(), d2.cpu().numpy(), i1.cpu().numpy(), i2.cpu().numpy(), cg, cx,
                           non_reg=non_reg)
    for k in R.FIELDS:
        atol = 1e-6 if k in ("t1", "t2", "dcd") else 0.0
        np.testing.assert_allclose(getattr(res, k).cpu().numpy(), ref[k], rtol=1e-5, atol=atol, equal_nan=True,
                                   err_msg=k)
    B = gt.shape[0]
    for k, (n, m) in enumerate(zip(R.clamp_counts(cg, B, gt.shape[1]), R.clamp_counts(cx, B, x.shape[1]))):
        if n == 0 or m == 0:
            assert all(torch.isnan(getattr(res, f)[k]) for f in R.FIELDS)   # the empty-side row is NaN
            continue
        f1, p1, p2 = M.fscore(d1[k:k + 1, :n], d2[k:k + 1, :m])
        assert torch.equal(res.p1[k:k + 1], p1) and torch.equal(res.p2[k:k + 1], p2) and torch.equal(res.f1[k:k + 1], f1)
    return res, (d1, d2, i1, i2)


@pytest.mark.parametrize("non_reg", [False, True])
def test_metrics_golden_and_restatement(dev, gcase, non_reg):
    M = _M()
    gt, x, cg, cx = gcase
    res, _ = _check_metrics(dev, gt, x, R.GOLDEN_COUNTS1, R.GOLDEN_COUNTS2, non_reg)
    ref = golden("chamfer_counts.npz")
    top = M.completion_metrics(x, gt, non_reg=non_reg, output_counts=cx, gt_counts=cg)
    assert all(torch.equal(u, v) for u, v in zip(top, res))
    for row, key in enumerate(("dcd", "cd_p", "cd_t")):
        np.testing.assert_allclose(getattr(res, key).cpu().numpy(), ref["dcd_nonreg" if non_reg else "dcd"][row],
                                   rtol=0, atol=ATOL_GOLDEN, err_msg=key)
    np.testing.assert_allclose(res.f1.cpu().numpy(), ref["f1"], rtol=0, atol=ATOL_GOLDEN)


def test_metrics_empty_side_and_means_columns(dev):
    from svdformer_pointsea_amd import _lib

    rng = np.random.default_rng(15)
    cg, cx = [700, 0, 33, 513], [500, 500, 0, 31]
    gt, x = _clouds(rng, 4, 700, 500, cg, cx, "nan")
    res, (d1, d2, _, _) = _check_metrics(dev, T(gt, dev), T(x, dev), cg, cx)
    means = torch.full((4, 4), -1.0, device=dev)
    tg, tx = C(cg, dev), C(cx, dev)
    with torch.cuda.device(dev):
        _lib.call("means", _lib.lib().pcops_chamfer_counts_means, _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(tg),
                  _lib.ptr(tx), 4, 700, 500, _lib.ptr(means), _lib.stream_of(d1))
    assert not means[1:3].any()   # an empty side: no loss contribution
    for col, f in enumerate(("l1a", "l1b", "l2a", "l2b")):   # the same summation order: the same bits
        assert torch.equal(means[[0, 3], col], getattr(res, f)[[0, 3]])


def test_metrics_workspace_bins(dev):
    """More than 32768 valid targets: the hit counts live in the workspace."""
    from svdformer_pointsea_amd import _lib

    rng = np.random.default_rng(11)
    N, M = 40000, 33000
    assert _lib.lib().pcops_completion_metrics_workspace_bytes(2, N, M) > 0
    cg, cx = [40000, 35000], [33000, 20]
    gt = (rng.random((2, N, 3)) - 0.5).astype(np.float32)
    x = (gt[:, rng.integers(0, N, M)] + 0.01 * rng.standard_normal((2, M, 3))).astype(np.float32)
    _check_metrics(dev, T(_pad(gt, cg, "nan"), dev), T(_pad(x, cx, "zero"), dev), cg, cx)


# ------------------------------------------------------------------ data, capture
def test_seprate_point_cloud_return_counts(dev):
    from svdformer_pointsea_amd.data import seprate_point_cloud

    M = _M()
    xyz = T((np.random.default_rng(2).random((3, 8192, 3)) - 0.5).astype(np.float32), dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(5)
    plain = seprate_point_cloud(xyz, 8192, [2048, 6144], generator=gen(), want_crop=False)
    inp, crop, packed, counts = seprate_point_cloud(xyz, 8192, [2048, 6144], generator=gen(), want_crop=False,
                                                    return_counts=True)
    assert len(plain) == 2 and torch.equal(plain[0], inp) and crop is None
    assert packed.shape == (3, 8192 - 2048, 3) and counts.dtype == torch.int32 and counts.shape == (3,)
    c = counts.tolist()
    assert all(2048 <= n <= 6144 for n in c)
    assert all(not packed[k, n:].any() and packed[k, :n].abs().sum(-1).gt(0).all() for k, n in enumerate(c))
    pred = (xyz[:, :128].contiguous(), xyz[:, :512].contiguous(), xyz[:, :2048].contiguous())
    tot, _ = M.get_loss_PM(pred, packed, xyz, partial_counts=counts)
    want = M.get_loss(pred, xyz)[0] + M.chamfer_single_side_sqrt_counts_chain(packed, pred[2], counts)
    torch.testing.assert_close(tot, want, rtol=1e-5, atol=1e-6)


def test_graph_capture_replays_new_counts(dev):
    """A counted loss step (forward and backward) captured once: replays with other counts written into the
    same tensors equal the eager step bit for bit -- the counts are read on the device only."""
    M = _M()
    rng = np.random.default_rng(13)
    B, N, Mm = 4, 1500, 1100
    a = T((rng.random((B, N, 3)) - 0.5).astype(np.float32), dev)
    b = T((rng.random((B, Mm, 3)) - 0.5).astype(np.float32), dev)
    sets = [([1500, 700, 33, 1025], [1100, 512, 1100, 9]), ([5, 1500, 1024, 0], [1100, 1, 600, 300])]

    def step(p1, p2, c1, c2):
        loss = M.chamfer_sqrt(p1, p2, c1, c2)
        return (loss.detach(),) + torch.autograd.grad(loss, (p1, p2))

    eager = [step(a.clone().requires_grad_(True), b.clone().requires_grad_(True), C(s1, dev), C(s2, dev))
             for s1, s2 in sets]
    p1, p2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    c1, c2 = C(sets[0][0], dev), C(sets[0][1], dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(p1, p2, c1, c2)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step(p1, p2, c1, c2)
    for k in (1, 0, 1):
        c1.copy_(C(sets[k][0], dev))
        c2.copy_(C(sets[k][1], dev))
        for t in res:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(res, eager[k]))
