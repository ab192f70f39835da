"""GPU tests of the view-space ops: the point <-> pixel exchange kernels (pcops_pixel_splat /
pcops_pixel_gather, forward and backward, bit for bit against the numpy references of
tests/viewops_refs.py, into poisoned and guarded outputs), the differentiable PCViews.get_img
(pcops_points2depth_backward against the float64 reference inside its derived bound), PCViews.project,
the PCOPS_VIEWOPS_FUSED=0 chain in a child process, and one graph capture.  No comparison leaves
elements out."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import viewops_refs as VR
from conftest import ROOT, golden
from pointops_refs import Poisoned, T

pytestmark = pytest.mark.gpu

# (B, N, C, h, w): the shapes of the issue; coordinates uniform over [-0.2 P, 1.35 P) (about 35 % rejected)
CASES = {
    "small": (2, 300, 5, 3, 4),
    "oddC": (2, 4096, 33, 7, 7),
    "deep": (1, 20000, 64, 2, 2),       # ~3,200 points per pixel, 313 steps of the placing wave
    "sparse": (3, 1000, 1, 14, 14),
    "wide": (2, 2048, 256, 14, 14),
    "one_pixel": (2, 700, 6, 3, 3),     # every point in pixel 4
    "rejected": (2, 130, 4, 3, 3),      # every point rejected
    "special": (1, 70, 3, 2, 3),        # the special values, then random
    "manypix": (1, 500, 2, 95, 97),     # P = 9215 > the LDS cursor limit of the placing kernel
}
_CACHE = {}


def case(name):
    """fea, coord (float32), img (NCHW), upstream gradients and the numpy references, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    B, N, C, h, w = CASES[name]
    P = h * w
    rng = np.random.default_rng(sum(map(ord, name)))
    fea = rng.standard_normal((B, N, C)).astype(np.float32)
    coord = rng.uniform(-0.2 * P, 1.35 * P, (B, N)).astype(np.float32)
    if name == "one_pixel":
        coord[:] = 4.25
    elif name == "rejected":
        coord = np.where(coord >= 0, coord + P, coord).astype(np.float32)
        coord[:, ::7] = np.nan
    elif name == "special":
        sp = [0.0, -0.0, P - 1, P, -1, 3.7, -0.5, np.nan, np.inf, -np.inf, 1e20, -1e20, P - 0.5, 0.999]
        coord[0, :len(sp)] = np.asarray(sp, np.float32)
    img = rng.standard_normal((B, C, h, w)).astype(np.float32)
    d = dict(fea=fea, coord=coord, img=img, P=P,
             g_img=rng.standard_normal((B, P, C)).astype(np.float32),
             g_pts=rng.standard_normal((B, N, C)).astype(np.float32))
    d["splat"] = VR.splat(fea, coord, P)
    d["gather"] = VR.gather(VR.nchw_rows(img), coord)
    d["splat_bwd"] = VR.gather(d["g_img"], coord)              # d fea = the rows of the image gradient
    d["gather_bwd"] = VR.splat(d["g_pts"], coord, P)           # d img rows = the splat of the point gradient
    _CACHE[name] = d
    return d


def _dirty_workspace(dev, nbytes):
    from svdformer_pointsea_amd._lib import Workspace

    Workspace.get(dev, nbytes + 4096).fill_(0xA5)   # the splat's scratch may hold anything on entry


def _splat(dev, fea, coord, P, layout="rows", hw=None):
    """pcops_pixel_splat into a poisoned output: rows (B,P,C), or an image (B,C,h,w) in NCHW / channels_last
    memory; returns it as (B,P,C) rows."""
    from svdformer_pointsea_amd.model_utils import pixel_splat

    B, N, C = fea.shape
    _dirty_workspace(dev, 4 * B * (N + P) + 256)
    if layout == "nchw":
        p = Poisoned(dev, (B, C, P))
        pixel_splat(fea, coord, P, (C * P, 1, P), p.out)
        return np.ascontiguousarray(p.result("splat->nchw").transpose(0, 2, 1))
    p = Poisoned(dev, (B, P, C))                      # rows and channels_last share the addressing
    pixel_splat(fea, coord, P, (P * C, C, 1), p.out)
    return p.result("splat")


def _gather(dev, img, coord, P, C, layout):
    from svdformer_pointsea_amd.model_utils import pixel_gather

    B, N = coord.shape
    strides = (C * P, 1, P) if layout == "nchw" else (P * C, C, 1)
    p = Poisoned(dev, (B, N, C))
    pixel_gather(img, strides, C, coord, P, out=p.out)
    return p.result("gather")


@pytest.mark.parametrize("name", list(CASES))
def test_exchange_kernels_bitwise(dev, name):
    d = case(name)
    B, N, C, h, w = CASES[name]
    P = d["P"]
    fea, coord = T(d["fea"], dev), T(d["coord"], dev)
    a = _splat(dev, fea, coord, P)
    np.testing.assert_array_equal(a, d["splat"])
    np.testing.assert_array_equal(_splat(dev, fea, coord, P), a)          # two runs: the same bits
    if name == "rejected":
        assert not a.any()
    rows = T(VR.nchw_rows(d["img"]), dev)
    np.testing.assert_array_equal(_gather(dev, T(d["img"], dev), coord, P, C, "nchw"), d["gather"])
    np.testing.assert_array_equal(_gather(dev, rows, coord, P, C, "channels_last"), d["gather"])
    # the two gradients: the same kernels with the roles swapped, the image gradient in either memory format
    g_pts = T(d["g_pts"], dev)
    np.testing.assert_array_equal(_gather(dev, T(d["g_img"], dev), coord, P, C, "rows"), d["splat_bwd"])
    np.testing.assert_array_equal(_splat(dev, g_pts, coord, P, "nchw"), d["gather_bwd"])
    np.testing.assert_array_equal(_splat(dev, g_pts, coord, P, "channels_last"), d["gather_bwd"])
    np.testing.assert_array_equal(coord.cpu().numpy().view(np.int32), d["coord"].view(np.int32))
    np.testing.assert_array_equal(fea.cpu().numpy(), d["fea"])


@pytest.mark.parametrize("dtype", ["int64", "int32", "float64"])
def test_exchange_coordinate_dtypes(dev, dtype):
    d = case("small")
    B, N, C, h, w = CASES["small"]
    P = d["P"]
    if dtype == "float64":
        coord = d["coord"].astype(np.float64)
        coord[0, :6] = [P - 1 + 1e-9, -1e-300, 1e300, np.nan, P - 1, 0.0]
    else:
        coord = np.floor(d["coord"]).astype(dtype)
        coord[0, :6] = [np.iinfo(dtype).max, np.iinfo(dtype).min, P, P - 1, -1, 0]
    fea = d["fea"]
    c = T(coord, dev)
    np.testing.assert_array_equal(_splat(dev, T(fea, dev), c, P), VR.splat(fea, coord, P))
    np.testing.assert_array_equal(_gather(dev, T(d["img"], dev), c, P, C, "nchw"),
                                  VR.gather(VR.nchw_rows(d["img"]), coord))


def test_exchange_empty_shapes(dev):
    from svdformer_pointsea_amd.model_utils import distribute_img_fea_points, point_fea_img_fea

    z = _splat(dev, torch.empty(2, 0, 3, device=dev), torch.empty(2, 0, device=dev), 6)   # N = 0: exact zeros
    assert z.shape == (2, 6, 3) and not z.any()
    assert distribute_img_fea_points(torch.randn(2, 3, 2, 3, device=dev), torch.empty(2, 0, device=dev)).shape == (2, 0, 3)
    assert point_fea_img_fea(torch.empty(0, 5, 3, device=dev), torch.empty(0, 5, device=dev), 2, 3).shape == (0, 6, 3)
    assert distribute_img_fea_points(torch.empty(0, 3, 2, 3, device=dev), torch.empty(0, 5, device=dev)).shape == (0, 5, 3)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("name", ["small", "oddC"])
def test_exchange_public_functions_and_autograd(dev, name, layout):
    """The public functions under autograd: values, both gradients, the image gradient's memory format,
    inputs unchanged."""
    from svdformer_pointsea_amd.model_utils import distribute_img_fea_points, point_fea_img_fea

    d = case(name)
    B, N, C, h, w = CASES[name]
    fea = T(d["fea"], dev).requires_grad_(True)
    coord = T(d["coord"], dev)
    img = T(d["img"], dev)
    if layout == "channels_last":
        img = img.contiguous(memory_format=torch.channels_last)
    img.requires_grad_(True)
    out = point_fea_img_fea(fea, coord, h, w)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), d["splat"])
    out.backward(T(d["g_img"], dev))
    np.testing.assert_array_equal(fea.grad.cpu().numpy(), d["splat_bwd"])
    got = distribute_img_fea_points(img, coord)
    np.testing.assert_array_equal(got.detach().cpu().numpy(), d["gather"])
    got.backward(T(d["g_pts"], dev))
    assert img.grad.stride() == img.stride()
    np.testing.assert_array_equal(VR.nchw_rows(img.grad.cpu().numpy()), d["gather_bwd"])
    np.testing.assert_array_equal(coord.cpu().numpy().view(np.int32), d["coord"].view(np.int32))
    np.testing.assert_array_equal(fea.detach().cpu().numpy(), d["fea"])
    np.testing.assert_array_equal(img.detach().cpu().numpy(), d["img"])


# ------------------------------------------------------------------ depth
def _depth_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "golden":
        pts, R = golden("depth.npz")["points"].astype(np.float32), 224
    else:
        B, N, R, scale = {"shared": (2, 64, 8, 1.0), "single": (1, 1, 8, 1.0), "behind": (2, 512, 16, 2.0),
                          "halfzero": (2, 300, 16, 1.0)}[name]
        pts = ((rng.random((B, N, 3)) - 0.5) * scale).astype(np.float32)
    g = rng.standard_normal((pts.shape[0] * 3, R, R)).astype(np.float32)
    if name == "halfzero":
        g[:, :, R // 2:] = 0.0
    return pts, g, R


@pytest.mark.parametrize("name", ["shared", "single", "golden", "behind", "halfzero"])
def test_depth_gradient(dev, name):
    from svdformer_pointsea_amd.render import PCViews, points2depth_backward

    pts, g, R = _depth_case(name)
    B, N, _ = pts.shape
    view = PCViews(TRANS=-0.7, RESOLUTION=R)
    plain = view.get_img(T(pts, dev)).cpu().numpy()
    p = T(pts, dev).requires_grad_(True)
    img = view.get_img(p)
    assert img.requires_grad and img.shape == (B * 3, R, R)
    got = img.detach().cpu().numpy()
    np.testing.assert_array_equal(got != 0, plain != 0)
    np.testing.assert_allclose(got, plain, rtol=1e-6, atol=1e-7)
    if name == "golden":
        np.testing.assert_array_equal(got != 0, golden("depth.npz")["img"] != 0)
        np.testing.assert_allclose(got, golden("depth.npz")["img"], rtol=1e-6, atol=1e-7)
    _, _, _, imgs, wsum = img.grad_fn.saved_tensors   # before backward() releases them
    img.backward(T(g, dev))
    pix = view.project(p.detach()).cpu().numpy()
    ref, n, E = VR.depth_grad(pts, view.rot_mat.numpy(), view.translation.numpy(), pix, g)
    if name == "behind":
        assert (n == 0).any() and (n == 3).any()
    ratio = VR.assert_depth_grad(p.grad.cpu().numpy(), ref, n, E, name)
    print(f"{name}: largest error / derived bound = {ratio:.3f}")
    assert (p.grad != 0).any()
    np.testing.assert_array_equal(p.detach().cpu().numpy(), pts)
    # the gradient kernel alone, into poisoned outputs, twice from the same saved (img, wsum): the same bits
    rot, trans = view._consts(dev)
    outs = []
    for _ in range(2):
        po = Poisoned(dev, (B, N, 3))
        points2depth_backward(p.detach(), rot, trans, imgs, wsum, T(g, dev), out=po.out)
        outs.append(po.result("points2depth_backward"))
    np.testing.assert_array_equal(outs[0].view(np.int32), outs[1].view(np.int32))
    np.testing.assert_array_equal(outs[0].view(np.int32), p.grad.cpu().numpy().view(np.int32))


def test_no_grad_paths_stay_detached(dev):
    from svdformer_pointsea_amd.render import PCViews

    view = PCViews(TRANS=-0.7, RESOLUTION=8)
    p = torch.rand(1, 16, 3, device=dev).sub_(0.5).requires_grad_(True)
    with torch.no_grad():
        assert not view.get_img(p).requires_grad
    assert not view.get_img(p.detach()).requires_grad


def test_project_ties_the_exchange_to_the_depth_splat(dev):
    """project(p) >= 0 has exactly get_img's non-zero support, and splatting (w, z w) at project(p) with
    pcops_pixel_splat, divided as the reference divides, is get_img(p) at the forward's bar."""
    from svdformer_pointsea_amd.model_utils import point_fea_img_fea
    from svdformer_pointsea_amd.render import PCViews

    pts = golden("depth.npz")["points"].astype(np.float32)
    B, N, _ = pts.shape
    R = 224
    view = PCViews(TRANS=-0.7, RESOLUTION=R)
    img = view.get_img(T(pts, dev)).cpu().numpy()
    pix_t = view.project(T(pts, dev))
    assert pix_t.dtype == torch.int64 and pix_t.shape == (B * 3, N)
    pix = pix_t.cpu().numpy()
    hit = np.zeros((B * 3, R * R), bool)
    for r in range(B * 3):
        hit[r, pix[r][pix[r] >= 0]] = True
    np.testing.assert_array_equal(hit.reshape(-1, R, R), img != 0)
    z = np.einsum("bnk,vk->bvn", pts.astype(np.float64), view.rot_mat.numpy()[:, :, 2].astype(np.float64))
    z = (z - view.translation.numpy()[None, :, 2, None].astype(np.float64)).reshape(B * 3, N).astype(np.float32)
    w = np.float32(1) / (z + np.float32(1e-12))
    fea = np.stack([w, z * w], axis=-1).astype(np.float32)
    s = point_fea_img_fea(T(fea, dev), pix_t, R, R).cpu().numpy()
    ws = s[:, :, 0]
    tie = (s[:, :, 1] / np.where(ws == 0, ws + 1, ws)).reshape(-1, R, R)
    np.testing.assert_array_equal(tie != 0, img != 0)
    np.testing.assert_allclose(tie, img, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ PCOPS_VIEWOPS_FUSED=0
_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_viewops as TV
from svdformer_pointsea_amd import model_utils as MU, render
assert not render.viewops_fused()
dev = torch.device("cuda:0")
out = {}
fea, coord, img, g_img, g_pts, h, w = TV.chain_exchange_inputs()
f = torch.from_numpy(fea).to(dev).requires_grad_(True)
i = torch.from_numpy(img).to(dev).requires_grad_(True)
c = torch.from_numpy(coord).to(dev)
s = MU.point_fea_img_fea(f, c, h, w); s.backward(torch.from_numpy(g_img).to(dev))
d = MU.distribute_img_fea_points(i, c); d.backward(torch.from_numpy(g_pts).to(dev))
out.update(splat=s.detach().cpu().numpy(), splat_bwd=f.grad.cpu().numpy(), gather=d.detach().cpu().numpy(),
           gather_bwd=i.grad.cpu().numpy())
pts, g, R = TV._depth_case("behind")
p = torch.from_numpy(pts).to(dev).requires_grad_(True)
view = render.PCViews(TRANS=-0.7, RESOLUTION=R)
im = view.get_img(p); im.backward(torch.from_numpy(g).to(dev))
out.update(depth=im.detach().cpu().numpy(), depth_grad=p.grad.cpu().numpy(), pix=view.project(p.detach()).cpu().numpy())
np.savez(sys.argv[2], **out)
"""


def chain_exchange_inputs():
    """Integer-valued features and gradients (|v| <= 8): every partial sum is exact in fp32, so the chain's
    float-atomic scatter_add, whatever its order, and the ordered kernel must agree bit for bit."""
    B, N, C, h, w = CASES["small"]
    d = case("small")
    rng = np.random.default_rng(99)
    ints = lambda *s: rng.integers(-8, 9, s).astype(np.float32)  # noqa: E731
    return ints(B, N, C), d["coord"], ints(B, C, h, w), ints(B, h * w, C), ints(B, N, C), h, w


def test_chain_switch_agrees_with_the_kernels(dev, tmp_path):
    from svdformer_pointsea_amd.model_utils import distribute_img_fea_points, point_fea_img_fea
    from svdformer_pointsea_amd.render import PCViews, viewops_fused

    assert viewops_fused()
    path = str(tmp_path / "chain.npz")
    env = dict(os.environ, PCOPS_VIEWOPS_FUSED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ch = np.load(path)
    fea, coord, img, g_img, g_pts, h, w = chain_exchange_inputs()
    f, i, c = T(fea, dev).requires_grad_(True), T(img, dev).requires_grad_(True), T(coord, dev)
    s = point_fea_img_fea(f, c, h, w)
    s.backward(T(g_img, dev))
    d = distribute_img_fea_points(i, c)
    d.backward(T(g_pts, dev))
    for k, v in dict(splat=s, splat_bwd=f.grad, gather=d, gather_bwd=i.grad).items():
        np.testing.assert_array_equal(v.detach().cpu().numpy(), ch[k], err_msg=k)
    pts, g, R = _depth_case("behind")
    view = PCViews(TRANS=-0.7, RESOLUTION=R)
    pix = view.project(T(pts, dev)).cpu().numpy()
    np.testing.assert_array_equal(pix, ch["pix"])
    img_k = view.get_img(T(pts, dev)).cpu().numpy()
    np.testing.assert_array_equal(ch["depth"] != 0, img_k != 0)
    np.testing.assert_allclose(ch["depth"], img_k, rtol=1e-6, atol=1e-7)
    ref, n, E = VR.depth_grad(pts, view.rot_mat.numpy(), view.translation.numpy(), pix, g)
    VR.assert_depth_grad(ch["depth_grad"], ref, n, E, "chain")


# ------------------------------------------------------------------ capture
def test_capture_replays_equal_eager(dev):
    """The splat, the gather and the depth forward + backward captured on one stream (no forks), replayed
    twice with changed inputs and every output poisoned before each replay: equal to eager."""
    from svdformer_pointsea_amd.model_utils import distribute_img_fea_points, point_fea_img_fea
    from svdformer_pointsea_amd.render import PCViews

    d = case("small")
    B, N, C, h, w = CASES["small"]
    view = PCViews(TRANS=-0.7, RESOLUTION=16)
    rng = np.random.default_rng(5)
    fea, coord, img = T(d["fea"], dev), T(d["coord"], dev), T(d["img"], dev)
    pts = T((rng.random((2, 200, 3)) - 0.5).astype(np.float32), dev).requires_grad_(True)
    g = T(rng.standard_normal((6, 16, 16)).astype(np.float32), dev)
    res = {}

    def run():
        res["splat"] = point_fea_img_fea(fea, coord, h, w)
        res["gather"] = distribute_img_fea_points(img, coord)
        res["depth"] = view.get_img(pts)
        (res["grad"],) = torch.autograd.grad(res["depth"], pts, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    outs = dict(res)
    for it in range(2):
        with torch.no_grad():
            fea.copy_(torch.roll(fea, it + 1, 1) * (it + 2))
            coord.copy_(torch.roll(coord, 3 * it + 1, 1))
            img.mul_(-1.5)
            pts.copy_(torch.roll(pts, 1, 2) * 0.9)
            g.copy_(torch.roll(g, 1, 0))
        for t in outs.values():
            t.detach().fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.detach().clone() for k, t in outs.items()}
        run()
        torch.cuda.synchronize()
        for k in ("splat", "gather"):
            assert torch.equal(got[k], res[k].detach()), k
        # the depth image is summed with float atomics (run-to-run order); its gradient reads that image
        np.testing.assert_array_equal((got["depth"] != 0).cpu().numpy(), (res["depth"] != 0).cpu().numpy())
        torch.testing.assert_close(got["depth"], res["depth"].detach(), rtol=1e-6, atol=1e-7)
        pix = view.project(pts.detach()).cpu().numpy()
        ref, n, E = VR.depth_grad(pts.detach().cpu().numpy(), view.rot_mat.numpy(), view.translation.numpy(), pix,
                                  g.cpu().numpy())
        VR.assert_depth_grad(got["grad"].cpu().numpy(), ref, n, E, f"replay {it}")
