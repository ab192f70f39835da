"""CPU tests of the view-space ops: the numpy references of tests/viewops_refs.py and the torch chains
(what CPU tensors and PCOPS_VIEWOPS_FUSED=0 run) against tests/golden/viewops.npz, which
tests/golden/make_golden_viewops.py made from the reference's own functions.  Every comparison covers
every element."""
import numpy as np
import pytest
import torch

import viewops_refs as VR
from conftest import golden


@pytest.fixture(scope="module")
def G():
    return golden("viewops.npz")


@pytest.fixture(scope="module")
def depth_npz():
    return golden("depth.npz")


@pytest.mark.parametrize("name", list(VR.EXCHANGE_GOLDEN))
def test_numpy_references_match_the_reference(G, name):
    case = VR.EXCHANGE_GOLDEN[name]
    _, B, N, C, h, w = case
    fea, coord, img = VR.exchange_inputs(*case)
    np.testing.assert_array_equal(VR.splat(fea, coord, h * w), G[f"x_{name}_splat"])
    np.testing.assert_array_equal(VR.gather(VR.nchw_rows(img), coord), G[f"x_{name}_gather"])


@pytest.mark.parametrize("name", list(VR.EXCHANGE_GOLDEN))
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_exchange_chain_on_cpu(G, name, layout):
    from svdformer_pointsea_amd.model_utils import distribute_img_fea_points, point_fea_img_fea

    case = VR.EXCHANGE_GOLDEN[name]
    _, B, N, C, h, w = case
    fea0, coord0, img0 = VR.exchange_inputs(*case)
    fea, coord, img = torch.from_numpy(fea0.copy()), torch.from_numpy(coord0.copy()), torch.from_numpy(img0.copy())
    if layout == "channels_last":
        img = img.contiguous(memory_format=torch.channels_last)
    fea.requires_grad_(True)
    img.requires_grad_(True)
    out = point_fea_img_fea(fea, coord, h, w)
    np.testing.assert_array_equal(out.detach().numpy(), G[f"x_{name}_splat"])
    got = distribute_img_fea_points(img, coord)
    np.testing.assert_array_equal(got.detach().numpy(), G[f"x_{name}_gather"])
    # each op's gradient is the other op
    rng = np.random.default_rng(7)
    go = rng.standard_normal(out.shape).astype(np.float32)
    out.backward(torch.from_numpy(go))
    np.testing.assert_array_equal(fea.grad.numpy(), VR.gather(go, coord0))
    gg = rng.standard_normal(got.shape).astype(np.float32)
    got.backward(torch.from_numpy(gg))
    np.testing.assert_array_equal(VR.nchw_rows(img.grad.numpy()), VR.splat(gg, coord0, h * w))
    # the inputs are not modified (the reference zeroes them in place)
    np.testing.assert_array_equal(fea.detach().numpy(), fea0)
    np.testing.assert_array_equal(coord.numpy(), coord0)
    np.testing.assert_array_equal(img.detach().numpy(), img0)


def test_exchange_chain_integer_and_nonfinite_coordinates():
    from svdformer_pointsea_amd.model_utils import distribute_img_fea_points, point_fea_img_fea

    rng = np.random.default_rng(3)
    fea = rng.standard_normal((1, 12, 3)).astype(np.float32)
    img = rng.standard_normal((1, 3, 2, 3)).astype(np.float32)
    f = np.asarray([[0, 5, 6, -1, 3.7, -0.5, np.nan, np.inf, -np.inf, 1e20, 2, 2]], np.float32)
    i = np.asarray([[0, 5, 6, -1, 3, 2 ** 40, -2 ** 40, 7, 1, 1, 2, 2]], np.int64)
    for coord in (f, i, i.astype(np.int32)):
        c = torch.from_numpy(coord.copy())
        np.testing.assert_array_equal(point_fea_img_fea(torch.from_numpy(fea), c, 2, 3).numpy(), VR.splat(fea, coord, 6))
        np.testing.assert_array_equal(distribute_img_fea_points(torch.from_numpy(img), c).numpy(),
                                      VR.gather(VR.nchw_rows(img), coord))
        np.testing.assert_array_equal(c.numpy(), coord)


def test_batched_index_select():
    from svdformer_pointsea_amd.model_utils import batched_index_select

    x = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3)
    idx = torch.tensor([[4, 0, 0], [1, 2, 3]])
    out = batched_index_select(x, 1, idx)
    assert out.shape == (2, 3, 3)
    for b in range(2):
        assert torch.equal(out[b], x[b][idx[b]])
    y = x.transpose(1, 2).contiguous()
    assert torch.equal(batched_index_select(y, 2, idx), out.transpose(1, 2))


def _view(R):
    from svdformer_pointsea_amd.render import PCViews

    return PCViews(TRANS=-0.7, RESOLUTION=R)


@pytest.mark.parametrize("name", list(VR.DEPTH_GOLDEN))
def test_depth_chain_and_gradient_on_cpu(G, depth_npz, name):
    """points2depth_chain on CPU: the golden image (same non-zero mask, same values), a gradient that
    agrees with the reference's autograd result, and the float64 reference pinned against the same."""
    from svdformer_pointsea_amd.render import points2depth_chain

    _, B, N, R = VR.DEPTH_GOLDEN[name]
    pts0, g = VR.depth_inputs(name, depth_npz)
    view = _view(R)
    p = torch.from_numpy(pts0.copy()).requires_grad_(True)
    img = view.get_img(p)                      # a CPU tensor that needs a gradient: the chain
    assert img.requires_grad
    want = depth_npz["img"] if name == "r224" else G[f"d_{name}_img"]
    got = img.detach().numpy()
    np.testing.assert_array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(points2depth_chain(p.detach(), view.rot_mat, view.translation, R).numpy(), got)
    img.backward(torch.from_numpy(g))
    np.testing.assert_array_equal(p.detach().numpy(), pts0)
    gold = G[f"d_{name}_grad"]
    assert np.isfinite(gold).all() and (gold != 0).any()
    pix = view.project(p.detach()).numpy()
    ref, n, E = VR.depth_grad(pts0, view.rot_mat.numpy(), view.translation.numpy(), pix, g)
    r_gold = VR.assert_depth_grad(gold, ref, n, E, f"{name}: float64 reference vs the reference's autograd")
    r_chain = VR.assert_depth_grad(p.grad.numpy(), ref, n, E, f"{name}: chain autograd")
    print(f"{name}: err/bound golden {r_gold:.3f} chain {r_chain:.3f}; "
          f"max |ref - golden| / max |golden| = {np.abs(ref - gold).max() / np.abs(gold).max():.3g}")


def test_project_matches_the_image_support_on_cpu(depth_npz):
    view = _view(224)
    pts = torch.from_numpy(depth_npz["points"])
    pix = view.project(pts).numpy()
    hit = np.zeros((pix.shape[0], 224 * 224), bool)
    for r in range(pix.shape[0]):
        hit[r, pix[r][pix[r] >= 0]] = True
    np.testing.assert_array_equal(hit.reshape(-1, 224, 224), depth_npz["img"] != 0)


def test_no_grad_input_keeps_the_forward_only_path():
    """Without requires_grad get_img stays the forward-only product path (no CPU fallback there)."""
    view = _view(8)
    with pytest.raises(RuntimeError):
        view.get_img(torch.zeros(1, 4, 3))
