"""CPU tests of the neighbour-distance helpers: the numpy restatements of tests/neighbour_refs.py against
the reference's own results (tests/golden/neighbours.npz), the *_chain functions and the composed helpers
on CPU tensors, the small modules, the public signatures and the new C-ABI symbols."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import neighbour_refs as NR
from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
from weights import fill_state  # noqa: E402

_C = {}


def clouds():
    """The fixture's input clouds (stored in the .npz next to the reference's results)."""
    if not _C:
        g = golden("neighbours.npz")
        _C.update({k[3:]: g[k] for k in g.files if k.startswith("in_")})
    return _C


@pytest.fixture(scope="module")
def gold():
    return golden("neighbours.npz")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close_root(got, ref, K, what):
    """|got - ref| <= (K + 3) u ref on the rows the reference resolves (finite and positive)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref) & (ref > 0)
    assert ok.any(), what
    err = np.abs(got - ref)[ok]
    assert (err <= NR.root_rtol(K) * ref[ok]).all(), (what, float((err / ref[ok]).max() / NR.U32))


# ------------------------------------------------------------------ restatements against the fixture
def test_stored_clouds_are_the_seeded_ones():
    c = clouds()
    for k, v in NR.fixture_clouds().items():
        assert np.array_equal(c[k], v), k


def test_form_a_restatement_is_square_distance(gold):
    c = clouds()
    assert np.array_equal(NR.dist_matrix(c["x"], c["y"], "A"), gold["sqd_xy"])


def test_form_b_restatement_is_the_sorted_row(gold):
    c = clouds()
    Bm = NR.dist_matrix(c["x"], c["y"], "B")
    assert np.array_equal(np.sort(Bm, axis=2), gold["gni_row"])
    v, i = NR.select(Bm, 4)
    assert np.array_equal(v, gold["gni4_dis"])
    assert np.array_equal(i, gold["gni4_idx"])


def test_root_restatements_against_the_reference(gold):
    c = clouds()
    v, _ = NR.nn_dist(c["x"], c["y"], 1)
    close_root(NR.root(v), gold["nd_xy"][:, :, 0], 1, "nearest")
    for n in "sw":
        v, i = NR.nn_dist(c[n], c[n], 1, "A", True)
        close_root(NR.root(v), gold[f"snd_{n}"][:, :, 0], 1, f"self {n}")
    own = i[:, :, 0] == np.arange(c["w"].shape[2])[None]      # on the wide cloud some diagonals win, not all
    assert 0 < own.sum() < own.size
    for n, k in (("s", 3), ("w", 3), ("w", 5)):
        v, _ = NR.nn_dist(c[n], c[n], k, "A", True)
        assert (v > 0).all()
        close_root(NR.root(v), gold[f"sndk{k}_{n}"][:, :, 0], k, f"self K {n} {k}")


def test_nan_mask_of_the_tiled_cloud_is_the_negative_minimum(gold):
    c = clouds()
    m = NR.dist_matrix(c["t"], c["t"], "A").min(2)
    assert (m < 0).any()
    assert np.array_equal(np.isnan(gold["nd_tt"][:, :, 0]), m < 0)
    assert np.array_equal(np.isnan(NR.root(m[:, :, None])), m < 0)


def test_reference_gradients_are_inside_the_bound(gold):
    """The bar the GPU tests hold the kernels to, applied to the reference's own fp32 autograd result."""
    c = clouds()
    v, i = NR.nn_dist(c["x"], c["y"], 1)
    g = np.ones(v.shape[:2], np.float32)
    gq, Eq, gp, Ep = NR.grad_ref(c["x"], c["y"], i, g, rooted=True)
    NR.assert_in_bound(gold["g_nd_x"], gq, Eq, "reference grad x")
    NR.assert_in_bound(gold["g_nd_y"], gp, Ep, "reference grad y")
    for key, n, k in (("g_snd_s", "s", 1), ("g_snd_w", "w", 1), ("g_sndk3_s", "s", 3), ("g_sndk3_w", "w", 3),
                      ("g_sndk5_w", "w", 5)):
        v, i = NR.nn_dist(c[n], c[n], k, "A", True)
        gs, Es, _, _ = NR.grad_ref(c[n], c[n], i, np.ones(v.shape[:2], np.float32), self_diag=True, rooted=True,
                                   same=True)
        NR.assert_in_bound(gold[key], gs, Es, key)


# ------------------------------------------------------------------ chains and composed helpers on CPU tensors
def test_chain_functions_on_cpu(gold):
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    x, y = T(c["x"]), T(c["y"])
    # a CPU tensor takes the chain through the public name too
    for fn in (M.nearest_distances_chain, M.nearest_distances):
        out = fn(x, y)
        assert out.shape == (2, 257, 1) and out.dtype == torch.float32
        close_root(out.numpy()[:, :, 0], gold["nd_xy"][:, :, 0], 1, "nearest chain")
    for n in "sw":
        close_root(M.self_nearest_distances(T(c[n])).numpy()[:, :, 0], gold[f"snd_{n}"][:, :, 0], 1, n)
    for n, k in (("s", 3), ("w", 3), ("w", 5)):
        close_root(M.self_nearest_distances_K(T(c[n]), k).numpy()[:, :, 0], gold[f"sndk{k}_{n}"][:, :, 0], k, n)
    idx, dis = M.get_nearest_index(x, y, k=4, return_dis=True)
    assert idx.dtype == torch.int64 and idx.shape == (2, 257, 4) and dis.shape == (2, 257, 4)
    assert np.array_equal(idx.numpy(), gold["gni4_idx"])
    assert np.array_equal(dis.numpy(), gold["gni4_dis"])
    assert np.array_equal(M.get_nearest_index(x, y, k=4).numpy(), gold["gni4_idx"])
    sq = M.square_distance(x.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous())
    assert np.array_equal(sq.numpy(), gold["sqd_xy"])


def test_composed_helpers_on_cpu(gold):
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    out = M.indexing_neighbor(T(c["f"]), T(gold["ixn_index"]).long())
    assert np.array_equal(out.numpy(), gold["ixn"])
    s = T(c["s"])
    idx = M.knn(s, 5)
    assert idx.dtype == torch.int64
    assert np.array_equal(idx.numpy(), gold["knn_s"])
    assert np.array_equal(M.get_graph_feature(s, k=5).numpy(), gold["ggf_s"])
    assert np.array_equal(M.get_graph_feature(s, idx=T(gold["knn_s"]).long()).numpy(), gold["ggf_s"])


def test_errors_on_cpu():
    from svdformer_pointsea_amd import model_utils as M

    x = torch.zeros(2, 3, 5)
    with pytest.raises(RuntimeError):
        M.self_nearest_distances_K(x, 6)
    with pytest.raises(RuntimeError):
        M.get_nearest_index(x, torch.zeros(2, 3, 3), k=4)
    with pytest.raises(RuntimeError):
        M.nearest_distances(x, torch.zeros(3, 3, 5))
    with pytest.raises(RuntimeError):
        M.nearest_distances(x, torch.zeros(2, 4, 5))


@pytest.mark.parametrize("name", list(NR.MODULES))
def test_modules_load_and_match(gold, name):
    from svdformer_pointsea_amd import model_utils as M

    cls, _, wseed, _, _ = NR.MODULES[name]
    kw = NR.module_kwargs(name)
    m = getattr(M, cls)(**kw)
    if cls == "PointNetFeatureExtractor":
        assert kw == NR.MODULES[name][1]          # the caller's list is not edited
    fill_state(m, wseed).eval()                   # load_state_dict is strict: the reference's keys
    with torch.no_grad():
        out = m(T(NR.module_input(name))).numpy()
    ref = gold[f"{name}_out"]
    assert out.shape == ref.shape
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())


def test_module_state_keys_are_the_references():
    from svdformer_pointsea_amd import model_utils as M

    assert sorted(M.MLP(4, [8, 2], bn=True).state_dict()) == sorted(
        [f"mlp.{i}.{k}" for i in (0, 3) for k in ("weight", "bias")]
        + [f"mlp.1.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")])
    assert sorted(M.MLP_Res(4, 5, 6).state_dict()) == sorted(
        [f"{n}.{k}" for n in ("conv_1", "conv_2", "conv_shortcut") for k in ("weight", "bias")])
    keys = set(M.PointNetFeatureExtractor(3, 8, [4]).state_dict())
    assert {"conv_layers.0.weight", "conv_layers.1.bias", "bn_layers.1.running_var"} <= keys


def test_public_signatures():
    from svdformer_pointsea_amd import model_utils as M

    want = {
        "nearest_distances": "(x, y)",
        "self_nearest_distances": "(x)",
        "self_nearest_distances_K": "(x, k=3)",
        "get_nearest_index": "(target, source, k=1, return_dis=False)",
        "indexing_neighbor": "(x, index)",
        "square_distance": "(src, dst)",
        "knn": "(x, k)",
        "get_graph_feature": "(x, k=20, idx=None)",
        "nn_dist_raw": "(q, p, k, form='A', self_diag=False)",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(M, name))) == sig, name
    assert list(inspect.signature(M.MLP.__init__).parameters) == ["self", "in_channel", "layer_dims", "bn"]
    assert list(inspect.signature(M.MLP_Res.__init__).parameters) == ["self", "in_dim", "hidden_dim", "out_dim"]
    assert list(inspect.signature(M.PointNetFeatureExtractor.__init__).parameters) == [
        "self", "in_channels", "feat_size", "layer_dims", "global_feat", "activation", "batchnorm", "transposed_input"]
    for name in want:
        if name not in ("square_distance", "knn", "get_graph_feature", "nn_dist_raw", "indexing_neighbor"):
            assert callable(getattr(M, name + "_chain"))


def test_new_symbols_are_bound():
    from svdformer_pointsea_amd import _lib

    assert {"pcops_nn_dist_forward", "pcops_nn_dist_backward", "pcops_nn_dist_backward_workspace_bytes"} <= set(
        _lib.exported_symbols())
    L = _lib.lib()
    assert L.pcops_abi_version() == 2
    assert L.pcops_nn_dist_backward_workspace_bytes(0, 5, 5, 1, 0) == 0
    pairs = 2 * 257 * 4
    assert L.pcops_nn_dist_backward_workspace_bytes(2, 257, 130, 4, 0) >= pairs * 16
    assert os.path.getsize(os.path.join(GOLDEN, "neighbours.npz")) < 1 << 20
