"""GPU tests of the neighbour-distance helpers: pcops_nn_dist_forward bit for bit against the numpy
restatements of tests/neighbour_refs.py (both forms, the diagonal, ties, every list size and launch
shape), the public functions against the reference's results (tests/golden/neighbours.npz),
pcops_nn_dist_backward (grad_q bit-equal to its restatement, the ordered target-side sum inside the
derived bound of the float64 gradient and bit-equal run to run), containment of a non-finite row, the
dispatch rules, the PCOPS_NEIGHBOURS_FUSED=0 chain in a child process and one graph capture."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbour_refs as NR
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


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


# ------------------------------------------------------------------ nn_dist_raw against the restatement
# (name, B, S, N, K, self, cloud): tile and wave-merge edges first, then one per remaining list size / launch shape
RAW = [
    ("below_tile_k1", 2, 257, 130, 1, False, "unit"),      # S no multiple of 64, N below one tile
    ("below_tile_k4", 2, 257, 130, 4, False, "unit"),
    ("cross_tile", 2, 1030, 1030, 3, True, "unit"),        # crosses a 1024-candidate tile, every wave merges
    ("wide_k1", 1, 64, 64, 1, True, "wide"),               # some index equals the row
    ("wide_k5", 1, 64, 64, 5, True, "wide"),
    ("k_is_n", 3, 5, 5, 5, False, "unit"),
    ("one_point", 1, 1, 1, 1, True, "unit"),               # the value is d_00 + 2
    ("form_b_k16", 2, 300, 4099, 16, False, "unit"),
    ("many_blocks", 48, 1024, 70, 2, False, "unit"),       # 768 blocks: the 4-wave, 512-candidate-tile launch
    ("list20", 1, 70, 90, 20, False, "unit"),              # two waves per query
    ("list32", 1, 70, 90, 27, False, "unit"),
    ("list64", 1, 70, 64, 64, False, "unit"),              # one wave per query, K == N == the limit
]
FORMS = {"below_tile_k1": "AB", "below_tile_k4": "AB", "form_b_k16": "B"}


def raw_inputs(name, B, S, N, self_):
    rng = np.random.default_rng(sum(map(ord, name)))
    gen = (lambda n: ((rng.random((B, 3, n)) - 0.5) * 6.0).astype(np.float32)) if "wide" in name else \
        (lambda n: rng.random((B, 3, n)).astype(np.float32))
    p = gen(N)
    return (p, p) if self_ else (gen(S), p)


@pytest.mark.parametrize("name,B,S,N,K,self_,kind", RAW, ids=[r[0] for r in RAW])
def test_raw_is_the_restatement(dev, name, B, S, N, K, self_, kind):
    from svdformer_pointsea_amd.model_utils import nn_dist_raw

    q, p = raw_inputs(name + kind, B, S, N, self_)
    for form in FORMS.get(name, "A"):
        v, i = NR.nn_dist(q, p, K, form, self_)
        dist, idx = nn_dist_raw(T(q, dev), T(p, dev), K, form=form, self_diag=self_)
        assert idx.dtype == torch.int32 and dist.shape == (B, S, K)
        np.testing.assert_array_equal(N_(idx), i, err_msg=f"{name} {form} idx")
        np.testing.assert_array_equal(N_(dist), v, err_msg=f"{name} {form} dist")
    if name == "one_point":
        assert v[0, 0, 0] == NR.dist_matrix(q, p)[0, 0, 0] + np.float32(2)
    if name.startswith("wide"):
        assert (i[:, :, 0] == np.arange(S)[None]).any()


def test_ties_go_to_the_lowest_index(dev, gold):
    """Every source point stored twice: rank 2r and 2r + 1 hold the pair (2 j_r, 2 j_r + 1), the distances
    per rank are the fixture's."""
    from svdformer_pointsea_amd.model_utils import nn_dist_raw

    c = clouds()
    y2 = np.repeat(c["y"], 2, axis=2)
    v, i = NR.nn_dist(c["x"], y2, 8, "B")
    dist, idx = nn_dist_raw(T(c["x"], dev), T(y2, dev), 8, form="B")
    np.testing.assert_array_equal(N_(idx), i)
    np.testing.assert_array_equal(N_(idx)[:, :, 0::2], 2 * gold["gni4_idx"])
    np.testing.assert_array_equal(N_(idx)[:, :, 1::2], 2 * gold["gni4_idx"] + 1)
    np.testing.assert_array_equal(N_(dist)[:, :, 0::2], gold["gni4_dis"])
    np.testing.assert_array_equal(N_(dist)[:, :, 1::2], gold["gni4_dis"])


# ------------------------------------------------------------------ the public functions
def close_root(got, ref, K, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref) & (ref > 0)
    err = np.abs(got - ref)[ok]
    print(f"{what}: max |got - ref| / ref = {float((err / ref[ok]).max() / NR.U32):.3f} u, bound {K + 3} u")
    assert (err <= NR.root_rtol(K) * ref[ok]).all(), what


def test_public_functions_against_the_fixture(dev, gold):
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    x, y = T(c["x"], dev), T(c["y"], dev)
    out = M.nearest_distances(x, y)
    assert out.shape == (2, 257, 1) and out.dtype == torch.float32
    v, _ = NR.nn_dist(c["x"], c["y"], 1)
    np.testing.assert_array_equal(N_(out)[:, :, 0], np.sqrt(v[:, :, 0]))
    close_root(N_(out), gold["nd_xy"], 1, "nearest_distances")
    for n in "sw":
        out = M.self_nearest_distances(T(c[n], dev))
        v, _ = NR.nn_dist(c[n], c[n], 1, "A", True)
        np.testing.assert_array_equal(N_(out)[:, :, 0], np.sqrt(v[:, :, 0]))
        close_root(N_(out), gold[f"snd_{n}"], 1, f"self_nearest_distances {n}")
    for n, k in (("s", 3), ("w", 3), ("w", 5)):
        out = M.self_nearest_distances_K(T(c[n], dev), k)
        assert out.shape == (c[n].shape[0], c[n].shape[2], 1)
        v, _ = NR.nn_dist(c[n], c[n], k, "A", True)
        np.testing.assert_array_equal(N_(out)[:, :, 0], NR.root(v))
        close_root(N_(out), gold[f"sndk{k}_{n}"], k, f"self_nearest_distances_K {n} {k}")
    idx, dis = M.get_nearest_index(x, y, k=4, return_dis=True)
    assert idx.dtype == torch.int64 and idx.shape == (2, 257, 4) and dis.shape == (2, 257, 4)
    np.testing.assert_array_equal(N_(idx), gold["gni4_idx"])
    np.testing.assert_array_equal(N_(dis), gold["gni4_dis"])
    np.testing.assert_array_equal(N_(M.get_nearest_index(x, y, k=4)), gold["gni4_idx"])
    # the long lists: the root over two and over one wave per query
    for k in (20, 40):
        out = M.self_nearest_distances_K(T(c["s"], dev), k)
        np.testing.assert_array_equal(N_(out)[:, :, 0], NR.root(NR.nn_dist(c["s"], c["s"], k, "A", True)[0]))


def test_tiled_cloud_nan_mask_and_presqrt_values(dev, gold):
    from svdformer_pointsea_amd import model_utils as M

    t = clouds()["t"]
    tt = T(t, dev)
    m = NR.dist_matrix(t, t, "A").min(2)
    out = N_(M.nearest_distances(tt, tt))[:, :, 0]
    np.testing.assert_array_equal(np.isnan(out), m < 0)
    np.testing.assert_array_equal(np.isnan(out), np.isnan(gold["nd_tt"][:, :, 0]))
    np.testing.assert_array_equal(N_(M.nn_dist_raw(tt, tt, 1)[0])[:, :, 0], m)
    for k in (1, 3):
        v, _ = NR.nn_dist(t, t, k, "A", True)
        np.testing.assert_array_equal(N_(M.nn_dist_raw(tt, tt, k, self_diag=True)[0]), v)
        fn = M.self_nearest_distances if k == 1 else (lambda a: M.self_nearest_distances_K(a, 3))
        got, ref = N_(fn(tt))[:, :, 0], gold["snd_t" if k == 1 else "sndk3_t"][:, :, 0]
        np.testing.assert_array_equal(got, NR.root(v))
        pos = (v > 0).all(2)
        close_root(got[pos], ref[pos], k, f"tiled self k={k}")


def test_composed_helpers_on_the_gpu(dev, gold):
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    out = M.indexing_neighbor(T(c["f"], dev), T(gold["ixn_index"], dev).long())
    np.testing.assert_array_equal(N_(out), gold["ixn"])
    s = T(c["s"], dev)
    idx = M.knn(s, 5)
    assert idx.dtype == torch.int64
    np.testing.assert_array_equal(N_(idx), gold["knn_s"])
    np.testing.assert_array_equal(N_(M.get_graph_feature(s, k=5)), gold["ggf_s"])
    sq = M.square_distance(T(c["x"], dev).transpose(1, 2).contiguous(), T(c["y"], dev).transpose(1, 2).contiguous())
    # two evaluations of the expanded form, each within 6 u A of the exact value; A <= 12 in the unit cube
    np.testing.assert_allclose(N_(sq), gold["sqd_xy"], rtol=0, atol=2 * 6 * NR.U32 * 12.0)


# ------------------------------------------------------------------ gradients
def _backward(fn, *arrays, dev, g=None):
    ts = [T(a, dev).requires_grad_(True) for a in arrays]
    out = fn(*ts)
    out.backward(torch.ones_like(out) if g is None else g)
    torch.cuda.synchronize()
    return [N_(t.grad) for t in ts]


def test_gradients_two_clouds(dev, gold):
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    x, y = c["x"], c["y"]
    gx, gy = _backward(M.nearest_distances, x, y, dev=dev)
    v, i = NR.nn_dist(x, y, 1)
    ones = np.ones(v.shape[:2], np.float32)
    np.testing.assert_array_equal(gx, NR.grad_q_fp32(x, y, i, ones, NR.root(v)))
    rq, Eq, rp, Ep = NR.grad_ref(x, y, i, ones, rooted=True)
    print("grad x err/bound", NR.assert_in_bound(gx, rq, Eq, "grad x"))
    print("grad y err/bound", NR.assert_in_bound(gy, rp, Ep, "grad y"))
    NR.assert_in_bound(gold["g_nd_x"], rq, Eq, "reference grad x")
    NR.assert_in_bound(gold["g_nd_y"], rp, Ep, "reference grad y")
    gx2, gy2 = _backward(M.nearest_distances, x, y, dev=dev)
    np.testing.assert_array_equal(gx, gx2)
    np.testing.assert_array_equal(gy, gy2)
    assert (gy[:, :, np.bincount(i[0].ravel(), minlength=130) == 0][0] == 0).all()   # an unpointed target is +0


def test_gradients_one_side_only(dev):
    """Only one cloud requires a gradient: the other side is not computed (grad_p NULL: no pair list, no
    splat; grad_q NULL: the splat alone).  The side that is computed is the two-sided run's bits."""
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    x, y = c["x"], c["y"]
    gx, gy = _backward(M.nearest_distances, x, y, dev=dev)
    v, i = NR.nn_dist(x, y, 1)
    xt, yt = T(x, dev).requires_grad_(True), T(y, dev)
    M.nearest_distances(xt, yt).sum().backward()
    np.testing.assert_array_equal(N_(xt.grad), NR.grad_q_fp32(x, y, i, np.ones(v.shape[:2], np.float32), NR.root(v)))
    np.testing.assert_array_equal(N_(xt.grad), gx)
    assert yt.grad is None
    xt, yt = T(x, dev), T(y, dev).requires_grad_(True)
    M.nearest_distances(xt, yt).sum().backward()
    np.testing.assert_array_equal(N_(yt.grad), gy)
    assert xt.grad is None
    g = np.random.default_rng(11).standard_normal((2, 257, 4)).astype(np.float32)
    xt, yt = T(x, dev).requires_grad_(True), T(y, dev)
    M.get_nearest_index(xt, yt, k=4, return_dis=True)[1].backward(T(g, dev))
    np.testing.assert_array_equal(N_(xt.grad), NR.grad_q_fp32(x, y, NR.nn_dist(x, y, 4, "B")[1], g))


def test_gradients_of_get_nearest_index(dev):
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    x, y = c["x"], c["y"]
    g = np.random.default_rng(7).standard_normal((2, 257, 4)).astype(np.float32)
    gx, gy = _backward(lambda a, b: M.get_nearest_index(a, b, k=4, return_dis=True)[1], x, y, dev=dev, g=T(g, dev))
    _, i = NR.nn_dist(x, y, 4, "B")
    np.testing.assert_array_equal(gx, NR.grad_q_fp32(x, y, i, g))
    rq, Eq, rp, Ep = NR.grad_ref(x, y, i, g)
    NR.assert_in_bound(gx, rq, Eq, "grad target")
    print("grad source err/bound", NR.assert_in_bound(gy, rp, Ep, "grad source"))
    idx = M.get_nearest_index(T(x, dev).requires_grad_(True), T(y, dev), k=4)
    assert not idx.requires_grad


SELF = [("unit1030_k1", 1), ("unit1030_k3", 3), ("s_k3", 3), ("w_k1", 1), ("w_k3", 3), ("w_k5", 5)]


@pytest.mark.parametrize("name,k", SELF, ids=[s[0] for s in SELF])
def test_gradients_one_cloud(dev, gold, name, k):
    from svdformer_pointsea_amd import model_utils as M

    a = NR.cloud_unit(540, 2, 1030) if name.startswith("unit") else clouds()[name[0]]
    fn = M.self_nearest_distances if k == 1 else (lambda t: M.self_nearest_distances_K(t, k))
    (ga,) = _backward(fn, a, dev=dev)
    v, i = NR.nn_dist(a, a, k, "A", True)
    ref, E, _, _ = NR.grad_ref(a, a, i, np.ones(v.shape[:2], np.float32), self_diag=True, rooted=True, same=True)
    print(name, "err/bound", NR.assert_in_bound(ga, ref, E, name))
    key = {"s_k3": "g_sndk3_s", "w_k1": "g_snd_w", "w_k3": "g_sndk3_w", "w_k5": "g_sndk5_w"}.get(name)
    if key:
        NR.assert_in_bound(gold[key], ref, E, "reference " + key)
    (gb,) = _backward(fn, a, dev=dev)
    np.testing.assert_array_equal(ga, gb)
    if name == "w_k1":
        # a point whose own diagonal is its minimum and that is nobody's neighbour gets exactly 0
        n = a.shape[2]
        own = i[0, :, 0] == np.arange(n)
        lonely = own & (np.bincount(i[0, ~own, 0], minlength=n) == 0)
        assert lonely.any()
        assert (ga[0][:, lonely] == 0).all()


def test_diagonal_rows_are_exactly_zero(dev):
    """The diagonal with the two sides apart (the cloud passed twice, `same` off): grad_q of a row whose
    minimum is its own diagonal is exactly 0, every row is the restatement's bits."""
    from svdformer_pointsea_amd.model_utils import _NNDist

    w = clouds()["w"]
    q, p = T(w, dev).requires_grad_(True), T(w, dev).requires_grad_(True)
    for k in (1, 3):
        q.grad = p.grad = None
        val, idx = _NNDist.apply(q, p, k, "A", True, True)
        val.sum().backward()
        v, i = NR.nn_dist(w, w, k, "A", True)
        np.testing.assert_array_equal(N_(idx), i)
        np.testing.assert_array_equal(N_(q.grad), NR.grad_q_fp32(w, w, i, np.ones(v.shape[:2], np.float32), NR.root(v),
                                                                 self_diag=True))
        if k == 1:
            own = i[0, :, 0] == np.arange(w.shape[2])
            assert own.any() and (N_(q.grad)[0][:, own] == 0).all()
            assert (N_(p.grad)[0][:, np.bincount(i[0, ~own, 0], minlength=w.shape[2]) == 0] == 0).all()


def test_a_zero_row_stays_contained(dev):
    """One duplicated pair makes row 7's forward exactly 0 (non-finite gradient terms).  Every other row of
    grad_q, and every target row 7 does not point at, equals the result without the pair."""
    from svdformer_pointsea_amd import model_utils as M

    rng = np.random.default_rng(8)
    x = rng.random((1, 3, 40)).astype(np.float32)
    y = rng.random((1, 3, 30)).astype(np.float32)
    y[0, :, 11] = (0.5, 0.25, 0.75)            # dyadic: every product exact, so d is exactly 0
    xz = x.copy()
    xz[0, :, 7] = y[0, :, 11]
    assert NR.nn_dist(xz, y, 1)[0][0, 7, 0] == 0
    gx0, gy0 = _backward(M.nearest_distances, x, y, dev=dev)
    gx1, gy1 = _backward(M.nearest_distances, xz, y, dev=dev)
    assert np.isfinite(gx0).all() and np.isfinite(gy0).all()
    assert not np.isfinite(gx1[0, :, 7]).any()
    rows = np.arange(40) != 7
    np.testing.assert_array_equal(gx1[:, :, rows], gx0[:, :, rows])
    j0 = NR.nn_dist(x, y, 1)[1][0, 7, 0]
    tg = ~np.isin(np.arange(30), [11, j0])
    np.testing.assert_array_equal(gy1[:, :, tg], gy0[:, :, tg])


# ------------------------------------------------------------------ dispatch
def test_dispatch(dev):
    from svdformer_pointsea_amd import model_utils as M

    rng = np.random.default_rng(9)
    x4, y4 = T(rng.random((2, 4, 70)).astype(np.float32), dev), T(rng.random((2, 4, 50)).astype(np.float32), dev)
    assert torch.equal(M.nearest_distances(x4, y4), M.nearest_distances_chain(x4, y4))
    i, d = M.get_nearest_index(x4, y4, k=3, return_dis=True)
    ic, dc = M.get_nearest_index_chain(x4, y4, 3, True)
    assert torch.equal(i, ic) and torch.equal(d, dc)
    x = T(rng.random((1, 3, 80)).astype(np.float32), dev)
    assert torch.equal(M.self_nearest_distances_K(x, 65), M.self_nearest_distances_K_chain(x, 65))
    xc = x.cpu()
    assert torch.equal(M.self_nearest_distances(xc), M.self_nearest_distances_chain(xc))
    assert M.self_nearest_distances(xc).device.type == "cpu"
    xd = x.double()
    assert M.self_nearest_distances(xd).dtype == torch.float64
    with pytest.raises(RuntimeError):
        M.self_nearest_distances_K(x, 81)
    with pytest.raises(RuntimeError):
        M.get_nearest_index(x, x[:, :, :3], k=4)
    with pytest.raises(RuntimeError):
        M.nn_dist_raw(x, x[:, :, :3], 4)
    with pytest.raises(RuntimeError):
        M.nearest_distances(x, torch.zeros(2, 3, 5, device=dev))
    e = M.nearest_distances(torch.zeros(0, 3, 5, device=dev), torch.zeros(0, 3, 6, device=dev))
    assert e.shape == (0, 5, 1)
    q0 = torch.zeros(2, 3, 0, device=dev, requires_grad=True)
    p0 = torch.rand(2, 3, 6, device=dev, requires_grad=True)
    e = M.nearest_distances(q0, p0)
    assert e.shape == (2, 0, 1)
    e.sum().backward()
    assert p0.grad.shape == (2, 3, 6) and (p0.grad == 0).all()
    i, d = M.get_nearest_index(q0, p0, k=2, return_dis=True)
    assert i.shape == (2, 0, 2) and i.dtype == torch.int64 and d.shape == (2, 0, 2)


# ------------------------------------------------------------------ the chain switch
_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import neighbour_refs as NR
from svdformer_pointsea_amd import model_utils as M
assert not M._NEIGHBOURS_FUSED
g = np.load(sys.argv[1] + "/tests/golden/neighbours.npz")
c = {k[3:]: torch.from_numpy(g[k]).cuda() for k in g.files if k.startswith("in_")}
out = {}
out["nd"] = M.nearest_distances(c["x"], c["y"])
i, d = M.get_nearest_index(c["x"], c["y"], k=4, return_dis=True)
out["gni_i"], out["gni_d"] = i, d
out["snd_s"] = M.self_nearest_distances(c["s"])
out["sndk3_s"] = M.self_nearest_distances_K(c["s"], 3)
out["sndk5_w"] = M.self_nearest_distances_K(c["w"], 5)
out["ixn"] = M.indexing_neighbor(c["f"], i[:, :50] % 40)
torch.cuda.synchronize()
np.savez(sys.argv[2], **{k: v.cpu().numpy() for k, v in out.items()})
"""


def _chain_bound(q, p, k, form, self_diag):
    """|kernel - chain| per row for sqrt(mean_k d): both evaluate d within E_d = 6 u A of the exact value (module
    docstring of neighbour_refs), so the radicands differ by at most 2 mean(E_d) + 2 K u m; through the square
    root: that / (2 val), plus (K + 3) u val for the two roots and means."""
    v, i = NR.nn_dist(q, p, k, form, self_diag)
    q64, p64 = q.astype(np.float64), p.astype(np.float64)
    pj = np.stack([p64[b][:, i[b]] for b in range(q.shape[0])])
    A = (q64 ** 2).sum(1)[:, :, None] + (pj ** 2).sum(1) + 2 * np.abs(q64[:, :, :, None] * pj).sum(1)
    Ed = 6 * NR.U32 * A
    return v, i, Ed


def test_chain_switch_agrees_with_the_kernels(dev, tmp_path):
    from svdformer_pointsea_amd import model_utils as M

    assert M._NEIGHBOURS_FUSED
    path = str(tmp_path / "chain.npz")
    env = dict(os.environ, PCOPS_NEIGHBOURS_FUSED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ch = np.load(path)
    c = clouds()
    x, y = T(c["x"], dev), T(c["y"], dev)
    i, d = M.get_nearest_index(x, y, k=4, return_dis=True)
    np.testing.assert_array_equal(N_(i), ch["gni_i"])
    v, _, Ed = _chain_bound(c["x"], c["y"], 4, "B", False)
    assert (np.abs(N_(d).astype(np.float64) - ch["gni_d"]) <= 2 * Ed).all()
    np.testing.assert_array_equal(N_(M.indexing_neighbor(T(c["f"], dev), i[:, :50] % 40)), ch["ixn"])
    for key, fn, q, p, k, sd in (("nd", lambda: M.nearest_distances(x, y), c["x"], c["y"], 1, False),
                                 ("snd_s", lambda: M.self_nearest_distances(T(c["s"], dev)), c["s"], c["s"], 1, True),
                                 ("sndk3_s", lambda: M.self_nearest_distances_K(T(c["s"], dev), 3), c["s"], c["s"], 3, True),
                                 ("sndk5_w", lambda: M.self_nearest_distances_K(T(c["w"], dev), 5), c["w"], c["w"], 5, True)):
        got = N_(fn())[:, :, 0].astype(np.float64)
        v, _, Ed = _chain_bound(q, p, k, "A", sd)
        val = NR.root(v).astype(np.float64)
        m = v.astype(np.float64).mean(2)
        bound = (2 * Ed.mean(2) + 2 * k * NR.U32 * m) / (2 * val) * 1.01 + (k + 3) * NR.U32 * val
        err = np.abs(got - ch[key][:, :, 0])
        print(key, "max err/bound", float((err / bound).max()))
        assert (err <= bound).all(), key


# ------------------------------------------------------------------ capture
def test_capture_replays_equal_eager(dev):
    """One forward + backward of each reduction captured on one stream, replayed twice with changed inputs and
    every output poisoned before each replay: bit-equal to eager."""
    from svdformer_pointsea_amd import model_utils as M

    c = clouds()
    x, y = T(c["x"], dev).requires_grad_(True), T(c["y"], dev).requires_grad_(True)
    s = T(c["s"], dev).requires_grad_(True)
    g = torch.rand(2, 257, 4, device=dev)
    res = {}

    def run():
        res["nd"] = M.nearest_distances(x, y)
        res["nd_gx"], res["nd_gy"] = torch.autograd.grad(res["nd"].sum(), (x, y))
        res["k3"] = M.self_nearest_distances_K(s, 3)
        (res["k3_g"],) = torch.autograd.grad(res["k3"].sum(), s)
        idx, dis = M.get_nearest_index(x, y, k=4, return_dis=True)
        res["gni_i"], res["gni_d"] = idx, dis
        res["gni_gx"], res["gni_gy"] = torch.autograd.grad(dis, (x, y), g)

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
            x.copy_(torch.roll(x, it + 1, 2) * 0.9)
            y.copy_(torch.roll(y, 1, 2) * 1.1)
            s.copy_(torch.roll(s, 2, 1))
            g.copy_(torch.roll(g, 1, 1))
        for t in outs.values():
            t.detach().fill_(-1 if t.dtype == torch.int64 else float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.detach().clone() for k, t in outs.items()}
        run()
        torch.cuda.synchronize()
        for k in got:
            assert torch.equal(got[k], res[k].detach()), (it, k)
