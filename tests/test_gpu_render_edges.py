"""Edge shapes of the depth renderers (csrc/render.hip) against the CPU oracle.

grid2image at resolutions that are no multiple of its 32 x 32 tile (partial-tile guards,
the -inf max-pool padding and the zero conv padding on a ragged edge), points2grid and
points2depth through the C ABI at other sizes than the models' (H != W: aspect != 1; more
than 8192 * 256 splatted points: the stride loop), outputs inside NaN-poisoned buffers
that start 4 bytes past a 16-byte boundary (pc_fill_kernel's byte head and tail)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from pointops_refs import Poisoned, T
from svdformer_pointsea_amd._lib import call, lib, ptr, stream_of

pytestmark = pytest.mark.gpu

f32 = np.float32


def _cloud(rng, B, N):
    """Half uniform, half a tight cluster (many points per voxel / pixel); never degenerate."""
    p = (rng.random((B, N, 3)) - 0.5).astype(f32)
    p[:, N // 2 + 1:] = (0.2 + 0.01 * rng.standard_normal((B, N - N // 2 - 1, 3))).astype(f32)
    return p


# ------------------------------------------------------------------ grid2image
def _grid2image(dev, real, grid):
    return real.grid2image(T(grid, dev)).cpu().numpy()


@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("R", [5, 31, 32, 33, 37, 65, 224])
def test_grid2image_bitexact(dev, R, D):
    """PCViews_Real.grid2image against oracle.grid2image on the oracle's own grids of two
    different clouds.  The kernel compares, maximises and accumulates the 3 x 3 Gaussian in the
    oracle's order (an out-of-image tap adds kw * 0 = 0 exactly), so the images are equal bit
    for bit, all three channels."""
    from svdformer_pointsea_amd.render import PCViews_Real

    rng = np.random.default_rng(R * 10 + D)
    grid = O.points2grid(_cloud(rng, 2, 500), R, D)
    assert all(grid[b].max() > 0 for b in range(2))
    real = PCViews_Real()
    got = _grid2image(dev, real, grid)
    ref = O.grid2image(grid, real.kernel.numpy())
    assert got.shape == ref.shape == (2, 3, R, R)
    if not np.array_equal(got, ref):
        k = tuple(int(v) for v in np.argwhere(got != ref)[0])
        raise AssertionError(f"first differing pixel (bv, channel, x, y) = {k}: got {got[k]!r}, oracle {ref[k]!r}; "
                             f"{int((got != ref).sum())} of {got.size} differ")
    np.testing.assert_array_equal(got[:, 0], got[:, 1])
    np.testing.assert_array_equal(got[:, 0], got[:, 2])


# ------------------------------------------------------------------ points2grid
def _signed_perm(perm, signs):
    m = np.zeros((3, 3), f32)
    for k, (c, s) in enumerate(zip(perm, signs)):
        m[k, c] = s
    return m


def _points2grid(dev, pts, rot, rot2, trans, R, D):
    (B, N, _), V = pts.shape, rot.shape[0]
    pt, rt, r2t, tt = T(pts, dev), T(rot, dev), T(rot2, dev), T(trans, dev)
    p = Poisoned(dev, (B * V, D, R, R))
    call("points2grid", lib().pcops_points2grid, ptr(pt), ptr(rt), ptr(r2t), ptr(tt), B, N, V, R, D, ptr(p.out),
         stream_of(pt))
    return p.result("points2grid")


@pytest.mark.parametrize("N", [2, 255, 257, 3000])
@pytest.mark.parametrize("R,D", [(37, 5), (32, 3), (224, 8)])
def test_points2grid_bitexact(dev, R, D, N):
    """pcops_points2grid against oracle.points2grid, which takes the transformed points.  View 0:
    both rotations the identity and a zero translation (the kernel's fma chain returns the point
    itself); view 1: signed permutation matrices and a non-zero translation -- the transformed
    point is an exact permutation of the coordinates minus one fp32 subtraction, done here in
    numpy float32.  B = 2 clouds x V = 2 views."""
    rng = np.random.default_rng(R * D + N)
    B, V = 2, 2
    pts = _cloud(rng, B, N) if N > 2 else (rng.random((B, N, 3)) - 0.5).astype(f32)
    rot = np.stack([np.eye(3, dtype=f32), _signed_perm((1, 2, 0), (1, -1, 1))])
    rot2 = np.stack([np.eye(3, dtype=f32), _signed_perm((2, 1, 0), (-1, 1, 1))])
    trans = np.array([[0, 0, 0], [0.25, -0.5, 0.125]], f32)
    tp = np.empty((B, V, N, 3), f32)
    for v in range(V):
        tp[:, v] = ((pts @ rot[v]).astype(f32) @ rot2[v]).astype(f32) - trans[v]
    ref = O.points2grid(tp.reshape(B * V, N, 3), R, D)
    got = _points2grid(dev, pts, rot, rot2, trans, R, D)
    assert (ref > 0).any()
    np.testing.assert_array_equal(got, ref)


# ------------------------------------------------------------------ points2depth
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _depth_counts(points, rot, trans, H, W):
    """Points per pixel, (B*V, H, W): the projection of csrc/render.hip / the oracle restated in
    numpy float32 (the fma chain as one float64 operation rounded to fp32).  Used for the error
    bound only; its hit mask is checked against the oracle's."""
    B, N, _ = points.shape
    V = rot.shape[0]
    p = points[:, None]                                     # (B,1,N,3)
    q = []
    for c in range(3):
        t = p[..., 0] * rot[None, :, None, 0, c]
        t = _fma32(p[..., 1], rot[None, :, None, 1, c], t)
        t = _fma32(p[..., 2], rot[None, :, None, 2, c], t)
        q.append((t - trans[None, :, None, c]).astype(f32))
    eps, aspect = f32(1e-12), f32(W / H)
    with np.errstate(all="ignore"):
        z = q[2]
        cx = (q[0] / (z + eps)) * aspect
        cy = q[1] / (z + eps)
        ex = np.ceil(((cx + f32(1)) * f32(H)) / f32(2) + f32(-0.5))
        ey = np.ceil(((cy + f32(1)) * f32(W)) / f32(2) + f32(-0.5))
        ok = (ex >= 0) & (ex <= H - 1) & (ey >= 0) & (ey <= W - 1) & (z >= 0)
    bv = np.broadcast_to(np.arange(B * V).reshape(B, V, 1), ok.shape)
    pix = (bv[ok] * H + ex[ok].astype(np.int64)) * W + ey[ok].astype(np.int64)
    return np.bincount(pix, minlength=B * V * H * W).reshape(B * V, H, W)


def _views(V):
    """View 0: identity, no translation (the camera at the origin looks along +z); with V = 4
    also the three views of PCViews(TRANS=-0.7)."""
    rot, trans = [np.eye(3, dtype=f32)], [np.zeros(3, f32)]
    if V > 1:
        from svdformer_pointsea_amd.render import PCViews

        pv = PCViews(TRANS=-0.7, RESOLUTION=224)
        rot += list(pv.rot_mat.numpy())
        trans += list(pv.translation.numpy())
    return np.ascontiguousarray(np.stack(rot[:V])), np.ascontiguousarray(np.stack(trans[:V]))


def _depth_cloud(rng, B, N, H, W):
    """Points in front of and behind the view-0 camera, inside and outside its image, plus a
    lattice at z = 1 that lands on rows -1, 0, H-1, H and columns -1, 0, W-1, W of view 0."""
    p = np.empty((B, N, 3), f32)
    p[..., :2] = rng.uniform(-1.2, 1.2, (B, N, 2))
    p[..., 2] = rng.uniform(-0.5, 2.0, (B, N))
    aspect = W / H
    k = 0
    for r in (-1, 0, H - 1, H):
        for c in (-1, 0, W - 1, W):
            p[:, k] = [(2 * (r + 0.25) / H - 1) / aspect, 2 * (c + 0.25) / W - 1, 1.0]
            k += 1
    return p


def _points2depth(dev, pts, rot, trans, H, W, short=0):
    (B, N, _), V = pts.shape, rot.shape[0]
    pt, rt, tt = T(pts, dev), T(rot, dev), T(trans, dev)
    p = Poisoned(dev, (B * V, H, W))
    wsb = lib().pcops_points2depth_workspace_bytes(B, V, H, W)
    assert wsb == B * V * H * W * 4
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    call("points2depth", lib().pcops_points2depth, ptr(pt), ptr(rt), ptr(tt), B, N, V, H, W, ptr(p.out), ptr(ws),
         wsb - short, stream_of(rt))
    return p.result("points2depth")


def _check_depth(got, ref, counts):
    np.testing.assert_array_equal(ref != 0, counts > 0)     # the restated projection is the oracle's
    np.testing.assert_array_equal(got != 0, ref != 0)       # hit mask
    # every summed term is positive: an fp32 sum of n of them in any order is within (n - 1) 2^-24
    # of exact, relatively -- numerator and denominator, oracle and kernel
    tol = 2.0 * counts.max() * 2.0 ** -24
    err = np.abs(got.astype(np.float64) - ref) / np.where(ref != 0, np.abs(ref), 1.0)
    assert err.max() <= tol, (float(err.max()), tol, int(counts.max()))


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("H,W", [(20, 33), (33, 20), (48, 64)])
def test_points2depth_vs_oracle(dev, H, W, V):
    rng = np.random.default_rng(H * 100 + W + V)
    pts = _depth_cloud(rng, 2, 600, H, W)
    rot, trans = _views(V)
    ref = O.points2depth(pts, rot, trans, H, W)
    counts = _depth_counts(pts, rot, trans, H, W)
    # the lattice reaches the four corners of view 0 (rows / columns 0 and H-1 / W-1) ...
    for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert counts[0, r, c] > 0 and counts[V, r, c] > 0
    # ... and some points lie behind the camera
    assert (pts[..., 2] < 0).any()
    _check_depth(_points2depth(dev, pts, rot, trans, H, W), ref, counts)


def test_points2depth_stride_loop(dev):
    """B * V * N = 2,097,600 > 8192 * 256 points into 48 x 64 images: the splat loop runs a
    second time, hundreds of points per pixel."""
    rng = np.random.default_rng(81)
    H, W = 48, 64
    pts = _depth_cloud(rng, 2, 262200, H, W)
    rot, trans = _views(4)
    ref = O.points2depth(pts, rot, trans, H, W)
    counts = _depth_counts(pts, rot, trans, H, W)
    assert counts.max() > 100
    _check_depth(_points2depth(dev, pts, rot, trans, H, W), ref, counts)


def test_points2depth_empty_cloud_and_short_workspace(dev):
    rot, trans = _views(4)
    img = _points2depth(dev, np.zeros((2, 0, 3), f32), rot, trans, 20, 33)
    assert img.shape == (8, 20, 33) and not img.any()
    pts = _depth_cloud(np.random.default_rng(83), 1, 64, 20, 33)
    with pytest.raises(RuntimeError, match="workspace"):
        _points2depth(dev, pts, rot, trans, 20, 33, short=4)
