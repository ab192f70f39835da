"""pcops_ball_group (csrc/pointnet2.hip) on the GPU: raw C-ABI calls into poisoned outputs.

idx must be bit-equal to the CPU oracle's ball_query and to the present pcops_ball_query; the rows
bit-equal to pcops_sa_group on that idx (fp32 and bf16); the guard words around every output
intact.  Built clouds pin the scan's rules: the cut inside a 64-candidate step, steps without a
hit, exactly K hits, the first-hit fill, the all-zero row, the strict `<`, NaN never hitting.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointops_refs import GUARD, LEAD, NAN_BITS, Poisoned, T, assert_grad, group_grad  # noqa: E402


def _O():
    from oracle import oracle as O
    return O


def raw(xyz, new_xyz, pts, radius, K, dev, bf16=False):
    """-> (status, idx (B,S,K) numpy, rows (B,S,K,3+C) torch in fp32 or bf16), guards checked."""
    from svdformer_pointsea_amd._lib import lib, ptr, stream_of

    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    C = 0 if pts is None else pts.shape[2]
    x, q = T(xyz, dev), T(new_xyz, dev)
    p = None if pts is None else T(pts, dev)
    n = B * S * K * (3 + C)
    if n == 0:
        # nothing to write: both outputs point into one poisoned block that must stay untouched
        blk = torch.full((2 * GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
        st = lib().pcops_ball_group(ptr(x), ptr(q), ptr(p), B, N, S, K, C, float(radius), ptr(blk[GUARD:]),
                                    ptr(blk[GUARD:]), 1 if bf16 else 0, stream_of(x))
        torch.cuda.synchronize()
        assert (blk.cpu().numpy() == NAN_BITS).all(), "an empty call wrote"
        dt = torch.bfloat16 if bf16 else torch.float32
        return st, np.zeros((B, S, K), np.int32), torch.zeros(B, S, K, 3 + C, dtype=dt, device=dev)
    idx = Poisoned(dev, (B, S, K), torch.int32)
    if bf16:
        words = (n + 1) // 2
        buf = torch.full((LEAD + words + GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
        out = buf[LEAD:LEAD + words].view(torch.bfloat16)[:n].view(B, S, K, 3 + C)
    else:
        po = Poisoned(dev, (B, S, K, 3 + C))
        out = po.out
    st = lib().pcops_ball_group(ptr(x), ptr(q), ptr(p), B, N, S, K, C, float(radius), ptr(idx.out), ptr(out),
                                1 if bf16 else 0, stream_of(x))
    if st != 0:
        return st, None, None
    got_idx = idx.result("ball_group idx")
    if bf16:
        torch.cuda.synchronize()
        bits = buf.cpu().numpy()
        assert (bits[:LEAD] == NAN_BITS).all() and (bits[LEAD + words:] == NAN_BITS).all(), "bf16 rows: guards"
        rows = out.clone()
        assert not torch.isnan(rows.float()).any()
    else:
        rows = torch.from_numpy(po.result("ball_group rows")).to(dev)
    return st, got_idx, rows


def expect_rows(xyz, new_xyz, pts, idx, dev, dtype):
    """pcops_sa_group on idx (numpy for an empty cloud, which that entry point does not take)."""
    from svdformer_pointsea_amd.model_utils import _SAGroup

    B, N, _ = xyz.shape
    if N == 0:
        S, K = idx.shape[1:]
        C = 0 if pts is None else pts.shape[2]
        rows = np.zeros((B, S, K, 3 + C), np.float32)
        rows[..., :3] = 0.0 - new_xyz[:, :, None, :]
        return torch.from_numpy(rows).to(dev).to(dtype)
    return _SAGroup.apply(T(xyz, dev), T(new_xyz, dev), None if pts is None else T(pts, dev), T(idx, dev), dtype)


def check(xyz, new_xyz, pts, radius, K, dev, want_idx=None):
    from svdformer_pointsea_amd.pointnet2_utils import ball_query

    O = _O()
    st, idx, rows = raw(xyz, new_xyz, pts, radius, K, dev)
    assert st == 0
    ref = O.ball_query(radius, K, xyz, new_xyz)
    assert np.array_equal(idx, ref), "idx vs the oracle"
    if xyz.shape[0] * new_xyz.shape[1] * K:
        cur = ball_query(radius, K, T(xyz, dev), T(new_xyz, dev)).cpu().numpy()
        assert np.array_equal(idx, cur), "idx vs pcops_ball_query"
    if want_idx is not None:
        assert np.array_equal(idx, np.broadcast_to(want_idx, idx.shape)), (idx, want_idx)
    assert torch.equal(rows, expect_rows(xyz, new_xyz, pts, idx, dev, torch.float32)), "fp32 rows"
    st, idx16, rows16 = raw(xyz, new_xyz, pts, radius, K, dev, bf16=True)
    assert st == 0 and np.array_equal(idx16, ref)
    want16 = expect_rows(xyz, new_xyz, pts, idx, dev, torch.bfloat16)
    assert torch.equal(rows16.view(torch.int16), want16.view(torch.int16)), "bf16 rows"
    return idx


def cloud(B, N, S, C, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
    pick = rng.integers(0, max(N, 1), (B, S))
    new_xyz = (np.take_along_axis(xyz, pick[..., None], 1) if N else rng.uniform(0, 1, (B, S, 3))).astype(np.float32)
    pts = rng.standard_normal((B, N, C)).astype(np.float32) if C else None
    return xyz, new_xyz, pts


# every N of {1, 7, 63, 64, 65, 100, 200}, K of {1, 8, 64, 80}, C of {0, 1, 5, 64}, B of {1, 3}, S of {1, 16},
# and the empty sizes of the header's index rule
GRID = [(1, 1, 1, 1, 0), (3, 7, 16, 8, 1), (1, 63, 16, 64, 5), (3, 64, 1, 80, 64), (1, 65, 16, 8, 5),
        (3, 100, 16, 80, 0), (1, 200, 16, 64, 64), (3, 200, 1, 1, 1), (1, 100, 16, 8, 64),
        (2, 0, 3, 4, 2), (0, 10, 4, 4, 1), (2, 10, 0, 4, 1)]


@pytest.mark.parametrize("B,N,S,K,C", GRID)
def test_grid(dev, B, N, S, K, C):
    xyz, new_xyz, pts = cloud(B, N, S, C, 11 * N + K)
    idx = check(xyz, new_xyz, pts, 0.3, K, dev)
    if B * S and N > 1:
        full = (idx != idx[..., :1]).any(-1) | (K == 1)
        print(f"\n[ball_group B={B} N={N} S={S} K={K} C={C}] rows with more than one point: {int(full.sum())} of {B * S}")


def built(N, near, K, C=5, seed=3):
    """One centre at (0.5, 0.5, 0.5), radius 0.1: the points of `near` within it, every other far away."""
    rng = np.random.default_rng(seed)
    xyz = (10.0 + rng.uniform(0, 1, (1, N, 3))).astype(np.float32)
    near = np.asarray(near, np.int64)
    xyz[0, near] = (0.5 + rng.uniform(-0.03, 0.03, (near.size, 3))).astype(np.float32)
    new_xyz = np.full((1, 1, 3), 0.5, np.float32)
    pts = rng.standard_normal((1, N, C)).astype(np.float32)
    return xyz, new_xyz, pts


def _filled(hits, K):
    hits = list(hits)[:K]
    return np.array(hits + [hits[0]] * (K - len(hits)), np.int32) if hits else np.zeros(K, np.int32)


@pytest.mark.parametrize("name,N,near,K", [
    ("cut inside a step", 64, range(64), 8),
    ("cut inside the second step", 130, range(3, 130, 2), 40),
    ("hits in the second and fourth step only", 256, list(range(64, 128)) + list(range(192, 256)), 80),
    ("exactly K hits", 100, [2, 17, 40, 63, 64, 65, 90, 99], 8),
    ("one hit, the fill", 100, [37], 8),
    ("no hit", 100, [], 8),
])
def test_built_clouds(dev, name, N, near, K):
    xyz, new_xyz, pts = built(N, near, K)
    check(xyz, new_xyz, pts, 0.1, K, dev, want_idx=_filled(near, K))


def test_no_hit_after_shifting_the_centres(dev):
    xyz, new_xyz, pts = cloud(3, 100, 16, 5, 5)
    idx = check(xyz, new_xyz + 5.0, pts, 0.3, 8, dev)
    assert (idx == 0).all()


def test_strict_less_than_at_exactly_the_radius(dev):
    xyz = np.array([[[0.5, 0, 0], [0.25, 0, 0], [0, 0.5, 0]]], np.float32)
    check(xyz, np.zeros((1, 1, 3), np.float32), None, 0.5, 4, dev, want_idx=np.full(4, 1, np.int32))


def test_nan_coordinate_never_hits(dev):
    xyz, new_xyz, pts = built(70, [0, 5, 66], 4)
    xyz[0, 0, 1] = np.nan
    st, idx, rows = raw(xyz, new_xyz, pts, 0.1, 4, dev)
    assert st == 0 and np.array_equal(idx[0, 0], [5, 66, 5, 5])
    assert np.array_equal(idx, _O().ball_query(0.1, 4, xyz, new_xyz))


def test_k_beyond_the_limit_is_refused_and_the_python_layer_takes_the_chain(dev, monkeypatch):
    from svdformer_pointsea_amd import model_utils as mu
    from svdformer_pointsea_amd.pointnet2_utils import ball_query

    assert mu.BALL_GROUP_MAX_K == 1024
    xyz, new_xyz, pts = cloud(2, 100, 4, 5, 9)
    assert raw(xyz, new_xyz, pts, 0.3, 2048, dev)[0] == 1          # PCOPS_ERR_INVALID
    assert raw(xyz, new_xyz, pts, 0.3, 1025, dev)[0] == 1
    check(xyz, new_xyz, pts, 0.3, 1024, dev)
    x, q, p = T(xyz, dev), T(new_xyz, dev), T(pts, dev)
    rows, idx = mu.ball_group_rows(x, q, p, 0.3, 2048)
    ref = ball_query(0.3, 2048, x, q)
    assert torch.equal(idx, ref) and torch.equal(rows, mu._SAGroup.apply(x, q, p, ref, torch.float32))
    # the module: fused switch on and off give the same bits
    torch.manual_seed(0)
    sa = mu.PointNet_SA_Module(4, 2048, 0.3, 5, [8]).to(dev).eval()
    feat = p.transpose(1, 2).contiguous()
    with torch.no_grad():
        a = sa(x.transpose(1, 2).contiguous(), feat)
        monkeypatch.setattr(mu, "_PN2_FUSED", False)
        b = sa(x.transpose(1, 2).contiguous(), feat)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("bf16", [False, True])
def test_backward_through_ball_group_cl(dev, bf16):
    from svdformer_pointsea_amd import model_utils as mu

    B, N, S, K, C = 3, 100, 16, 8, 5
    xyz, _, pts = cloud(B, N, S, C, 21)
    p = T(pts, dev).requires_grad_(True)
    dt = torch.bfloat16 if bf16 else torch.float32
    _, feat, idx = mu.ball_group_cl(T(xyz, dev).transpose(1, 2).contiguous(), p, S, K, 0.3, dt)
    assert feat.shape == (B, 3 + C, S, K) and feat.is_contiguous(memory_format=torch.channels_last)
    g = torch.randn(B, 3 + C, S, K, generator=torch.Generator().manual_seed(1)).to(dev).to(dt)
    feat.backward(g.contiguous(memory_format=torch.channels_last))
    ref, n, Sm = group_grad(g[:, 3:].float().cpu().numpy(), idx.cpu().numpy(), N)
    r = assert_grad(p.grad.transpose(1, 2).cpu().numpy(), ref, n, Sm, "ball_group_cl grad")
    print(f"\n[ball_group_cl backward bf16={bf16}] worst error / bound {r:.3g}")


def test_autocast_rows_are_sa_group_bf16(dev):
    from svdformer_pointsea_amd import model_utils as mu

    xyz, _, pts = cloud(2, 100, 16, 5, 23)
    x, p = T(xyz, dev), T(pts, dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        new_xyz, feat, idx = mu.ball_group_cl(x.transpose(1, 2).contiguous(), p, 16, 8, 0.3, mu._rows_dtype())
    assert feat.dtype == torch.bfloat16
    want = mu._SAGroup.apply(x, new_xyz.transpose(1, 2).contiguous(), p, idx, torch.bfloat16)
    assert torch.equal(feat.permute(0, 2, 3, 1).contiguous().view(torch.int16), want.view(torch.int16))
