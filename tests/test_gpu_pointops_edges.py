"""Edge shapes of the pointnet2 primitives (csrc/pointops.hip, the gather kernels of
csrc/sampling.hip, pc_fill_kernel of csrc/common.h) through the C ABI.

Every call writes into a caller-allocated output that lives inside a larger poisoned
tensor: the output starts one float past a 16-byte boundary, 64+ guard words lie on each
side, every word holds the NaN bit pattern before the call.  After the call every output
element must have been written and the guards must be bitwise untouched.

Forward results and indices are compared bit for bit (float64 references of
tests/pointops_refs.py, CPU oracle); scatter-add gradients per element against
(n + 1) * 2^-24 * S with n and S from the reference (pointops_refs.grad_bound).

Paths the shapes reach: the second and third LDS tile of three_nn_kernel and its j >= N
lanes; a second iteration of every grid-stride loop (more than 8192 * 256 elements, more
than 8192 * 64 ball queries); xcd_span's ragged last range, ranges that start at or past
the total, chunks that are no multiple of 256 and its stride loop; pc_fill_kernel's byte
head and tail and its stride loop (a buffer over 8 MiB); the out-of-range index rule."""
import numpy as np
import pytest
import torch

import pointops_refs as R
from pointops_refs import Poisoned, T
from oracle import oracle as O
from svdformer_pointsea_amd._lib import call, lib, ptr, stream_of

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


# ------------------------------------------------------------------ C-ABI wrappers
def c_gather(dev, f, idx):
    (B, C, N), M = f.shape, idx.shape[1]
    ft, it, p = T(f, dev), T(idx, dev), Poisoned(dev, (B, C, M))
    call("gather_points", lib().pcops_gather_points, ptr(ft), ptr(it), B, C, N, M, ptr(p.out), stream_of(ft))
    return p.result("gather_points")


def c_group(dev, f, idx):
    (B, C, N), (_, S, K) = f.shape, idx.shape
    ft, it, p = T(f, dev), T(idx, dev), Poisoned(dev, (B, C, S, K))
    call("group_points", lib().pcops_group_points, ptr(ft), ptr(it), B, C, N, S, K, ptr(p.out), stream_of(ft))
    return p.result("group_points")


def c_three_interpolate(dev, f, idx, w):
    (B, C, M), N = f.shape, idx.shape[1]
    ft, it, wt, p = T(f, dev), T(idx, dev), T(w, dev), Poisoned(dev, (B, C, N))
    call("three_interpolate", lib().pcops_three_interpolate, ptr(ft), ptr(it), ptr(wt), B, C, M, N, ptr(p.out),
         stream_of(it))
    return p.result("three_interpolate")


def c_gather_grad(dev, go, idx, N, runs=1):
    """`runs` calls into ONE poisoned buffer (the output is overwritten, never accumulated)."""
    B, C, M = go.shape
    gt, it, p = T(go, dev), T(idx, dev), Poisoned(dev, (B, C, N))
    out = []
    for _ in range(runs):
        call("gather_points_grad", lib().pcops_gather_points_grad, ptr(gt), ptr(it), B, C, N, M, ptr(p.out),
             stream_of(gt))
        out.append(p.result("gather_points_grad"))
    return out


def c_group_grad(dev, go, idx, N, runs=1):
    B, C, S, K = go.shape
    gt, it, p = T(go, dev), T(idx, dev), Poisoned(dev, (B, C, N))
    out = []
    for _ in range(runs):
        call("group_points_grad", lib().pcops_group_points_grad, ptr(gt), ptr(it), B, C, N, S, K, ptr(p.out),
             stream_of(gt))
        out.append(p.result("group_points_grad"))
    return out


def c_three_interpolate_grad(dev, go, idx, w, M, runs=1):
    B, C, N = go.shape
    gt, it, wt, p = T(go, dev), T(idx, dev), T(w, dev), Poisoned(dev, (B, C, M))
    out = []
    for _ in range(runs):
        call("three_interpolate_grad", lib().pcops_three_interpolate_grad, ptr(gt), ptr(it), ptr(wt), B, C, N, M,
             ptr(p.out), stream_of(gt))
        out.append(p.result("three_interpolate_grad"))
    return out


def c_three_nn(dev, unknown, known):
    (B, N, _), M = unknown.shape, known.shape[1]
    ut, kt = T(unknown, dev), T(known, dev)
    d, i = Poisoned(dev, (B, N, 3)), Poisoned(dev, (B, N, 3), torch.int32)
    call("three_nn", lib().pcops_three_nn, ptr(ut), ptr(kt), B, N, M, ptr(d.out), ptr(i.out), stream_of(ut))
    return d.result("three_nn dist2"), i.result("three_nn idx")


def c_ball_query(dev, radius, nsample, xyz, new_xyz):
    (B, N, _), M = xyz.shape, new_xyz.shape[1]
    xt, nt, p = T(xyz, dev), T(new_xyz, dev), Poisoned(dev, (B, M, nsample), torch.int32)
    call("ball_query", lib().pcops_ball_query, ptr(nt), ptr(xt), B, N, M, float(radius), int(nsample), ptr(p.out),
         stream_of(nt))
    return p.result("ball_query")


# ------------------------------------------------------------------ inputs
def make_idx(rng, shape, n, oob=False):
    """Indices into [0, n) with heavy duplication: per batch row a third all equal, a third
    sorted, the rest random; batch 0 of three or more all equal.  oob: about a tenth of the
    positions replaced by -1, n, INT32_MIN, INT32_MAX, n + 7 (all skipped by the kernels'
    unsigned compare, never used as an address)."""
    idx = rng.integers(0, n, shape).astype(np.int32)
    flat = idx.reshape(shape[0], -1)
    L = flat.shape[1]
    for b in range(shape[0]):
        flat[b, :L // 3] = flat[b, 0]
        flat[b, L // 3:2 * L // 3].sort()
    if shape[0] >= 3:
        flat[0, :] = flat[0, 0]
    if oob:
        bad = np.array([-1, n, I32_MIN, I32_MAX, n + 7], np.int64).astype(np.int32)
        hit = rng.random(flat.shape) < 0.1
        k = min(len(bad), L)
        hit[:, :k] = True
        vals = bad[rng.integers(0, len(bad), flat.shape)]
        vals[:, :k] = bad[:k]
        flat[hit] = vals[hit]
    return idx


# (B, C, N, M): total % 8 != 0 and M > N; N = 1; total 9 (xcd ranges starting past the total); chunk % 256 != 0;
# total > 8192 * 256 (every stride loop iterates)
GATHER_SHAPES = [(3, 5, 37, 41), (1, 1, 1, 7), (1, 3, 4, 3), (2, 3, 9, 300011), (2, 65, 130, 16400)]
# (B, C, N, S, K)
GROUP_SHAPES = [(3, 5, 37, 41, 3), (1, 1, 1, 7, 1), (2, 3, 9, 27273, 11), (2, 65, 129, 129, 130)]
# (B, C, M, N) of three_interpolate: points (B,C,M), N queries
INTERP_SHAPES = [(3, 5, 37, 41), (1, 1, 1, 7), (2, 3, 9, 300011), (2, 65, 130, 16400)]


# ------------------------------------------------------------------ forward, bit-exact
@pytest.mark.parametrize("oob", [False, True], ids=["inrange", "oob"])
@pytest.mark.parametrize("B,C,N,M", GATHER_SHAPES)
def test_gather_forward_bitexact(dev, B, C, N, M, oob):
    rng = np.random.default_rng(B * C * N + M + oob)
    f = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = make_idx(rng, (B, M), N, oob)
    got = c_gather(dev, f, idx)
    np.testing.assert_array_equal(got, R.gather(f, idx).astype(np.float32))
    if oob:
        bad = (idx.astype(np.int64) < 0) | (idx.astype(np.int64) >= N)
        assert bad.any() and (got[np.broadcast_to(bad[:, None, :], got.shape)] == 0).all()


@pytest.mark.parametrize("oob", [False, True], ids=["inrange", "oob"])
@pytest.mark.parametrize("B,C,N,S,K", GROUP_SHAPES)
def test_group_forward_bitexact(dev, B, C, N, S, K, oob):
    rng = np.random.default_rng(B * C * N + S * K + oob)
    f = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = make_idx(rng, (B, S, K), N, oob)
    got = c_group(dev, f, idx)
    np.testing.assert_array_equal(got, R.group(f, idx).astype(np.float32))
    if oob:
        bad = (idx.astype(np.int64) < 0) | (idx.astype(np.int64) >= N)
        assert bad.any() and (got[np.broadcast_to(bad[:, None], got.shape)] == 0).all()


@pytest.mark.parametrize("oob", [False, True], ids=["inrange", "oob"])
@pytest.mark.parametrize("B,C,M,N", INTERP_SHAPES)
def test_three_interpolate_forward_bitexact(dev, B, C, M, N, oob):
    """Against the float64 restatement of the kernel's fma chain (equal to the oracle on
    in-range indices: tests/test_pointops_refs_cpu.py); the last shape runs the stride loop."""
    rng = np.random.default_rng(B * C * M + N + oob)
    f = rng.standard_normal((B, C, M)).astype(np.float32)
    idx = make_idx(rng, (B, N, 3), M, oob)
    w = rng.random((B, N, 3)).astype(np.float32)
    got = c_three_interpolate(dev, f, idx, w)
    np.testing.assert_array_equal(got, R.three_interpolate(f, idx, w).astype(np.float32))
    if not oob and B * C * N <= 100000:
        np.testing.assert_array_equal(got, O.three_interpolate(f, idx, w))


# ------------------------------------------------------------------ scatter-add grads
# the shapes above; (1, 3, 750002, 5): a 9,000,024-byte grad buffer (> 8 MiB: the fill's stride loop),
# 12-byte head and 12-byte tail
@pytest.mark.parametrize("oob", [False, True], ids=["inrange", "oob"])
@pytest.mark.parametrize("B,C,N,M", GATHER_SHAPES + [(1, 3, 750002, 5)])
def test_gather_grad_bound(dev, B, C, N, M, oob):
    rng = np.random.default_rng(B * C * N + M + 2 * oob)
    go = rng.standard_normal((B, C, M)).astype(np.float32)
    idx = make_idx(rng, (B, M), N, oob)
    ref, n, S = R.gather_grad(go, idx, N)
    runs = 2 if (B, C, N, M) == GATHER_SHAPES[0] else 1
    for k, got in enumerate(c_gather_grad(dev, go, idx, N, runs)):
        R.assert_grad(got, ref, n, S, f"gather_grad run {k}")


@pytest.mark.parametrize("oob", [False, True], ids=["inrange", "oob"])
@pytest.mark.parametrize("B,C,N,S,K", GROUP_SHAPES)
def test_group_grad_bound(dev, B, C, N, S, K, oob):
    rng = np.random.default_rng(B * C * N + S * K + 2 * oob)
    go = rng.standard_normal((B, C, S, K)).astype(np.float32)
    idx = make_idx(rng, (B, S, K), N, oob)
    ref, n, Sm = R.group_grad(go, idx, N)
    runs = 2 if (B, C, N, S, K) == GROUP_SHAPES[0] else 1
    for k, got in enumerate(c_group_grad(dev, go, idx, N, runs)):
        R.assert_grad(got, ref, n, Sm, f"group_grad run {k}")


@pytest.mark.parametrize("oob", [False, True], ids=["inrange", "oob"])
@pytest.mark.parametrize("B,C,M,N", INTERP_SHAPES)
def test_three_interpolate_grad_bound(dev, B, C, M, N, oob):
    rng = np.random.default_rng(B * C * M + N + 2 * oob)
    go = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = make_idx(rng, (B, N, 3), M, oob)
    w = rng.random((B, N, 3)).astype(np.float32)
    ref, n, S = R.three_interpolate_grad(go, idx, w, M)
    runs = 2 if (B, C, M, N) == INTERP_SHAPES[0] else 1
    for k, got in enumerate(c_three_interpolate_grad(dev, go, idx, w, M, runs)):
        R.assert_grad(got, ref, n, S, f"three_interpolate_grad run {k}")


@pytest.mark.parametrize("op", ["gather", "group", "three_interpolate"])
def test_grad_all_indices_equal(dev, op):
    """About 10^5 terms onto ONE column per channel (a flat rtol = atol = 1e-5 does not hold
    for a sum of 10^5 O(1) terms in arbitrary order; the (n, S) bound does), every other
    column exactly 0."""
    rng = np.random.default_rng(len(op))
    if op == "gather":
        go = rng.standard_normal((1, 2, 100000)).astype(np.float32)
        idx = np.full((1, 100000), 17, np.int32)
        ref, n, S = R.gather_grad(go, idx, 50)
        got = c_gather_grad(dev, go, idx, 50)[0]
    elif op == "group":
        go = rng.standard_normal((1, 2, 6250, 16)).astype(np.float32)
        idx = np.full((1, 6250, 16), 17, np.int32)
        ref, n, S = R.group_grad(go, idx, 50)
        got = c_group_grad(dev, go, idx, 50)[0]
    else:
        go = rng.standard_normal((1, 2, 33334)).astype(np.float32)
        idx = np.full((1, 33334, 3), 3, np.int32)
        w = rng.random((1, 33334, 3)).astype(np.float32)
        ref, n, S = R.three_interpolate_grad(go, idx, w, 8)
        got = c_three_interpolate_grad(dev, go, idx, w, 8)[0]
    assert n.max() >= 100000 and (n > 0).sum() == 2
    R.assert_grad(got, ref, n, S, op + "_grad, all indices equal")


def test_group_grad_graph_replay(dev):
    """pcops_group_points_grad (fill kernel + scatter-add) captured on one stream, replayed
    three times with a new input gradient each time: every replay overwrites the output and
    meets the bound for its own input."""
    B, C, N, S, K = 2, 3, 19, 23, 5
    rng = np.random.default_rng(31)
    idx = make_idx(rng, (B, S, K), N, oob=True)
    gos = [rng.standard_normal((B, C, S, K)).astype(np.float32) * s for s in (1.0, 100.0, 0.01)]
    it, go_s, p = T(idx, dev), T(gos[0], dev).clone(), Poisoned(dev, (B, C, N))

    def run():
        call("group_points_grad", lib().pcops_group_points_grad, ptr(go_s), ptr(it), B, C, N, S, K, ptr(p.out),
             stream_of(go_s))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k in (1, 2, 0):
        go_s.copy_(T(gos[k], dev))
        graph.replay()
        ref, n, Sm = R.group_grad(gos[k], idx, N)
        R.assert_grad(p.result("group_points_grad replay"), ref, n, Sm, f"replay with input {k}")


# ------------------------------------------------------------------ three_nn
def _interp_weights(d2):
    """The models' inverse-distance weights (fp32), 0 for the inf distances of M < 3."""
    with np.errstate(over="ignore"):
        r = (np.float32(1.0) / (np.sqrt(d2) + np.float32(1e-8))).astype(np.float32)
    return (r / r.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("N", [1, 255, 257, 300])
@pytest.mark.parametrize("M", [1, 2, 3, 1023, 1024, 1025, 2500])
def test_three_nn_bitexact(dev, M, N):
    """idx and dist^2 against the oracle, bit for bit: one, two and three 1024-point LDS tiles
    (and the tile boundary), N off the 256-thread block (the clamped j >= N lanes), M < 3 (inf
    distances and index 0, as the reference's 1e40 initialisation), two different clouds."""
    rng = np.random.default_rng(M * 1000 + N)
    unknown = rng.random((2, N, 3)).astype(np.float32)
    known = rng.random((2, M, 3)).astype(np.float32)
    d2, idx = c_three_nn(dev, unknown, known)
    _, oidx, od2 = O.three_nn(unknown, known)
    np.testing.assert_array_equal(idx, oidx)
    np.testing.assert_array_equal(d2, od2)
    if M < 3:
        assert np.isinf(d2[..., M:]).all() and (idx[..., M:] == 0).all()
    # three_interpolate with these neighbours and weights
    w = _interp_weights(d2)
    f = rng.standard_normal((2, 3, M)).astype(np.float32)
    got = c_three_interpolate(dev, f, idx, w)
    np.testing.assert_array_equal(got, O.three_interpolate(f, oidx, w))
    np.testing.assert_array_equal(got, R.three_interpolate(f, idx, w).astype(np.float32))


def test_three_nn_planted_neighbours(dev):
    """Neighbours that only a correct tile walk finds: one known point duplicated at indices 7,
    1023 and 1024 (last of tile 0, first of tile 1) and queried exactly -> (7, 1023, 1024)
    with zero distances (strict '<': the first of equals wins); a query whose three nearest
    all lie in the third tile (k = t0 + e with t0 = 2048)."""
    rng = np.random.default_rng(41)
    M, N = 2500, 300
    known = rng.random((2, M, 3)).astype(np.float32)
    unknown = rng.random((2, N, 3)).astype(np.float32)
    P = np.array([0.3125, 0.625, 0.875], np.float32)
    known[:, [7, 1023, 1024]] = P
    unknown[:, 0] = P
    Q = np.array([5.0, 5.0, 5.0], np.float32)
    known[0, [2100, 2300, 2499]] = Q + np.array([[0.01, 0, 0], [0, 0.02, 0], [0, 0, 0.03]], np.float32)
    known[1, [2048, 2049, 2050]] = Q + np.array([[0, 0, 0.03], [0.01, 0, 0], [0, 0.02, 0]], np.float32)
    unknown[:, 299] = Q
    d2, idx = c_three_nn(dev, unknown, known)
    _, oidx, od2 = O.three_nn(unknown, known)
    np.testing.assert_array_equal(idx, oidx)
    np.testing.assert_array_equal(d2, od2)
    for b in range(2):
        assert idx[b, 0].tolist() == [7, 1023, 1024] and (d2[b, 0] == 0).all()
    assert idx[0, 299].tolist() == [2100, 2300, 2499]
    assert idx[1, 299].tolist() == [2049, 2050, 2048]


def test_three_nn_no_known_points(dev):
    """M = 0: every distance inf, every index 0 (the reference's initial values); interpolating
    with those indices (all out of range of an empty cloud) gives zeros.  Empty tensors have a
    NULL data pointer: the entry points accept it for a cloud they never read."""
    rng = np.random.default_rng(43)
    unknown = rng.random((2, 257, 3)).astype(np.float32)
    d2, idx = c_three_nn(dev, unknown, np.zeros((2, 0, 3), np.float32))
    assert np.isposinf(d2).all() and (idx == 0).all()
    _, oidx, od2 = O.three_nn(unknown, np.zeros((2, 0, 3), np.float32))
    np.testing.assert_array_equal(idx, oidx)
    np.testing.assert_array_equal(d2, od2)
    w = np.full((2, 257, 3), 1 / 3, np.float32)
    out = c_three_interpolate(dev, np.zeros((2, 4, 0), np.float32), idx, w)
    assert out.shape == (2, 4, 257) and not out.any()


# ------------------------------------------------------------------ ball_query
@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("nsample", [1, 8])
def test_ball_query_small_bitexact(dev, M, nsample):
    """M off the 64-lane block, nsample > N = 3 (a row is the first hit repeated, then the hits)."""
    rng = np.random.default_rng(M + nsample)
    xyz = rng.random((2, 3, 3)).astype(np.float32)
    new = rng.random((2, M, 3)).astype(np.float32)
    for radius in (0.4, 0.9, 3.0):
        got = c_ball_query(dev, radius, nsample, xyz, new)
        np.testing.assert_array_equal(got, O.ball_query(radius, nsample, xyz, new))


def test_ball_query_empty_cloud(dev):
    """N = 0: no hit, rows of zeros (the reference's zero-initialised output)."""
    new = np.random.default_rng(51).random((2, 65, 3)).astype(np.float32)
    got = c_ball_query(dev, 0.5, 4, np.zeros((2, 0, 3), np.float32), new)
    assert got.shape == (2, 65, 4) and not got.any()


def test_ball_query_strict_boundary_and_nan(dev):
    """d2 < r2 is strict: with radius 0.5 a point at distance exactly 0.5 is out and one at
    nextafter(0.5, 0) is in -> [0, 2, 3, 0].  A NaN query coordinate hits nothing."""
    below = np.nextafter(np.float32(0.5), np.float32(0))
    xyz = np.array([[[0, 0, 0], [0.5, 0, 0], [below, 0, 0], [0, 0.25, 0]]], np.float32)
    new = np.array([[[0, 0, 0], [np.nan, 0, 0], [0, 0, np.nan], [0.5, 0, 0]]], np.float32)
    got = c_ball_query(dev, 0.5, 4, xyz, new)
    ref = O.ball_query(0.5, 4, xyz, new)
    assert ref[0, 0].tolist() == [0, 2, 3, 0]
    np.testing.assert_array_equal(got, ref)
    assert got[0, 0].tolist() == [0, 2, 3, 0]
    assert not got[0, 1].any() and not got[0, 2].any()


def test_ball_query_stride_loop(dev):
    """B * M = 524,418 > 8192 * 64 queries: the query loop runs a second time."""
    rng = np.random.default_rng(53)
    B, M, N, ns = 2, 262209, 8, 4
    xyz = rng.random((B, N, 3)).astype(np.float32)
    new = rng.random((B, M, 3)).astype(np.float32)
    new[:, ::1000] += 7.0   # rows with no hit
    got = c_ball_query(dev, 0.45, ns, xyz, new)
    np.testing.assert_array_equal(got, O.ball_query(0.45, ns, xyz, new))


# ------------------------------------------------------------------ QueryAndGroup / GroupAll
@pytest.mark.parametrize("use_xyz", [True, False])
def test_query_and_group(dev, use_xyz):
    from svdformer_pointsea_amd.pointnet2_utils import QueryAndGroup

    rng = np.random.default_rng(61 + use_xyz)
    B, N, M, C, ns, radius = 2, 100, 37, 5, 8, 0.3
    xyz = rng.random((B, N, 3)).astype(np.float32)
    new = np.ascontiguousarray(xyz[:, rng.permutation(N)[:M]])
    new[:, 0] += 9.0   # a query with no neighbour: a row of index 0
    feat = rng.standard_normal((B, C, N)).astype(np.float32)
    ft = T(feat, dev).requires_grad_(True)
    out = QueryAndGroup(radius, ns, use_xyz=use_xyz)(T(xyz, dev), T(new, dev), ft)
    idx = O.ball_query(radius, ns, xyz, new)
    gx = O.grouping_operation(np.ascontiguousarray(xyz.transpose(0, 2, 1)), idx) - new.transpose(0, 2, 1)[..., None]
    gf = O.grouping_operation(feat, idx)
    ref = np.concatenate([gx, gf], 1) if use_xyz else gf
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    go = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(T(go, dev))
    r, n, S = R.group_grad(np.ascontiguousarray(go[:, 3:] if use_xyz else go), idx, N)
    R.assert_grad(ft.grad.cpu().numpy(), r, n, S, "QueryAndGroup feature grad")
    # xyz alone
    only = QueryAndGroup(radius, ns)(T(xyz, dev), T(new, dev)).cpu().numpy()
    np.testing.assert_array_equal(only, gx)


@pytest.mark.parametrize("use_xyz", [True, False])
def test_group_all(dev, use_xyz):
    from svdformer_pointsea_amd.pointnet2_utils import GroupAll

    rng = np.random.default_rng(71 + use_xyz)
    B, N, C = 2, 33, 5
    xyz = rng.random((B, N, 3)).astype(np.float32)
    feat = rng.standard_normal((B, C, N)).astype(np.float32)
    ft = T(feat, dev).requires_grad_(True)
    out = GroupAll(use_xyz=use_xyz)(T(xyz, dev), None, ft)
    gx = xyz.transpose(0, 2, 1)[:, :, None]
    ref = np.concatenate([gx, feat[:, :, None]], 1) if use_xyz else feat[:, :, None]
    np.testing.assert_array_equal(out.detach().cpu().numpy(), ref)
    go = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(T(go, dev))
    np.testing.assert_array_equal(ft.grad.cpu().numpy(), (go[:, 3:] if use_xyz else go)[:, :, 0])
    np.testing.assert_array_equal(GroupAll()(T(xyz, dev), None).cpu().numpy(), gx)
