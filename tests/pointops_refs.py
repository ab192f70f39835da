"""Plain numpy float64 references of the pointnet2 gather / group / three_interpolate
ops and their scatter-add gradients (a helper module of the tests, not a conftest).

Index rule (include/pcops.h): an index outside [0, n) contributes zero -- the forward
reads 0 there, the gradient adds nothing -- and is never used as an address.

Forward references return float64 arrays holding the exact result (gather, group: a
copy; three_interpolate: the kernel's fma chain restated with float64 arithmetic and a
rounding to fp32 after each step), so `.astype(np.float32)` is the expected output bit
for bit.

Gradient references return (ref, n, S), per output element:
  ref  float64 sum of the terms (each term is an fp32 number: grad_out itself, or the
       fp32 product grad_out * weight),
  n    how many terms were added,
  S    sum of |term|.
fp32 additions of n terms in ANY order (float atomics) differ from `ref` by at most
(n - 1) * 2^-24 * S to first order; `grad_bound` is the tests' margin
(n + 1) * 2^-24 * S, and an element with n == 0 must be exactly 0.
"""
import numpy as np

U32 = 2.0 ** -24  # fp32 unit roundoff


def _split(idx, n):
    """int index array -> (in-range mask, int64 indices with the out-of-range ones set to 0)."""
    a = np.asarray(idx).astype(np.int64)
    ok = (a >= 0) & (a < n)
    return ok, np.where(ok, a, 0)


def gather(points, idx):
    """points (B,C,N), idx (B,M) -> (B,C,M) float64: points[b,c,idx[b,m]], 0 out of range."""
    points = np.asarray(points)
    B, C, N = points.shape
    M = idx.shape[1]
    if N == 0:
        return np.zeros((B, C, M), np.float64)
    ok, a = _split(idx, N)
    out = np.take_along_axis(points.astype(np.float64), np.broadcast_to(a[:, None, :], (B, C, M)), axis=2)
    return np.where(ok[:, None, :], out, 0.0)


def group(points, idx):
    """points (B,C,N), idx (B,S,K) -> (B,C,S,K) float64."""
    B, S, K = idx.shape
    return gather(points, np.asarray(idx).reshape(B, S * K)).reshape(B, points.shape[1], S, K)


def _scatter(terms, ok, a, n_out):
    """terms (B,C,L) float64, ok/a (B,L) -> (ref, n, S) of shape (B,C,n_out)."""
    B, C, L = terms.shape
    if n_out == 0:
        z = np.zeros((B, C, 0))
        return z, z.astype(np.int64), z.copy()
    rows = np.arange(B * C, dtype=np.int64).reshape(B, C, 1) * n_out
    flat = (rows + a[:, None, :])[np.broadcast_to(ok[:, None, :], (B, C, L))]
    t = terms[np.broadcast_to(ok[:, None, :], (B, C, L))]
    size = B * C * n_out
    ref = np.bincount(flat, weights=t, minlength=size).reshape(B, C, n_out)
    cnt = np.bincount(flat, minlength=size).reshape(B, C, n_out)
    mag = np.bincount(flat, weights=np.abs(t), minlength=size).reshape(B, C, n_out)
    return ref, cnt, mag


def gather_grad(grad_out, idx, n):
    """grad_out (B,C,M), idx (B,M) -> (ref, n, S) of shape (B,C,n)."""
    ok, a = _split(idx, n)
    return _scatter(np.asarray(grad_out, np.float32).astype(np.float64), ok, a, n)


def group_grad(grad_out, idx, n):
    """grad_out (B,C,S,K), idx (B,S,K) -> (ref, n, S) of shape (B,C,n)."""
    B, C, S, K = grad_out.shape
    return gather_grad(np.asarray(grad_out).reshape(B, C, S * K), np.asarray(idx).reshape(B, S * K), n)


def _f32(x):
    return x.astype(np.float32).astype(np.float64)


def three_interpolate(points, idx, weight):
    """points (B,C,M), idx / weight (B,N,3) -> (B,C,N) float64 holding fp32 values:
    fma(p2, w2, fma(p0, w0, p1 * w1)), each step rounded to fp32 (a product of two fp32
    numbers is exact in float64, so each step is one float64 operation, then the rounding)."""
    B, N, _ = idx.shape
    w = np.asarray(weight, np.float32).astype(np.float64)
    p = [gather(points, np.asarray(idx)[:, :, r]) for r in range(3)]  # (B,C,N) each
    t = _f32(p[1] * w[:, None, :, 1])
    t = _f32(p[0] * w[:, None, :, 0] + t)
    return _f32(p[2] * w[:, None, :, 2] + t)


def three_interpolate_grad(grad_out, idx, weight, m):
    """grad_out (B,C,N), idx / weight (B,N,3) -> (ref, n, S) of shape (B,C,m); the terms are
    the fp32 products grad_out[b,c,j] * weight[b,j,r]."""
    g = np.asarray(grad_out, np.float32)
    w = np.asarray(weight, np.float32)
    B, C, N = g.shape
    terms = (g[:, :, :, None] * w[:, None, :, :]).astype(np.float64).reshape(B, C, N * 3)  # fp32 product
    ok, a = _split(np.asarray(idx).reshape(B, N * 3), m)
    return _scatter(terms, ok, a, m)


def grad_bound(n, S):
    """(n + 1) * 2^-24 * S: the first-order worst-case bound of an fp32 sum of n terms in any
    order, (n - 1) * u * S, plus 2 u S.  Derived, not measured.  (The worst case's second-order
    term, about (n u)^2 S / 2, is not covered once n exceeds a few thousand; it needs every
    rounding error to point the same way, and real sums err by about sqrt(n) u S.)"""
    return (n + 1) * U32 * S


def assert_grad(got, ref, n, S, what=""):
    """got fp32 array against a (ref, n, S) triple: the bound per element, exact zeros where
    nothing was added.  Returns the largest error / bound ratio (0 when every n <= 1)."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), f"{what}: NaN in the gradient"
    empty = n == 0
    assert (got[empty] == 0).all(), f"{what}: a zero-contribution element is not exactly 0"
    err = np.abs(got.astype(np.float64) - ref)
    tol = grad_bound(n, S)
    bad = err > tol
    if bad.any():
        k = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: |got - ref| = {err[k]:.6g} > bound {tol[k]:.6g} at {k} "
                             f"(n = {n[k]}, S = {S[k]:.6g}); {int(bad.sum())} elements over")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, 0.0)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------ poisoned output buffers (GPU tests)
NAN_BITS = 0x7FC00000          # torch's / numpy's quiet NaN; as an int32 it is no valid index
GUARD = 64
LEAD = GUARD + 1               # 65 words = 16 * 16 + 4 bytes: the output starts 4 bytes past a 16-B boundary


def T(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Poisoned:
    """A caller-allocated output of `shape` (fp32, or int32 with dtype=torch.int32) inside a larger
    tensor whose every word holds the NaN bit pattern: the output starts one word past a 16-byte
    boundary, with LEAD words before it and GUARD words after it."""

    def __init__(self, dev, shape, dtype=None):
        import torch

        dtype = dtype or torch.float32
        self.shape, self.numel = tuple(shape), int(np.prod(shape, dtype=np.int64))
        self.buf = torch.full((LEAD + self.numel + GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.buf[LEAD:LEAD + self.numel].view(dtype).view(self.shape)
        assert self.out.data_ptr() % 16 == 4
        self.np_dtype = np.float32 if dtype == torch.float32 else np.int32

    def result(self, what):
        """Guards bitwise untouched, every element written (no NaN left) -> the output as numpy."""
        import torch

        torch.cuda.synchronize()
        bits = self.buf.cpu().numpy()
        assert (bits[:LEAD] == NAN_BITS).all(), f"{what}: wrote before the output"
        assert (bits[LEAD + self.numel:] == NAN_BITS).all(), f"{what}: wrote past the output"
        body = bits[LEAD:LEAD + self.numel]
        left = int((body == NAN_BITS).sum())
        assert left == 0, f"{what}: {left} of {self.numel} output elements not written"
        out = body.view(self.np_dtype).reshape(self.shape).copy()
        if self.np_dtype == np.float32:
            assert not np.isnan(out).any(), f"{what}: NaN in the output"
        return out
