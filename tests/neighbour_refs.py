"""Plain numpy restatements of the neighbour-distance helpers (a helper module of the tests, not a
conftest), the seeded clouds tests/golden/neighbours.npz was made from, and the derived bounds.

Pinned fp32 order (the bits of torch's CPU kernels; the fixture's matrices pin it):
  dot   = fma(q_z, p_z, fma(q_y, p_y, q_x * p_x))       the sequential fma chain over the channels
  |v|^2 = (v_x^2 + v_y^2) + v_z^2
  form A  d = ((-2 dot) + |q|^2) + |p|^2                 nearest_distances, self_*, square_distance
  form B  d = (|p|^2 + |q|^2) - 2 dot                    get_nearest_index
  self_diag: + 2 on the diagonal (an addition: the diagonal can still be a row's minimum)
Selection: ascending (distance, index); an exact tie goes to the lower index.
Root: sqrt((...(d_0 + d_1) + ... + d_{K-1}) / K), rank order, division and sqrt correctly rounded
(np.sqrt and numpy's fp32 division are).

Bounds (u = 2^-24; derived here, nothing is taken from the code under test)

  root_rtol(K) = (K + 3) u  -- |sqrt(mean_K) - the reference's| <= (K + 3) u * ref on rows whose K terms
  are all positive: two summation orders of K non-negative terms differ by at most 2 (K - 1) u of the sum
  ((K - 1) u each against the exact sum), each side's division adds u (2 u), so the radicands differ by
  at most 2 K u relative; the square root halves that (K u) and adds its own rounding (u) on our side and
  rounding plus torch's ulp (2 u) on the reference's: (K + 3) u.  For K = 1 the radicands are equal bits and
  the difference is torch's 1 ulp alone, which the same formula (4 u) covers.

  grad_ref(...)   -- per element, against the float64 gradient of the reference's expression with the fp32
  selection held fixed.  A pair (i, k) with target j = idx_ik contributes t = c * 2 (q_i - p_j) to
  grad_q[:, i] and -t to grad_p[:, j], c the gradient arriving on d_ik.
    * forward error in d.  The expanded form rounds |q|^2 and |p|^2 (3 u each of their value: three products,
      two additions), the dot (3 u of sum_c |q_c p_c|: one product, two fmas) and the two outer additions
      (u each of a partial sum that is at most A = |q|^2 + |p|^2 + 2 sum_c |q_c p_c|): |d^ - d| <= 5 u A; 6 u A
      is used.  E_d = 6 u A.
    * root: m = mean_k d_k.  |m^ - m| <= mean_k E_d,k + (K - 1) u mean_k |d_k| + u |m|, rho_m = that / m;
      val = sqrt(m^) has rho_v = rho_m / 2 + 2 u (its rounding, and torch's ulp for the reference), and
      c = (g / (2 val)) / K has rel_c = rho_v / (1 - rho_v) + 2 u (two divisions).  Rows with rho_m >= 1/2
      (m not resolved by fp32) get an infinite bound: nothing is claimed there.
      none: c = g exactly, rel_c = 0.
    * t = c * (2 (q - p)): one subtraction and one product, 2 u: |t^ - t| <= |t| (rel_c + 2 u).
    * the reference does not form q - p: its backward goes through the expanded form, 2 c q_c and 2 c p_c
      rounded separately (u each), and the |x|^2 paths and the matmul path are added (up to 2 more roundings
      on those magnitudes).  So that the bound is not tighter than the reference deserves, every pair also
      gets 3 u (|2 c q_c| + |2 c p_c|).
    * the sums.  grad_q adds K terms: (K - 1) u sum |t|.  grad_p adds the n_j terms that point at j:
      (n_j - 1) u of their magnitudes.  One cloud (`same`): target j's sum holds its n_j pair terms and its
      own row's sum, n_j more additions over all those magnitudes.
    * a margin of 2 u on the summed magnitudes, as viewops_refs.depth_grad has.
"""
import numpy as np

U32 = 2.0 ** -24
f32 = np.float32


def root_rtol(K):
    return (K + 3) * U32


# ------------------------------------------------------------------ pinned-order forward
def _fma32(a, b, c):
    """fp32 fma(a, b, c) exactly: the product is exact in float64; the sum is rounded to odd in float64
    (TwoSum gives the rounding error), which makes the second rounding to fp32 the correct one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64) if s.flags.c_contiguous else np.ascontiguousarray(s).view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(f32)


def sumsq(v):
    """(B,3,N) -> (B,N): (x^2 + y^2) + z^2 in fp32."""
    v = np.asarray(v, f32)
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def dot3(q, p):
    """q (B,3,S), p (B,3,N) -> (B,S,N): the sequential fma chain."""
    q, p = np.asarray(q, f32), np.asarray(p, f32)
    d = q[:, 0, :, None] * p[:, 0, None, :]
    d = _fma32(q[:, 1, :, None], p[:, 1, None, :], d)
    return _fma32(q[:, 2, :, None], p[:, 2, None, :], d)


def dist_matrix(q, p, form="A", self_diag=False):
    """The (B,S,N) fp32 matrix the helpers select from."""
    dot = dot3(q, p)
    qn, pn = sumsq(q)[:, :, None], sumsq(p)[:, None, :]
    if form == "A":
        d = (f32(-2.0) * dot + qn) + pn
    else:
        d = (pn + qn) - f32(2.0) * dot
    if self_diag:
        n = d.shape[1]
        assert d.shape[2] == n
        d = d.copy()
        d[:, np.arange(n), np.arange(n)] += f32(2.0)
    return d.astype(f32)


def select(d, k):
    """The k smallest of every row in ascending (distance, index) order -> (values (B,S,k), idx int32)."""
    order = np.argsort(d, axis=2, kind="stable")[:, :, :k]
    return np.take_along_axis(d, order, 2), order.astype(np.int32)


def root(vals):
    """(B,S,K) sorted distances -> (B,S) fp32: the rank-order sum, / K, sqrt."""
    vals = np.asarray(vals, f32)
    K = vals.shape[2]
    acc = vals[:, :, 0].copy()
    for k in range(1, K):
        acc = acc + vals[:, :, k]
    with np.errstate(invalid="ignore"):
        return np.sqrt(acc / f32(K))


def nn_dist(q, p, k, form="A", self_diag=False):
    return select(dist_matrix(q, p, form, self_diag), k)


# ------------------------------------------------------------------ gradients
def _gather(p, idx):
    """p (B,3,N), idx (B,S,K) -> (B,3,S,K)."""
    return np.stack([p[b][:, idx[b]] for b in range(p.shape[0])])


def grad_q_fp32(q, p, idx, g, val=None, self_diag=False):
    """grad_q in the documented fp32 order: c = g (none, g (B,S,K)) or (g / (2 val)) / K (root, g and val (B,S));
    t_k = c * (2 (q - p_j)), 0 for a diagonal pair; ((0 + t_0) + t_1) + ...  -> (B,3,S)."""
    q, p = np.asarray(q, f32), np.asarray(p, f32)
    B, _, S = q.shape
    K = idx.shape[2]
    with np.errstate(all="ignore"):
        if val is None:
            c = np.asarray(g, f32)
        else:
            c = ((np.asarray(g, f32) / (f32(2.0) * np.asarray(val, f32))) / f32(K))[:, :, None].repeat(K, 2)
        pj = _gather(p, idx)                                          # (B,3,S,K)
        t = c[:, None] * (f32(2.0) * (q[:, :, :, None] - pj))
        if self_diag:
            diag = idx == np.arange(S)[None, :, None]
            t = np.where(diag[:, None], f32(0), t)
        acc = np.zeros((B, 3, S), f32)
        for k in range(K):
            acc = acc + t[:, :, :, k]
    return acc


def grad_ref(q, p, idx, g, self_diag=False, rooted=False, same=False):
    """The float64 gradient of the reference's expression with the selection `idx` held fixed, and the bound of
    the module docstring.  g: (B,S,K) (none) or (B,S) (root).  Returns (gq, Eq, gp, Ep), each (B,3,*);
    same: (g_sum, E_sum, None, None) for the one cloud."""
    q32, p32 = np.asarray(q, f32), np.asarray(p, f32)
    q, p = q32.astype(np.float64), p32.astype(np.float64)
    B, _, S = q.shape
    N = p.shape[2]
    K = idx.shape[2]
    idx = np.asarray(idx).astype(np.int64)
    pj = _gather(p, idx)                                              # (B,3,S,K)
    diff = q[:, :, :, None] - pj
    diag = (idx == np.arange(S)[None, :, None]) if self_diag else np.zeros(idx.shape, bool)
    d = (diff ** 2).sum(1) + 2.0 * diag                               # (B,S,K), exact distances
    A = (q ** 2).sum(1)[:, :, None] + (pj ** 2).sum(1) + 2 * np.abs(q[:, :, :, None] * pj).sum(1)
    g = np.asarray(g, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        if rooted:
            m = d.mean(2)
            em = (6 * U32 * A).mean(2) + (K - 1) * U32 * np.abs(d).mean(2) + U32 * np.abs(m)
            rho_m = em / m
            rho_v = rho_m / 2 + 2 * U32
            rel_c = np.where((rho_m < 0.5) & (m > 0), rho_v / (1 - rho_v) + 2 * U32, np.inf)
            c = (g / (2 * np.sqrt(m)) / K)[:, :, None].repeat(K, 2)
            rel_c = rel_c[:, :, None].repeat(K, 2)
        else:
            c, rel_c = g, np.zeros(idx.shape)
        t = np.where(diag[:, None], 0.0, c[:, None] * 2 * diff)       # (B,3,S,K)
        at = np.abs(t)
        et = at * (rel_c[:, None] + 2 * U32) + 3 * U32 * np.abs(2 * c[:, None]) * (np.abs(q[:, :, :, None]) + np.abs(pj))
        et = np.where(diag[:, None], 0.0, et)
        et = np.where(np.isnan(et), np.inf, et)
    gq, aq = t.sum(3), at.sum(3)
    Eq = et.sum(3) + (K - 1 + 2) * U32 * aq
    gp = np.zeros((B, 3, N))
    ap = np.zeros((B, 3, N))
    ep = np.zeros((B, 3, N))
    n = np.zeros((B, N))
    live = ~diag
    for b in range(B):
        j = idx[b][live[b]]
        n[b] = np.bincount(j, minlength=N)
        for ch in range(3):
            gp[b, ch] = -np.bincount(j, weights=np.nan_to_num(t[b, ch][live[b]], nan=0.0, posinf=0.0, neginf=0.0),
                                     minlength=N)
            ap[b, ch] = np.bincount(j, weights=np.nan_to_num(at[b, ch][live[b]], nan=0.0, posinf=0.0, neginf=0.0),
                                    minlength=N)
            e = et[b, ch][live[b]]
            ep[b, ch] = np.bincount(j, weights=np.where(np.isfinite(e), e, 0.0), minlength=N)
            ep[b, ch][np.bincount(j, weights=~np.isfinite(e), minlength=N) > 0] = np.inf
    if not same:
        Ep = ep + (np.maximum(n - 1, 0)[:, None] + 2) * U32 * ap
        return gq, Eq, gp, Ep
    tot = aq + ap
    return gq + gp, Eq + ep + (n[:, None] + 2) * U32 * tot, None, None


def assert_in_bound(got, ref, E, what=""):
    """|got - ref| <= E per element; elements with an infinite bound are not compared.  Returns the largest
    error / bound ratio over the finite ones."""
    got = np.asarray(got).astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(E)
    assert fin.any(), f"{what}: no element has a finite bound"
    assert np.isfinite(got[fin]).all(), f"{what}: non-finite gradient where the bound is finite"
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    bad = fin & (err > E)
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err - np.where(fin, E, 0), -np.inf)), err.shape)
        raise AssertionError(f"{what}: |got - ref| = {err[k]:.6g} > bound {E[k]:.6g} at {k} (ref {ref[k]:.6g}); "
                             f"{int(bad.sum())} elements over")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(fin & (E > 0), err / E, 0.0)
    return float(r.max())


# ------------------------------------------------------------------ seeded clouds of the fixture
def cloud_unit(seed, B, N):
    """random in the unit cube, (B,3,N)."""
    return np.random.default_rng(seed).random((B, 3, N)).astype(f32)


def cloud_wide(seed, B, N):
    """spread over +-3: most points are farther than sqrt(2) from every other, so diagonals win."""
    return ((np.random.default_rng(seed).random((B, 3, N)) - 0.5) * 6.0).astype(f32)


def cloud_tiled(seed, B, n_unique, N):
    """PCN-style: n_unique points tiled up to N (duplicates: zero and slightly negative minima)."""
    rng = np.random.default_rng(seed)
    u = (rng.random((B, 3, n_unique)) - 0.5).astype(f32)
    idx = np.concatenate([np.arange(n_unique), rng.integers(0, n_unique, N - n_unique)])
    return np.ascontiguousarray(u[:, :, idx])


def fixture_clouds():
    """name -> array; the inputs the generator runs the reference on (regenerated by the tests, not stored)."""
    return {
        "x": cloud_unit(500, 2, 257),       # queries
        "y": cloud_unit(501, 2, 130),       # targets
        "s": cloud_unit(502, 2, 300),       # self cloud (unit cube)
        "w": cloud_wide(503, 1, 64),        # +-3: diagonals win
        "t": cloud_tiled(504, 2, 100, 257), # duplicates: pre-sqrt only
        "f": np.random.default_rng(505).standard_normal((2, 6, 40)).astype(f32),   # features for the gathers
    }


def min_gap_ulp(d, k):
    """Smallest gap, in ulp of the larger value, between consecutive entries among every row's first k + 1."""
    v = np.sort(d, axis=2)[:, :, :k + 1].astype(np.float64)
    gap = np.diff(v, axis=2)
    return float((gap / np.spacing(np.abs(v[:, :, 1:]).astype(f32)).astype(np.float64)).min())


# name -> (class, kwargs, weight seed (tests/golden/weights.fill_state), input seed, input shape)
MODULES = {
    "mlp": ("MLP", dict(in_channel=16, layer_dims=[32, 8], bn=True), 530, 520, (5, 16)),
    "res": ("MLP_Res", dict(in_dim=16, hidden_dim=24, out_dim=12), 531, 521, (2, 16, 33)),
    "pfe": ("PointNetFeatureExtractor", dict(in_channels=3, feat_size=32, layer_dims=[8, 16], global_feat=False),
            532, 522, (2, 33, 3)),
}


def module_kwargs(name):
    """A fresh copy: the reference's PointNetFeatureExtractor edits the list it is given."""
    return {k: (list(v) if isinstance(v, list) else v) for k, v in MODULES[name][1].items()}


def module_input(name):
    _, _, _, seed, shape = MODULES[name]
    return np.random.default_rng(seed).standard_normal(shape).astype(f32)
