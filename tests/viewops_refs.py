"""Plain numpy references of the view-space ops (a helper module of the tests, not a conftest),
and the seeded inputs the goldens in tests/golden/viewops.npz were made from.

Index rule (include/pcops.h, the one of pointops_refs): a coordinate c takes part iff
0 <= c <= P - 1, tested on the stored value before any conversion, and its pixel is trunc(c);
anything else contributes nothing, reads as 0 and is never used as an address.

  pixel_of(coord, P)          -> (ok mask, int64 pixel with the rejected ones at 0)
  splat(fea, coord, P)        -> (B,P,C) fp32: every element the fp32 sum of its terms added one
                                 by one in ascending point index, starting from +0 (the bits of a
                                 sequential scatter_add onto zeros)
  gather(rows, coord)         -> (B,N,C) fp32: rows[b, pix] or 0
  depth_grad(...)             -> (ref, n, E): the gradient of PCViews.get_img in float64, see there
"""
import numpy as np

U32 = 2.0 ** -24  # fp32 unit roundoff
EPS = 1e-12       # the reference's epsilon (models/model_utils.py:1021, :1091)


def pixel_of(coord, P):
    c = np.asarray(coord)
    with np.errstate(invalid="ignore"):
        if c.dtype.kind == "f":
            ok = (c >= 0) & (c <= c.dtype.type(P - 1))
        else:
            ok = (c >= 0) & (c <= P - 1)
        pix = np.where(ok, c, 0).astype(np.int64)  # truncation toward zero; rejected values never converted
    return ok, pix


def splat(fea, coord, P):
    fea = np.asarray(fea, np.float32)
    B, N, C = fea.shape
    ok, pix = pixel_of(coord, P)
    out = np.zeros((B, P, C), np.float32)
    for b in range(B):
        o = out[b]
        for i in np.nonzero(ok[b])[0]:
            o[pix[b, i]] += fea[b, i]  # fp32 add, in ascending i
    return out


def gather(rows, coord):
    rows = np.asarray(rows, np.float32)
    B, P, C = rows.shape
    ok, pix = pixel_of(coord, P)
    N = pix.shape[1]
    if P == 0:
        return np.zeros((B, N, C), np.float32)
    out = np.take_along_axis(rows, np.broadcast_to(pix[:, :, None], (B, N, C)), axis=1)
    return np.where(ok[:, :, None], out, np.float32(0))


def nchw_rows(img):
    """(B,C,H,W) -> (B, H*W, C), the image side both exchange ops address."""
    B, C, H, W = img.shape
    return np.ascontiguousarray(np.transpose(img, (0, 2, 3, 1)).reshape(B, H * W, C))


def depth_grad(points, rot, trans, pix, g):
    """Gradient of PCViews.get_img with respect to the points, in float64, over the pixels of the fp32
    projection: points (B,N,3), rot (V,3,3) as stored (transposed), trans (V,3), pix (B*V, N) int64 (the
    pixel of each pair, -1 where the splat rejects it), g (B*V, R, R) the upstream gradient.
    Returns (ref, n, E) of shapes (B,N,3), (B,N), (B,N,3):
      ref  the float64 gradient,
      n    in how many views the point is kept (n == 0: the row must be exactly 0),
      E    a derived bound on |fp32 result - ref| per element.

    With z = p . rot[:, 2] - t_z, w = 1/(z + eps), per pixel Sw = sum w (or 1 where empty),
    Vs = sum z w, img = Vs / Sw:   dz = g[pix] w^2 (eps + img[pix]) / Sw[pix],
    grad[b,i,:] = sum_v dz_v rot_v[:, 2]   (only the depth carries a gradient: the pixel passes through ceil).

    Derivation of E (first order in u = 2^-24; nothing here is measured):
      * z in fp32 is an fma chain of three products and a subtraction: |z^ - z| <= 4 u A with
        A = sum_k |p_k rot[k,2]| + |t_z|, so z + eps has relative error kappa = 4 u A / (z + eps) (+ u for the
        add), and w = 1/(z + eps) has kappa + 2u.
      * Sw is the fp32 sum, in any order (float atomics), of the c weights of its pixel, all positive:
        relative error E_S = sum_j w_j (kappa_j + 2u) / Sw + (c - 1) u.
      * a term z w = z/(z + eps) is computed from the same z^: its relative error is kappa eps w + 3u
        (the sensitivity of z w to z is eps w^2); Vs sums c of them: E_V = sum_j t_j (...) / Vs + (c - 1) u.
      * img = Vs / Sw: E_V + E_S + u; eps + img: one more u.
      * dz = (((g w) w)(eps + img)) / Sw: 2 (kappa_i + 2u) for w^2, E_V + E_S + 2u for eps + img, E_S for
        Sw, 4u for the four operations: rel = 2 kappa_i + E_V + 2 E_S + 10 u.
      * the product with rot[k,2] and the at most V - 1 additions: 1 u + (V - 1) u on the sum of magnitudes.
      E = sum_v |dz_v rot_v[k,2]| (rel_v + V u) plus a margin of 2 u on the same sum, as grad_bound has.
    c enters through the (c - 1) u terms of E_S and E_V.
    The tests hold the torch chain's fp32 autograd result (the reference's own in the goldens, and the
    PCOPS_VIEWOPS_FUSED=0 path) to this same E; that is the bar they set, not a consequence of the derivation."""
    points = np.asarray(points, np.float32)
    B, N, _ = points.shape
    V = rot.shape[0]
    Pn = int(np.prod(g.shape[1:]))
    p = points.astype(np.float64)
    r2 = np.asarray(rot)[:, :, 2].astype(np.float64)
    tz = np.asarray(trans)[:, 2].astype(np.float64)
    z = np.einsum("bnk,vk->bvn", p, r2) - tz[None, :, None]
    A = np.einsum("bnk,vk->bvn", np.abs(p), np.abs(r2)) + np.abs(tz)[None, :, None]
    pix = np.asarray(pix).reshape(B, V, N)
    ok = pix >= 0
    z = np.where(ok, np.maximum(z, 0.0), 1.0)   # a kept pair has z^ >= 0; z itself is within 4 u A of it
    d = z + EPS
    w = ok / d
    kap = 4 * U32 * A / d
    idx = np.arange(B * V, dtype=np.int64).reshape(B, V, 1) * Pn + np.where(ok, pix, 0)
    flat, size = idx[ok], B * V * Pn
    cnt = np.bincount(flat, minlength=size)
    Sw = np.bincount(flat, weights=w[ok], minlength=size)
    Sw_err = np.bincount(flat, weights=(w * (kap + 2 * U32))[ok], minlength=size)
    t = z * w
    Vs = np.bincount(flat, weights=t[ok], minlength=size)
    Vs_err = np.bincount(flat, weights=(t * (kap * EPS * w + 3 * U32))[ok], minlength=size)
    Sw1 = np.where(Sw == 0, 1.0, Sw)
    img = Vs / Sw1
    more = np.maximum(cnt - 1, 0) * U32
    E_S = Sw_err / Sw1 + more
    with np.errstate(divide="ignore", invalid="ignore"):
        E_V = np.where(Vs > 0, Vs_err / Vs, 0.0) + more
    gp = np.asarray(g, np.float32).astype(np.float64).reshape(-1)[idx]
    dz = np.where(ok, gp * w * w * (EPS + img[idx]) / Sw1[idx], 0.0)
    rel = 2 * kap + E_V[idx] + 2 * E_S[idx] + 10 * U32 + V * U32 + 2 * U32
    ref = np.einsum("bvn,vk->bnk", dz, r2)
    E = np.einsum("bvn,vk->bnk", np.abs(dz) * rel, np.abs(r2))
    return ref, ok.sum(axis=1), E


def assert_depth_grad(got, ref, n, E, what=""):
    """got fp32 (B,N,3) against a depth_grad triple: the derived bound per element, exact zeros where the
    point is kept in no view.  Returns the largest error / bound ratio."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite gradient"
    assert (got[n == 0] == 0).all(), f"{what}: a row masked in every view is not exactly 0"
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > E
    if bad.any():
        k = np.unravel_index(np.argmax(err - E), err.shape)
        raise AssertionError(f"{what}: |got - ref| = {err[k]:.6g} > bound {E[k]:.6g} at {k} (ref {ref[k]:.6g}); "
                             f"{int(bad.sum())} elements over")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E > 0, err / E, 0.0)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------ seeded inputs of the goldens
# name -> (seed, B, N, C, h, w): the exchange cases tests/golden/make_golden_viewops.py runs through the
# reference's point_fea_img_fea / distribute_img_fea_points (float coordinates; the reference cannot take
# integer ones, nor NaN / inf, which it would turn into an index)
EXCHANGE_GOLDEN = {
    "small": (300, 2, 300, 5, 3, 4),
    "odd": (301, 2, 1000, 7, 7, 7),
    "deep": (302, 1, 10000, 2, 1, 2),
    "sparse": (303, 3, 200, 1, 14, 14),
}
SPECIAL = [0.0, -0.0, 3.7, -0.5, -1.0, 0.99, 1e20, -1e20]   # finite specials; P-1, P are added per case


def exchange_inputs(seed, B, N, C, h, w):
    """fea (B,N,C), coord (B,N) float32 with about 35 % outside [0, P-1] and the special values in front,
    img (B,C,h,w)."""
    P = h * w
    rng = np.random.default_rng(seed)
    fea = rng.standard_normal((B, N, C)).astype(np.float32)
    coord = rng.uniform(-0.2 * P, 1.35 * P, (B, N)).astype(np.float32)
    sp = np.asarray(SPECIAL + [P - 1, P, P - 0.5, P - 1.5], np.float32)
    k = min(len(sp), N)
    coord[:, :k] = sp[:k]
    img = rng.standard_normal((B, C, h, w)).astype(np.float32)
    return fea, coord, img


# name -> (seed, B, N, R): depth-gradient cases; "golden" takes the cloud of depth.npz
DEPTH_GOLDEN = {"r224": (310, 2, 2048, 224), "r8": (311, 2, 64, 8), "r16": (312, 2, 300, 16)}


def depth_inputs(name, depth_npz=None):
    """points (B,N,3) and the upstream gradient g (B*3, R, R) of a DEPTH_GOLDEN case."""
    seed, B, N, R = DEPTH_GOLDEN[name]
    rng = np.random.default_rng(seed)
    if name == "r224":
        pts = np.asarray(depth_npz["points"], np.float32)
    else:
        pts = (rng.random((B, N, 3)) - 0.5).astype(np.float32)
    g = rng.standard_normal((B * 3, R, R)).astype(np.float32)
    return pts, g
