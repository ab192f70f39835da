"""float64 numpy restatements of the counted Chamfer ops (clouds of unequal size in one padded batch),
each as a loop over cloud pairs cut to their counts:

  forward_counts / backward_counts   oracle.chamfer_forward / oracle.chamfer_backward per slice, absent
                                     rows (0, 0) / zero gradient rows
  metrics_counts                     the formulas of tests/test_gpu_completion_metrics.py::_np_raw
                                     (loss_utils.py:98-155, fscore.py:3-16) per slice; NaN row for a
                                     pair with an empty side
  loss_counts                        the four Chamfer losses (loss_utils.py:10-31) per slice -> (B,);
                                     the counted loss is their mean, 0 for a pair with an empty side

and the shared golden case (tests/golden/make_golden_chamfer_counts.py).  Not a test module.
"""
import numpy as np

from oracle import oracle as O

FIELDS = ("l1a", "l1b", "l2a", "l2b", "cd_p", "cd_t", "p1", "p2", "f1", "t1", "t2", "dcd")

# the golden case: cloud 1 is the gt / partial side (N rows), cloud 2 the output side (M rows)
GOLDEN_SEED, GOLDEN_B, GOLDEN_N, GOLDEN_M = 41, 4, 600, 520
GOLDEN_COUNTS1 = (600, 257, 33, 1)
GOLDEN_COUNTS2 = (1, 520, 512, 100)


def golden_case():
    """(xyz1 (4, 600, 3), xyz2 (4, 520, 3)) fp32: cloud 2 lies near cloud 1's leading points (noise
    0.004, a fifth of the points off the surface), so the F-score at the 1e-4 threshold is non-trivial
    for every truncation."""
    rng = np.random.default_rng(GOLDEN_SEED)
    a = rng.uniform(-0.5, 0.5, (GOLDEN_B, GOLDEN_N, 3)).astype(np.float32)
    base = a[:, rng.integers(0, 33, GOLDEN_M)]
    far = rng.random((GOLDEN_B, GOLDEN_M, 1)) < 0.2
    b = (base + rng.normal(0.0, 0.004, base.shape) + far * rng.uniform(-0.2, 0.2, base.shape)).astype(np.float32)
    return a, b


def clamp_counts(counts, B, n):
    return [n] * B if counts is None else [int(min(max(int(c), 0), n)) for c in counts]


def forward_counts(a, b, counts1=None, counts2=None):
    """(dist1, dist2, idx1, idx2), padded: oracle.chamfer_forward on every pair cut to its counts."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    c1, c2 = clamp_counts(counts1, B, N), clamp_counts(counts2, B, M)
    d1, d2 = np.zeros((B, N), np.float32), np.zeros((B, M), np.float32)
    i1, i2 = np.zeros((B, N), np.int32), np.zeros((B, M), np.int32)
    for k in range(B):
        if c1[k] == 0 or c2[k] == 0:
            continue
        r = O.chamfer_forward(a[k:k + 1, :c1[k]], b[k:k + 1, :c2[k]])
        d1[k, :c1[k]], d2[k, :c2[k]], i1[k, :c1[k]], i2[k, :c2[k]] = r[0][0], r[1][0], r[2][0], r[3][0]
    return d1, d2, i1, i2


def backward_counts(a, b, counts1, counts2, gd1, gd2, i1, i2):
    """(gradxyz1, gradxyz2), padded: oracle.chamfer_backward per slice; absent rows zero, and the
    incoming gradient of an absent row never read."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    c1, c2 = clamp_counts(counts1, B, N), clamp_counts(counts2, B, M)
    g1, g2 = np.zeros((B, N, 3), np.float32), np.zeros((B, M, 3), np.float32)
    for k in range(B):
        if c1[k] == 0 or c2[k] == 0:
            continue
        r = O.chamfer_backward(a[k:k + 1, :c1[k]], b[k:k + 1, :c2[k]], gd1[k:k + 1, :c1[k]], gd2[k:k + 1, :c2[k]],
                               i1[k:k + 1, :c1[k]], i2[k:k + 1, :c2[k]])
        g1[k, :c1[k]], g2[k, :c2[k]] = r[0][0], r[1][0]
    return g1, g2


def _np_row(d1, d2, i1, i2, alpha, th, non_reg):
    """One pair: d1 / i1 (n_gt,), d2 / i2 (n_x,) -- _np_raw's expressions."""
    d1, d2 = d1.astype(np.float64), d2.astype(np.float64)
    n_gt, n_x = d1.shape[0], d2.shape[0]
    f12, f21 = n_x / n_gt, n_gt / n_x
    if non_reg:
        f12, f21 = max(1, f12), max(1, f21)

    def term(d, idx, n_t, frac):
        cnt = np.bincount(idx, minlength=n_t)[idx].astype(np.float64)
        return (1 - np.exp(-d * alpha) / (cnt + 1e-6) * frac).mean()

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = dict(l1a=np.sqrt(d1).mean(), l1b=np.sqrt(d2).mean(), l2a=d1.mean(), l2b=d2.mean(),
                 p1=(d1 < np.float32(th)).mean(), p2=(d2 < np.float32(th)).mean(),
                 t1=term(d1, i1, n_x, f21), t2=term(d2, i2, n_gt, f12))
        r["cd_p"] = (r["l1a"] + r["l1b"]) / 2
        r["cd_t"] = r["l2a"] + r["l2b"]
        r["f1"] = float(np.nan_to_num(2 * r["p1"] * r["p2"] / (r["p1"] + r["p2"])))
        r["dcd"] = (r["t1"] + r["t2"]) / 2
    return r


def metrics_counts(d1, d2, i1, i2, counts1=None, counts2=None, alpha=1000.0, th=1e-4, non_reg=False):
    """{field: (B,) float64} of a padded Chamfer result chamfer(gt, output) with gt counts1, output counts2."""
    B, N, M = d1.shape[0], d1.shape[1], d2.shape[1]
    c1, c2 = clamp_counts(counts1, B, N), clamp_counts(counts2, B, M)
    out = {k: np.full(B, np.nan) for k in FIELDS}
    for k in range(B):
        if c1[k] == 0 or c2[k] == 0:
            continue
        r = _np_row(d1[k, :c1[k]], d2[k, :c2[k]], i1[k, :c1[k]], i2[k, :c2[k]], alpha, th, non_reg)
        for f in FIELDS:
            out[f][k] = r[f]
    return out


def loss_counts(d1, d2, counts1=None, counts2=None, root=True, both=True):
    """(B,) float64: the reference's loss of every pair on its valid distances -- chamfer_sqrt (root, both),
    chamfer (both), chamfer_single_side_sqrt (root), chamfer_single_side; 0 for a pair with an empty side."""
    B, N, M = d1.shape[0], d1.shape[1], d2.shape[1]
    c1, c2 = clamp_counts(counts1, B, N), clamp_counts(counts2, B, M)
    out = np.zeros(B)
    for k in range(B):
        if c1[k] == 0 or c2[k] == 0:
            continue
        x, y = d1[k, :c1[k]].astype(np.float64), d2[k, :c2[k]].astype(np.float64)
        if root:
            x, y = np.sqrt(x), np.sqrt(y)
        out[k] = x.mean() if not both else ((x.mean() + y.mean()) / 2 if root else x.mean() + y.mean())
    return out
