"""Generate tests/golden/neighbours.npz from the REFERENCE's own neighbour helpers (run where the
reference is available; only the .npz is committed).  The seeded clouds (tests/neighbour_refs.py,
fixture_clouds) are stored with the results, so the tests do not depend on numpy's generator streams.

  in_<c>                          the input clouds x, y, s, w, t and the feature cloud f
  nd_xy, snd_<c>, sndk<k>_<c>     models/model_utils.py:288-321 nearest_distances(x, y), self_nearest_distances,
                                  self_nearest_distances_K on the clouds s (unit cube), w (+-3), t (tiled)
  g_*                             the reference's fp32 autograd gradients of sum(out) of those
  gni4_idx / gni4_dis / gni_row   :501-521 get_nearest_index(x, y, k=4) and the whole sorted row (k = v2):
                                  pins form B
  sqd_xy                          :258-279 square_distance of the same clouds: pins form A
  ixn, knn_s, ggf_s               :523-540 indexing_neighbor, :911-943 knn and get_graph_feature
  mlp_* / res_* / pfe_*           :45-60, 79-95, 631-805 with weights from tests/golden/weights.py

The generator asserts what the tests rely on: the restatements of neighbour_refs are bit-equal to the
reference's matrices, and wherever a test compares indices the first k + 1 distances of every row are at
least 8 ulp apart.

Usage:  python tests/golden/make_golden_neighbours.py
"""
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, _load, _stub_modules  # noqa: E402
from weights import fill_state  # noqa: E402
import neighbour_refs as NR  # noqa: E402


def _grad(fn, *clouds):
    ts = [torch.from_numpy(c).clone().requires_grad_(True) for c in clouds]
    fn(*ts).sum().backward()
    return [t.grad.numpy() for t in ts]


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    mu = _load(os.path.join(REF, "models/model_utils.py"), "ref_model_utils")
    c = NR.fixture_clouds()
    T = {k: torch.from_numpy(v) for k, v in c.items()}
    out = {f"in_{k}": v for k, v in c.items()}
    with torch.no_grad():
        out["nd_xy"] = mu.nearest_distances(T["x"], T["y"]).numpy()
        out["nd_tt"] = mu.nearest_distances(T["t"], T["t"]).numpy()
        for n in "swt":
            out[f"snd_{n}"] = mu.self_nearest_distances(T[n]).numpy()
        for n, k in (("s", 3), ("w", 3), ("w", 5), ("t", 3)):
            out[f"sndk{k}_{n}"] = mu.self_nearest_distances_K(T[n], k).numpy()
        i4, d4 = mu.get_nearest_index(T["x"], T["y"], k=4, return_dis=True)
        _, row = mu.get_nearest_index(T["x"], T["y"], k=c["y"].shape[2], return_dis=True)
        out["gni4_idx"], out["gni4_dis"], out["gni_row"] = i4.numpy().astype(np.int32), d4.numpy(), row.numpy()
        sqd = mu.square_distance(T["x"].transpose(1, 2).contiguous(), T["y"].transpose(1, 2).contiguous()).numpy()
        out["sqd_xy"] = sqd
        index = torch.from_numpy(np.random.default_rng(510).integers(0, 40, (2, 50, 4)))
        out["ixn_index"] = index.numpy().astype(np.int32)
        out["ixn"] = mu.indexing_neighbor(T["f"], index).numpy()
        out["knn_s"] = mu.knn(T["s"], 5).numpy().astype(np.int32)
        cpu = torch.device("cpu")
        with mock.patch.object(torch, "device", lambda *_: cpu):   # get_graph_feature hard-codes 'cuda'
            out["ggf_s"] = mu.get_graph_feature(T["s"], k=5).numpy()
        for name, (cls, kw, wseed, _, _) in NR.MODULES.items():
            m = fill_state(getattr(mu, cls)(**NR.module_kwargs(name)), wseed).eval()
            out[f"{name}_out"] = m(torch.from_numpy(NR.module_input(name))).numpy()
    out["g_nd_x"], out["g_nd_y"] = _grad(mu.nearest_distances, c["x"], c["y"])
    for n in "sw":
        (out[f"g_snd_{n}"],) = _grad(mu.self_nearest_distances, c[n])
    for n, k in (("s", 3), ("w", 3), ("w", 5)):
        (out[f"g_sndk{k}_{n}"],) = _grad(lambda t: mu.self_nearest_distances_K(t, k), c[n])

    # ---- what the tests rely on
    A = NR.dist_matrix(c["x"], c["y"], "A")
    Bm = NR.dist_matrix(c["x"], c["y"], "B")
    assert np.array_equal(A, sqd), "form A restatement != square_distance"
    assert np.array_equal(np.sort(Bm, axis=2), out["gni_row"]), "form B restatement != get_nearest_index row"
    v, i = NR.select(Bm, 4)
    assert np.array_equal(v, out["gni4_dis"]) and np.array_equal(i, out["gni4_idx"])
    gaps = {"B(x,y) k4": NR.min_gap_ulp(Bm, 4), "A(x,y) k1": NR.min_gap_ulp(A, 1)}
    for n, k in (("s", 3), ("w", 5)):
        gaps[f"A({n}) diag k{k}"] = NR.min_gap_ulp(NR.dist_matrix(c[n], c[n], "A", True), k)
    sT = T["s"]
    inner = -2 * torch.matmul(sT.transpose(2, 1), sT)
    xx = torch.sum(sT ** 2, dim=1, keepdim=True)
    gaps["knn(s) k5"] = NR.min_gap_ulp((-(-xx - inner - xx.transpose(2, 1))).numpy(), 5)
    for what, gap in gaps.items():
        assert gap >= 8, (what, gap)
    print({k: round(v, 1) for k, v in gaps.items()})
    # the NaN mask of the tiled cloud is min < 0 of the restatement
    At = NR.dist_matrix(c["t"], c["t"], "A")
    assert np.array_equal(np.isnan(out["nd_tt"][:, :, 0]), At.min(2) < 0)
    print("negative minima on the tiled cloud:", int((At.min(2) < 0).sum()), "of", At.shape[0] * At.shape[1])
    assert all(np.isfinite(out[k]).all() for k in out if k.startswith("g_")), "non-finite reference gradient"

    path = os.path.join(HERE, "neighbours.npz")
    np.savez_compressed(path, **out)
    print("neighbours.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
