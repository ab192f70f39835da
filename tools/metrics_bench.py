"""completion_metrics (one Chamfer search + pcops_completion_metrics) against the sequence it replaces,
calc_cd(calc_f1=True) + calc_dcd, and the evaluation protocols built on it.

  python tools/metrics_bench.py                    HIP events around 100 warm calls of each, per shape
  python tools/metrics_bench.py --count fused      1 warm + 10 calls of one variant at B = 1, 8192^2 and
  python tools/metrics_bench.py --count torch      nothing else: run under `rocprofv3 --kernel-trace --stats`,
                                                   launches per call = kernel dispatches / 11
  python tools/metrics_bench.py --evaluate         wall time of evaluate_55 (PointSea, 16 synthetic shapes,
                                                   median): the B = 1 per-view loop of core/test_55.py,
                                                   batched eager, batched graph=True
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import metrics as M  # noqa: E402

SHAPES = [(1, 8192, 8192), (8, 8192, 8192), (1, 16384, 16384)]


def clouds(B, n, m, dev, seed=0):
    rng = np.random.default_rng(seed)
    gt = (rng.random((B, n, 3)) - 0.5).astype(np.float32)
    x = (gt[:, rng.integers(0, n, m)] + 0.004 * rng.standard_normal((B, m, 3))).astype(np.float32)
    return torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)


def fused(x, gt):
    return M.completion_metrics(x, gt)


def parent(x, gt):
    cd_p, cd_t, f1 = M.calc_cd(x, gt, calc_f1=True)
    return cd_p, cd_t, f1, M.calc_dcd(x, gt)[0]


def events_ms(fn, x, gt, calls=100):
    for _ in range(10):
        fn(x, gt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn(x, gt)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def timings(dev):
    rows = []
    with torch.no_grad():
        for B, n, m in SHAPES:
            x, gt = clouds(B, n, m, dev)
            # three rounds, alternating, the median of each
            f, p = zip(*[(events_ms(fused, x, gt), events_ms(parent, x, gt)) for _ in range(3)])
            rows.append({"B": B, "n_gt": n, "n_out": m, "fused_ms": round(sorted(f)[1], 4),
                         "calc_cd_plus_calc_dcd_ms": round(sorted(p)[1], 4),
                         "speedup": round(sorted(p)[1] / sorted(f)[1], 2)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def count(which, dev):
    x, gt = clouds(1, 8192, 8192, dev)
    with torch.no_grad():
        for _ in range(11):
            (fused if which == "fused" else parent)(x, gt)
    torch.cuda.synchronize()


def evaluate(dev):
    from svdformer_pointsea_amd import evaluate as E
    from svdformer_pointsea_amd.data import seprate_point_cloud
    from svdformer_pointsea_amd.model_utils import fps_subsample
    from svdformer_pointsea_amd.pointsea import Config55, Model
    from svdformer_pointsea_amd.render import PCViews_Real

    torch.manual_seed(0)
    model = Model(Config55).to(dev).eval()
    render = PCViews_Real(TRANS=-Config55.NETWORK.view_distance)
    rng = np.random.default_rng(1)
    gts = torch.from_numpy((rng.random((16, 8192, 3)) - 0.5).astype(np.float32))
    tax = ["%08d" % (k % 4) for k in range(16)]

    def batches(bs):
        for k in range(0, 16, bs):
            yield tax[k:k + bs], [str(i) for i in range(k, k + bs)], {"gtcloud": gts[k:k + bs]}

    def loop_b1():
        """core/test_55.py:59-82 as written there."""
        meter = E.AverageMeter(["CD", "DCD", "F1"])
        with torch.no_grad():
            for _, _, data in batches(1):
                gt = data["gtcloud"].to(dev)
                npoints = gt.shape[1]
                for item in E.VIEWPOINTS_55:
                    partial, _ = seprate_point_cloud(gt, npoints, int(npoints * 0.5), fixed_points=torch.Tensor(item))
                    partial = fps_subsample(partial, 2048)
                    pred = model(partial.contiguous(), render.get_img(partial))
                    cdl1, cdl2, f1 = M.calc_cd(pred[-1], gt, calc_f1=True)
                    dcd, _, _ = M.calc_dcd(pred[-1], gt)
                    meter.update([cdl2.mean().item() * 1e3, dcd.mean().item(), f1.mean().item()])
        return meter.avg()

    def timed(fn):
        fn()   # warm: kernel caches, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    res = {}
    res["loop_b1_s"], ref = timed(loop_b1)
    print(json.dumps({"loop_b1_s": round(res["loop_b1_s"], 3), "overall": ref}), flush=True)
    for name, kw in (("batched_eager_s", {}), ("batched_graph_s", {"graph": True})):
        res[name], out = timed(lambda: E.evaluate_55(model, batches(2), render.get_img, "median", **kw))
        print(json.dumps({name: round(res[name], 3), "overall": out["overall"]}), flush=True)
    return {k: round(v, 3) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", choices=["fused", "torch"])
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.count:
        return count(a.count, dev)
    if a.evaluate:
        res = {"evaluate_55_16_shapes_median_pointsea": evaluate(dev)}
    else:
        res = {"completion_metrics": timings(dev)}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
