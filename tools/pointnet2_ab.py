"""A/B of the PointNet++ grouping and feature-propagation stages with the fused launches
(csrc/pointnet2.hip) against the unfused chain of the existing ops, each from the sampled centres
to the token-major / channels_last tensor the first GEMM reads:

  SA   fused: ONE pcops_ball_group (model_utils.ball_group_rows)
       chain: QueryAndGroup (ball_query, group_points x 2, subtract, cat) + the channels_last copy
       at (B 32, N 2048, S 512, K 32, C 64) and (B 32, N 16384, S 2048, K 32, C 3)
  FP   fused: ONE pcops_fp_interp_forward (model_utils.fp_interp_cl)
       chain: three_nn, sqrt, the weight arithmetic, three_interpolate, cat, the token-major copy
       at (B 32, N 2048, M 512, C2 256, C1 128)

forward only, and forward + backward for the feature inputs.  Both variants run in ONE process in
interleaved rounds on the same data; the report gives the per-round median, minimum and maximum of
each and the GPU kernel launches of one pass of each (torch.profiler).  Usage:

    python tools/pointnet2_ab.py [--rounds 10] [--iters 10] [--out profiles/pointnet2_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import model_utils as MU  # noqa: E402
from svdformer_pointsea_amd import pointnet2_utils as PU  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # the profiler is an optional extra of this report
        return f"n/a ({type(exc).__name__})"


def sa_legs(B, N, S, K, C, radius, dev):
    g = torch.Generator().manual_seed(N + C)
    xyz = torch.rand(B, N, 3, generator=g).to(dev)
    new_xyz = xyz[:, torch.randperm(N, generator=g)[:S]].contiguous()
    feat = torch.randn(B, C, N, generator=g).to(dev).requires_grad_(True)        # channel-major: the chain's operand
    feat_t = feat.detach().transpose(1, 2).contiguous().requires_grad_(True)     # token-major: the fused operand
    grouper = PU.QueryAndGroup(radius, K)
    go = torch.randn(B, S, K, 3 + C, generator=g).to(dev)

    def fused():
        return MU.ball_group_rows(xyz, new_xyz, feat_t, radius, K)[0]

    def chain():
        return grouper(xyz, new_xyz, feat).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)

    idx = PU.ball_query(radius, K, xyz, new_xyz)
    full = float((idx[..., -1] != idx[..., 0]).float().mean())
    same = torch.equal(fused(), chain())
    return fused, chain, (feat_t, feat), go, f"rows bit-equal: {same}; centres with a last slot that is a new hit: {full:.2f}"


def fp_legs(B, N, M, C2, C1, dev):
    g = torch.Generator().manual_seed(N + M)
    unknown = torch.rand(B, N, 3, generator=g).to(dev)
    known = unknown[:, torch.randperm(N, generator=g)[:M]].contiguous()
    p2 = torch.randn(B, C2, M, generator=g).to(dev).requires_grad_(True)
    p1 = torch.randn(B, C1, N, generator=g).to(dev).requires_grad_(True)
    p2_t = p2.detach().transpose(1, 2).contiguous().requires_grad_(True)
    p1_t = p1.detach().transpose(1, 2).contiguous().requires_grad_(True)
    go = torch.randn(B, N, C2 + C1, generator=g).to(dev)

    def fused():
        return MU.fp_interp_cl(unknown, known, p1_t, p2_t, 0)

    def chain():
        return MU.fp_interp_chain(unknown, known, p1, p2, 0)

    err = float((fused() - chain()).abs().max())
    return fused, chain, (p2_t, p1_t, p2, p1), go, f"max |fused - chain| {err:.3g}"


def report(title, legs, args, lines):
    fused, chain, leaves, go, note = legs
    lines.append(f"{title}  [{note}]")

    def fwd(fn):
        with torch.no_grad():
            fn()

    def fwd_bwd(fn):
        for t in leaves:
            t.grad = None
        fn().backward(go)

    for name, run in (("forward", fwd), ("forward + backward", fwd_bwd)):
        variants = (("fused", lambda: run(fused)), ("chain", lambda: run(chain)))
        ms = {k: [] for k, _ in variants}
        for k, fn in variants:      # warm up both
            timed(fn, 3)
        for _ in range(args.rounds):
            for k, fn in variants:
                ms[k].append(timed(fn, args.iters))
        lines.append(f"  {name}")
        for k, fn in variants:
            lines.append(f"    {k:6s} median {statistics.median(ms[k]):.4f}  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}"
                         f"  GPU launches per pass: {launches(fn)}")
        lines.append(f"    median ratio chain / fused: {statistics.median(ms['chain']) / statistics.median(ms['fused']):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["PointNet++ grouping / feature propagation, fused launch against the unfused chain of existing ops, fp32, MI355X",
             f"{args.rounds} interleaved rounds of {args.iters} iterations in one process, ms per iteration"]
    report("SA  B 32, N 2048, S 512, K 32, C 64, radius 0.2", sa_legs(32, 2048, 512, 32, 64, 0.2, dev), args, lines)
    report("SA  B 32, N 16384, S 2048, K 32, C 3, radius 0.1", sa_legs(32, 16384, 2048, 32, 3, 0.1, dev), args, lines)
    report("FP  B 32, N 2048, M 512, C2 256, C1 128, mode 0", fp_legs(32, 2048, 512, 256, 128, dev), args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
