"""A/B of the ShapeNet-55 discriminator's point MLP + max with the fused pass (csrc/pointmlp.hip) on
and off (PCOPS_POINT_MLP_FUSED), at the trainer's shapes (B, 8192, 128), B = 16 and 32: forward only,
and forward + backward for x and the six parameters.  The off leg is the reference's own op sequence
in torch on the same card.  Both variants run in ONE process in interleaved rounds on the same random
data; the report gives the per-round median and the minimum of each, the GPU kernel launches of one
pass of each (torch.profiler), the worst deviation of both from a float64 evaluation at the timed
shape, and the kernel's resource figures as given on the command line (they come from the build:
hipcc -Rpass-analysis=kernel-resource-usage).  Usage:

    python tools/point_mlp_ab.py [--rounds 15] [--iters 20] [--resources "..."] [--out profiles/adv55_point_mlp_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import adversarial as ADV  # noqa: E402

ENV = "PCOPS_POINT_MLP_FUSED"


def fwd(leaves):
    with torch.no_grad():
        return ADV.point_mlp_max(*leaves)


def fwd_bwd(leaves, go):
    for t in leaves:
        t.grad = None
    ADV.point_mlp_max(*leaves).backward(go)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H = 8192, 128
    lines = [f"point MLP 3 -> {H} -> {H} -> {H} + max over N = {N} points, fp32, MI355X",
             f"{args.rounds} interleaved rounds of {args.iters} iterations in one process, ms per iteration"]
    for B in (16, 32):
        torch.manual_seed(B)
        dis = ADV.SimplePointDiscriminator(hidden=H).to(dev)
        m = dis.mlp
        leaves = [(0.5 * torch.randn(B, N, 3, device=dev)).requires_grad_(True)]
        leaves += [t.detach().clone().requires_grad_(True) for t in (
            m[0].weight.squeeze(-1), m[0].bias, m[2].weight.squeeze(-1), m[2].bias, m[4].weight.squeeze(-1), m[4].bias)]
        go = torch.randn(B, H, device=dev)
        legs = (("forward", lambda: fwd(leaves)), ("forward + backward", lambda: fwd_bwd(leaves, go)))
        # both against float64 at the timed shape
        with torch.no_grad():
            d = [t.double() for t in leaves]
            h = torch.nn.functional.leaky_relu(torch.nn.functional.linear(d[0], d[1], d[2]), 0.2)
            h = torch.nn.functional.leaky_relu(torch.nn.functional.linear(h, d[3], d[4]), 0.2)
            top = torch.nn.functional.linear(h, d[5], d[6]).max(1)[0]
            del h
        err = {}
        for on in ("1", "0"):
            os.environ[ENV] = on
            err[on] = float((fwd(leaves).double() - top).abs().max())
        lines.append(f"B = {B}: max |out - float64|  fused {err['1']:.3g}  op chain {err['0']:.3g}")
        for name, fn in legs:
            ms = {"1": [], "0": []}
            for on in ("1", "0"):      # warm up both
                os.environ[ENV] = on
                timed(fn, 5)
            for _ in range(args.rounds):
                for on in ("1", "0"):
                    os.environ[ENV] = on
                    ms[on].append(timed(fn, args.iters))
            n = {}
            for on in ("1", "0"):
                os.environ[ENV] = on
                n[on] = launches(fn)
            lines.append(f"B = {B}, {name}")
            for on, tag in (("1", f"fused ({ENV}=1)"), ("0", f"op chain ({ENV}=0)")):
                lines.append(f"  {tag:36s} median {statistics.median(ms[on]):.4f}  min {min(ms[on]):.4f}  "
                             f"max {max(ms[on]):.4f}  GPU launches per pass: {n[on]}")
            lines.append(f"  median ratio chain / fused: {statistics.median(ms['0']) / statistics.median(ms['1']):.3f}")
        os.environ[ENV] = "1"
    flops = 2.0 * N * (3 * H + 2 * H * H)
    lines.append(f"forward work: {flops * 16 / 1e9:.2f} GFLOP at B = 16, {flops * 32 / 1e9:.2f} GFLOP at B = 32 "
                 "(fp32 FMA counted as 2)")
    if args.resources:
        lines.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): " + args.resources)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
