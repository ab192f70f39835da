"""A/B of GeoSpecNet's MSGSpecConv forward + backward with the fused spectral pooling pass
(csrc/spectral.hip) on and off (PCOPS_SPECTRAL_FUSED), at the reference's shape B = 12, N = 128,
C = 256, k_list = [16, 32].  The off leg is the reference's own op sequence in torch on the same
card.  Both variants run in ONE process in interleaved rounds on the same random data; the report
gives the per-round median and the minimum of each, and the GPU kernel launches of one forward +
backward of each (torch.profiler).  Usage:

    python tools/spectral_ab.py [--rounds 15] [--iters 20] [--out profiles/geospec_adapter_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import geospecnet as GS  # noqa: E402


def step(m, xyz, feats, gout):
    m.zero_grad(set_to_none=True)
    feats.grad = None
    m(xyz, feats).backward(gout)


def timed(m, xyz, feats, gout, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step(m, xyz, feats, gout)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def launches(m, xyz, feats, gout):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            step(m, xyz, feats, gout)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # the profiler is an optional extra of this report
        return f"n/a ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N, C = 12, 128, 256
    torch.manual_seed(0)
    m = GS.MSGSpecConv(C, C, [16, 32]).to(dev)
    xyz = (torch.rand(B, 3, N, device=dev) - 0.5)
    feats = torch.randn(B, C, N, device=dev, requires_grad=True)
    gout = torch.randn(B, C, N, device=dev)
    ms = {True: [], False: []}
    for on in (True, False):      # warm up both
        GS._SPECTRAL_FUSED = on
        timed(m, xyz, feats, gout, 5)
    for _ in range(args.rounds):
        for on in (True, False):
            GS._SPECTRAL_FUSED = on
            ms[on].append(timed(m, xyz, feats, gout, args.iters))
    n = {}
    for on in (True, False):
        GS._SPECTRAL_FUSED = on
        n[on] = launches(m, xyz, feats, gout)
    lines = [f"MSGSpecConv({C}, {C}, [16, 32]) forward + backward, B = {B}, N = {N}, fp32, MI355X",
             f"{args.rounds} interleaved rounds of {args.iters} iterations in one process, ms per iteration"]
    for on, name in ((True, "fused (PCOPS_SPECTRAL_FUSED=1)"), (False, "op chain (PCOPS_SPECTRAL_FUSED=0)")):
        lines.append(f"  {name:36s} median {statistics.median(ms[on]):.4f}  min {min(ms[on]):.4f}  max {max(ms[on]):.4f}"
                     f"  GPU launches per forward+backward: {n[on]}")
    lines.append(f"  median ratio chain / fused: {statistics.median(ms[False]) / statistics.median(ms[True]):.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
