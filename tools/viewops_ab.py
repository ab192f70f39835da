"""A/B of the view-space ops: the libpcops kernels (csrc/viewops.hip, pcops_points2depth_backward in
csrc/render.hip) against the reference's op chain in torch on the GPU (what PCOPS_VIEWOPS_FUSED=0
runs, and all the parent commit offers):

  splat   point_fea_img_fea          kernels: count + place + ordered sum (pcops_pixel_splat)
                                     chain:   mask, where, index repeat over C, zeros, float-atomic scatter_add
  gather  distribute_img_fea_points  kernels: ONE pcops_pixel_gather reading the NCHW map in place
                                     chain:   permuted copy of the map, mask, gather, where
          at (B 32, N 2048, C 256, 14x14) and (B 96, N 2048, C 64, 56x56)
  depth   PCViews.get_img under grad kernels: pcops_points2depth (+ pcops_points2depth_backward)
                                     chain:   render.points2depth_chain through autograd
          at (B 32, N 2048, R 224) and (B 32, N 16384, R 224)
  and one shape outside the issue's four, the splat's scaling limit: (B 1, N 65536, C 64, 14x14), where the
  single placing wave of the one cloud walks 1024 dependent steps

forward (autograd graph recorded), and forward + backward.  Both variants run in ONE process in
interleaved rounds on the same data; the report gives the per-round median, minimum and maximum of each
and the GPU kernel launches of one pass of each (torch.profiler).  Usage:

    python tools/viewops_ab.py [--rounds 10] [--iters 200] [--out profiles/viewops_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import model_utils as MU  # noqa: E402
from svdformer_pointsea_amd import render  # noqa: E402


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


def exchange_legs(B, N, C, h, w, dev):
    g = torch.Generator().manual_seed(N + C + h)
    P = h * w
    coord = (torch.rand(B, N, generator=g) * 1.2 * P - 0.1 * P).to(dev)      # about 17 % outside the image
    fea = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True)
    img = torch.randn(B, C, h, w, generator=g).to(dev).requires_grad_(True)
    go_s = torch.randn(B, P, C, generator=g).to(dev)
    go_g = torch.randn(B, N, C, generator=g).to(dev)
    splat = (lambda: MU.point_fea_img_fea(fea, coord, h, w), lambda: MU.point_fea_img_fea_chain(fea, coord, h, w))
    gather = (lambda: MU.distribute_img_fea_points(img, coord), lambda: MU.distribute_img_fea_points_chain(img, coord))
    with torch.no_grad():
        err = float((splat[0]() - splat[1]()).abs().max())
        same = torch.equal(gather[0](), gather[1]())
        twice = torch.equal(splat[0](), splat[0]())
    return ((splat[0], splat[1], (fea,), go_s, f"max |kernels - chain| {err:.3g} (the chain's sum is float-atomic); "
             f"kernels bit-equal run to run: {twice}"),
            (gather[0], gather[1], (img,), go_g, f"rows bit-equal: {same}"))


def depth_legs(B, N, R, dev):
    g = torch.Generator().manual_seed(N + R)
    pts = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev).requires_grad_(True)
    view = render.PCViews(TRANS=-0.7, RESOLUTION=R)
    rot, trans = view._consts(dev)
    go = torch.randn(B * 3, R, R, generator=g).to(dev)

    def fused():
        return view.get_img(pts)

    def chain():
        return render.points2depth_chain(pts, rot, trans, R)

    a, b = fused(), chain()
    ga, = torch.autograd.grad(a, pts, go)
    gb, = torch.autograd.grad(b, pts, go)
    a, b = a.detach(), b.detach()
    note = (f"same support: {torch.equal(a != 0, b != 0)}; max |img diff| {float((a - b).abs().max()):.3g}; "
            f"max |grad diff| / max |grad| {float((ga - gb).abs().max() / gb.abs().max()):.3g}")
    return fused, chain, (pts,), go, note


def report(title, legs, args, lines):
    fused, chain, leaves, go, note = legs
    lines.append(f"{title}  [{note}]")

    def fwd(fn):
        fn()

    def fwd_bwd(fn):
        for t in leaves:
            t.grad = None
        fn().backward(go)

    for name, run in (("forward", fwd), ("forward + backward", fwd_bwd)):
        variants = (("kernels", lambda: run(fused)), ("chain", lambda: run(chain)))
        ms = {k: [] for k, _ in variants}
        for k, fn in variants:      # warm up both
            timed(fn, 20)
        for _ in range(args.rounds):
            for k, fn in variants:
                ms[k].append(timed(fn, args.iters))
        lines.append(f"  {name}")
        for k, fn in variants:
            lines.append(f"    {k:7s} median {statistics.median(ms[k]):.4f}  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}"
                         f"  GPU launches per pass: {launches(fn)}")
        lines.append(f"    median ratio chain / kernels: "
                     f"{statistics.median(ms['chain']) / statistics.median(ms['kernels']):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)   # passes take 0.05-1 ms: windows of 10-200 ms
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    assert render.viewops_fused(), "PCOPS_VIEWOPS_FUSED=0 would time the chain against itself"
    lines = ["View-space ops, libpcops kernels against the reference's torch chain on the GPU, fp32, MI355X",
             f"{args.rounds} interleaved rounds of {args.iters} iterations in one process, ms per iteration"]
    for B, N, C, h, w in ((32, 2048, 256, 14, 14), (96, 2048, 64, 56, 56)):
        splat, gather = exchange_legs(B, N, C, h, w, dev)
        report(f"splat   B {B}, N {N}, C {C}, {h}x{w}", splat, args, lines)
        report(f"gather  B {B}, N {N}, C {C}, {h}x{w} (NCHW map)", gather, args, lines)
        del splat, gather
        torch.cuda.empty_cache()
    for B, N, R in ((32, 2048, 224), (32, 16384, 224)):
        report(f"depth   B {B}, N {N}, R {R}", depth_legs(B, N, R, dev), args, lines)
    splat, _ = exchange_legs(1, 65536, 64, 14, 14, dev)
    report("splat   B 1, N 65536, C 64, 14x14 (one cloud: the placing wave's serial limit)", splat, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
