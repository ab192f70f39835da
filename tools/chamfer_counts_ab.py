"""A/B of the counted Chamfer path (clouds of unequal size in one padded batch):

  1. the counted loss node metrics.chamfer_sqrt(p1, p2, counts1, counts2), forward and forward + backward,
     against its chain (chamfer_sqrt_counts_chain: a loop of B = 1 uniform calls with the counts read back
     to the host -- the only correct path without the counted kernels) and against the uniform
     chamfer_sqrt on the padded buffers (wrong: the zero rows are points to it; it is what a caller pays
     today, and shows whether stopping at the count saves time).  B 32, 2048 x 2048 and 2048 x 16384,
     counts uniform in [N / 2, N].
  2. the counted forward entry at FULL counts against the uniform entry (chamfer_forward_raw with and
     without counts), the same shapes plus 16384 x 16384 (where the uniform entry takes the culled search
     and the counted entry has none).

All variants of a row run in ONE process in interleaved rounds on the same data, timed with device events
after a warm-up of each; the report gives the per-round median, minimum and maximum.

    python tools/chamfer_counts_ab.py [--rounds 5] [--iters 10] [--out profiles/chamfer_counts_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import metrics as M  # noqa: E402
from svdformer_pointsea_amd.chamfer3D import chamfer_forward_raw  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(variants, args, lines):
    for _, fn in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            times[name].append(timed(fn, args.iters))
    for name, _ in variants:
        t = times[name]
        lines.append(f"    {name:<34s} median {statistics.median(t):8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}")


def clouds(B, n, m, dev, gen):
    a = (torch.rand(B, n, 3, device=dev, generator=gen) - 0.5)
    b = (torch.rand(B, m, 3, device=dev, generator=gen) - 0.5)
    c1 = torch.randint(n // 2, n + 1, (B,), device=dev, generator=gen).int()
    c2 = torch.randint(m // 2, m + 1, (B,), device=dev, generator=gen).int()
    keep1 = torch.arange(n, device=dev)[None, :, None] < c1[:, None, None]
    keep2 = torch.arange(m, device=dev)[None, :, None] < c2[:, None, None]
    return a * keep1, b * keep2, c1, c2   # zero padding, as pcops_crop_pack leaves it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    lines = [f"counted Chamfer A/B on {torch.cuda.get_device_name(0)}: {args.rounds} interleaved rounds of "
             f"{args.iters} calls each, device events, ms per call", ""]
    B = 32
    lines.append("1. chamfer_sqrt over counted clouds, B 32, counts uniform in [N/2, N] (zero-padded rows)")
    for n, m in ((2048, 2048), (2048, 16384)):
        a, b, c1, c2 = clouds(B, n, m, dev, gen)
        with torch.no_grad():
            node, chain = M.chamfer_sqrt(a, b, c1, c2), M.chamfer_sqrt_counts_chain(a, b, c1, c2)
            padded = M.chamfer_sqrt(a, b)
        lines.append(f"  {n} x {m}: mean counts {float(c1.float().mean()):.0f} / {float(c2.float().mean()):.0f}; "
                     f"node {float(node):.6f}, chain {float(chain):.6f}, uniform call on the padding "
                     f"{float(padded):.6f} (wrong)")
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)

        def fb(fn):
            def run():
                ar.grad = br.grad = None
                fn().backward()
            return run

        lines.append("   forward (graph recorded)")
        rounds([("counted node", lambda: M.chamfer_sqrt(ar, br, c1, c2)),
                ("chain of B = 1 calls", lambda: M.chamfer_sqrt_counts_chain(ar, br, c1, c2)),
                ("uniform on padded (wrong)", lambda: M.chamfer_sqrt(ar, br))], args, lines)
        lines.append("   forward + backward")
        rounds([("counted node", fb(lambda: M.chamfer_sqrt(ar, br, c1, c2))),
                ("chain of B = 1 calls", fb(lambda: M.chamfer_sqrt_counts_chain(ar, br, c1, c2))),
                ("uniform on padded (wrong)", fb(lambda: M.chamfer_sqrt(ar, br)))], args, lines)
    lines += ["", "2. forward entry at FULL counts against the uniform entry, B 32"]
    for n, m in ((2048, 2048), (2048, 16384), (16384, 16384)):
        a = torch.rand(B, n, 3, device=dev, generator=gen) - 0.5
        b = torch.rand(B, m, 3, device=dev, generator=gen) - 0.5
        c1 = torch.full((B,), n, dtype=torch.int32, device=dev)
        c2 = torch.full((B,), m, dtype=torch.int32, device=dev)
        same = all(torch.equal(x, y) for x, y in zip(chamfer_forward_raw(a, b, c1, c2), chamfer_forward_raw(a, b)))
        lines.append(f"  {n} x {m}: outputs equal bit for bit: {same}")
        rounds([("counted entry, full counts", lambda: chamfer_forward_raw(a, b, c1, c2)),
                ("uniform entry", lambda: chamfer_forward_raw(a, b))], args, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
