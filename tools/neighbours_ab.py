"""A/B of the neighbour-distance helpers: the libpcops scan (pcops_nn_dist_forward / _backward, csrc/knn.hip)
against the reference's torch expressions on the GPU (the *_chain functions: what PCOPS_NEIGHBOURS_FUSED=0
runs, and all the parent commit offers):

  self_nearest_distances_K(x, 3)   B 32, N 2048
  nearest_distances(x, y)          B 32, S 16384, M 2048
  self_nearest_distances(x)        B 8,  N 16384
  self_nearest_distances_K(x, 3)   B 8,  N 16384
  and ONE forward of self_nearest_distances_chain at the model's own output, B 32, N 16384, recorded as
  "does not fit" if an allocation fails

forward (autograd graph recorded) and forward + backward of sum(out).  Both variants run in ONE process in
interleaved rounds on the same data, timed with device events after a warm-up of each; the report gives the
per-round median, minimum and maximum of each, the peak memory of one pass of each
(torch.cuda.max_memory_allocated above what is held before the pass), and how far the two results are apart.

    python tools/neighbours_ab.py [--rounds 5] [--iters 5] [--out profiles/neighbours_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svdformer_pointsea_amd import model_utils as MU  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def report(title, fused, chain, leaves, args, lines):
    with torch.no_grad():
        a, b = fused(), chain()
        ok = torch.isfinite(a) & torch.isfinite(b) & (b > 0)
        rel = float(((a - b).abs()[ok] / b[ok]).max())
        note = f"max |kernels - chain| / chain {rel:.3g} over {int(ok.sum())} of {ok.numel()} rows"
        del a, b, ok
    lines.append(f"{title}  [{note}]")

    def fwd(fn):
        fn()

    def fwd_bwd(fn):
        for t in leaves:
            t.grad = None
        fn().sum().backward()

    for name, run in (("forward", fwd), ("forward + backward", fwd_bwd)):
        variants = (("kernels", lambda: run(fused)), ("chain", lambda: run(chain)))
        ms = {k: [] for k, _ in variants}
        for k, fn in variants:      # warm up both
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in variants:
                ms[k].append(timed(fn, args.iters))
        lines.append(f"  {name}")
        for k, fn in variants:
            lines.append(f"    {k:7s} median {statistics.median(ms[k]):9.4f}  min {min(ms[k]):9.4f}  max {max(ms[k]):9.4f}"
                         f"  peak memory of one pass {peak_mb(fn):10.1f} MiB")
        lines.append(f"    median ratio chain / kernels: "
                     f"{statistics.median(ms['chain']) / statistics.median(ms['kernels']):.3f}")
    for t in leaves:
        t.grad = None
    torch.cuda.empty_cache()


def cloud(B, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, N, generator=g) - 0.5).to(dev).requires_grad_(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)    # passes take 0.2-200 ms
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    assert MU._NEIGHBOURS_FUSED, "PCOPS_NEIGHBOURS_FUSED=0 would time the chain against itself"
    lines = ["Neighbour distances, libpcops kernels against the reference's torch chain on the GPU, fp32, MI355X",
             f"{args.rounds} interleaved rounds of {args.iters} iterations in one process, ms per iteration"]
    x = cloud(32, 2048, 1, dev)
    report("self_nearest_distances_K k 3   B 32, N 2048", lambda: MU.self_nearest_distances_K(x, 3),
           lambda: MU.self_nearest_distances_K_chain(x, 3), (x,), args, lines)
    x, y = cloud(32, 16384, 2, dev), cloud(32, 2048, 3, dev)
    report("nearest_distances              B 32, S 16384, M 2048", lambda: MU.nearest_distances(x, y),
           lambda: MU.nearest_distances_chain(x, y), (x, y), args, lines)
    del y
    x = cloud(8, 16384, 4, dev)
    report("self_nearest_distances         B 8, N 16384", lambda: MU.self_nearest_distances(x),
           lambda: MU.self_nearest_distances_chain(x), (x,), args, lines)
    report("self_nearest_distances_K k 3   B 8, N 16384", lambda: MU.self_nearest_distances_K(x, 3),
           lambda: MU.self_nearest_distances_K_chain(x, 3), (x,), args, lines)
    x = cloud(32, 16384, 5, dev)
    lines.append("self_nearest_distances         B 32, N 16384 (the model's output), forward only, no autograd graph")
    with torch.no_grad():
        lines.append(f"    kernels {timed(lambda: MU.self_nearest_distances(x), 3):9.4f} ms, peak memory of one pass "
                     f"{peak_mb(lambda: MU.self_nearest_distances(x)):.1f} MiB")
        try:
            mb = peak_mb(lambda: MU.self_nearest_distances_chain(x))
            lines.append(f"    chain   {timed(lambda: MU.self_nearest_distances_chain(x), 1):9.4f} ms, peak memory of one "
                         f"pass {mb:.1f} MiB (one (B,N,N) fp32 matrix is {32 * 16384 * 16384 * 4 / 2 ** 20:.0f} MiB)")
        except torch.OutOfMemoryError as exc:
            lines.append(f"    chain   does not fit: {str(exc).splitlines()[0][:160]}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
