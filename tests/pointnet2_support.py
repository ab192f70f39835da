"""Helpers of the PointNet++ module tests (not a conftest): build this package's module of a golden
case, its inputs, and run it the way tests/golden/make_golden_pointnet2.py ran the reference."""
import os
import sys

import numpy as np
import torch

from conftest import GOLDEN, golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from pointnet2_cases import CASES, GRAD_INPUTS, inputs, kwargs_of, loss_weight  # noqa: E402
from weights import fill_state  # noqa: E402

SCALE = 0.3
_G = {}


def gold():
    if "g" not in _G:
        _G["g"] = golden("pointnet2.npz")
    return _G["g"]


def build(case):
    """This package's module of `case`, with the golden weights (a strict load_state_dict)."""
    from svdformer_pointsea_amd import model_utils, pointnet2_modules

    src, cls, _, _, seed = CASES[case]
    mod = getattr(pointnet2_modules if src == "p2" else model_utils, cls)(**kwargs_of(case))
    return fill_state(mod, seed, scale=SCALE)


def case_inputs():
    if "ins" not in _G:
        _G["ins"] = inputs(gold()["fps_idx"])
    return _G["ins"]


def tensors(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [o for o in out if o is not None]


def run(case, dev, method="forward"):
    """-> dict: eval_<i>, train_<i>, pgrad_<i>, igrad_<name> as numpy, the generator's recipe."""
    mod = build(case).to(dev)
    names = CASES[case][3]
    ins = case_inputs()
    args = [None if n is None else torch.from_numpy(ins[n]).to(dev).requires_grad_(n in GRAD_INPUTS) for n in names]
    if method == "forward_tokens":
        # features token-major; coordinates token-major too for the model_utils classes
        args = [a if a is None or (a.shape[-1] == 3 and CASES[case][0] == "p2") else a.detach().transpose(1, 2)
                .contiguous().requires_grad_(a.requires_grad) for a in args]
    fn = getattr(mod, method)
    res = {}
    mod.eval()
    with torch.no_grad():
        for i, o in enumerate(tensors(fn(*args))):
            res[f"eval_{i}"] = o.float().cpu().numpy()
    mod.train()
    out = tensors(fn(*args))
    for i, o in enumerate(out):
        res[f"train_{i}"] = o.detach().float().cpu().numpy()
    feats = out[-1]
    shape = tuple(feats.shape)
    if method == "forward_tokens":
        shape = (shape[0], shape[2], shape[1])       # the loss weight is laid out as forward's output
    w = torch.from_numpy(loss_weight(case, shape)).to(dev)
    (feats * (w.transpose(1, 2) if method == "forward_tokens" else w)).sum().backward()
    params = dict(mod.named_parameters())
    for i, k in enumerate(sorted(params)):
        res[f"pgrad_{i}"] = params[k].grad.cpu().numpy()
    for n, a in zip(names, args):
        if n in GRAD_INPUTS:
            res[f"igrad_{n}"] = a.grad.cpu().numpy()
    return res


def golden_of(case):
    g = gold()
    pre = case + "/"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
