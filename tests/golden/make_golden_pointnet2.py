"""PointNet++ module golden vectors from the REFERENCE's own classes, run on the CPU in the build
container only; only the .npz output is committed.

The reference's four module files are loaded by path, unchanged:
  pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py     (the autograd Functions, QueryAndGroup, GroupAll)
  pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py   (PointnetSAModuleMSG, PointnetSAModule, PointnetFPModule)
  models/model_utils.py                                  (PointNet_SA_Module, PointNet_FP_Module)
Their compiled extension `pointnet2_ops._ext` is a stub whose nine functions call the CPU oracle
(oracle/pcops_oracle.c, which restates the same .cu files): furthest_point_sampling,
gather_points(_grad), group_points(_grad), ball_query, three_nn (returning d2),
three_interpolate(_grad).

  pointnet2.npz, per case of pointnet2_cases.CASES (prefix "<case>/"):
    keys, shapes          sorted state_dict keys and their shapes
    eval_<i>, train_<i>   the forward's tensor outputs in eval mode (fresh state) and in train mode
    pgrad_<i>             train mode, loss = sum(out * loss_weight): gradient of parameter i (sorted-key order
                          of named_parameters)
    igrad_<name>          the same loss's gradient for the feature inputs
    gaps, bar             SA cases: the positive top-2 gaps of the pre-max activations (train and eval mode)
                          and the bar 64 * 2^-24 * max|act| below which fp32 does not decide a winner
  fps_idx                 (B,S) the FPS indices the inputs' `known` points are

Weights: weights.fill_state(seed, scale=0.3).  The generator asserts the winner condition: among
the maxima with a positive top-2 gap, at most 2 % have a gap below the bar (exact ties -- ReLU
zeros, first-hit duplicates -- are decided by the first-index rule on both sides).

`fp_noknown` (known=None): the reference's expand branch (pointnet2_modules.py:195-197) adds a
list to a torch.Size and raises TypeError; the case records the reference module's own `mlp` on the
tensor that branch describes (known_feats expanded to n points, concatenated with unknow_feats).

Usage:  python tests/golden/make_golden_pointnet2.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden_models import REF  # noqa: E402
from oracle import oracle as O  # noqa: E402
from pointnet2_cases import CASES, GRAD_INPUTS, SA_CASES, S, inputs, kwargs_of, loss_weight  # noqa: E402
from weights import fill_state  # noqa: E402

SCALE, CAP = 0.3, 0.02


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _n(t):
    return t.detach().contiguous().numpy()


def _ext_stub():
    ext = types.ModuleType("pointnet2_ops._ext")
    ext.furthest_point_sampling = lambda xyz, npoint: _t(O.furthest_point_sample(_n(xyz), int(npoint)))
    ext.gather_points = lambda f, idx: _t(O.gather_operation(_n(f), _n(idx)))
    ext.gather_points_grad = lambda g, idx, n: _t(O.gather_operation_grad(_n(g), _n(idx), int(n)))
    ext.group_points = lambda f, idx: _t(O.grouping_operation(_n(f), _n(idx)))
    ext.group_points_grad = lambda g, idx, n: _t(O.grouping_operation_grad(_n(g), _n(idx), int(n)))
    ext.ball_query = lambda new_xyz, xyz, radius, nsample: _t(O.ball_query(radius, nsample, _n(xyz), _n(new_xyz)))

    def three_nn(unknown, known):
        _, idx, d2 = O.three_nn(_n(unknown), _n(known))
        return _t(d2), _t(idx)

    ext.three_nn = three_nn
    ext.three_interpolate = lambda f, idx, w: _t(O.three_interpolate(_n(f), _n(idx), _n(w)))
    ext.three_interpolate_grad = lambda g, idx, w, m: _t(O.three_interpolate_grad(_n(g), _n(idx), _n(w), int(m)))
    return ext


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    """-> {"p2": pointnet2_modules, "mu": model_utils} of the reference, on the oracle."""
    pkg = types.ModuleType("pointnet2_ops")
    pkg.__path__ = []
    sys.modules["pointnet2_ops"] = pkg
    sys.modules["pointnet2_ops._ext"] = pkg._ext = _ext_stub()
    lib = os.path.join(REF, "pointnet2_ops_lib", "pointnet2_ops")
    pkg.pointnet2_utils = _load(os.path.join(lib, "pointnet2_utils.py"), "pointnet2_ops.pointnet2_utils")
    p2 = _load(os.path.join(lib, "pointnet2_modules.py"), "pointnet2_ops.pointnet2_modules")
    mu = _load(os.path.join(REF, "models", "model_utils.py"), "ref_model_utils")
    return {"p2": p2, "mu": mu}


def _pre_max(case, mod):
    """The modules whose output is the pre-max activation tensor (B,C,S,K)."""
    return list(mod.mlps) if CASES[case][0] == "p2" else [mod.mlp_conv]


def _gaps(acts):
    """positive top-2 gaps over the last dim and the bar of a list of (B,C,S,K) activations."""
    gaps, amax = [], 0.0
    for a in acts:
        a = a.double().numpy()
        amax = max(amax, float(np.abs(a).max()))
        if a.shape[-1] < 2:
            continue
        srt = np.sort(a, axis=-1)
        g = (srt[..., -1] - srt[..., -2]).ravel()
        gaps.append(g[g > 0])
    return (np.concatenate(gaps) if gaps else np.zeros(0)), 64 * 2.0 ** -24 * amax


def _forward(case, mod, args):
    if case == "fp_noknown":
        try:
            return mod(*args)
        except TypeError:
            unknown, _, uf, kf = args
            x = torch.cat([kf.expand(kf.shape[0], kf.shape[1], unknown.shape[1]), uf], dim=1)
            return mod.mlp(x.unsqueeze(-1)).squeeze(-1)
    return mod(*args)


def _tensors(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [o for o in out if o is not None]


def run_case(ref, case, ins, out):
    src, cls, _, names, seed = CASES[case]
    mod = fill_state(getattr(ref[src], cls)(**kwargs_of(case)), seed, scale=SCALE)
    sd = mod.state_dict()
    keys = sorted(sd)
    out[f"{case}/keys"] = np.array(keys)
    out[f"{case}/shapes"] = np.array([str(tuple(sd[k].shape)) for k in keys])
    acts = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: acts.append(o.detach().clone()))
             for m in (_pre_max(case, mod) if case in SA_CASES else ())]
    args = [None if n is None else _t(ins[n]).requires_grad_(n in GRAD_INPUTS) for n in names]

    mod.eval()
    with torch.no_grad():
        for i, o in enumerate(_tensors(_forward(case, mod, args))):
            out[f"{case}/eval_{i}"] = _n(o)
    mod.train()
    res = _tensors(_forward(case, mod, args))
    for i, o in enumerate(res):
        out[f"{case}/train_{i}"] = _n(o)
    feats = res[-1]      # the feature output (SA modules return new_xyz first)
    (feats * _t(loss_weight(case, tuple(feats.shape)))).sum().backward()
    params = dict(mod.named_parameters())
    for i, k in enumerate(sorted(params)):
        out[f"{case}/pgrad_{i}"] = _n(params[k].grad)
    for n, a in zip(names, args):
        if n in GRAD_INPUTS:
            out[f"{case}/igrad_{n}"] = _n(a.grad)
    for h in hooks:
        h.remove()
    if case in SA_CASES:
        gaps, bar = _gaps(acts)
        close = int((gaps < bar).sum())
        print(f"{case}: bar {bar:.3g}, {close} of {gaps.size} positive gaps below it, smallest {gaps.min():.3g}")
        assert close <= CAP * gaps.size, (case, close, gaps.size)
        out[f"{case}/gaps"], out[f"{case}/bar"] = gaps.astype(np.float32), np.array(bar)


def main():
    torch.manual_seed(0)
    ref = load_reference()
    fps_idx = O.furthest_point_sample(inputs(None)["xyz_t"], S)
    ins = inputs(fps_idx)
    out = {"fps_idx": fps_idx}
    for case in CASES:
        run_case(ref, case, ins, out)
    path = os.path.join(HERE, "pointnet2.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
