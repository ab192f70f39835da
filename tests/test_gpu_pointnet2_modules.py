"""The PointNet++ SA / FP modules on the GPU against tests/golden/pointnet2.npz (the reference's own
classes on the CPU oracle) and against their own unfused chain (PCOPS_PN2_FUSED=0).

  state      every case loads the golden weights with a strict load_state_dict.
  SA         the fused path equals the unfused path bitwise, train and eval mode: the same rows
             go into the same code.
  golden     per output and per gradient tensor, e_fused = max |fused - golden| stays within
             4 x e_unfused = max |unfused - golden| (the factor test_gpu_capture_fork.py uses for
             eager spread); the figures are printed.
  tokens     forward_tokens equals forward up to the transposes, bitwise.
  stack      SA -> SA -> FP -> FP at (B 2, N 256), forward and backward, fused and unfused, both
             measured against a float64 run of the unfused stack (indices from the fp32 searches):
             the same 4 x bar per tensor.

Measured on an MI355X (the figures the tests print; profiles/pointnet2_tests.txt has the run):
  SA cases: e_fused = e_unfused in every output and parameter gradient (the forward is bitwise the same);
    outputs within 2.7e-06 of the golden (mu_sa_all train), parameter gradients within 4.0e-05 at max|golden| 23
    (mu_sa pgrad_1); sa_msg igrad_feat: 9.54e-07 both (float atomics in both; 8.94e-07 fused in another run)
  FP cases, worst e_fused / e_unfused: 1.33 (mu_fp pgrad_1: 2.86e-06 -> 3.81e-06; also fp igrad_feat 3.58e-07 ->
    4.77e-07); outputs: fp train_0 3.58e-07 both, mu_fp train_0 3.58e-07 both, fp_noskip train_0 8.34e-06 both
    the conv biases under a BatchNorm (exact gradient 0, e.g. mu_fp pgrad_2, max|golden| 2.15e-06): e_unfused
    2.62e-06, e_fused 2.15e-06 -- rounding residue on both sides
  stack: out e_chain 4.54e-06, e_fused 4.18e-06 at max|f64| 5.28; worst e_fused / e_chain over the 20 tensors 1.52
    (d_fp2.mlp.1.bias 7.97e-06 -> 1.21e-05); an earlier run gave 1.60 at d_sa1.mlps.0.4.bias (1.39e-05 -> 2.23e-05),
    which in the recorded run is 1.70e-05 -> 1.65e-05: the spread of the float atomics
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointnet2_support import CASES, golden_of, run  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from pointnet2_cases import SA_CASES  # noqa: E402

FACTOR = 4.0
_RUNS = {}


def runs(case, dev, monkeypatch):
    """(fused, unfused) results of a case, computed once and shared by the tests."""
    if case not in _RUNS:
        from svdformer_pointsea_amd import model_utils as mu

        fused = run(case, dev)
        monkeypatch.setattr(mu, "_PN2_FUSED", False)
        _RUNS[case] = (fused, run(case, dev))
    return _RUNS[case]


@pytest.mark.parametrize("case", SA_CASES)
def test_sa_fused_equals_unfused_bitwise(dev, monkeypatch, case):
    fused, unfused = runs(case, dev, monkeypatch)
    for k in fused:
        if k.startswith(("eval", "train")):
            assert np.array_equal(fused[k], unfused[k]), (case, k)


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_the_golden(dev, monkeypatch, case):
    fused, unfused = runs(case, dev, monkeypatch)
    g = golden_of(case)
    for k in sorted(fused):
        assert fused[k].shape == g[k].shape, (case, k, fused[k].shape, g[k].shape)
        e_f = float(np.abs(fused[k].astype(np.float64) - g[k]).max())
        e_u = float(np.abs(unfused[k].astype(np.float64) - g[k]).max())
        print(f"[{case} {k}] max|golden| {float(np.abs(g[k]).max()):.3g}  e_unfused {e_u:.3g}  e_fused {e_f:.3g}")
        assert e_f <= FACTOR * e_u, (case, k, e_f, e_u)


@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_tokens_equals_forward(dev, case):
    a, b = run(case, dev), run(case, dev, "forward_tokens")
    for k in a:
        if k.startswith(("eval", "train")):
            got = b[k]
            if got.shape != a[k].shape:
                got = got.transpose(0, 2, 1)
            assert np.array_equal(a[k], got), (case, k)


# ------------------------------------------------------------------ the two-level stack
C0 = 5


def make_stack(dev):
    from svdformer_pointsea_amd.pointnet2_modules import PointnetFPModule, PointnetSAModule

    torch.manual_seed(3)
    return nn.ModuleDict(dict(sa1=PointnetSAModule([C0, 16, 32], npoint=64, radius=0.25, nsample=16),
                              sa2=PointnetSAModule([32, 32, 64], npoint=16, radius=0.5, nsample=16),
                              fp2=PointnetFPModule([64 + 32, 32]), fp1=PointnetFPModule([32 + C0, 32]))).to(dev)


def run_stack(net, xyz, f0):
    x1, f1 = net["sa1"].forward_tokens(xyz, f0)
    x2, f2 = net["sa2"].forward_tokens(x1, f1)
    u1 = net["fp2"].forward_tokens(x1, x2, f1, f2)
    return net["fp1"].forward_tokens(xyz, x1, f0, u1)


def _rows(t, idx):
    return t[torch.arange(t.shape[0], device=t.device).view(-1, 1, 1), idx]


def mlp64(seq, x):
    """A build_shared_mlp stack in float64; the 1x1 convs as einsums (no convolution library needed)."""
    for m in seq:
        if isinstance(m, nn.Conv2d):
            x = torch.einsum("bcsk,oc->bosk", x, m.weight[:, :, 0, 0])
            if m.bias is not None:
                x = x + m.bias.view(1, -1, 1, 1)
        elif isinstance(m, nn.ReLU):
            x = torch.relu(x)
        else:
            x = m(x)
    return x


def sa64(m, xyz, feats):
    from svdformer_pointsea_amd import pointnet2_utils as pu

    fidx = pu.furthest_point_sample(xyz.float().contiguous(), m.npoint).long()
    new_xyz = _rows(xyz, fidx.unsqueeze(-1)).squeeze(2)
    g = m.groupers[0]
    idx = pu.ball_query(g.radius, g.nsample, xyz.float().contiguous(), new_xyz.float().contiguous()).long()
    x = torch.cat([_rows(xyz, idx) - new_xyz.unsqueeze(2), _rows(feats, idx)], -1).permute(0, 3, 1, 2)
    return new_xyz, mlp64(m.mlps[0], x).max(3)[0].transpose(1, 2)


def fp64(m, unknown, known, uf, kf):
    from svdformer_pointsea_amd import pointnet2_utils as pu

    idx = pu.three_nn(unknown.float().contiguous(), known.float().contiguous())[1].long()
    d = (unknown.unsqueeze(2) - _rows(known, idx)).norm(dim=-1)
    r = 1.0 / (d + 1e-8)
    w = r / r.sum(-1, keepdim=True)
    x = torch.cat([(_rows(kf, idx) * w.unsqueeze(-1)).sum(2), uf], -1)
    return mlp64(m.mlp, x.transpose(1, 2).unsqueeze(-1)).squeeze(-1).transpose(1, 2)


def run_stack64(net, xyz, f0):
    x1, f1 = sa64(net["sa1"], xyz, f0)
    x2, f2 = sa64(net["sa2"], x1, f1)
    return fp64(net["fp1"], xyz, x1, f0, fp64(net["fp2"], x1, x2, f1, f2))


def _grads(net, out, f0, w):
    net.zero_grad()
    (out * w.to(out.dtype)).sum().backward()
    res = {"out": out.detach().double().cpu().numpy(), "d_f0": f0.grad.double().cpu().numpy()}
    for k, p in net.named_parameters():
        res["d_" + k] = p.grad.double().cpu().numpy()
    return res


def test_two_level_stack(dev, monkeypatch):
    from svdformer_pointsea_amd import model_utils as mu

    B, N = 2, 256
    rng = np.random.default_rng(12)
    xyz = torch.from_numpy(rng.uniform(0, 1, (B, N, 3)).astype(np.float32)).to(dev)
    f0_np = rng.standard_normal((B, N, C0)).astype(np.float32)
    w = torch.from_numpy(rng.standard_normal((B, N, 32))).to(dev)
    net = make_stack(dev).train()
    net64 = copy.deepcopy(net).double()

    def one(n, x, dtype):
        f0 = torch.from_numpy(f0_np).to(dev).to(dtype).requires_grad_(True)
        return _grads(n, (run_stack64 if dtype == torch.float64 else run_stack)(n, x, f0), f0, w)

    ref = one(net64, xyz.double(), torch.float64)
    fused = one(net, xyz, torch.float32)
    monkeypatch.setattr(mu, "_PN2_FUSED", False)
    chain = one(net, xyz, torch.float32)
    for k in sorted(ref):
        e_f, e_c = float(np.abs(fused[k] - ref[k]).max()), float(np.abs(chain[k] - ref[k]).max())
        print(f"[stack {k}] max|f64| {float(np.abs(ref[k]).max()):.3g}  e_chain {e_c:.3g}  e_fused {e_f:.3g}")
        assert e_f <= FACTOR * e_c, (k, e_f, e_c)
