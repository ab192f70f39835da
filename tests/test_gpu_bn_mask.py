"""BatchNorm backward without reading the forward output (pcops_batchnorm_fwd_save / _bwd_saved,
csrc/batchnorm.hip), each form behind a switch read per call:

  PCOPS_BN_RECOMPUTE_MASK  no residual: the backward recomputes the activation's decision from x and
                           the forward's saved (scale, shift) instead of reading y
  PCOPS_BN_MASK_BITS       with a residual: the forward leaves one bit per element, the backward
                           reads it instead of y

Each form must give BITWISE the outputs, gradients and running statistics of the y-reading form
(pcops_batchnorm_fwd / _bwd, held against float64 by tests/test_gpu_batchnorm.py): the decision is a
function of the stored y alone, so nothing may differ -- there is no tolerance anywhere in this file."""
import copy

import pytest
import torch
from torch import nn

import svdformer_pointsea_amd.batchnorm as BN
import svdformer_pointsea_amd.svdformer as S

CASES = [  # (N, C, H, W): the shapes of tests/test_gpu_batchnorm.py
    (4, 16, 32, 32),
    (2, 32, 24, 40),
    (3, 64, 12, 12),
    (2, 128, 7, 9),
    (2, 512, 7, 7),
    (5, 24, 10, 10),
]
SWITCHES = ("PCOPS_BN_RECOMPUTE_MASK", "PCOPS_BN_MASK_BITS")


def _set(monkeypatch, on):
    for k in SWITCHES:
        monkeypatch.setenv(k, "1" if on else "0")


def _run(dev, shape, dtype, act, res, training=True):
    g = torch.Generator().manual_seed(hash((shape, act, res)) % 1000)
    N, C, H, W = shape
    cl = torch.channels_last
    x = (torch.randn(shape, generator=g) * 1.7 + 0.8).to(dev, dtype).contiguous(memory_format=cl)
    dy = torch.randn(shape, generator=g).to(dev, dtype).contiguous(memory_format=cl)
    r = None
    if res:
        r = torch.randn(shape, generator=g)
        r[: N // 2 + 1, 1] = 0.0   # with gamma = beta = 0 below: bn + res is exactly 0 there
        r = r.to(dev, dtype).contiguous(memory_format=cl)
    bn = nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.1)
        # channel 1: the zero-initialised bn2 weight of a ResNet block, y exactly 0;
        # channel 2: a negative scale
        bn.weight[1] = 0.0
        bn.bias[1] = 0.0
        bn.weight[2] = -0.7
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    bn.train(training)
    xg = x.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True) if res else None
    y = BN.bn_act(xg, bn, act, 0.2, rg)
    saved_y = any(t is not None and t.data_ptr() == y.data_ptr() for t in y.grad_fn.saved_tensors)
    y.backward(dy)
    out = {"y": y.detach(), "dx": xg.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "rmean": bn.running_mean, "rvar": bn.running_var, "nbt": bn.num_batches_tracked}
    if res:
        out["dres"] = rg.grad
    return out, saved_y


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        # bit patterns, so that NaN == NaN and +0 != -0
        u, v = (t.contiguous().reshape(-1).view(torch.uint8) for t in (a[k], b[k]))
        assert torch.equal(u, v), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", [BN.ACT_RELU, BN.ACT_LEAKY])
@pytest.mark.parametrize("res", [False, True])
def test_bn_bwd_without_y_bitwise(dev, monkeypatch, shape, dtype, act, res):
    _set(monkeypatch, False)
    a, fa = _run(dev, shape, dtype, act, res)
    _set(monkeypatch, True)
    b, fb = _run(dev, shape, dtype, act, res)
    _same(a, b, (shape, dtype, act, res))
    # the two runs really took the two forms: y is among the saved tensors of the first only
    assert fa and not fb
    assert (a["y"][:, 1] == 0).any()   # the exact zeros are there


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("res", [False, True])
def test_bn_bwd_without_y_eval_bitwise(dev, monkeypatch, dtype, res):
    """Eval mode: the saved (scale, shift) come from the running statistics."""
    _set(monkeypatch, False)
    a, _ = _run(dev, (3, 64, 14, 14), dtype, BN.ACT_RELU, res, training=False)
    _set(monkeypatch, True)
    b, _ = _run(dev, (3, 64, 14, 14), dtype, BN.ACT_RELU, res, training=False)
    _same(a, b, (dtype, res))
    assert int(b["nbt"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
def test_bn_switches_are_independent(dev, monkeypatch, switch):
    """Each switch alone changes only its own form, and the results stay bitwise equal."""
    _set(monkeypatch, False)
    ref = {res: _run(dev, (4, 16, 32, 32), torch.bfloat16, BN.ACT_RELU, res)[0] for res in (False, True)}
    monkeypatch.setenv(switch, "1")
    for res in (False, True):
        got, saved_y = _run(dev, (4, 16, 32, 32), torch.bfloat16, BN.ACT_RELU, res)
        _same(ref[res], got, (switch, res))
        mine = res == (switch == "PCOPS_BN_MASK_BITS")
        assert saved_y != mine


def _block(dev, C):
    torch.manual_seed(C)
    blk = S.BasicBlock(C, C).to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
        blk.bn2.weight[3] = 0.0   # a zero-initialised residual branch channel
    return blk


@pytest.mark.gpu
@pytest.mark.parametrize("C,HW", [(16, 56), (32, 28)])
def test_basic_block_bitwise_and_graph_replays(dev, monkeypatch, C, HW):
    """A stride-1 BasicBlock under bf16 autocast (both forms in one block: bn1's backward recomputes,
    bn2's reads bits): bitwise the block with both switches off; then
    its forward + backward captured once and replayed four times, every output and gradient buffer
    overwritten between replays, each replay bitwise the eager result."""
    blk = _block(dev, C)
    x = torch.randn(4, C, HW, HW, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(4, C, HW, HW, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def eager(on):
        _set(monkeypatch, on)
        m = copy.deepcopy(blk)
        xg = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(xg)
        y.backward(dy)
        return [y.detach(), xg.grad] + [p.grad for p in m.parameters()] + [b for b in m.buffers()]

    a, b = eager(False), eager(True)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i

    m = copy.deepcopy(blk)
    for bn in (m.bn1, m.bn2):   # replays must not depend on the running statistics' history
        bn.momentum = 1.0
    xg = x.clone().requires_grad_(True)
    params = list(m.parameters())

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(xg)
        gs = torch.autograd.grad(y, [xg] + params, dy)
        return [y.detach()] + list(gs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ref = [t.clone() for t in step()]
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(4):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (u, v) in enumerate(zip(ref, outs)):
            assert torch.equal(u, v), i


@pytest.mark.gpu
def test_non_eligible_gpu_shape_takes_torch(dev, monkeypatch):
    """C % 8 != 0 is not fusable: torch's modules run, whatever the switches say."""
    _set(monkeypatch, True)
    torch.manual_seed(0)
    bn = nn.BatchNorm2d(12).to(dev)
    ref = copy.deepcopy(bn)
    x = torch.randn(2, 12, 9, 9, device=dev).contiguous(memory_format=torch.channels_last)
    r = torch.randn_like(x)
    y = BN.bn_act(x, bn, BN.ACT_RELU, residual=r)
    assert torch.equal(y, torch.relu(ref(x) + r))
    assert torch.equal(bn.running_var, ref.running_var)


def test_cpu_block_takes_torch(monkeypatch):
    """With every switch on, a CPU BasicBlock is the plain modules' composition."""
    _set(monkeypatch, True)
    torch.manual_seed(1)
    blk = S.BasicBlock(16, 16)
    ref = copy.deepcopy(blk)
    x = torch.randn(2, 16, 12, 12)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = blk(xa)
    yb = torch.relu(ref.bn2(ref.conv2(torch.relu(ref.bn1(ref.conv1(xb))))) + xb)
    assert torch.equal(ya, yb)
    dy = torch.randn_like(ya)
    ya.backward(dy)
    yb.backward(dy)
    assert torch.equal(xa.grad, xb.grad)
    for p, q in zip(blk.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)
    for p, q in zip(blk.buffers(), ref.buffers()):
        assert torch.equal(p, q)

