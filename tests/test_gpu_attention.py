"""GPU parity of the attention core (fp32 MFMA path: 1e-5 abs, the north-star
tolerance; bf16 path: bf16-appropriate tolerance) and of the reference's
attention blocks against golden vectors from the reference's own modules."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [  # (B, H, Lq, Lk, E)
    (2, 4, 3, 3, 256),      # SVFNet viewattn
    (2, 4, 128, 128, 512),  # SVFNet sa (hd 128)
    (1, 8, 512, 512, 768),  # refine1 (hd 96)
    (1, 8, 200, 77, 512),   # ragged cross (hd 64)
    (1, 8, 2048, 512, 512), # refine2 cross
    (1, 8, 333, 250, 1024), # ragged hd 128 (split dK/dV path)
    (2, 2, 70, 130, 64),    # hd 32
    (2, 8, 2048, 2048, 512),   # refine2 self-attention at its real length (hd 64, 32 key tiles)
    (2, 8, 2048, 2048, 1024),  # refine2 decoder sa2 at its real length (hd 128)
    (2, 8, 1024, 1024, 768),   # PointSea ShapeNet-55 refine1 (hd 96 at L = 1024, models_PointSea/model_utils.py:385-509)
    (3, 4, 49, 49, 512),       # PointSea viewattn1: 7x7 ResNet-18 view tokens (hd 128, PointSea.py:188-229)
]


def _qkv(B, H, Lq, Lk, E, dev, dtype=torch.float32, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(Lq, B, E, generator=g)
    k = torch.randn(Lk, B, E, generator=g)
    v = torch.randn(Lk, B, E, generator=g)
    return [t.to(dev, dtype) for t in (q, k, v)]


def _ref(q, k, v, H):
    """float64 math of nn.MultiheadAttention's core on (L,B,E) inputs."""
    Lq, B, E = q.shape
    hd = E // H
    qq = q.double().reshape(Lq, B * H, hd).transpose(0, 1)
    kk = k.double().reshape(-1, B * H, hd).transpose(0, 1)
    vv = v.double().reshape(-1, B * H, hd).transpose(0, 1)
    s = qq @ kk.transpose(1, 2) / math.sqrt(hd)
    o = torch.softmax(s, -1) @ vv
    return o.transpose(0, 1).reshape(Lq, B, E)


@pytest.mark.parametrize("B,H,Lq,Lk,E", SHAPES)
def test_core_forward_fp32(dev, B, H, Lq, Lk, E):
    from svdformer_pointsea_amd.attention import attention_core

    q, k, v = _qkv(B, H, Lq, Lk, E, dev)
    o = attention_core(q, k, v, H)
    ref = _ref(q, k, v, H)
    err = (o.double() - ref).abs().max().item()
    assert err < 1e-5, err
    # oracle cross-check on one head
    hd = E // H
    oo = O.attention_core(q[:, 0, :hd].cpu().numpy()[None], k[:, 0, :hd].cpu().numpy()[None],
                          v[:, 0, :hd].cpu().numpy()[None])[0]
    np.testing.assert_allclose(o[:, 0, :hd].cpu().numpy(), oo, atol=1e-5)


@pytest.mark.parametrize("B,H,Lq,Lk,E", SHAPES)
def test_core_backward_fp32(dev, B, H, Lq, Lk, E):
    from svdformer_pointsea_amd.attention import attention_core

    q, k, v = _qkv(B, H, Lq, Lk, E, dev, seed=1)
    g = torch.randn(Lq, B, E, generator=torch.Generator().manual_seed(5)).to(dev)
    qs, ks, vs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    (attention_core(qs, ks, vs, H) * g).sum().backward()
    qd, kd, vd = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    (_ref(qd, kd, vd, H) * g.double()).sum().backward()
    # the north-star bar, absolute: measured max |err| over SHAPES is 2.3e-6 (dk/dv at
    # 2048 x 512, hd 64) against max |grad| 0.3-3.6 (tools/attn_err.py, profiles/r3_attn_err.jsonl)
    for a, b in [(qs.grad, qd.grad), (ks.grad, kd.grad), (vs.grad, vd.grad)]:
        err = (a.double() - b).abs().max().item()
        assert err < 1e-5, err


@pytest.mark.parametrize("B,H,Lq,Lk,E", SHAPES)
def test_core_bf16(dev, B, H, Lq, Lk, E):
    from svdformer_pointsea_amd.attention import attention_core

    q, k, v = _qkv(B, H, Lq, Lk, E, dev, seed=2)
    qb, kb, vb = [t.to(torch.bfloat16).requires_grad_(True) for t in (q, k, v)]
    o = attention_core(qb, kb, vb, H)
    assert o.dtype == torch.bfloat16
    ref = _ref(qb.detach().float(), kb.detach().float(), vb.detach().float(), H)
    assert (o.double() - ref).abs().max().item() < 3e-2
    g = torch.randn(Lq, B, E, generator=torch.Generator().manual_seed(6)).to(dev)
    (o.float() * g).sum().backward()
    qd, kd, vd = [t.detach().double().clone().requires_grad_(True) for t in (qb, kb, vb)]
    (_ref(qd, kd, vd, H) * g.double()).sum().backward()
    for a, b in [(qb.grad, qd.grad), (kb.grad, kd.grad), (vb.grad, vd.grad)]:
        rel = (a.double() - b).norm().item() / max(b.norm().item(), 1e-6)
        assert rel < 3e-2, rel


@pytest.mark.parametrize("B,H,Lq,Lk,E", [(2, 8, 2048, 2048, 512), (2, 8, 2048, 2048, 1024), (2, 4, 130, 129, 128),
                                         (1, 8, 333, 250, 1024)])
def test_core_bf16_run_to_run_bitwise(dev, B, H, Lq, Lk, E):
    """The bf16 kernels are deterministic: four forward + backward passes on the same
    inputs agree bit for bit (round 3: the 8-wave forward read MFMA accumulators
    through an inline-asm v_max3 before the MFMA had written them -- no hazard wait
    states are inserted for asm -- and its output moved in the last bit run to run)."""
    from svdformer_pointsea_amd.attention import attention_core

    q, k, v = [t.to(torch.bfloat16) for t in _qkv(B, H, Lq, Lk, E, dev, seed=3)]
    g = torch.randn(Lq, B, E, generator=torch.Generator().manual_seed(8)).to(dev, torch.bfloat16)
    runs = []
    for _ in range(4):
        qs, ks, vs = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = attention_core(qs, ks, vs, H)
        o.backward(g)
        runs.append((o.detach(), qs.grad, ks.grad, vs.grad))
    for r in runs[1:]:
        for name, a, b in zip(("o", "dq", "dk", "dv"), runs[0], r):
            assert torch.equal(a, b), name


def _nrand(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def test_blocks_match_reference_golden(dev):
    import sys

    from conftest import GOLDEN

    sys.path.insert(0, GOLDEN)
    from weights import fill_state

    from svdformer_pointsea_amd import attention as A

    g = golden("attention.npz")
    tol = dict(atol=2e-5, rtol=2e-5)
    sa = fill_state(A.self_attention(256, 512, nhead=8), seed=100).eval().to(dev)
    x, pos = _nrand(101, 2, 256, 64).to(dev), _nrand(102, 64, 2, 512).to(dev)
    with torch.no_grad():
        np.testing.assert_allclose(sa(x, pos).cpu().numpy(), g["sa_y"], **tol)
        np.testing.assert_allclose(sa(x).cpu().numpy(), g["sa_y_nopos"], **tol)
        ca = fill_state(A.cross_attention(512, 512, nhead=8), seed=110).eval().to(dev)
        y = ca(_nrand(111, 2, 512, 64).to(dev), _nrand(112, 2, 512, 32).to(dev))
        np.testing.assert_allclose(y.cpu().numpy(), g["ca_y"], **tol)
        dec = fill_state(A.SDG_Decoder(512, 64, 8), seed=120).eval().to(dev)
        np.testing.assert_allclose(dec(_nrand(121, 2, 512, 48).to(dev)).cpu().numpy(), g["dec_y"], **tol)
        wo = fill_state(A.self_attention_woinp(768, 768, nhead=8), seed=130).eval().to(dev)
        np.testing.assert_allclose(wo(_nrand(131, 2, 768, 40).to(dev)).cpu().numpy(), g["woinp_y"], **tol)
        sv = fill_state(A.self_attention(384, 256, nhead=4), seed=140).eval().to(dev)
        y = sv(_nrand(141, 2, 384, 3).to(dev), _nrand(142, 3, 2, 256).to(dev))
        np.testing.assert_allclose(y.cpu().numpy(), g["sav_y"], **tol)


def _torch_block(blk, x, pos=None, x2=None):
    """The reference's self_attention / cross_attention forward
    (models/model_utils.py:542-617) in plain torch ops, on blk's parameters."""
    import torch.nn.functional as F

    C = blk.norm13.weight.shape[0]
    mha = blk.multihead_attn

    def inp(t):
        t = F.conv1d(t, blk.input_proj.weight, blk.input_proj.bias) if hasattr(blk, "input_proj") else t
        return F.layer_norm(t.permute(2, 0, 1), (C,), blk.norm13.weight, blk.norm13.bias, blk.norm13.eps)

    s1 = inp(x)
    kv = s1 if x2 is None else inp(x2)
    q = s1 if pos is None else s1 + pos
    k = q if x2 is None else kv
    a = F.multi_head_attention_forward(q, k, kv, C, mha.num_heads, mha.in_proj_weight, mha.in_proj_bias, None, None,
                                       False, 0.0, mha.out_proj.weight, mha.out_proj.bias, training=False,
                                       need_weights=False)[0]
    s1 = F.layer_norm(s1 + a, (C,), blk.norm12.weight, blk.norm12.bias, blk.norm12.eps)
    f = blk.linear12(blk.activation1(blk.linear11(s1)))
    return (s1 + f).permute(1, 2, 0)


@pytest.mark.parametrize("kind", ["self", "self_pos", "cross", "woinp"])
def test_block_gradients_match_torch(dev, kind):
    """Fused token-major block (packed projections, fused LayerNorm/transpose
    kernels, MFMA core) == the reference block in torch ops: outputs, input and
    parameter gradients, fp32."""
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(0)
    if kind == "cross":
        blk = A.cross_attention(64, 128, nhead=4).to(dev)
    elif kind == "woinp":
        blk = A.self_attention_woinp(128, 128, nhead=4).to(dev)
    else:
        blk = A.self_attention(64, 128, nhead=4).to(dev)
    cin = 128 if kind == "woinp" else 64
    x = torch.randn(2, cin, 50, device=dev)
    x2 = torch.randn(2, cin, 37, device=dev) if kind == "cross" else None
    pos = torch.randn(50, 2, 128, device=dev) if kind == "self_pos" else None
    ins = [t.clone().requires_grad_(True) for t in (x, x2) if t is not None]
    y = blk(*ins, pos) if kind != "woinp" else blk(ins[0])
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    g_ours = {n: p.grad.clone() for n, p in blk.named_parameters()}
    gin_ours = [t.grad.clone() for t in ins]
    blk.zero_grad()
    ins2 = [t.detach().clone().requires_grad_(True) for t in ins]
    y2 = _torch_block(blk, ins2[0], pos, ins2[1] if kind == "cross" else None)
    (y2 * gy).sum().backward()
    torch.testing.assert_close(y, y2, rtol=1e-4, atol=2e-5)
    for a, b in zip(gin_ours, ins2):
        torch.testing.assert_close(a, b.grad, rtol=1e-4, atol=2e-5)
    for n, p in blk.named_parameters():
        torch.testing.assert_close(g_ours[n], p.grad, rtol=1e-4, atol=5e-5, msg=n)


def test_block_bf16_autocast_close_to_fp32(dev):
    """Under bf16 autocast (the training configuration) the fused block stays
    within bf16 tolerance of its fp32 result, forward and backward."""
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(1)
    dec = A.SDG_Decoder(256, 32, 8).to(dev)  # head dims 32 / 32
    x = torch.randn(2, 256, 300, device=dev, requires_grad=True)
    y = dec(x)
    y.square().mean().backward()
    g32 = {n: p.grad.clone() for n, p in dec.named_parameters()}
    gx = x.grad.clone()
    dec.zero_grad()
    x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yb = dec(x)
    assert yb.dtype == torch.float32
    yb.square().mean().backward()
    assert (yb - y).norm() / y.norm() < 2e-2
    assert (x.grad - gx).norm() / gx.norm() < 5e-2
    for n, p in dec.named_parameters():
        rel = (p.grad - g32[n]).norm() / max(g32[n].norm(), 1e-12)
        assert rel < 8e-2, (n, rel.item())


@pytest.mark.parametrize("B,L,C", [(3, 70, 768), (1, 40001, 512), (2, 65536, 128)])
def test_layernorm_and_transpose_kernels(dev, B, L, C):
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(2)
    norm = torch.nn.LayerNorm(C).to(dev)
    with torch.no_grad():
        norm.weight.normal_()
        norm.bias.normal_()
    a = torch.randn(B, L, C, device=dev, requires_grad=True)
    b = torch.randn(B, L, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    y, _ = A.layer_norm(norm, a, b)
    ref = torch.nn.functional.layer_norm(a + b.float(), (C,), norm.weight, norm.bias, norm.eps)
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)
    g = torch.randn_like(y)
    (y * g).sum().backward()
    ga, gb, gw, gbeta = a.grad.clone(), b.grad.clone(), norm.weight.grad.clone(), norm.bias.grad.clone()
    a.grad = b.grad = None
    norm.zero_grad()
    (torch.nn.functional.layer_norm(a + b.float(), (C,), norm.weight, norm.bias, norm.eps) * g).sum().backward()
    torch.testing.assert_close(ga, a.grad, rtol=1e-4, atol=1e-5)
    assert gb.dtype == torch.bfloat16
    torch.testing.assert_close(gb.float(), b.grad.float(), rtol=1e-2, atol=1e-2)
    tol = 1e-4 * max(1.0, (B * L) ** 0.5 / 10)   # fp32 sums over B*L rows in different orders
    torch.testing.assert_close(gw, norm.weight.grad, rtol=1e-4, atol=tol)
    torch.testing.assert_close(gbeta, norm.bias.grad, rtol=1e-4, atol=tol)
    if L > 1000:
        return
    # (B, C, L) <-> (B, L, C), ragged tiles, with an add and a dtype change
    x = torch.randn(2, 130, 67, device=dev)
    t = A.to_tokens(x)
    torch.testing.assert_close(t, x.transpose(1, 2))
    z = A.to_channels(t, t.to(torch.bfloat16), torch.bfloat16)
    torch.testing.assert_close(z.float(), (x + x.to(torch.bfloat16).float()).to(torch.bfloat16).float())


@pytest.mark.parametrize("adt,bdt", [(torch.float32, None), (torch.bfloat16, None), (torch.bfloat16, torch.float32),
                                     (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("C", [96, 512, 768, 1024])
def test_layernorm_operand_configs(dev, adt, bdt, C):
    """Every compiled operand configuration of pcops_layernorm_fwd/bwd (a / b
    dtypes, residual or not, both output copies with gradients on both), at a
    full-lane C (512, 1024) and partial-chunk C (96, 768), against torch."""
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(C)
    rows = 999
    norm = torch.nn.LayerNorm(C).to(dev)
    with torch.no_grad():
        norm.weight.normal_()
        norm.bias.normal_()
    a = torch.randn(rows, C, device=dev).to(adt).requires_grad_(True)
    b = None if bdt is None else torch.randn(rows, C, device=dev).to(bdt).requires_grad_(True)
    y32, y16 = A._LayerNorm.apply(a, b, norm.weight, norm.bias, norm.eps, True)
    x = a.float() + (0 if b is None else b.float())
    ref = torch.nn.functional.layer_norm(x, (C,), norm.weight, norm.bias, norm.eps)
    torch.testing.assert_close(y32, ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(y16, y32.to(torch.bfloat16))
    g1, g2 = torch.randn_like(y32), torch.randn_like(y32).to(torch.bfloat16)
    torch.autograd.backward([y32, y16], [g1, g2])
    xr = x.detach().requires_grad_(True)
    w = norm.weight.detach().clone().requires_grad_(True)
    bb = norm.bias.detach().clone().requires_grad_(True)
    (torch.nn.functional.layer_norm(xr, (C,), w, bb, norm.eps) * (g1 + g2.float())).sum().backward()
    tol = dict(rtol=1e-4, atol=1e-5) if adt == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    assert a.grad.dtype == adt
    torch.testing.assert_close(a.grad.float(), xr.grad.to(adt).float(), **tol)
    if b is not None:
        assert b.grad.dtype == bdt
        torch.testing.assert_close(b.grad.float(), xr.grad.to(bdt).float(),
                                   **(dict(rtol=1e-4, atol=1e-5) if bdt == torch.float32 else dict(rtol=1e-2, atol=1e-2)))
    torch.testing.assert_close(norm.weight.grad, w.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(norm.bias.grad, bb.grad, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("cin,cout,T", [(40, 8, 999), (512, 512, 65536), (64, 3072, 16384)])
def test_linear_splitk_wgrad(dev, amp, cin, cout, T):
    """attention.linear (split-K weight gradient) vs F.linear, fwd + bwd."""
    import torch.nn.functional as F

    from svdformer_pointsea_amd import attention

    g = torch.Generator().manual_seed(cout)
    x = torch.randn(T, cin, generator=g).to(dev)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    go = torch.randn(T, cout, generator=g).to(dev)
    outs = []
    for fn in (attention._Linear.apply, F.linear):
        xs, ws, bs = [t.clone().requires_grad_(True) for t in (x, w, b)]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = fn(xs, ws, bs)
        (y.float() * go).sum().backward()
        outs.append((y.float(), xs.grad, ws.grad, bs.grad))
    for a, r in zip(*outs):
        scale = max(1.0, r.abs().max().item())
        torch.testing.assert_close(a, r, rtol=0, atol=(2e-2 if amp else 1e-4) * scale)


@pytest.mark.parametrize("rows,C,dtype", [
    (65536, 512, torch.bfloat16), (8192, 1024, torch.bfloat16), (1000, 8, torch.bfloat16),
    (4099, 24, torch.float32), (3, 1032, torch.float32), (70000, 64, torch.float32), (0, 64, torch.bfloat16),
    (524288, 3, torch.bfloat16), (65536, 3, torch.float32), (1001, 3, torch.bfloat16), (4096, 6, torch.bfloat16)])
def test_colsum_matches_float64(dev, rows, C, dtype):
    """pcops_colsum (the blocks' bias gradient) vs a float64 column sum; fp32
    accumulation in a fixed order, so two calls agree bitwise."""
    from svdformer_pointsea_amd import attention

    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g).to(dtype)
    out = attention.colsum(x.to(dev))
    again = attention.colsum(x.to(dev))
    assert out.dtype == dtype and out.shape == (C,)
    assert torch.equal(out, again)
    ref = x.double().sum(0)
    atol = 1e-5 * max(1, rows) ** 0.5 + (2 ** -7 * ref.abs() if dtype == torch.bfloat16 else 0)
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= atol + 1e-4 * ref.abs()).all()), err.max()


@pytest.mark.parametrize("wdt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T,Cout,Cin", [(65536, 512, 512), (16384, 768, 256), (8192, 1024, 512),
                                        (32 * 2048 * 16, 32, 6), (1000, 64, 6),
                                        # small weights: up to 512 slices, summed by the sliced pcops_sum_rows
                                        (32 * 16384, 3, 64), (1 << 20, 64, 32), (32 * 16384, 128, 128)])
def test_split_k_wgrad_matches_float64(dev, wdt, T, Cout, Cin):
    """The blocks' split-K weight gradient (bmm partials + pcops_sum_rows: fixed-order sum,
    one rounding) -- and EdgeConv's 6-channel one (pcops_wgrad_skinny) -- vs float64 g^T x:
    within fp32 accumulation error (+ one bf16 rounding)."""
    from svdformer_pointsea_amd import attention

    g = torch.Generator(device=dev).manual_seed(T + Cout)
    g2 = torch.randn(T, Cout, device=dev, generator=g).to(torch.bfloat16)
    x2 = torch.randn(T, Cin, device=dev, generator=g).to(torch.bfloat16)
    out = attention._wgrad(g2, x2, wdt)
    assert out.dtype == wdt and out.shape == (Cout, Cin)
    assert torch.equal(out, attention._wgrad(g2, x2, wdt))      # deterministic
    ref = (g2.double().t() @ x2.double()).cpu()
    err = (out.double().cpu() - ref).abs()
    tol = 1e-5 * T ** 0.5 + (2 ** -8 * ref.abs() if wdt == torch.bfloat16 else 1e-5 * ref.abs())
    assert bool((err <= tol).all()), float(err.max())


@pytest.mark.parametrize("hd", [64, 128])
def test_core_bf16_growing_row_max(dev, hd):
    """Scores that grow along the keys at a per-row rate, so row maxima rise
    by 0.3..20 (log2 units) per 64-key tile: the forward's deferred-rescale
    branch (keep the running max while growth <= 2^8) and the rescale branch
    both fire, with mixed lanes in one wave.  bf16 inputs, float64 reference."""
    from svdformer_pointsea_amd.attention import attention_core

    B, H, Lq, Lk = 2, 2, 96, 640
    E = H * hd
    g = torch.Generator().manual_seed(hd)
    rate = torch.rand(Lq, B, H, 1, generator=g) * 1.2 + 0.02          # per (query, head) growth
    q = torch.randn(Lq, B, H, hd, generator=g) * 0.1
    q[..., 0] = rate[..., 0] * math.sqrt(hd)                           # score ~ rate * key_position
    k = torch.randn(Lk, B, H, hd, generator=g) * 0.1
    k[..., 0] = torch.arange(Lk, dtype=torch.float32).view(Lk, 1, 1) / 64.0 * 8.0
    v = torch.rand(Lk, B, H, hd, generator=g) * 2 - 1
    qb, kb, vb = [t.reshape(t.shape[0], B, E).to(dev, torch.bfloat16) for t in (q, k, v)]
    o = attention_core(qb, kb, vb, H)
    ref = _ref(qb.float(), kb.float(), vb.float(), H)
    err = (o.double() - ref).abs().max().item()
    assert err < 2e-2, err
    # the log-sum-exp the forward leaves for both backward passes, built from a
    # row max that the deferral may have kept stale: exact math says it must
    # still equal logsumexp(scale * q k^T) per (batch*head, query)
    lse = _forward_lse(qb, kb, vb, H)
    s = torch.einsum("qbhd,kbhd->bhqk", qb.float().double().reshape(Lq, B, H, hd),
                     kb.float().double().reshape(Lk, B, H, hd)) / math.sqrt(hd)
    ref_lse = torch.logsumexp(s, -1).reshape(B * H, Lq)
    assert (lse.double() - ref_lse).abs().max().item() < 1e-3
    # and the two backward passes that read it.  Nearly one-hot rows make
    # dS = P o (dP - delta) a difference of close numbers, so the reference
    # takes delta = rowsum(dO o O) from the kernel's own bf16 O (what the dQ
    # launch reads); everything else is float64 on the bf16 inputs
    gq = torch.randn(Lq, B, E, generator=torch.Generator().manual_seed(7)).to(dev)
    qs, ks, vs = [t.detach().clone().requires_grad_(True) for t in (qb, kb, vb)]
    (attention_core(qs, ks, vs, H).float() * gq).sum().backward()
    sc = 1.0 / math.sqrt(hd)
    qd, kd, vd, od, gd = [t.double().reshape(t.shape[0], B, H, hd).permute(1, 2, 0, 3)
                          for t in (qb.float(), kb.float(), vb.float(), o.float(), gq.to(torch.bfloat16).float())]
    P = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", qd, kd) * sc, -1)
    dP = torch.einsum("bhqd,bhkd->bhqk", gd, vd)
    dS = P * (dP - (gd * od).sum(-1, keepdim=True))
    ref = {"dq": torch.einsum("bhqk,bhkd->bhqd", dS, kd) * sc, "dk": torch.einsum("bhqk,bhqd->bhkd", dS, qd) * sc,
           "dv": torch.einsum("bhqk,bhqd->bhkd", P, gd)}
    # bf16 MFMA operands (P, dS rounded to bf16): each output element may err by
    # ~2^-8 of the sum of its terms' magnitudes -- large where those terms cancel
    # (dQ = sum_j dS_ij k_j with key coordinates up to 80 here)
    bound = {"dq": torch.einsum("bhqk,bhkd->bhqd", dS.abs(), kd.abs()) * sc,
             "dk": torch.einsum("bhqk,bhqd->bhkd", dS.abs(), qd.abs()) * sc,
             "dv": torch.einsum("bhqk,bhqd->bhkd", P, gd.abs())}
    for name, a in (("dq", qs.grad), ("dk", ks.grad), ("dv", vs.grad)):
        a = a.double().reshape(a.shape[0], B, H, hd).permute(1, 2, 0, 3)
        err = (a - ref[name]).abs()
        lim = 2.0 ** -7 * bound[name] + 1e-3 * ref[name].abs().max()
        assert bool((err <= lim).all()), (name, (err / lim).max().item())


@pytest.mark.parametrize("hd", [64, 128])
def test_core_fp32_growing_row_max(dev, hd):
    """The same growing-row-max scores through the exact fp32 path: output
    within 1e-5 and dQ/dK/dV within 1e-4 (relative to the largest gradient)
    of float64 autograd."""
    from svdformer_pointsea_amd.attention import attention_core

    B, H, Lq, Lk = 2, 2, 96, 640
    E = H * hd
    g = torch.Generator().manual_seed(hd + 1)
    rate = torch.rand(Lq, B, H, 1, generator=g) * 1.2 + 0.02
    q = torch.randn(Lq, B, H, hd, generator=g) * 0.1
    q[..., 0] = rate[..., 0] * math.sqrt(hd)
    k = torch.randn(Lk, B, H, hd, generator=g) * 0.1
    k[..., 0] = torch.arange(Lk, dtype=torch.float32).view(Lk, 1, 1) / 64.0 * 8.0
    v = torch.rand(Lk, B, H, hd, generator=g) * 2 - 1
    q, k, v = [t.reshape(t.shape[0], B, E).to(dev) for t in (q, k, v)]
    qs, ks, vs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = attention_core(qs, ks, vs, H)
    qd, kd, vd = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    ref = _ref(qd, kd, vd, H)
    # scores reach ~100 here: their fp32 rounding alone (~100 * 2^-24 in the
    # exponent) moves P by ~6e-6 relative, hence 3e-5 rather than 1e-5
    err = (o.double() - ref).abs().max().item()
    assert err < 3e-5, err
    gq = torch.randn(Lq, B, E, generator=torch.Generator().manual_seed(8)).to(dev)
    (o * gq).sum().backward()
    (ref * gq.double()).sum().backward()
    # scores reach ~100 (the adversarial case, not the SHAPES sweep): the fp32 rounding of the
    # scores alone moves P by ~6e-6 relative, so the gradients are held relative to their size
    for a, b in [(qs.grad, qd.grad), (ks.grad, kd.grad), (vs.grad, vd.grad)]:
        err = (a.double() - b).abs().max().item()
        assert err < 1e-4 * max(1.0, b.abs().max().item()), err


def _forward_lse(q, k, v, H):
    """Call pcops_attention_forward directly and return its (B*H, Lq) log-sum-exp."""
    from svdformer_pointsea_amd import _lib
    from svdformer_pointsea_amd._lib import lib, ptr, stream_of

    Lq, B, E = q.shape
    Lk, hd = k.shape[0], E // H
    o = torch.empty_like(q)
    lse = torch.empty(B * H, Lq, dtype=torch.float32, device=q.device)
    dt = 1 if q.dtype == torch.bfloat16 else 0
    st = (q.stride(1), hd, q.stride(0), k.stride(1), hd, k.stride(0), v.stride(1), hd, v.stride(0),
          o.stride(1), hd, o.stride(0))
    _lib.call("attention forward", lib().pcops_attention_forward, ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, H,
              Lq, Lk, hd, 1.0 / math.sqrt(hd), dt, *st, stream_of(q))
    torch.cuda.synchronize()
    return lse


def _large_case(name):
    import sys

    from conftest import GOLDEN

    sys.path.insert(0, GOLDEN)
    from make_golden_attn_large import CASES, inputs

    return CASES[name], inputs(CASES[name])


def _stage_block(blk, x, pos=None, x2=None, f32=()):
    """The reference's self/cross_attention forward (models/model_utils.py:542-617)
    in float64 except for the stages named in f32."""
    C = blk.norm13.weight.shape[0]
    mha = blk.multihead_attn

    def lin(t, w, b):
        if "linear" in f32:
            return F.linear(t.float(), w.float(), b.float()).double()
        return F.linear(t, w, b)

    def ln(t, norm):
        if "layernorm" in f32:
            from svdformer_pointsea_amd import attention as A

            y, _ = A.layer_norm(norm.float(), t.float().contiguous())
            norm.double()
            return y.double()
        return F.layer_norm(t, (C,), norm.weight, norm.bias, norm.eps)

    def inp(t):
        if hasattr(blk, "input_proj"):
            w, b = blk.input_proj.weight, blk.input_proj.bias
            if "conv" in f32:
                t = F.conv1d(t.float(), w.float(), b.float()).double()
            else:
                t = F.conv1d(t, w, b)
        return ln(t.permute(2, 0, 1), blk.norm13)

    s1 = inp(x)
    kv = s1 if x2 is None else inp(x2)
    q = s1 if pos is None else s1 + pos
    k = q if x2 is None else kv
    W, Bi = mha.in_proj_weight, mha.in_proj_bias
    qp, kp, vp = lin(q, W[:C], Bi[:C]), lin(k, W[C:2 * C], Bi[C:2 * C]), lin(kv, W[2 * C:], Bi[2 * C:])
    if "core" in f32:
        from svdformer_pointsea_amd import attention as A

        a = A.attention_core(qp.float().contiguous(), kp.float().contiguous(), vp.float().contiguous(),
                             mha.num_heads).double()
    else:
        L, B, _ = qp.shape
        H = mha.num_heads
        hd = C // H
        qq, kk, vv = (t.reshape(t.shape[0], B * H, hd).transpose(0, 1) for t in (qp, kp, vp))
        a = (torch.softmax(qq @ kk.transpose(1, 2) / hd ** 0.5, -1) @ vv).transpose(0, 1).reshape(L, B, C)
    a = lin(a, mha.out_proj.weight, mha.out_proj.bias)
    s1 = ln(s1 + a, blk.norm12)
    f = lin(F.gelu(lin(s1, blk.linear11.weight, blk.linear11.bias)), blk.linear12.weight, blk.linear12.bias)
    return (s1 + f).permute(1, 2, 0)



def _stage_run(name, dev, f32):
    """Block `name` of the large fixture in float64 with the stages in f32 on the GPU."""
    import sys

    from conftest import GOLDEN

    sys.path.insert(0, GOLDEN)
    from weights import fill_state

    from svdformer_pointsea_amd import attention as A

    c, args = _large_case(name)
    if c["kind"] == "self":
        m = A.self_attention(c["cin"], c["cout"], nhead=8)
    elif c["kind"] == "cross":
        m = A.cross_attention(c["cin"], c["cout"], nhead=8)
    else:
        m = A.SDG_Decoder(c["cin"], c["cout"], c["ratio"])
    m = fill_state(m, seed=c["wseed"]).eval().to(dev).double()
    xs = [a.to(dev).double() for a in args]
    if c["kind"] == "self":
        return _stage_block(m, xs[0], xs[1] if len(xs) > 1 else None, f32=f32)
    if c["kind"] == "cross":
        return _stage_block(m, xs[0], None, xs[1], f32=f32)
    return _stage_block(m.sa2, _stage_block(m.sa1, xs[0], f32=f32), f32=f32)


LARGE = ["sa2048", "ca2048x512", "dec2048", "sa512"]


@pytest.mark.parametrize("name", LARGE)
def test_blocks_large_golden(dev, name):
    """Blocks at the PCN step's real lengths (L = 2048 self, 2048 x 512 cross,
    hd 64 / 96 / 128) against the reference's own modules
    (tests/golden/make_golden_attn_large.py).

    The stages this build owns meet the north-star 1e-5 on their own: the
    block run in float64 with ONLY the libpcops attention core, or ONLY the
    libpcops LayerNorms, in fp32 stays within 1e-5 of the all-float64 block.
    The fp32 GEMMs are the rest: hipBLASLt's fp32 projections / FFN alone
    reach 0.8-1.6e-5 on these blocks (tools/block_err.py), the reference's own
    fp32 CPU output is 0.4-1.8e-5 from float64 (fixture `_ref_err`).  So the
    whole fp32 block is held to 2.5e-5 of float64 and, against the
    reference's fp32 output, to the sum of the two errors; the per-channel /
    per-token sums within 2.5e-5 per summed element."""
    g = golden("attention_large.npz")
    with torch.no_grad():
        exact = _stage_run(name, dev, ())
        for st in (("core",), ("layernorm",)):
            e = (_stage_run(name, dev, st) - exact).abs().max().item()
            assert e < 1e-5, (st, e)
        c, args = _large_case(name)
        m = _block_module(c, dev)
        y = m(*[a.to(dev) for a in args])
    y, t = y.cpu().double(), exact.cpu()
    err_ours = (y - t).abs().max().item()
    assert err_ours < 2.5e-5, err_ours
    ref = torch.from_numpy(g[f"{name}_cols"]).double()
    err_ref = float(g[f"{name}_ref_err"][0])
    err_pair = (y[..., :128] - ref).abs().max().item()
    assert err_pair <= err_ours + err_ref + 1e-7, (err_pair, err_ours, err_ref)
    L, C = y.shape[2], y.shape[1]
    np.testing.assert_allclose(y.sum(2).numpy(), g[f"{name}_csum"], rtol=0, atol=2.5e-5 * L)
    np.testing.assert_allclose(y.sum(1).numpy(), g[f"{name}_tsum"], rtol=0, atol=2.5e-5 * C)


def _block_module(c, dev):
    import sys

    from conftest import GOLDEN

    sys.path.insert(0, GOLDEN)
    from weights import fill_state

    from svdformer_pointsea_amd import attention as A

    if c["kind"] == "self":
        m = A.self_attention(c["cin"], c["cout"], nhead=8)
    elif c["kind"] == "cross":
        m = A.cross_attention(c["cin"], c["cout"], nhead=8)
    else:
        m = A.SDG_Decoder(c["cin"], c["cout"], c["ratio"])
    return fill_state(m, seed=c["wseed"]).eval().to(dev)


@pytest.mark.parametrize("amp", [False, True])
def test_layernorm_fused_bias_colsum(dev, monkeypatch, amp):
    """input_proj / out_proj bias gradients summed inside the LayerNorm backward
    (pcops_layernorm_bwd_colsum) and linear11's inside the GELU backward
    (pcops_gelu_bwd_colsum) equal the separate colsum path; the separate
    colsum runs for exactly those three layers fewer."""
    import copy

    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(0)
    blk = A.self_attention(64, 128, nhead=2).to(dev)
    x = torch.randn(4, 64, 2048, device=dev)            # 8192 tokens: the _Linear path
    calls = []
    real = A.colsum
    monkeypatch.setattr(A, "colsum", lambda g, **kw: calls.append(g.shape) or real(g, **kw))

    monkeypatch.setattr(A, "_GELU_SUM", True)

    def run(fused):
        monkeypatch.setattr(A, "_FUSED_BIAS_SUM", fused)
        m = copy.deepcopy(blk)
        calls.clear()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = m(x)
        (y.float() ** 2).mean().backward()
        return {n: p.grad.float().clone() for n, p in m.named_parameters()}, len(calls)

    g_ref, n_ref = run(False)
    g_fus, n_fus = run(True)
    assert n_ref - n_fus == 3, (n_ref, n_fus)
    for n in g_ref:
        # fused sums are fp32 over the stored (bf16 under autocast) dx; the
        # separate colsum rounds its result to the gradient's dtype
        tol = dict(rtol=1e-2, atol=1e-5) if amp else dict(rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(g_fus[n], g_ref[n], **tol, msg=n)


@pytest.mark.parametrize("mode", ["kv", "qk", "all"])
def test_in_proj_row_split_bitwise(dev, monkeypatch, mode):
    """The packed in_proj weight / bias taken in row blocks through _RowSplit (one concatenation
    assembles their gradients) against plain slices (SliceBackward + accumulation), bf16 autocast as
    in the step: output and every gradient bitwise equal."""
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(7)
    E, H, L, S, B = 256, 4, 96, 130, 3
    mha = A.MultiheadAttention(E, H, batch_first=True).to(dev)
    with torch.no_grad():
        mha.in_proj_bias.normal_()
    q = torch.randn(B, L, E, device=dev)
    k = torch.randn(B, S, E, device=dev)
    v = torch.randn(B, S if mode != "qk" else L, E, device=dev)
    g = torch.randn(B, L, E, device=dev)
    res = {}
    for split in (False, True):
        monkeypatch.setattr(A, "_ROW_SPLIT", split)
        mha.zero_grad(set_to_none=True)
        xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
        qq, kk, vv = xs
        args = {"kv": (qq, kk, kk), "qk": (qq, qq, vv), "all": (qq, kk, vv)}[mode]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            o, _ = mha(*args)
        o.float().backward(g)
        res[split] = [o.detach(), mha.in_proj_weight.grad, mha.in_proj_bias.grad] + [x.grad for x in xs if x.grad is not None]
    for u, w in zip(res[False], res[True]):
        assert torch.equal(u, w), (u.float() - w.float()).abs().max().item()


def test_fused_bias_sum_in_bias_dtype_bitwise(dev, monkeypatch):
    """With bf16 biases (bench.py's FlatParams shadows) the fused bias sums of the LayerNorm and GELU
    backwards are stored in bf16 by the summing launch itself (round 5), so the Linear backward takes
    them without a cast launch: every gradient bitwise equal to the fp32-sum-then-cast path."""
    import copy

    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(1)
    blk = A.self_attention(64, 128, nhead=2).to(dev)
    for n, p in blk.named_parameters():
        if n.endswith("bias") and "norm" not in n and "in_proj" not in n:
            p.data = p.data.to(torch.bfloat16)
    x = torch.randn(4, 64, 2048, device=dev)            # 8192 tokens: the _Linear path
    monkeypatch.setattr(A, "_GELU_SUM", True)
    monkeypatch.setattr(A, "_FUSED_BIAS_SUM", True)

    def run(flag):
        monkeypatch.setattr(A, "_SUM_IN_BIAS_DTYPE", flag)
        m = copy.deepcopy(blk)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        (y.float() ** 2).mean().backward()
        return {n: p.grad.clone() for n, p in m.named_parameters()}

    a, b = run(False), run(True)
    assert any(g.dtype == torch.bfloat16 for g in b.values())
    for n in a:
        assert a[n].dtype == b[n].dtype and torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("S", [16, 32, 64, 128, 256, 512])
@pytest.mark.parametrize("N", [192, 2048, 8192, 16384, 32768, 65536, 131072, 1 << 20])
def test_sum_rows_matches_float64(dev, S, N):
    """pcops_sum_rows (the split-K partial sum: plain form for S < 32, sliced form above):
    every (slices, columns) combination the weight gradients produce, fp32 and bf16 out."""
    from svdformer_pointsea_amd._lib import call, lib, ptr, stream_of

    part = torch.randn(S, N, device=dev, generator=torch.Generator(device=dev).manual_seed(S * 7 + N))
    ref = part.double().sum(0)
    for odt, dt in ((0, torch.float32), (1, torch.bfloat16)):
        out = torch.empty(N, dtype=dt, device=dev)
        call("sum_rows", lib().pcops_sum_rows, ptr(part), S, N, ptr(out), odt, stream_of(part))
        torch.cuda.synchronize()
        tol = 1e-5 * S ** 0.5 + (2 ** -8 * ref.abs() if odt else 0)
        assert bool(((out.double() - ref).abs() <= tol).all()), (odt, float((out.double() - ref).abs().max()))


@pytest.mark.parametrize("S,N", [(64, 16384), (128, 8192), (512, 192), (32, 32768)])
def test_sum_rows_graph_replay(dev, S, N):
    """The split-K partial sum captured in a HIP graph with the bmm that produces its input
    (as the bench step does): every replay equals the eager result bitwise."""
    from svdformer_pointsea_amd._lib import call, lib, ptr, stream_of

    T = S * 1024
    Cin = 64
    Cout = N // Cin
    gen = torch.Generator(device=dev).manual_seed(S + N)
    g2 = torch.randn(T, Cout, device=dev, generator=gen).to(torch.bfloat16)
    x2 = torch.randn(T, Cin, device=dev, generator=gen).to(torch.bfloat16)

    def run(out):
        part = torch.bmm(g2.view(S, T // S, Cout).transpose(1, 2), x2.view(S, T // S, Cin), out_dtype=torch.float32)
        call("sum_rows", lib().pcops_sum_rows, ptr(part), S, N, ptr(out), 1, stream_of(part))

    eager = torch.empty(N, dtype=torch.bfloat16, device=dev)
    run(eager)
    out = torch.empty_like(eager)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(out)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    for _ in range(5):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("n", [8, 1000, 1003, 1 << 20])
def test_add_kernel_bitwise(dev, n):
    """pcops_add: the sum in the promoted dtype (fp32 unless both operands are
    bf16), stored as the output dtype -- bitwise, every dtype combination,
    including a non-multiple-of-8 tail.  torch.add(out=bf16) agrees for the
    combination the blocks use (fp32 residual + bf16 FFN output); for a bf16
    FIRST operand with an fp32 second it rounds the fp32 operand to bf16 before
    adding (measured), which is not the promoted-dtype sum."""
    from svdformer_pointsea_amd._lib import call, lib, ptr, stream_of
    from svdformer_pointsea_amd.attention import _DT

    g = torch.Generator().manual_seed(n)
    for adt in (torch.float32, torch.bfloat16):
        for bdt in (torch.float32, torch.bfloat16):
            for odt in (torch.float32, torch.bfloat16):
                a = (torch.randn(n, generator=g) * 3).to(adt).to(dev)
                b = (torch.randn(n, generator=g) * 3).to(bdt).to(dev)
                out = torch.empty(n, dtype=odt, device=dev)
                call("add", lib().pcops_add, ptr(a), _DT[adt], ptr(b), _DT[bdt], ptr(out), _DT[odt], n,
                     stream_of(a))
                both16 = adt == bdt == torch.bfloat16
                ref = (a.float() + b.float()).to(torch.bfloat16 if both16 else torch.float32).to(odt)
                assert torch.equal(out, ref), (adt, bdt, odt)
                if (adt, bdt, odt) == (torch.float32, torch.bfloat16, torch.bfloat16):
                    tref = torch.empty(n, dtype=odt, device=dev)
                    torch.add(a, b, out=tref)
                    assert torch.equal(out, tref)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,C", [(999, 1024), (8192, 3072), (300, 40)])
def test_gelu_backward_kernel(dev, dt, rows, C):
    """pcops_gelu_bwd_colsum vs torch's exact-GELU backward and g.sum(0)."""
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(rows)
    u = (torch.randn(rows, C, device=dev) * 2).to(dt).requires_grad_(True)
    g = torch.randn(rows, C, device=dev).to(dt)
    h = A._Gelu.apply(u, True)
    assert torch.equal(h, torch.nn.functional.gelu(u.detach()))
    (du,) = torch.autograd.grad(h, u, g)
    ur = u.detach().clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(torch.nn.functional.gelu(ur), ur, g)
    tol = dict(rtol=1e-5, atol=1e-6) if dt == torch.float32 else dict(rtol=1e-2, atol=1e-3)
    torch.testing.assert_close(du.float(), ref.float(), **tol)
    dsum = A._take_sum(du)
    assert A._take_sum(du) is None   # handed over exactly once
    torch.testing.assert_close(dsum, du.float().sum(0), rtol=1e-4, atol=1e-3)



@pytest.mark.parametrize("B,H,Lq,Lk,E,packed,bf", [
    (2, 8, 2048, 2048, 512, True, False),    # refine2 self-attention (hd 64), one (L, B, 3E) source
    (2, 8, 2048, 2048, 1024, True, True),    # hd 128, batch-first
    (1, 8, 333, 250, 1024, False, False),    # ragged cross, hd 128 (the pipelined dK/dV pass)
    (1, 8, 512, 512, 768, True, True),       # hd 96
    (2, 2, 70, 130, 64, False, True),        # hd 32, ragged
    (3, 4, 49, 49, 512, True, False),        # short rows: one partial block per (batch, head)
    (2, 4, 130, 129, 128, False, False)])
def test_attention_bwd_colsum(dev, B, H, Lq, Lk, E, packed, bf):
    """pcops_attention_bwd_*_colsum: the gradients are bitwise those of the plain
    passes, and the column sums they hand to the in_proj bias gradient equal the
    float64 column sums of the stored bf16 gradients (fp32 accumulation bound)."""
    from svdformer_pointsea_amd.attention import AttentionCore, _take_sum

    got = {}

    class Grab(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, i):
            ctx.i = i
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            got[ctx.i] = (g.clone(), _take_sum(g))
            return g, None

    gen = torch.Generator().manual_seed(11)
    shp = (lambda L, W: (B, L, W)) if bf else (lambda L, W: (L, B, W))
    if packed:
        assert Lq == Lk
        srcs = [torch.randn(*shp(Lq, 3 * E), generator=gen)]
        wins = ((0, 0), (0, E), (0, 2 * E))
    else:
        srcs = [torch.randn(*shp(Lq, E), generator=gen), torch.randn(*shp(Lk, 2 * E), generator=gen)]
        wins = ((0, 0), (1, 0), (1, E))
    srcs = [s.to(dev, torch.bfloat16).requires_grad_(True) for s in srcs]
    g = torch.randn(*shp(Lq, E), generator=gen).to(dev, torch.bfloat16)
    scale = 1.0 / math.sqrt(E // H)
    res = []
    for want in (None, (True,) * len(srcs)):
        got.clear()
        meta = (H, scale, E, bf, *wins) + ((want,) if want else ())
        o = AttentionCore.apply(meta, *[Grab.apply(s, i) for i, s in enumerate(srcs)])
        o.backward(g)
        res.append([got[i] for i in range(len(srcs))])
    for (g0, s0), (g1, s1) in zip(*res):
        assert s0 is None and s1 is not None and s1.dtype == torch.float32
        assert torch.equal(g0, g1)
        ref = g1.double().reshape(-1, g1.shape[-1]).sum(0)
        bound = 2e-6 * g1.double().abs().reshape(-1, g1.shape[-1]).sum(0) + 1e-6
        assert ((s1.double() - ref).abs() <= bound).all(), (s1.double() - ref).abs().max().item()


@pytest.mark.parametrize("rows,C,ld,dtype", [(65536, 1024, 2048, torch.bfloat16), (16384, 128, 256, torch.bfloat16),
                                             (999, 64, 72, torch.float32), (4096, 512, 1024, torch.float32)])
def test_colsum_row_strided(dev, rows, C, ld, dtype):
    """pcops_colsum_ld on a channel slice of a wider matrix: bitwise the contiguous colsum of the same
    values, and within the fp32 accumulation bound of float64."""
    from svdformer_pointsea_amd.attention import colsum

    wide = torch.randn(rows, ld, generator=torch.Generator().manual_seed(rows + C)).to(dev, dtype)
    g = wide[:, ld - C:]
    assert not g.is_contiguous()
    out = colsum(g, out_dtype=torch.float32)
    ref = colsum(g.contiguous(), out_dtype=torch.float32)
    assert torch.equal(out, ref)
    exact = g.double().sum(0)
    assert ((out.double() - exact).abs() <= 2e-6 * g.double().abs().sum(0) + 1e-6).all()


@pytest.mark.parametrize("amp", [False, True])
def test_linear_sliced_output_gradient(dev, monkeypatch, amp):
    """A Linear whose output is concatenated with another tensor gets a row-strided gradient
    view: the in-place path (GEMMs with a leading dimension, pcops_colsum_ld) matches the
    contiguous-copy path."""
    from svdformer_pointsea_amd import attention as A

    torch.manual_seed(3)
    x = torch.randn(8, 2048, 256, device=dev)
    w = torch.randn(512, 256, device=dev) * 0.05
    b = torch.randn(512, device=dev) * 0.1
    other = torch.randn(8, 2048, 384, device=dev)

    def run(strided):
        monkeypatch.setattr(A, "_STRIDED_G", strided)
        xs, ws, bs = [t.clone().requires_grad_(True) for t in (x, w, b)]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = A._Linear.apply(xs, ws, bs, bs.dtype)
            out = torch.cat([other.to(y.dtype), y], -1)
        (out.float() ** 2).sum().backward()
        return xs.grad, ws.grad, bs.grad

    ref, got = run(False), run(True)
    for a, r in zip(got, ref):
        torch.testing.assert_close(a, r, rtol=1e-2 if amp else 1e-5, atol=1e-3 if amp else 1e-5)


@pytest.mark.parametrize("B,H,Lq,Lk,E,packed,bf", [
    (2, 8, 2048, 2048, 1024, True, True),    # refine2 decoder sa2 (hd 128), packed batch-first
    (1, 8, 333, 250, 1024, False, False),    # ragged cross, hd 128: partial key block, partial query tiles
    (1, 8, 512, 512, 768, True, False),      # refine1 (hd 96)
    (3, 4, 49, 49, 512, True, True),         # PointSea view tokens: one partial tile each way
    (2, 8, 1024, 1024, 768, False, True),    # PointSea refine1 (hd 96 at L = 1024)
    (1, 2, 700, 1300, 256, False, False)])   # Lk > Lq, hd 128, ragged both ways
def test_attention_bwd_fused_equals_two_pass(dev, monkeypatch, B, H, Lq, Lk, E, packed, bf):
    """pcops_attention_bwd_fused (bf16, D >= 96: the dK/dV pass stores dS^T, dQ = dS K read
    back, no S / dP recompute) against the two-pass form (dQ pass recomputing S and dP, then
    dK/dV): dQ, dK and dV bitwise equal -- the same bf16 dS, the same MFMA order per
    accumulator -- and the in_proj bias column sums equal too."""
    from svdformer_pointsea_amd import attention as A

    gen = torch.Generator().manual_seed(21)
    shp = (lambda L, W: (B, L, W)) if bf else (lambda L, W: (L, B, W))
    if packed:
        assert Lq == Lk
        base = [torch.randn(*shp(Lq, 3 * E), generator=gen)]
        wins = ((0, 0), (0, E), (0, 2 * E))
    else:
        base = [torch.randn(*shp(Lq, E), generator=gen), torch.randn(*shp(Lk, 2 * E), generator=gen)]
        wins = ((0, 0), (1, 0), (1, E))
    base = [s.to(dev, torch.bfloat16) for s in base]
    g = torch.randn(*shp(Lq, E), generator=gen).to(dev, torch.bfloat16)
    scale = 1.0 / math.sqrt(E // H)
    got = {}

    class Grab(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, i):
            ctx.i = i
            return x.clone()

        @staticmethod
        def backward(ctx, gr):
            got[ctx.i] = (gr.clone(), A._take_sum(gr))
            return gr, None

    res = {}
    for fused in (True, False):
        monkeypatch.setattr(A, "_ATTN_FUSED", fused)
        for want in (None, (True,) * len(base)):
            got.clear()
            srcs = [s.clone().requires_grad_(True) for s in base]
            meta = (H, scale, E, bf, *wins) + ((want,) if want else ())
            o = A.AttentionCore.apply(meta, *[Grab.apply(s, i) for i, s in enumerate(srcs)])
            o.backward(g)
            res[(fused, want is not None)] = [got[i] for i in range(len(base))]
    for sums in (False, True):
        for (ga, sa), (gb, sb) in zip(res[(True, sums)], res[(False, sums)]):
            assert torch.isfinite(ga.float()).all()
            assert torch.equal(ga, gb), (ga.float() - gb.float()).abs().max().item()
            if sums:   # the dQ partial sums group 256 queries per block here, 128 in the D = 96 dQ pass
                bound = 2e-6 * ga.double().abs().reshape(-1, ga.shape[-1]).sum(0) + 1e-6
                assert ((sa.double() - sb.double()).abs() <= bound).all(), (sa - sb).abs().max().item()


def _one_head_backward(q, k, v, g, dq):
    """pcops_attention_forward then pcops_attention_backward on one (L, D) head (B = H = 1), called
    directly.  q and dq are (Lq, D) windows that share their row stride; k, v, g are contiguous."""
    from svdformer_pointsea_amd import _lib
    from svdformer_pointsea_amd._lib import lib, ptr, stream_of

    (Lq, D), Lk = q.shape, k.shape[0]
    assert q.stride() == dq.stride() and q.stride(1) == 1
    o, dk, dv = torch.empty_like(g), torch.empty_like(k), torch.empty_like(v)
    lse = torch.empty(1, Lq, dtype=torch.float32, device=q.device)
    st = (D, D, q.stride(0), D, D, k.stride(0), D, D, v.stride(0), D, D, o.stride(0))
    scale = 1.0 / math.sqrt(D)
    _lib.call("attention forward", lib().pcops_attention_forward, ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), 1, 1,
              Lq, Lk, D, scale, 1, *st, stream_of(q))
    wsb = lib().pcops_attention_bwd_workspace_bytes(1, 1, Lq, Lk, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    _lib.call("attention bwd", lib().pcops_attention_backward, ptr(q), ptr(k), ptr(v), ptr(o), ptr(g), ptr(lse),
              ptr(dq), ptr(dk), ptr(dv), 1, 1, Lq, Lk, D, scale, 1, *st, ptr(ws), wsb, stream_of(q))
    torch.cuda.synchronize()
    return dq, dk, dv


@pytest.mark.parametrize("D", [96, 128])
def test_attention_dkv_large_row_stride(dev, D):
    """bf16 dK/dV at D >= 96 with a q / dq row stride of 2^25 elements: 64 rows span 2^31, beyond the
    pipelined pass's 32-bit tile offsets, so the launcher falls back to the 8-wave split passes
    (attn_dkv2_kernel MODE 1 + MODE 2), their only use.  The same values in contiguous tensors take
    the pipelined pass; both orders of accumulation are the same, so dq, dk and dv are bitwise equal.
    Lq = 70: one full and one partial 64-row query tile; Lk = 300: partial in the 128-key blocks of
    the pipelined pass and in the 256-key blocks of the split ones."""
    Lq, Lk, row = 70, 300, 1 << 25
    gen = torch.Generator().manual_seed(300 + D)
    q, k, v, g = [torch.randn(L, D, generator=gen).to(dev, torch.bfloat16) for L in (Lq, Lk, Lk, Lq)]
    ref = _one_head_backward(q, k, v, g, torch.empty_like(q))
    buf = torch.empty(Lq, row, dtype=torch.bfloat16, device=dev)  # 4.7 GB, uninitialised but for the windows
    qs, dqs = buf[:, 0:D], buf[:, D:2 * D]
    qs.copy_(q)
    dqs.zero_()
    got = _one_head_backward(qs, k, v, g, dqs)
    for name, a, b in zip(("dq", "dk", "dv"), got, ref):
        assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all(), name
        diff = (a.float() - b.float()).abs().max().item()
        print(f"D={D} {name}: max |strided - contiguous| = {diff:.3e}, max |ref| = {b.float().abs().max().item():.3e}")
        assert torch.equal(a, b), (name, diff)


@pytest.mark.parametrize("B,N,H,sdt", [(2, 2048, 512, torch.float32), (3, 512, 768, torch.float32),
                                       (2, 1024, 256, torch.bfloat16), (1, 100, 64, torch.float32)])
def test_add_posemb_kernel(dev, B, N, H, sdt):
    """pcops_add_posemb (block_sum of an SDG query and its PosEmbedding under bf16 autocast)
    against the torch expression it replaces -- SinusoidalPositionalEmbedding, the raw
    .reshape(B, hidden, N).transpose, the fp32 add, one bf16 rounding: equal up to one bf16
    ulp where sinf / cosf differ in the last fp32 bit; gradient = the cast upstream gradient."""
    from svdformer_pointsea_amd.attention import PosEmbedding, block_sum
    from svdformer_pointsea_amd.svdformer import SinusoidalPositionalEmbedding

    gen = torch.Generator().manual_seed(B * N + H)
    emb = SinusoidalPositionalEmbedding(H).to(dev)
    cd = (torch.rand(B, N, generator=gen) * 40).to(dev)     # half_cd / sigma: O(10)
    s = torch.randn(B, N, H, generator=gen).to(dev, sdt).requires_grad_(True)
    pos = PosEmbedding(cd, emb, H)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = block_sum(s, pos)
    ref = (s.detach().float() + pos.tensor()).to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == (B, N, H)
    diff = (got.float() - ref.float()).abs()
    ulp = ref.float().abs().clamp_min(1e-30) * 2.0 ** -7
    assert (diff <= ulp).all(), diff.max().item()
    assert (got == ref).float().mean().item() > 0.999
    g = torch.randn(B, N, H, generator=gen).to(dev, torch.bfloat16)
    got.backward(g)
    assert s.grad.dtype == sdt and torch.equal(s.grad, g.to(sdt))


@pytest.mark.parametrize("L,C,Cout", [(512, 256, 256), (2048, 512, 512), (300, 128, 256)])
def test_block_sum_g16_handoff_bitwise(dev, monkeypatch, L, C, Cout):
    """The bf16 gradient of the block tail's LayerNorm output handed to its backward uncast
    (_AddToBf16 -> pcops_layernorm_bwd_bf16g) against the widening cast + pcops_layernorm_bwd:
    input and parameter gradients bitwise equal (fp32(a) + fp32(b) in the kernel is the same
    value as the pre-widened sum).  Second part: if the LayerNorm output also had another
    consumer, the hand-off must poison the gradient (NaN), never drop a term."""
    import svdformer_pointsea_amd.attention as A

    torch.manual_seed(L + C)
    blk = A.self_attention(C, Cout, nhead=8).to(dev)
    x0 = torch.randn(2, L, C, device=dev)
    g = torch.randn(2, L, Cout, device=dev).to(torch.bfloat16)

    def run(handoff):
        monkeypatch.setattr(A, "_LN_G16", handoff)
        blk.zero_grad()
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            s, f = blk.forward_tokens(x)
            y = A.block_sum(s, f, True)
        y.backward(g)
        return [x.grad.clone()] + [p.grad.clone() for p in blk.parameters()]

    got, ref = run(True), run(False)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    monkeypatch.setattr(A, "_LN_G16", True)
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        s, f = blk.forward_tokens(x)
        y = A.block_sum(s, f, True)        # claims single use ...
        z = (s * 2).sum()                  # ... but s has a second reader
    (y.float() * g.float()).sum().add(z).backward()
    assert torch.isnan(x.grad).any()


@pytest.mark.parametrize("shape,sdt", [((16, 2048, 512), torch.bfloat16), ((2, 300, 64), torch.bfloat16),
                                       ((3, 128, 256), torch.float32)])
def test_blend_bitwise(dev, monkeypatch, shape, sdt):
    """PointSea's path selection score * a + (1 - score) * b (pcops_blend_fwd / _bwd) against torch's
    four-op expression: output and the three gradients bitwise (bf16 score: 1 - s rounded to bf16,
    the score gradient as autograd's two bf16-cast contributions summed in bf16)."""
    import svdformer_pointsea_amd.attention as A

    torch.manual_seed(shape[-1])
    s0 = torch.sigmoid(torch.randn(shape, device=dev)).to(sdt)
    a0, b0 = torch.randn(shape, device=dev) * 3, torch.randn(shape, device=dev)
    g = torch.randn(shape, device=dev)

    def run(fused):
        monkeypatch.setattr(A, "_PCOPS_BLEND", fused)
        s, a, b = (t.clone().requires_grad_(True) for t in (s0, a0, b0))
        out = A.blend(s, a, b)
        out.backward(g)
        return out.detach(), s.grad, a.grad, b.grad

    for x, y in zip(run(True), run(False)):
        assert x.dtype == y.dtype and torch.equal(x, y)


def test_pointsea_decoder_pair_input_bitwise(dev, monkeypatch):
    """SDG_Decoder_PointSea fed the (s, f) pair (LayerNorm of s + f in one launch, linear12's bias
    gradient from the LayerNorm backward) against the materialised s + f: outputs, input and parameter
    gradients bitwise."""
    import svdformer_pointsea_amd.attention as A

    torch.manual_seed(3)
    dec = A.SDG_Decoder_PointSea(512, 64, 2).to(dev)
    s0 = torch.randn(2, 1024, 512, device=dev)
    f0 = torch.randn(2, 1024, 512, device=dev).to(torch.bfloat16)
    g = torch.randn(2, 1024, 512, device=dev)

    def run(pair):
        dec.zero_grad()
        s, f = s0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = dec.forward_tokens((s, f) if pair else s + f)
        y.float().backward(g)
        return [y.detach(), s.grad, f.grad] + [p.grad.clone() for p in dec.parameters()]

    for x, y in zip(run(True), run(False)):
        assert torch.equal(x, y)


def test_blend_gemm_operand_bitwise(dev, monkeypatch):
    """blend(..., gemm_only=True) under bf16 autocast emits the bf16 GEMM operand directly and takes
    the GEMM's bf16 input gradient: same output and gradients as the fp32 blend followed by the cast."""
    import svdformer_pointsea_amd.attention as A

    torch.manual_seed(11)
    shape = (4, 512, 256)
    s0 = torch.sigmoid(torch.randn(shape, device=dev)).to(torch.bfloat16)
    a0, b0 = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    g = torch.randn(shape, device=dev).to(torch.bfloat16)

    def run(direct):
        s, a, b = (t.clone().requires_grad_(True) for t in (s0, a0, b0))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = A.blend(s, a, b, gemm_only=True) if direct else A.blend(s, a, b).to(torch.bfloat16)
        out.backward(g)
        return out.detach(), s.grad, a.grad, b.grad

    got, ref = run(True), run(False)
    assert got[0].dtype == torch.bfloat16
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
