"""The fused point-MLP max (csrc/pointmlp.hip) and the ShapeNet-55 adversarial step on the GPU.

Values are held to a MEASURED bar: e_ref = max |torch fp32 chain - float64| of the
(B, H) maxima on the same inputs, and the kernel's e_k = max |kernel - float64| must
stay within 4 e_ref (the two are different, equally valid fp32 summation orders; the
factor is test_gpu_capture_fork.py's for eager spread).  Gradients likewise, per tensor.
Every test prints its figures before asserting.

Measured on an MI355X (the figures the tests print; profiles/adv55_point_mlp_ab.txt has the run):
  values, worst over B in {1, 3} x the eight N of test_kernel_matches_float64
    H = 64:   e_ref 8.64e-07, e_k 1.18e-06, worst e_k / e_ref of a case 1.64
    H = 128:  e_ref 1.26e-06, e_k 1.54e-06, worst e_k / e_ref of a case 1.68
  b3 = -100 (all f negative): H = 64 e_ref 3.83e-06, e_k 3.90e-06; H = 128 4.40e-06, 4.57e-06
    (with the bias as the accumulator's start instead of its last term e_k was 4.0e-05 and 7.3e-05:
    the kernel adds its biases last since)
  gradients (B = 2, N = T + 9), worst e_k / e_ref over dx and the six parameter gradients:
    H = 64: 1.60 (dx: e_ref 2.84e-07, e_k 4.53e-07);  H = 128: 1.81 (dw2: e_ref 6.69e-07, e_k 1.21e-06)
    the chain's own gradient error moves between runs (dw2, H = 64: 4.55e-07, 7.19e-07, 4.80e-07)
  memory around one forward + backward at (2, 4096, 128): peak + 762 368 B; one (B, H, N) tensor is 4 194 304 B
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T = 256   # PCOPS_POINT_MLP_TILE
FACTOR = 4.0


def _adv():
    from svdformer_pointsea_amd import adversarial
    return adversarial


def weights(H, seed, dev, scale=None, positive=False):
    """(w1, b1, w2, b2, w3, b3) seeded; `positive`: |.| weights and zero biases, so that for clouds
    (s, 0, 0) with s >= 0 every channel of f grows with s."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    k = scale if scale is not None else 1.0
    ws = [k * r(H, 3), 0.3 * r(H), k * r(H, H) / H ** 0.5, 0.3 * r(H), k * r(H, H) / H ** 0.5, 0.3 * r(H)]
    if positive:
        ws = [w.abs() if i % 2 == 0 else torch.zeros_like(w) for i, w in enumerate(ws)]
    return [w.to(dev).contiguous() for w in ws]


def cloud(B, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, N, 3, generator=g)).to(dev)


def features64(x, ws, slope=0.2):
    """f (B, N, H) in float64 on the device."""
    w1, b1, w2, b2, w3, b3 = (w.double() for w in ws)
    h = F.leaky_relu(F.linear(x.double(), w1, b1), slope)
    h = F.leaky_relu(F.linear(h, w2, b2), slope)
    return F.linear(h, w3, b3)


def raw(x, ws, slope=0.2):
    """A raw call with out, arg and the workspace poisoned (NaN, -1, 0xFF) -> (out, arg)."""
    from svdformer_pointsea_amd._lib import lib, ptr, stream_of

    B, N, _ = x.shape
    H = ws[0].shape[0]
    out = torch.full((B, H), float("nan"), device=x.device)
    arg = torch.full((B, H), -1, dtype=torch.int32, device=x.device)
    wsb = lib().pcops_point_mlp_max_workspace_bytes(B, N, H)
    assert wsb > 0
    wk = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=x.device)
    st = lib().pcops_point_mlp_max_forward(ptr(x), *(ptr(w) for w in ws), slope, B, N, H, ptr(out), ptr(arg), ptr(wk),
                                           wsb, stream_of(x))
    assert st == 0, st
    return out, arg


def value_errors(x, ws):
    """(e_ref, e_k, out, arg, f64): the chain's and the kernel's worst deviation from the float64 maxima."""
    f = features64(x, ws)
    top = f.max(1)[0]
    chain = _adv().point_mlp_max_chain(x, *ws)
    out, arg = raw(x, ws)
    return float((chain.double() - top).abs().max()), float((out.double() - top).abs().max()), out, arg, f


@pytest.mark.parametrize("N", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_matches_float64(dev, B, H, N):
    assert _adv().POINT_MLP_TILE == T
    x, ws = cloud(B, N, 100 + N, dev), weights(H, 7 + H, dev)
    e_ref, e_k, out, arg, f = value_errors(x, ws)
    print(f"\n[point_mlp_max B={B} H={H} N={N}] e_ref {e_ref:.3g} e_k {e_k:.3g}")
    assert not torch.isnan(out).any() and int(arg.min()) >= 0 and int(arg.max()) < N   # every element overwritten
    assert e_ref > 0 or e_k == 0
    assert e_k <= FACTOR * e_ref, (e_k, e_ref)
    at = f.gather(1, arg.long().unsqueeze(1)).squeeze(1)          # float64 value at the kernel's index
    assert float((f.max(1)[0] - at).max()) <= FACTOR * e_ref


@pytest.mark.parametrize("where", ["first", "last", "last_tile"])
@pytest.mark.parametrize("H", [64, 128])
def test_winner_placement(dev, H, where):
    """Monotone weights: the point with the largest s wins every channel."""
    N = 2 * T + 3
    ws = weights(H, 11, dev, positive=True)
    g = torch.Generator().manual_seed(5)
    s = torch.rand(2, N, generator=g) * 0.5
    n_win = {"first": 0, "last": N - 1, "last_tile": 2 * T + 1}[where]
    s[:, n_win] = 1.0
    x = torch.zeros(2, N, 3)
    x[:, :, 0] = s
    x = x.to(dev)
    out, arg = raw(x, ws)
    assert torch.equal(arg, torch.full_like(arg, n_win))
    single, _ = raw(x[:, n_win:n_win + 1].contiguous(), ws)
    assert torch.equal(out, single)


@pytest.mark.parametrize("H", [64, 128])
def test_all_negative_features(dev, H):
    ws = weights(H, 13, dev)
    ws[5] = torch.full_like(ws[5], -100.0)
    x = cloud(2, T + 7, 14, dev)
    e_ref, e_k, out, arg, f = value_errors(x, ws)
    print(f"\n[point_mlp_max negative H={H}] e_ref {e_ref:.3g} e_k {e_k:.3g} max out {float(out.max()):.4g}")
    assert float(f.max()) < 0 and float(out.max()) < 0
    assert e_k <= FACTOR * e_ref


@pytest.mark.parametrize("H", [64, 128])
def test_ties_name_the_lower_index(dev, H):
    """[p, q, p, ...]: the duplicates of the winning point sit in different tiles."""
    N = 2 * T + 3
    ws = weights(H, 17, dev, positive=True)
    g = torch.Generator().manual_seed(6)
    s = torch.rand(1, N, generator=g) * 0.5
    i0, i1, i2 = 5, T + 9, 2 * T + 2
    s[:, [i0, i1, i2]] = 1.0
    x = torch.zeros(1, N, 3)
    x[:, :, 0] = s
    x = x.to(dev)
    out, arg = raw(x, ws)
    assert torch.equal(arg, torch.full_like(arg, i0))
    single, _ = raw(x[:, i1:i1 + 1].contiguous(), ws)
    assert torch.equal(out, single)


@pytest.mark.parametrize("H", [64, 128])
def test_nan_wins_like_torch_max(dev, H):
    B, N, k = 3, T + 5, T + 2
    ws = weights(H, 19, dev)
    x = cloud(B, N, 20, dev)
    clean_out, clean_arg = raw(x, ws)
    x[1, k, 1] = float("nan")
    x[1, k + 2, 0] = float("nan")          # a later NaN: the first one's index is reported
    out, arg = raw(x, ws)
    assert torch.isnan(out[1]).all() and torch.equal(arg[1], torch.full_like(arg[1], k))
    for b in (0, 2):
        assert torch.equal(out[b], clean_out[b]) and torch.equal(arg[b], clean_arg[b])
    ref, ref_arg = torch.max(features64(x, ws).float(), dim=1)
    assert torch.isnan(ref[1]).all() and torch.equal(ref_arg[1], arg[1].long())


@pytest.mark.parametrize("H", [64, 128])
def test_position_independence(dev, H):
    N = 2 * T + 3
    ws = weights(H, 23, dev)
    x = cloud(2, N, 24, dev)
    out, arg = raw(x, ws)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(25)).to(dev)
    out_p, arg_p = raw(x[:, perm].contiguous(), ws)
    assert torch.equal(out, out_p)
    assert torch.equal(x[:, perm].gather(1, arg_p.long().unsqueeze(-1).expand(-1, -1, 3)),
                       x.gather(1, arg.long().unsqueeze(-1).expand(-1, -1, 3)))


def _fwd_bwd(x, ws, go):
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, *ws)]
    out = _adv().point_mlp_max(*leaves)
    grads = torch.autograd.grad(out, leaves, go)
    _, arg = _adv().point_mlp_max_raw(x, *ws)
    return [out.detach(), arg, *grads]


def test_forward_backward_deterministic(dev):
    B, N, H = 2, 40, 128
    ws = weights(H, 29, dev)
    x = cloud(B, N, 30, dev)
    go = cloud(B, H, 31, dev)[:, :, 0].contiguous()
    a = _fwd_bwd(x, ws, go)
    b = _fwd_bwd(x, ws, go)
    assert all(len(torch.unique(a[1][i])) < H for i in range(B))     # several channels share a winner
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_status_codes(dev):
    from svdformer_pointsea_amd._lib import lib, ptr, stream_of

    L = lib()
    B, N = 2, T + 1
    x = cloud(B, N, 33, dev)

    def call(H, n, wsb_given, wk_ok=True):
        ws = weights(H, 34, dev)
        out = torch.zeros(B, H, device=dev)
        arg = torch.zeros(B, H, dtype=torch.int32, device=dev)
        wk = torch.zeros(max(int(L.pcops_point_mlp_max_workspace_bytes(B, N, 128)), 16), dtype=torch.uint8, device=dev)
        return L.pcops_point_mlp_max_forward(ptr(x), *(ptr(w) for w in ws), 0.2, B, n, H, ptr(out), ptr(arg),
                                             ptr(wk) if wk_ok else None, wsb_given, stream_of(x))

    need = int(L.pcops_point_mlp_max_workspace_bytes(B, N, 128))
    assert need == B * 2 * 128 * 8
    assert call(32, N, need) == 4                 # PCOPS_ERR_UNSUPPORTED
    assert call(128, N, need - 1) == 3            # PCOPS_ERR_WORKSPACE
    assert call(128, N, need, wk_ok=False) == 3
    assert call(128, 0, need) == 1                # PCOPS_ERR_INVALID
    assert call(128, N, need) == 0
    torch.cuda.synchronize()


def test_unsupported_width_takes_the_chain(dev):
    from svdformer_pointsea_amd._lib import KernelTimer

    ws = weights(32, 37, dev)
    x = cloud(2, 100, 38, dev)
    KernelTimer.enable()
    try:
        out = _adv().point_mlp_max(x, *ws)
        assert "point_mlp_max_forward" not in KernelTimer.spans
    finally:
        KernelTimer.disable()
    top = features64(x, ws).max(1)[0]
    e_ref = float((_adv().point_mlp_max_chain(x, *ws).double() - top).abs().max())
    assert float((out.double() - top).abs().max()) <= FACTOR * e_ref


def _gap_safe_case(dev, B, N, H):
    """A seeded case whose float64 top-2 gaps all exceed 1e-4 max|f| (fp32 evaluation errs by ~1e-6 max|f|)."""
    for seed in range(40, 80):
        ws, x = weights(H, seed, dev), cloud(B, N, seed + 1000, dev)
        f = features64(x, ws)
        top2 = f.topk(2, dim=1)[0]
        if float((top2[:, 0] - top2[:, 1]).min()) >= 1e-4 * float(f.abs().max()):
            return ws, x
    raise AssertionError("no gap-safe seed")


@pytest.mark.parametrize("H", [64, 128])
def test_gradients_fused_vs_chain(dev, monkeypatch, H):
    from svdformer_pointsea_amd._lib import KernelTimer

    B, N = 2, T + 9
    ws, x = _gap_safe_case(dev, B, N, H)
    go = cloud(B, H, 39, dev)[:, :, 0].contiguous()

    def run(fused, dtype=torch.float32):
        monkeypatch.setenv("PCOPS_POINT_MLP_FUSED", "1" if fused else "0")
        leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, *ws)]
        KernelTimer.enable()
        try:
            if dtype == torch.float64:
                out = features64(leaves[0], leaves[1:]).max(1)[0]
            else:
                out = _adv().point_mlp_max(*leaves)
            grads = torch.autograd.grad(out, leaves, go.to(dtype))
            spans = set(KernelTimer.spans)
        finally:
            KernelTimer.disable()
        return out, grads, spans

    _, g64, _ = run(False, torch.float64)
    out_c, g_c, spans_c = run(False)
    out_f, g_f, spans_f = run(True)
    assert "point_mlp_max_forward" in spans_f and "point_mlp_max_scatter" in spans_f
    assert not spans_c
    names = ("dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")
    for n, a, c, r in zip(names, g_f, g_c, g64):
        e_ref, e_k = float((c.double() - r).abs().max()), float((a.double() - r).abs().max())
        print(f"\n[point_mlp_max grad H={H} {n}] e_ref {e_ref:.3g} e_k {e_k:.3g}")
        assert e_k <= FACTOR * e_ref, (n, e_k, e_ref)
    _, arg = _adv().point_mlp_max_raw(x, *ws)
    won = torch.zeros(B, N, dtype=torch.bool, device=dev)
    won.scatter_(1, arg.long(), True)
    assert float(g_f[0][~won].abs().max()) == 0.0 and float(g_f[0][won].abs().max()) > 0


def test_golden_through_the_fused_path(dev, monkeypatch):
    import test_adv55_golden as TG
    from svdformer_pointsea_amd._lib import KernelTimer

    monkeypatch.setenv("PCOPS_POINT_MLP_FUSED", "1")
    KernelTimer.enable()
    try:
        out = TG.golden_case(dev)
        assert "point_mlp_max_forward" in KernelTimer.spans
    finally:
        KernelTimer.disable()
    TG.check_case(out)
    D = TG.discriminator(dev)
    m = D.mlp
    ws = [t.detach().contiguous() for t in (m[0].weight.squeeze(-1), m[0].bias, m[2].weight.squeeze(-1), m[2].bias,
                                            m[4].weight.squeeze(-1), m[4].bias)]
    for tag in ("real", "fake"):
        _, arg = raw(torch.from_numpy(TG.G[tag]).to(dev), ws)
        safe = TG.G[f"gap_{tag}"] >= float(TG.G["gap_bar"])
        assert (~safe).mean() <= 0.02
        assert np.array_equal(arg.cpu().numpy()[safe], TG.G[f"win_{tag}"][safe])


def test_no_bhn_tensor_is_materialised(dev):
    B, N, H = 2, 4096, 128
    dis = _adv().SimplePointDiscriminator().to(dev)
    x = cloud(B, N, 41, dev).requires_grad_(True)

    def step():
        x.grad = None
        dis.zero_grad(set_to_none=True)
        dis(x).sum().backward()

    step()   # workspace, GEMM handles
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"\n[point_mlp_max memory] peak growth {grew} B, one (B, H, N) fp32 tensor {B * H * N * 4} B")
    assert grew < B * H * N * 4


def test_capture_replays_equal_eager(dev):
    B, N = 2, T + 1
    dis = _adv().SimplePointDiscriminator().to(dev)
    params = list(dis.parameters())
    xs = [cloud(B, N, 50 + i, dev) for i in range(3)]
    x = xs[0].clone().requires_grad_(True)

    def run():
        x.grad = None
        for p in params:
            p.grad = None
        s = dis(x).sum()
        s.backward()
        return [s.detach(), x.grad, *[p.grad for p in params]]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = []
    for xi in xs[1:]:
        with torch.no_grad():
            x.copy_(xi)
        eager.append([t.clone() for t in run()])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for xi, ref in zip(xs[1:], eager):
        with torch.no_grad():
            x.copy_(xi)
        for t in outs:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, ref):
            assert torch.equal(a, b)


def test_adv_train_step_svdformer(dev):
    import copy

    from bench import synth_pcn
    from svdformer_pointsea_amd.render import PCViews
    from svdformer_pointsea_amd.svdformer import Model, PCNConfig

    ADV = _adv()
    torch.manual_seed(1)
    model = Model(PCNConfig).cuda()
    dis = ADV.SimplePointDiscriminator().to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.0005)
    d_opt = ADV.make_d_optimizer(dis)
    partial, gt = synth_pcn(2, 8, "cuda")
    depth = PCViews(TRANS=-0.7, RESOLUTION=224).get_img(partial).unsqueeze(1)
    dis0 = copy.deepcopy(dis).eval()
    before = [p.detach().clone() for p in model.parameters()]
    # the prediction the step will see (train mode, same weights): g_adv through the PRE-step discriminator
    with torch.no_grad():
        p2 = model(partial, depth)[-1]
        g_adv_pre = float(ADV._bce(dis0(p2), 1.0))
    t = ADV.adv_train_step(model, dis, opt, d_opt, partial, depth, gt)
    torch.cuda.synchronize()
    assert sorted(t) == ["cd_p1", "cd_p2", "cd_pc", "d_loss", "g_adv", "loss_total"]
    assert all(bool(torch.isfinite(v)) and not v.requires_grad for v in t.values())
    print(f"\n[adv step] { {k: float(v) for k, v in t.items()} } g_adv through the pre-step D {g_adv_pre}")
    assert float(t["g_adv"]) != g_adv_pre
    assert any(not torch.equal(a, b) for a, b in zip(dis0.parameters(), dis.parameters()))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))


def test_adv_train_step_pointsea_flat_adam(dev):
    """The same step with pointsea.Model on FlatParams' bf16 shadows and train.FlatAdam over an AdamW."""
    from bench import synth_55
    from svdformer_pointsea_amd.pointsea import Config55, Model
    from svdformer_pointsea_amd.render import PCViews_Real
    from svdformer_pointsea_amd.train import FlatAdam, FlatParams

    ADV = _adv()
    torch.manual_seed(2)
    model = Model(Config55).cuda()
    fp = FlatParams(model, dev, bf16=True)
    flat = FlatAdam(torch.optim.AdamW([fp.master()], lr=1e-4, weight_decay=0.0005, fused=True), fp)
    fp.refresh()
    dis = ADV.SimplePointDiscriminator().to(dev)
    d_opt = ADV.make_d_optimizer(dis)
    partial, gt = synth_55(2, 6, "cuda")
    depth = PCViews_Real(TRANS=-Config55.NETWORK.view_distance).get_img(partial)
    master, shadow = fp.flat.clone(), fp.flat16.clone()
    d_before = [p.detach().clone() for p in dis.parameters()]
    t = ADV.adv_train_step(model, dis, flat, d_opt, partial, depth, gt)
    torch.cuda.synchronize()
    print(f"\n[adv step pointsea] { {k: float(v) for k, v in t.items()} }")
    assert all(bool(torch.isfinite(v)) and not v.requires_grad for v in t.values())
    assert not torch.equal(master, fp.flat) and not torch.equal(shadow, fp.flat16)
    assert bool(torch.isfinite(fp.flat).all())
    assert any(not torch.equal(a, b.detach()) for a, b in zip(d_before, dis.parameters()))
