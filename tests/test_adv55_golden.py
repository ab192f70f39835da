"""The ShapeNet-55 adversarial option against the reference's own code
(tests/golden/make_golden_adv55.py): the discriminator's state_dict (reference
weights load strictly), its logits, both losses, every gradient, the parameters
after the discriminator's Adam step and the generator term through the updated
discriminator; the order of adv_train_step; AdvConfig's defaults.  CPU: the point
MLP runs the torch op chain here (the fused pass is GPU-only,
tests/test_gpu_adv55.py), the Chamfer terms of the step run through the oracle.

Bars.  Both sides are the same fp32 torch CPU ops, whose reductions split by thread
count, so each quantity is held to 256 u of its largest reference entry
(u = 2^-24; four times the 64 u the generator allows the fp32 chain itself, for
the head, the BCE and the backward on top).  A parameter after the Adam step moves
by lr g / (|g| + eps): its bar is the gradient's bar times lr / (|g| + eps), the
slope of that update, plus one rounding of the parameter.
"""
import os
import sys

import numpy as np
import torch

from conftest import golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from weights import fill_state  # noqa: E402
from make_golden_adv55 import SCALE, SEED_D, clouds  # noqa: E402
from oracle.cpu_path import cpu_ops  # noqa: E402
from svdformer_pointsea_amd import adversarial as ADV  # noqa: E402

G = golden("adv55.npz")
U = 2.0 ** -24
KEYS = list(G["keys"])


def bar(ref, mult=256):
    return mult * U * float(np.abs(ref).max())


def check(name, got, ref, mult=256):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    d, lim = float(np.abs(got - ref).max()), bar(ref, mult)
    print(f"[adv55 {name}] max|d| {d:.3g} bar {lim:.3g}")
    assert d <= lim, (name, d, lim)


def discriminator(device="cpu"):
    return fill_state(ADV.SimplePointDiscriminator(), SEED_D, scale=SCALE).to(device)


def golden_case(device="cpu"):
    """The generator's sequence on `device` -> dict of everything it recorded."""
    D = discriminator(device)
    real_np, fake_np = clouds()
    np.testing.assert_array_equal(real_np, G["real"])
    np.testing.assert_array_equal(fake_np, G["fake"])
    real = torch.from_numpy(real_np).to(device)
    fake = torch.from_numpy(fake_np).to(device).requires_grad_(True)
    params = dict(D.named_parameters())
    pre = {k: params[k].detach().clone() for k in KEYS}
    d_opt = ADV.make_d_optimizer(D)
    out = {}
    D.eval()
    g_adv = ADV._bce(D(fake), 1.0)
    g_adv.backward()
    out["g_adv"], out["g_dfake"] = float(g_adv.detach()), fake.grad.cpu().numpy()
    D.train()
    d_opt.zero_grad()
    out["logit_real"] = D(real).detach().cpu().numpy()
    out["logit_fake"] = D(fake.detach()).detach().cpu().numpy()
    d_loss = ADV.discriminator_loss(D, fake, real)
    d_loss.backward()
    out["d_loss"] = float(d_loss.detach())
    out["dgrad"] = [params[k].grad.detach().cpu().numpy().copy() for k in KEYS]
    d_opt.step()
    out["pre"] = [pre[k].cpu().numpy() for k in KEYS]
    out["post"] = [params[k].detach().cpu().numpy().copy() for k in KEYS]
    D.eval()
    with torch.no_grad():
        out["g_adv_post"] = float(ADV._bce(D(fake.detach()), 1.0))
    return out


def check_case(out):
    check("logit_real", out["logit_real"], G["logit_real"])
    check("logit_fake", out["logit_fake"], G["logit_fake"])
    for k in ("d_loss", "g_adv", "g_adv_post"):
        check(k, out[k], G[k])
    check("g_dfake", out["g_dfake"], G["g_dfake"])
    lr, eps = float(G["cfg_d_lr"]), 1e-8
    for i, k in enumerate(KEYS):
        g_ref = G[f"dgrad_{i}"].astype(np.float64)
        check(f"dgrad {k}", out["dgrad"][i], g_ref)
        lim = bar(g_ref) * lr / (np.abs(g_ref) + eps) + 2 * U * np.abs(G[f"post_{i}"]) + 1e-12
        d = np.abs(out["post"][i].astype(np.float64) - G[f"post_{i}"])
        assert (d <= lim).all(), (k, float((d / lim).max()))
        assert not np.array_equal(out["post"][i], out["pre"][i]), k   # the step moved it


def test_state_dict_matches_reference_and_loads_strictly():
    D = ADV.SimplePointDiscriminator()
    sd = D.state_dict()
    assert sorted(sd) == KEYS
    assert [str(tuple(sd[k].shape)) for k in KEYS] == list(G["shapes"])
    ref = {k: torch.from_numpy(G[f"post_{i}"]) for i, k in enumerate(KEYS)}
    D.load_state_dict(ref, strict=True)
    assert all(torch.equal(D.state_dict()[k], ref[k]) for k in KEYS)


def test_adv_config_defaults_are_config_55():
    C = ADV.AdvConfig
    assert C.ENABLED is False and bool(G["cfg_enabled"]) is False
    assert (C.LAMBDA_G, C.D_LR, C.D_STEPS) == (float(G["cfg_lambda_g"]), float(G["cfg_d_lr"]), int(G["cfg_d_steps"]))
    assert tuple(C.BETAS) == tuple(float(v) for v in G["cfg_betas"])
    opt = ADV.make_d_optimizer(ADV.SimplePointDiscriminator())
    assert type(opt) is torch.optim.Adam
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["weight_decay"]) == (C.D_LR, tuple(C.BETAS), 0)


def test_losses_gradients_and_step_match_reference_cpu():
    check_case(golden_case("cpu"))


def test_chain_winners_match_float64():
    """The chain's own argmax agrees with the float64 winners wherever the top-2 gap exceeds the value bar."""
    D = discriminator()
    m = D.mlp
    for tag in ("real", "fake"):
        x = torch.from_numpy(G[tag])
        with torch.no_grad():
            f = m(x.transpose(1, 2).contiguous())
            out = ADV.point_mlp_max(x, m[0].weight.squeeze(-1), m[0].bias, m[2].weight.squeeze(-1), m[2].bias,
                                    m[4].weight.squeeze(-1), m[4].bias)
        safe = G[f"gap_{tag}"] >= float(G["gap_bar"])
        assert (~safe).mean() <= 0.02
        assert np.array_equal(f.max(2)[1].numpy()[safe], G[f"win_{tag}"][safe])
        assert float(np.abs(out.numpy() - G[f"fmax_{tag}"]).max()) <= float(G["gap_bar"])


def test_point_mlp_max_is_fp32_under_autocast():
    D = discriminator()
    x = torch.from_numpy(G["real"])
    with torch.no_grad():
        want = D(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            got = D(x.to(torch.bfloat16).float())
            got2 = D(x)
    assert got2.dtype == torch.float32 and torch.equal(got2, want)
    assert got.dtype == torch.float32


class _StubModel(torch.nn.Module):
    """Returns fixed clouds shifted by one learnable offset (so the generator's step has something to move)."""

    def __init__(self, clouds):
        super().__init__()
        self.shift = torch.nn.Parameter(torch.zeros(3))
        self.clouds = clouds

    def forward(self, partial, depth):
        return tuple(c + self.shift for c in self.clouds)


def _step_inputs():
    rng = np.random.default_rng(77)
    t = lambda n, s: torch.from_numpy((s * rng.standard_normal((2, n, 3))).astype(np.float32))  # noqa: E731
    gt, partial = t(256, 0.4), t(64, 0.4)
    return partial, gt, (t(32, 0.4), t(128, 0.4), t(256, 0.4))


def test_adv_train_step_is_the_reference_order():
    """adv_train_step against the same pieces called by hand in train_55.py:152-180's order: the discriminator
    steps BEFORE the generator term is taken."""
    from svdformer_pointsea_amd.metrics import get_loss_PM

    partial, gt, pcs = _step_inputs()
    cfg = ADV.AdvConfig

    def fresh():
        model, dis = _StubModel(pcs), discriminator()
        return model, dis, torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.0005), ADV.make_d_optimizer(dis)

    with cpu_ops():
        model, dis, opt, d_opt = fresh()
        got = ADV.adv_train_step(model, dis, opt, d_opt, partial, None, gt)
        assert not dis.training   # the generator term ran in eval mode

        m2, d2, o2, do2 = fresh()
        pred = m2(partial, None)
        loss_total, losses = get_loss_PM(pred, partial, gt, sqrt=False)
        g_adv_before = ADV._bce(d2(pred[-1]), 1.0).detach()
        for _ in range(cfg.D_STEPS):
            d2.train()
            do2.zero_grad()
            d_loss = (ADV._bce(d2(gt), 1.0) + ADV._bce(d2(pred[-1].detach()), 0.0)) * 0.5
            d_loss.backward()
            do2.step()
        d2.eval()
        g_adv = ADV._bce(d2(pred[-1]), 1.0)
        loss_total = loss_total + cfg.LAMBDA_G * g_adv
        o2.zero_grad()
        loss_total.backward()
        o2.step()

    want = {"loss_total": loss_total, "cd_pc": losses[0], "cd_p1": losses[1], "cd_p2": losses[2], "d_loss": d_loss,
            "g_adv": g_adv}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert not got[k].requires_grad
        assert float(got[k]) == float(v.detach()), k
    assert float(got["g_adv"]) != float(g_adv_before)   # taken through the UPDATED discriminator
    assert torch.equal(model.shift.detach(), m2.shift.detach()) and float(model.shift.detach().abs().sum()) > 0
    for (k, a), (_, b) in zip(dis.state_dict().items(), d2.state_dict().items()):
        assert torch.equal(a, b), k


def test_adv_losses_terms():
    partial, gt, pcs = _step_inputs()
    model, dis = _StubModel(pcs), discriminator()
    with cpu_ops():
        t = ADV.adv_losses(model, dis, partial, None, gt)
    d = {k: v.detach() for k, v in t.items() if k != "pcds"}
    assert float(d["total"]) == float(d["loss_total"] + ADV.AdvConfig.LAMBDA_G * d["g_adv"])
    assert all(torch.isfinite(t[k]) for k in ("loss_total", "cd_pc", "cd_p1", "cd_p2", "d_loss", "g_adv"))


def test_tile_constant_mirrors_the_header():
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "include", "pcops.h")).read()
    assert int(re.search(r"#define PCOPS_POINT_MLP_TILE (\d+)", src).group(1)) == ADV.POINT_MLP_TILE


def test_sparse_backward_equals_the_chain_autograd():
    """winner_grads (the fused path's backward without its two launches) against autograd through the op chain,
    on the golden clouds: the same gradients, with dx placed at the winners by hand."""
    D = discriminator()
    m = D.mlp
    ws = [t.detach() for t in (m[0].weight.squeeze(-1), m[0].bias, m[2].weight.squeeze(-1), m[2].bias,
                               m[4].weight.squeeze(-1), m[4].bias)]
    for tag in ("real", "fake"):
        x = torch.from_numpy(G[tag])
        B, N, _ = x.shape
        leaves = [t.clone().requires_grad_(True) for t in (x, *ws)]
        out = ADV.point_mlp_max_chain(*leaves)
        dout = torch.from_numpy(np.random.default_rng(9).standard_normal(out.shape).astype(np.float32))
        want = torch.autograd.grad(out, leaves, dout)
        arg = torch.from_numpy(G[f"win_{tag}"]).to(torch.int32)
        assert len(torch.unique(arg[0])) < arg.shape[1]            # channels share winners
        got = ADV.winner_grads(x, *ws, arg, dout, 0.2)
        dx = torch.zeros(B * N, 3).index_add_(0, (arg.long() + N * torch.arange(B).view(B, 1)).reshape(-1), got[0])
        check(f"sparse dx {tag}", dx.view(B, N, 3).numpy(), want[0].numpy())
        for k, a, b in zip(("dw1", "db1", "dw2", "db2", "dw3", "db3"), got[1:], want[1:]):
            check(f"sparse {k} {tag}", a.numpy(), b.numpy())
