"""ShapeNet-55 adversarial-option golden vectors from the REFERENCE's own code
(core/train_55.py: SimplePointDiscriminator :21-46, the discriminator step and the
generator term :156-176; config_55.py:70-81), run in the build container only; only
the .npz output is committed.

  adv55.npz
    keys / shapes                    state_dict of SimplePointDiscriminator()
    cfg_enabled, cfg_lambda_g, cfg_d_lr, cfg_d_steps, cfg_betas    TRAIN.ADV and TRAIN.BETAS
    real, fake                       seeded clouds (2, 96, 3)
    logit_real, logit_fake           D on both (train mode)
    d_loss, g_adv                    (BCE(real, 1) + BCE(fake, 0)) / 2;  BCE(D(fake), 1), before the step
    dgrad_<i>                        gradient of d_loss for parameter keys[i]
    g_dfake                          gradient of g_adv for the fake cloud
    post_<i>                         parameter keys[i] after one Adam(lr = D_LR, betas = BETAS) step on d_loss
    g_adv_post                       g_adv through the updated D (eval mode)
    win_real, win_fake               (2, 128) the float64 winners of the point-MLP max (lowest index)
    gap_real, gap_fake               (2, 128) float64 gap between the best and the second-best point
    fmax_real, fmax_fake             (2, 128) the float64 maxima
    gap_bar                          the value bar below which a (b, c) pair's winner is not decided in fp32

The float64 evaluation is the generator's own (numpy) on the same weights.  gap_bar is
64 u max|f| with u = 2^-24: three layers of <= 128-term fp32 dot products, each with a
typical error of sqrt(128) u |f| ~ 11 u |f|, doubled.  The generator asserts that at
most 2 % of the (b, c) pairs have a gap below it and that the reference's own fp32
winners agree with the float64 ones on every other pair.

Weights: tests/golden/weights.py fill_state(SEED_D, scale = 0.3).  Stubbed for the import
of core/train_55.py: tensorboardX, easydict, utils.data_loaders and make_golden_models'
stand-ins.  Usage:  python tests/golden/make_golden_adv55.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_models import REF, _stubs  # noqa: E402
from weights import fill_state  # noqa: E402

SEED_D, SEED_IN, SCALE = 555, 556, 0.3
B, N = 2, 96
CAP = 0.02


def clouds():
    """(real, fake): seeded (B, N, 3) fp32 clouds."""
    rng = np.random.default_rng(SEED_IN)
    return (rng.uniform(-0.5, 0.5, (B, N, 3)).astype(np.float32),
            (0.4 * rng.standard_normal((B, N, 3))).astype(np.float32))


def features64(sd, x):
    """f (B, N, H) of the point MLP in float64 numpy."""
    w = [sd[f"mlp.{i}.weight"].double().numpy()[:, :, 0] for i in (0, 2, 4)]
    b = [sd[f"mlp.{i}.bias"].double().numpy() for i in (0, 2, 4)]
    h = x.astype(np.float64)
    for i in range(3):
        h = h @ w[i].T + b[i]
        if i < 2:
            h = np.where(h > 0, h, 0.2 * h)
    return h


def winners64(f):
    """(winner, gap, max) per (b, c) of f (B, N, H)."""
    win = f.argmax(1)
    srt = np.sort(f, axis=1)
    return win.astype(np.int64), srt[:, -1] - srt[:, -2], srt[:, -1]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _more_stubs():
    tb = types.ModuleType("tensorboardX")
    tb.SummaryWriter = object
    sys.modules["tensorboardX"] = tb
    ed = types.ModuleType("easydict")

    class EasyDict(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    ed.EasyDict = EasyDict
    sys.modules["easydict"] = ed
    sys.modules["utils.data_loaders"] = types.ModuleType("utils.data_loaders")
    sys.modules["metrics.CD"].fscore = _load(os.path.join(REF, "metrics/CD/fscore.py"), "metrics.CD.fscore")
    sys.modules["metrics.CD.chamfer3D"].dist_chamfer_3D = sys.modules["metrics.CD.chamfer3D.dist_chamfer_3D"]


def main():
    _stubs()
    sys.path.insert(0, REF)
    _more_stubs()
    torch.manual_seed(0)
    from core.train_55 import SimplePointDiscriminator
    cfg = _load(os.path.join(REF, "config_55.py"), "ref_config_55").cfg

    out = {}
    adv = cfg.TRAIN.ADV
    out.update(cfg_enabled=np.array(bool(adv.ENABLED)), cfg_lambda_g=np.array(float(adv.LAMBDA_G)),
               cfg_d_lr=np.array(float(adv.D_LR)), cfg_d_steps=np.array(int(adv.D_STEPS)),
               cfg_betas=np.array([float(v) for v in cfg.TRAIN.BETAS]))

    D = fill_state(SimplePointDiscriminator(), SEED_D, scale=SCALE)
    sd = {k: v.clone() for k, v in D.state_dict().items()}
    keys = sorted(sd)
    out["keys"] = np.array(keys)
    out["shapes"] = np.array([str(tuple(sd[k].shape)) for k in keys])
    real_np, fake_np = clouds()
    out.update(real=real_np, fake=fake_np)
    real = torch.from_numpy(real_np)
    fake = torch.from_numpy(fake_np).requires_grad_(True)
    bce = torch.nn.BCEWithLogitsLoss()

    # float64 winners and gaps; the reference's own fp32 winners must agree wherever the gap decides
    bar = 0.0
    for tag, x in (("real", real_np), ("fake", fake_np)):
        f = features64(sd, x)
        win, gap, fmax = winners64(f)
        out[f"win_{tag}"], out[f"gap_{tag}"], out[f"fmax_{tag}"] = win, gap, fmax
        bar = max(bar, 64 * 2.0 ** -24 * float(np.abs(f).max()))
    out["gap_bar"] = np.array(bar)
    close = 0
    for tag, x in (("real", real), ("fake", fake.detach())):
        with torch.no_grad():
            ref_win = torch.max(D.mlp(x.transpose(1, 2).contiguous()), dim=2)[1].numpy()
        safe = out[f"gap_{tag}"] >= bar
        close += int((~safe).sum())
        assert np.array_equal(ref_win[safe], out[f"win_{tag}"][safe]), tag
    total = 2 * out["win_real"].size
    print("gap_bar", bar, "pairs below it", close, "of", total)
    assert close <= CAP * total

    # train_55.py:160-170, one discriminator step
    params = dict(D.named_parameters())
    d_opt = torch.optim.Adam(D.parameters(), lr=adv.D_LR, betas=cfg.TRAIN.BETAS)
    D.eval()
    g_adv = bce(D(fake), torch.ones(B, 1))
    g_adv.backward()
    out["g_adv"] = np.array(float(g_adv.detach()), np.float64)
    out["g_dfake"] = fake.grad.numpy().copy()
    D.train()
    d_opt.zero_grad()
    real_logits = D(real)
    fake_logits = D(fake.detach())
    d_loss = (bce(real_logits, torch.ones_like(real_logits)) + bce(fake_logits, torch.zeros_like(fake_logits))) * 0.5
    d_loss.backward()
    out.update(logit_real=real_logits.detach().numpy(), logit_fake=fake_logits.detach().numpy(),
               d_loss=np.array(float(d_loss.detach()), np.float64))
    for i, k in enumerate(keys):
        out[f"dgrad_{i}"] = params[k].grad.numpy().copy()
    d_opt.step()
    for i, k in enumerate(keys):
        out[f"post_{i}"] = params[k].detach().numpy().copy()
    # train_55.py:173-175 through the updated discriminator
    D.eval()
    with torch.no_grad():
        lg = D(fake.detach())
        out["g_adv_post"] = np.array(float(bce(lg, torch.ones_like(lg))), np.float64)
    print("d_loss", out["d_loss"], "g_adv", out["g_adv"], "g_adv_post", out["g_adv_post"])
    path = os.path.join(HERE, "adv55.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
