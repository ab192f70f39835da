"""The adversarial option of the ShapeNet-55 trainer (core/train_55.py:21-46,
:115-122, :156-176; config_55.py:76-81 TRAIN.ADV) on this package's hot path.

The discriminator is a shared per-point MLP 3 -> 128 -> 128 -> 128 (LeakyReLU 0.2
between the layers, none after the last) and a max over the N points, then two
Linear layers.  It runs three times per step (gt, the detached prediction, the
attached prediction) on N = 8192 points.  As torch ops every pass writes and
re-reads five (B, 128, N) fp32 tensors and autograd keeps them; here the MLP and
the max are one libpcops pass (csrc/pointmlp.hip, DESIGN.md "Point-MLP max") that
returns the (B, 128) maxima and their point indices.  The gradient of a maximum
enters the MLP at its winning point only, so the backward recomputes the chain on
the <= 128 winners per cloud in torch and scatters their dx back with a
deterministic accumulate; no (B, H, N) tensor exists in either direction.

Module / attribute names follow the reference, so its weights load with
strict=True.  The reference saves no discriminator in its ShapeNet-55
checkpoints (train_55.py:227-230), so train.checkpoint_state is unchanged.

Reference map:
  SimplePointDiscriminator                 core/train_55.py:21-46
  the discriminator's optimizer            core/train_55.py:115-122
  the adversarial part of the step         core/train_55.py:152-180
  TRAIN.ADV                                config_55.py:76-81, BETAS :70
"""
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from ._lib import Workspace, call, lib, ptr, stream_of
from .metrics import get_loss_PM

# PCOPS_POINT_MLP_FUSED=0: the reference's op chain in torch instead of the fused pass (A/B runs, parity tests)
_FUSED_ENV = "PCOPS_POINT_MLP_FUSED"

# points per workgroup of pcops_point_mlp_max_forward (PCOPS_POINT_MLP_TILE in include/pcops.h)
POINT_MLP_TILE = 256


def _fused_on():
    return os.environ.get(_FUSED_ENV, "1") != "0"


def point_mlp_max_eligible(x, w1):
    """What pcops_point_mlp_max_forward accepts (include/pcops.h)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == 3 and w1.shape[0] in (64, 128)
            and x.shape[0] >= 1 and x.shape[1] >= 1)


def _mlp_rows(x, w1, b1, w2, b2, w3, b3, slope):
    """The three layers on rows of points: x (..., 3) -> (..., H)."""
    h = F.leaky_relu(F.linear(x, w1, b1), slope)
    h = F.leaky_relu(F.linear(h, w2, b2), slope)
    return F.linear(h, w3, b3)


def point_mlp_max_chain(x, w1, b1, w2, b2, w3, b3, slope=0.2):
    """The reference's op chain (train_55.py:40-44) in torch: x (B, N, in) -> Conv1d, LeakyReLU, Conv1d,
    LeakyReLU, Conv1d on (B, in, N) -> max over N -> (B, H).  What runs on the CPU."""
    f = x.transpose(1, 2).contiguous()
    f = F.leaky_relu(F.conv1d(f, w1.unsqueeze(-1), b1), slope)
    f = F.leaky_relu(F.conv1d(f, w2.unsqueeze(-1), b2), slope)
    f = F.conv1d(f, w3.unsqueeze(-1), b3)
    return torch.max(f, dim=2, keepdim=False)[0]


def point_mlp_max_raw(x, w1, b1, w2, b2, w3, b3, slope=0.2):
    """pcops_point_mlp_max_forward on contiguous fp32 GPU tensors -> (out (B, H) fp32, arg (B, H) int32)."""
    B, N, _ = x.shape
    H = w1.shape[0]
    out = torch.empty(B, H, dtype=torch.float32, device=x.device)
    arg = torch.empty(B, H, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        wsb = lib().pcops_point_mlp_max_workspace_bytes(B, N, H)
        ws = Workspace.get(x.device, wsb)
        call("point_mlp_max_forward", lib().pcops_point_mlp_max_forward, ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
             ptr(w3), ptr(b3), float(slope), B, N, H, ptr(out), ptr(arg), ptr(ws), wsb, stream_of(x))
    return out, arg


def winner_grads(x, w1, b1, w2, b2, w3, b3, arg, dout, slope, need=(True,) * 7):
    """The sparse backward's torch part: gradients of sum(dout * out) for (x's winners, w1, b1, w2, b2, w3, b3),
    None where `need` is False.  The first is per (b, c) row, (B*H, 3): the gradient for point arg[b, c], non-zero
    only on the first row of each distinct point."""
    B, H = arg.shape
    # the <= H winners of each cloud, one row per (b, c)
    a = arg.long()
    xw = x.gather(1, a.unsqueeze(-1).expand(B, H, 3)).reshape(B * H, 3)
    # Channels that share a winner have identical rows.  Row (b, c) receives dout[b, c] at f[b, c, c]; all of a
    # point's channels are handed to its FIRST row (the lowest channel it won) instead, so the sums over rows see
    # one row per distinct point, as the op chain's sums over n do, and exact zeros elsewhere
    ch = torch.arange(H, device=x.device)
    owner = torch.where(a.unsqueeze(2) == a.unsqueeze(1), ch.view(1, 1, H), H).amin(dim=2)            # (B, H)
    dout = dout.to(torch.float32)
    df = torch.where(owner.unsqueeze(1) == ch.view(1, H, 1), dout.unsqueeze(1), torch.zeros_like(dout[:1, :1]))
    with torch.enable_grad():
        leaves = [t.detach().requires_grad_(n) for t, n in zip((xw, w1, b1, w2, b2, w3, b3), need)]
        f = _mlp_rows(*leaves, slope)                                          # (B*H, H); df is [b, row, c]
        wanted = [t for t, n in zip(leaves, need) if n]
        got = iter(torch.autograd.grad(f, wanted, df.reshape(B * H, H)))
    return [next(got) if n else None for n in need]


class _PointMlpMax(torch.autograd.Function):
    """out[b,c] = max_n f[b,n,c]: pcops_point_mlp_max_forward; the backward recomputes f on the winners
    arg[b,:] in torch (winner_grads), backpropagates dout[b,c] through f[b, arg[b,c], c] and places the
    winners' dx with pcops_point_mlp_max_scatter (fixed order)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, slope):
        out, arg = point_mlp_max_raw(x, w1, b1, w2, b2, w3, b3, slope)
        ctx.save_for_backward(x, w1, b1, w2, b2, w3, b3, arg)
        ctx.slope = slope
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        *tensors, arg = ctx.saved_tensors
        x = tensors[0]
        B, N, _ = x.shape
        H = arg.shape[1]
        grads = winner_grads(*tensors, arg, dout, ctx.slope, ctx.needs_input_grad[:7])
        if grads[0] is not None:
            dxw = grads[0].contiguous()
            dx = torch.empty_like(x)
            with torch.cuda.device(x.device):
                call("point_mlp_max_scatter", lib().pcops_point_mlp_max_scatter, ptr(dxw), ptr(arg), B, N, H,
                     ptr(dx), stream_of(x))
            grads[0] = dx
        return (*grads, None)


def point_mlp_max(x, w1, b1, w2, b2, w3, b3, slope=0.2):
    """max over the points of the shared MLP: x (B, N, 3), w1 (H, 3), w2 / w3 (H, H) [out][in], b (H) -> (B, H).
    One libpcops pass when the tensors are on the GPU, the shape is eligible and PCOPS_POINT_MLP_FUSED is not
    "0"; the op chain otherwise.  fp32 always: under autocast the inputs are cast up and autocast is off inside."""
    args = (x, w1, b1, w2, b2, w3, b3)
    if torch.is_autocast_enabled(x.device.type) or any(t.dtype != torch.float32 for t in args):
        with torch.autocast(x.device.type, enabled=False):
            return point_mlp_max(*(t.float() for t in args), slope=slope)
    if _fused_on() and point_mlp_max_eligible(x, w1):
        return _PointMlpMax.apply(*(t.contiguous() for t in args), float(slope))
    return point_mlp_max_chain(*args, slope)


class SimplePointDiscriminator(nn.Module):
    """train_55.py:21-46: shared point MLP, max over the points, two Linear layers; x (B, N, 3) -> (B, 1) logits."""

    def __init__(self, in_dim=3, hidden=128):
        super().__init__()
        self.mlp = nn.Sequential(
            nn.Conv1d(in_dim, hidden, 1), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv1d(hidden, hidden, 1), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv1d(hidden, hidden, 1))
        self.head = nn.Sequential(nn.Linear(hidden, hidden), nn.LeakyReLU(0.2, inplace=True), nn.Linear(hidden, 1))

    def forward(self, x):
        m = self.mlp
        with torch.autocast(x.device.type, enabled=False):   # the discriminator is always fp32
            g = point_mlp_max(x.float(), m[0].weight.squeeze(-1), m[0].bias, m[2].weight.squeeze(-1), m[2].bias,
                              m[4].weight.squeeze(-1), m[4].bias, slope=0.2)
            return self.head(g)


class AdvConfig:
    """config_55.py:76-81 TRAIN.ADV, and TRAIN.BETAS (:70) the discriminator's Adam reads."""
    ENABLED = False
    LAMBDA_G = 0.05
    D_LR = 0.0001
    D_STEPS = 1
    BETAS = (.9, .999)


def make_d_optimizer(dis, cfg=AdvConfig):
    """train_55.py:121: plain Adam on the discriminator."""
    return torch.optim.Adam(dis.parameters(), lr=cfg.D_LR, betas=cfg.BETAS)


def _bce(logit, target):
    return F.binary_cross_entropy_with_logits(logit, torch.full_like(logit, target))


def discriminator_loss(dis, fake, gt):
    """train_55.py:162-168: D on the real cloud and on the DETACHED prediction, halved."""
    return (_bce(dis(gt), 1.0) + _bce(dis(fake.detach()), 0.0)) * 0.5


def adv_losses(model, dis, partial, depth, gt, cfg=AdvConfig, sqrt=False):
    """The terms of the reference step (train_55.py:152-176) without the optimizer steps between them:
    loss_total and the three CD terms of get_loss_PM, d_loss (D sees the last cloud detached), g_adv (D sees
    it attached) and total = loss_total + LAMBDA_G * g_adv."""
    pcds = model(partial, depth)
    loss_total, (cdc, cd1, cd2) = get_loss_PM(pcds, partial, gt, sqrt=sqrt)
    d_loss = discriminator_loss(dis, pcds[-1], gt)
    g_adv = _bce(dis(pcds[-1]), 1.0)
    return {"loss_total": loss_total, "cd_pc": cdc, "cd_p1": cd1, "cd_p2": cd2, "d_loss": d_loss, "g_adv": g_adv,
            "total": loss_total + cfg.LAMBDA_G * g_adv, "pcds": pcds}


def adv_train_step(model, dis, optimizer, d_opt, partial, depth, gt, cfg=AdvConfig, sqrt=False):
    """One eager step in the reference's order (train_55.py:152-180): forward and get_loss_PM; D_STEPS
    discriminator steps (train mode, real and detached-fake BCE, halved, backward, d_opt.step()); eval mode
    and g_adv through the UPDATED discriminator on the attached last cloud; loss_total += LAMBDA_G g_adv;
    zero grad, backward and step on `optimizer`.

    `optimizer` is a torch optimizer over model.parameters(), or a train.FlatAdam: then the forward runs on
    its FlatParams' bf16 shadows under bf16 autocast (refresh them once before the first step; every update
    writes them) and the gradients are collected into its buckets before the update.
    Returns the detached terms loss_total (with the adversarial term), cd_pc, cd_p1, cd_p2, d_loss, g_adv."""
    from .train import FlatAdam

    flat = optimizer.fp if isinstance(optimizer, FlatAdam) else None
    if flat is not None:
        with torch.autocast(partial.device.type, dtype=torch.bfloat16, enabled=bool(flat.shadow)):
            pcds = flat.forward(partial, depth)
            loss_total, (cdc, cd1, cd2) = get_loss_PM(pcds, partial, gt, sqrt=sqrt)
    else:
        pcds = model(partial, depth)
        loss_total, (cdc, cd1, cd2) = get_loss_PM(pcds, partial, gt, sqrt=sqrt)
    p2 = pcds[-1]
    d_loss = None
    for _ in range(cfg.D_STEPS):
        dis.train()
        d_opt.zero_grad()
        d_loss = discriminator_loss(dis, p2, gt)
        d_loss.backward()
        d_opt.step()
    dis.eval()
    g_adv = _bce(dis(p2), 1.0)
    loss_total = loss_total + cfg.LAMBDA_G * g_adv
    if flat is not None:
        flat.zero_grad()
        loss_total.backward()
        flat.collect(widen=False)
        optimizer.step()
    else:
        optimizer.zero_grad()
        loss_total.backward()
        optimizer.step()
    zero = loss_total.detach().new_zeros(())
    return {"loss_total": loss_total.detach(), "cd_pc": cdc.detach(), "cd_p1": cd1.detach(), "cd_p2": cd2.detach(),
            "d_loss": zero if d_loss is None else d_loss.detach(), "g_adv": g_adv.detach()}
