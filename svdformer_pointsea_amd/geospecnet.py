"""GeoSpecNet (models/GeoSpecNet.py, core/train_geospec.py) restated on this
package's hot path: the SVFNetGS encoder (SVFNet with a spectral point-feature
extractor), the multi-scale SpectralAdapter, the PointNet discriminator of the
adversarial step, and the step's losses.

Module / attribute names follow the reference, so its checkpoints
({'G', 'D', 'g_optim', 'd_optim'} with DataParallel's 'module.' prefix) load
with strict=True.  Everything the model shares with SVDFormer (SVFNet,
local_encoder, SDG, PointNet_SA_Module_KNN, the forward with its side-stream
fork and shared FPS) is svdformer.py's; what is new is the adapter, whose
gather -> DCT -> gate -> inverse DCT -> weighted-sum chain runs as one libpcops
pass each way (csrc/spectral.hip, DESIGN.md "Spectral pooling").

Reference map:
  _create_dct_matrix / SpectralAdapter / MSGSpecConv       models/GeoSpecNet.py:22-129
  SpectralFeatureExtractor / SVFNetGS / Model / Discriminator   :132-257
  the adversarial train step                               core/train_geospec.py:101-130
  checkpoint layout                                        core/train_geospec.py:184, core/test_geospec.py:31

FPS, gather and kNN are reached through the modules svdformer / model_utils at
call time (never imported by name), so oracle/cpu_path.py's attribute swap
covers this model too.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import model_utils, svdformer
from ._lib import Workspace, call, lib, ptr, stream_of
from .metrics import get_loss_PM

# PCOPS_SPECTRAL_FUSED=0: the reference's op chain in torch instead of the fused pass (A/B runs, parity tests)
_SPECTRAL_FUSED = os.environ.get("PCOPS_SPECTRAL_FUSED", "1") != "0"

_DTC = {torch.float32: 0, torch.bfloat16: 1}


def dct_matrix(k, device):
    """The orthonormal DCT-II matrix W (k, k) of GeoSpecNet.py:22-29, W[n, m] = c_m cos(pi (n + 1/2) m / k),
    evaluated in fp32 on `device` in the reference's order of operations."""
    n = torch.arange(k, dtype=torch.float32, device=device).view(-1, 1)
    m = torch.arange(k, dtype=torch.float32, device=device).view(1, -1)
    w = torch.cos(torch.pi * (n + 0.5) * m / k)
    w[:, 0] = w[:, 0] / torch.sqrt(torch.tensor(2.0, device=device))
    return w * torch.sqrt(torch.tensor(2.0 / k, device=device))


def spectral_eligible(x_tok, K):
    """What pcops_spectral_pool_* accepts (include/pcops.h)."""
    return (x_tok.is_cuda and x_tok.dtype in _DTC and K in (4, 8, 16, 32) and x_tok.shape[1] * K <= 16384
            and x_tok.shape[0] * x_tok.shape[1] > 0 and x_tok.shape[2] >= 1)


class _SpectralPool(torch.autograd.Function):
    """out[b,n,c] = sum_m g[c,m] (W^T a)[b,n,m] (W^T x[b, idx[b,n,:], c])[m]: pcops_spectral_pool_forward, and
    pcops_spectral_pool_backward for dx, da and dg (deterministic: no atomics, fixed summation order)."""

    @staticmethod
    def forward(ctx, x, idx, a, g, basis):
        B, N, C = x.shape
        K = idx.shape[2]
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            call("spectral_pool_forward", lib().pcops_spectral_pool_forward, ptr(x), _DTC[x.dtype], ptr(idx), ptr(a),
                 ptr(g), ptr(basis), B, N, K, C, ptr(out), stream_of(x))
        ctx.save_for_backward(x, idx, a, g, basis)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, idx, a, g, basis = ctx.saved_tensors
        B, N, C = x.shape
        K = idx.shape[2]
        dout = dout.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        da = torch.empty_like(a)
        dg = torch.empty_like(g)
        with torch.cuda.device(x.device):
            wsb = lib().pcops_spectral_pool_workspace_bytes(B, N, K, C)
            ws = Workspace.get(x.device, wsb)
            call("spectral_pool_backward", lib().pcops_spectral_pool_backward, ptr(x), _DTC[x.dtype], ptr(dout),
                 _DTC[dout.dtype], ptr(idx), ptr(a), ptr(g), ptr(basis), B, N, K, C, ptr(dx), ptr(da), ptr(dg),
                 ptr(ws), wsb, stream_of(x))
        return dx, None, da, dg, None


def spectral_pool_chain(x_tok, idx, attn, gate, W):
    """The reference's op chain (GeoSpecNet.py:83-105) in torch: x_tok (B, N, C) token-major features, idx
    (B, N, K) neighbour indices, attn (B, 1, N, K) softmax weights, gate (C, K), W (K, K) -> (B, C, N)."""
    B, N, C = x_tok.shape
    K = idx.shape[2]
    batch = torch.arange(B, device=x_tok.device).view(B, 1, 1)
    neigh = x_tok[batch, idx.long()].permute(0, 3, 1, 2).contiguous()             # (B, C, N, K)
    x_hat = torch.matmul(neigh.view(B * C * N, K), W).view(B, C, N, K)
    gamma = gate.view(1, C, K).repeat(B, 1, 1).view(B * C, K)
    x_hat = x_hat * gamma.view(B, C, 1, K)
    x_filt = torch.matmul(x_hat.view(B * C * N, K), W.t()).view(B, C, N, K)
    return torch.sum(x_filt * attn.view(B, 1, N, K), dim=-1)


def spectral_pool(x_tok, idx, attn, gate, W):
    """SpectralAdapter's pooling between the softmax and the channel MLP -> (B, C, N).  One libpcops pass each
    way when the switch is on, the features are on the GPU and the shape is eligible; the op chain otherwise."""
    K = idx.shape[2]
    if _SPECTRAL_FUSED and spectral_eligible(x_tok, K):
        B, N, _ = x_tok.shape
        out = _SpectralPool.apply(x_tok.contiguous(), idx.to(torch.int32).contiguous(),
                                  attn.reshape(B, N, K).float().contiguous(), gate.float().contiguous(),
                                  W.float().contiguous())
        return out.transpose(1, 2)
    return spectral_pool_chain(x_tok, idx, attn, gate, W)


class SpectralAdapter(nn.Module):
    """GeoSpecNet.py:32-109: a fixed DCT basis along the kNN axis, learnable per-channel frequency gates,
    geometric softmax weights over the neighbours, then a channel MLP."""

    def __init__(self, in_channels, out_channels, k_neighbors=16, reduction=4):
        super().__init__()
        self.in_channels, self.out_channels, self.k = in_channels, out_channels, k_neighbors
        self.freq_gate = nn.Parameter(torch.randn(in_channels, self.k) * 0.02)
        self.geo_proj = nn.Sequential(nn.Conv2d(1, 16, kernel_size=1), nn.ReLU(inplace=True),
                                      nn.Conv2d(16, 1, kernel_size=1))
        hidden = max(in_channels // reduction, 16)
        self.proj = nn.Sequential(nn.Conv1d(in_channels, hidden, kernel_size=1), nn.ReLU(inplace=True),
                                  nn.Conv1d(hidden, out_channels, kernel_size=1))
        self._bases = {}

    def _dct(self, device):
        if device not in self._bases:
            self._bases[device] = dct_matrix(self.k, device)
        return self._bases[device]

    def forward(self, xyz, feats):
        """xyz (B, 3, N), feats (B, C, N) -> (B, out_channels, N)."""
        # neighbours in topk's ascending-distance order (the DCT runs along K)
        group_xyz, idx = model_utils.group_local(xyz, k=self.k, return_idx=True)
        # as the reference's code has it: the norm of the neighbours' absolute coordinates
        dists = torch.norm(group_xyz, dim=1, keepdim=True)                         # (B, 1, N, K)
        attn = torch.softmax(-self.geo_proj(dists), dim=-1)
        pooled = spectral_pool(feats.transpose(1, 2).contiguous(), idx, attn, self.freq_gate, self._dct(feats.device))
        return self.proj(pooled)


class MSGSpecConv(nn.Module):
    """GeoSpecNet.py:112-129: SpectralAdapters over several K, concatenated and fused."""

    def __init__(self, in_channels, out_channels, k_list):
        super().__init__()
        self.branches = nn.ModuleList([SpectralAdapter(in_channels, out_channels, k) for k in k_list])
        self.fuse = nn.Sequential(nn.Conv1d(out_channels * len(k_list), out_channels, kernel_size=1),
                                  nn.ReLU(inplace=True))

    def forward(self, xyz, feats):
        # each branch runs its own kNN (no sharing of the K = 32 result between the branches)
        return self.fuse(torch.cat([b(xyz, feats) for b in self.branches], dim=1))


class SpectralFeatureExtractor(nn.Module):
    """GeoSpecNet.py:132-155: the PointNet++ SA encoder with MSGSpecConv refining the 128-point level."""

    def __init__(self, out_dim=256):
        super().__init__()
        SA = svdformer.PointNet_SA_Module_KNN
        self.sa_module_1 = SA(512, 16, 3, [64, 128], group_all=False, if_bn=False, if_idx=True)
        self.sa_module_2 = SA(128, 16, 128, [128, 256], group_all=False, if_bn=False, if_idx=True)
        self.msg_spec = MSGSpecConv(in_channels=256, out_channels=256, k_list=[16, 32])
        self.sa_module_3 = SA(None, None, 256, [512, out_dim], group_all=True, if_bn=False)

    def forward(self, point_cloud, fidx=None):
        """fidx: a model_utils.SharedFPS of point_cloud (the model's shared partial-cloud FPS)."""
        l1_xyz, l1_points, _ = self.sa_module_1(point_cloud, point_cloud, fidx=fidx)
        l2_xyz, l2_points, _ = self.sa_module_2(l1_xyz, l1_points)
        l2_points = l2_points + self.msg_spec(l2_xyz, l2_points)   # spectral refinement at the mid scale
        _, l3_points = self.sa_module_3(l2_xyz, l2_points)
        return l3_points


class SVFNetGS(svdformer.SVFNet):
    """GeoSpecNet.py:158-200: SVFNet with the spectral point-feature extractor; the image branch, its fork and
    the fusion are SVFNet's."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.point_feature_extractor = SpectralFeatureExtractor()


class Model(svdformer.Model):
    """GeoSpecNet.py:203-232: (partial (B,N,3), depth (3B,1,224,224)) -> (coarse, fine1, fine2); the forward
    (local encoder on a side stream, shared partial-cloud FPS, token-major refinement) is svdformer.Model's."""

    def __init__(self, cfg):
        nn.Module.__init__(self)
        self.encoder = SVFNetGS(cfg)
        self.localencoder = svdformer.local_encoder(cfg)
        self.merge_points = cfg.NETWORK.merge_points
        dataset = getattr(getattr(cfg, "DATASET", None), "TEST_DATASET", "ShapeNet")
        self.refine1 = svdformer.SDG(ratio=cfg.NETWORK.step1, hidden_dim=768, dataset=dataset)
        self.refine2 = svdformer.SDG(ratio=cfg.NETWORK.step2, hidden_dim=512, dataset=dataset)
        for m in self.modules():   # NHWC 2-D convs (see svdformer.Model)
            if isinstance(m, nn.Conv2d):
                m.to(memory_format=torch.channels_last)


class Discriminator(nn.Module):
    """GeoSpecNet.py:235-257: PointNet global feature -> one logit per cloud; pcd (B, N, 3) -> (B,)."""

    def __init__(self, feat_size=256):
        super().__init__()
        self.stem = nn.Sequential(
            nn.Conv1d(3, 64, 1), nn.BatchNorm1d(64), nn.ReLU(inplace=True),
            nn.Conv1d(64, 128, 1), nn.BatchNorm1d(128), nn.ReLU(inplace=True),
            nn.Conv1d(128, feat_size, 1), nn.BatchNorm1d(feat_size), nn.ReLU(inplace=True))
        self.head = nn.Sequential(nn.Linear(feat_size, feat_size // 2), nn.ReLU(inplace=True),
                                  nn.Linear(feat_size // 2, 1))

    def forward(self, pcd):
        x = self.stem(pcd.transpose(1, 2).contiguous())
        return self.head(torch.max(x, dim=2, keepdim=False)[0]).squeeze(-1)


class GeoSpecConfig:
    """The NETWORK and TRAIN keys of config_geospec.py:33-53 the model and the step read; the optimizers'
    weight decay is the train script's (core/train_geospec.py:57-60), not the config's unused 0."""

    class NETWORK:
        N_SAMPLING_POINTS = 2048
        step1 = 4
        step2 = 8
        merge_points = 512
        local_points = 512
        view_distance = 0.7

    class DATASET:
        TEST_DATASET = "ShapeNet"

    class TRAIN:
        BATCH_SIZE = 12
        N_EPOCHS = 400
        SAVE_FREQ = 50
        LEARNING_RATE = 0.0001
        LR_DECAY_STEP = [40, 80, 120, 160, 200, 240, 280, 320, 360]
        WARMUP_STEPS = 300
        GAMMA = 0.7
        BETAS = (0.9, 0.999)
        WEIGHT_DECAY = 5e-4
        GAN_WEIGHT = 0.05


# ----------------------------------------------------------------- the adversarial step
def _bce(logit, target):
    return F.binary_cross_entropy_with_logits(logit, torch.full_like(logit, target))


def discriminator_loss(D, fake, gt):
    """core/train_geospec.py:111-117: D on the real cloud and on the DETACHED last prediction."""
    return (_bce(D(gt), 1.0) + _bce(D(fake.detach()), 0.0)) * 0.5


def geospec_losses(G, D, partial, depth, gt, gan_weight=GeoSpecConfig.TRAIN.GAN_WEIGHT):
    """The terms of the reference step (core/train_geospec.py:105-126) without the optimizer steps between
    them: loss_total and the three CD terms of get_loss_PM(sqrt=True), d_loss (D sees the last cloud
    detached), g_gan (D sees it attached) and total_g = loss_total + gan_weight * g_gan."""
    pcds = G(partial, depth)
    loss_total, (cdc, cd1, cd2) = get_loss_PM(pcds, partial, gt, sqrt=True)
    d_loss = discriminator_loss(D, pcds[-1], gt)
    g_gan = _bce(D(pcds[-1]), 1.0)
    return {"loss_total": loss_total, "cd_pc": cdc, "cd_p1": cd1, "cd_p2": cd2, "d_loss": d_loss, "g_gan": g_gan,
            "total_g": loss_total + gan_weight * g_gan, "pcds": pcds}


def make_optimizers(G, D, cfg=GeoSpecConfig):
    """core/train_geospec.py:57-60: AdamW on both nets, weight decay 5e-4."""
    kw = dict(lr=cfg.TRAIN.LEARNING_RATE, weight_decay=cfg.TRAIN.WEIGHT_DECAY)
    return (torch.optim.AdamW([p for p in G.parameters() if p.requires_grad], **kw),
            torch.optim.AdamW([p for p in D.parameters() if p.requires_grad], **kw))


def geospec_train_step(G, D, g_optim, d_optim, partial, depth, gt, gan_weight=GeoSpecConfig.TRAIN.GAN_WEIGHT):
    """One eager step in the reference's order (core/train_geospec.py:105-130): forward, reconstruction loss,
    the discriminator's backward and AdamW step, then the generator's adversarial term through the UPDATED
    discriminator, its backward and AdamW step.  Returns the detached terms."""
    pcds = G(partial, depth)
    loss_total, (cdc, cd1, cd2) = get_loss_PM(pcds, partial, gt, sqrt=True)
    d_loss = discriminator_loss(D, pcds[-1], gt)
    d_optim.zero_grad()
    d_loss.backward()
    d_optim.step()
    g_gan = _bce(D(pcds[-1]), 1.0)
    total_g = loss_total + gan_weight * g_gan
    g_optim.zero_grad()
    total_g.backward()
    g_optim.step()
    return {k: v.detach() for k, v in (("loss_total", loss_total), ("cd_pc", cdc), ("cd_p1", cd1), ("cd_p2", cd2),
                                       ("d_loss", d_loss), ("g_gan", g_gan), ("total_g", total_g))}


# ----------------------------------------------------------------- checkpoints
def _strip(sd, prefix):
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}


def checkpoint_state(G, D, g_optim, d_optim, prefix="module."):
    """The reference layout (core/train_geospec.py:184): {'G', 'D', 'g_optim', 'd_optim'}, the nets' keys with
    DataParallel's 'module.' prefix."""
    return {"G": {prefix + k: v for k, v in G.state_dict().items()},
            "D": {prefix + k: v for k, v in D.state_dict().items()},
            "g_optim": g_optim.state_dict(), "d_optim": d_optim.state_dict()}


def load_checkpoint_state(ckpt, G, D=None, g_optim=None, d_optim=None, prefix="module."):
    """Strict load of a reference checkpoint: the generator from 'G', or from 'model' as the reference's test
    script accepts (core/test_geospec.py:31); the discriminator and the optimizers when given and present."""
    G.load_state_dict(_strip(ckpt["G"] if "G" in ckpt else ckpt["model"], prefix), strict=True)
    if D is not None and "D" in ckpt:
        D.load_state_dict(_strip(ckpt["D"], prefix), strict=True)
    if g_optim is not None and "g_optim" in ckpt:
        g_optim.load_state_dict(ckpt["g_optim"])
    if d_optim is not None and "d_optim" in ckpt:
        d_optim.load_state_dict(ckpt["d_optim"])
