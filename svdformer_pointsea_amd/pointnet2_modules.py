"""Drop-in for `pointnet2_ops.pointnet2_modules` on libpcops.so (gfx950).

Same names, constructor arguments, state_dict keys (`mlps.{i}.{j}.*`, `mlp.{j}.*`) and forward
layouts as pointnet2_ops_lib/pointnet2_ops/pointnet2_modules.py:
  build_shared_mlp(mlp_spec, bn=True)                                   [:9-19]
  PointnetSAModuleMSG(npoint, radii, nsamples, mlps, bn, use_xyz)       [:77-115]
  PointnetSAModule(mlp, npoint, radius, nsample, bn, use_xyz)           [:118-146]
  PointnetFPModule(mlp, bn)                                             [:149-209]

Every module adds `forward_tokens`, which takes and returns token-major features ((B,N,C) instead of
(B,C,N)), so SA -> SA -> FP chains do not transpose at every boundary.

On the GPU, with coordinates that need no gradient, a scale's grouping is one pcops_ball_group
launch (model_utils.ball_group_rows) and feature propagation up to the MLP one
pcops_fp_interp_forward launch (model_utils.fp_interp_cl).  PCOPS_PN2_FUSED=0, or any other case,
runs the unfused chain of QueryAndGroup / three_nn / three_interpolate.  Both feed the same
shared-MLP code: the 1x1 convs as GEMMs on channels_last memory, BatchNorm + ReLU as one bn_act,
the maximum over the ball by pcops_max_k.  The `npoint=None` (GroupAll) and `known=None` (expand)
branches are plain torch and run on any device.
"""
from typing import List

import torch
import torch.nn as nn

from . import model_utils, pointnet2_utils
from .batchnorm import run_sequential


def build_shared_mlp(mlp_spec: List[int], bn: bool = True):
    layers = []
    for i in range(1, len(mlp_spec)):
        layers.append(nn.Conv2d(mlp_spec[i - 1], mlp_spec[i], kernel_size=1, bias=not bn))
        if bn:
            layers.append(nn.BatchNorm2d(mlp_spec[i]))
        layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


def _shared_mlp(seq, x):
    """A build_shared_mlp stack on a channels_last (B,C,S,K) tensor."""
    from .svdformer import conv1x1

    return run_sequential(seq, x, conv1x1)


class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None

    def _run(self, xyz, features, features_t):
        from .svdformer import max_over_neighbours_tokens

        new_xyz = None
        if self.npoint is not None:
            fidx = pointnet2_utils.furthest_point_sample(xyz, self.npoint)     # one FPS for every scale
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), fidx)
            new_xyz = new_xyz.transpose(1, 2).contiguous()
        fused = (model_utils._PN2_FUSED and self.npoint is not None and xyz.is_cuda and not xyz.requires_grad)
        toks = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            if fused and grouper.use_xyz:
                if features_t is None and features is not None:
                    features_t = features.transpose(1, 2)
                rows, _ = model_utils.ball_group_rows(xyz, new_xyz, features_t, grouper.radius, grouper.nsample,
                                                      model_utils._rows_dtype())
                x = rows.permute(0, 3, 1, 2)
            else:
                if features is None and features_t is not None:
                    features = features_t.transpose(1, 2).contiguous()
                x = grouper(xyz, new_xyz, features).contiguous(memory_format=torch.channels_last)
            toks.append(max_over_neighbours_tokens(_shared_mlp(mlp, x)))      # (B, npoint, mlp[-1])
        return new_xyz, torch.cat(toks, dim=2)

    def forward(self, xyz, features):
        """xyz (B,N,3), features (B,C,N) or None -> new_xyz (B,npoint,3) (None when npoint is None),
        new_features (B, sum_k mlps[k][-1], npoint)."""
        new_xyz, tok = self._run(xyz, features, None)
        return new_xyz, tok.transpose(1, 2).contiguous()

    def forward_tokens(self, xyz, features_t):
        """xyz (B,N,3), features_t (B,N,C) or None -> new_xyz, new_features (B, npoint, sum_k mlps[k][-1])."""
        return self._run(xyz, None, features_t)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping (pointnet2_modules.py:77-115): one FPS, then per
    scale a ball query, the shared MLP and the maximum over the ball."""

    def __init__(self, npoint, radii, nsamples, mlps, bn=True, use_xyz=True):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz)
                                 if npoint is not None else pointnet2_utils.GroupAll(use_xyz))
            mlp_spec = mlps[i]
            if use_xyz:
                mlp_spec[0] += 3      # in place, as the reference does
            self.mlps.append(build_shared_mlp(mlp_spec, bn))


class PointnetSAModule(PointnetSAModuleMSG):
    """Single-scale set abstraction (pointnet2_modules.py:118-146)."""

    def __init__(self, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz)


class PointnetFPModule(nn.Module):
    """Feature propagation (pointnet2_modules.py:149-209)."""

    def __init__(self, mlp, bn=True):
        super().__init__()
        self.mlp = build_shared_mlp(mlp, bn=bn)

    def _run(self, unknown, known, unknow_feats, unknow_feats_t, known_feats, known_feats_t):
        cm = model_utils._cm
        if known is None:
            # the reference's expand branch: one known feature row for every unknown point
            kf = known_feats_t if known_feats_t is not None else known_feats.transpose(1, 2)
            tok = kf.expand(kf.shape[0], unknown.shape[1], kf.shape[2])
            uf = unknow_feats_t if unknow_feats_t is not None or unknow_feats is None else unknow_feats.transpose(1, 2)
            if uf is not None:
                tok = torch.cat([tok, uf], dim=2)
            tok = tok.contiguous()
        elif model_utils._fp_fused(unknown, known):
            uf = unknow_feats_t if unknow_feats_t is not None or unknow_feats is None else unknow_feats.transpose(1, 2)
            kf = known_feats_t if known_feats_t is not None else known_feats.transpose(1, 2)
            tok = model_utils.fp_interp_cl(unknown, known, uf, kf, 1, model_utils._rows_dtype())
        else:
            tok = model_utils.fp_interp_chain(unknown, known, cm(unknow_feats, unknow_feats_t),
                                              cm(known_feats, known_feats_t), 1)
        # (B,n,C) rows are the channels_last memory of the reference's (B,C,n,1) tensor
        x = _shared_mlp(self.mlp, tok.unsqueeze(2).permute(0, 3, 1, 2))
        return x.permute(0, 2, 3, 1).squeeze(2)

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B,n,3), known (B,m,3) or None, unknow_feats (B,C1,n) or None, known_feats (B,C2,m)
        -> (B, mlp[-1], n)."""
        return self._run(unknown, known, unknow_feats, None, known_feats, None).transpose(1, 2).contiguous()

    def forward_tokens(self, unknown, known, unknow_feats_t, known_feats_t):
        """Token-major features: unknow_feats_t (B,n,C1) or None, known_feats_t (B,m,C2) -> (B,n,mlp[-1])."""
        return self._run(unknown, known, None, unknow_feats_t, None, known_feats_t)
