"""Hot-path pieces of models/model_utils.py (and models_PointSea/model_utils.py)
re-expressed on libpcops.so.  Names and signatures follow the reference so
its model classes can import them unchanged:

  query_knn(nsample, xyz, new_xyz, include_self=True)   model_utils.py:281-286
  query_knn_point(k, xyz, new_xyz)                      :807-810
  group_local(xyz, k=20, return_idx=False)              :812-826
  index_points(points, idx)                             :828-845
  fps_subsample(pcd, n_points=2048)                     :489-499
  sample_and_group_knn(xyz, points, npoint, k, ...)     :323-356
  sample_and_group_knn_cl (fused grouping, channels_last) :323-356 + the first conv's layout
  edge_features (EdgeConv's [x_i - x_j, x_i], channels_last) :812-845, 869-877
  Conv1d / sample_and_group / PointNet_SA_Module / PointNet_FP_Module   :9-25, 97-256
  ball_group_cl (fused ball query + grouping, channels_last) :97-130 + the first conv's layout
  fp_interp_cl (fused three-NN + weights + interpolation + skip concat, token-major) :243-253
  self_attention / cross_attention / SDG_Decoder        :542-629
  self_attention_woinp / SDG_Decoder_PointSea           models_PointSea/model_utils.py:463-509
  PCViews                                               :1179-1234
  batched_index_select / point_fea_img_fea / distribute_img_fea_points   :1119-1176
"""
import numpy as np
import os

import torch
from torch import nn

from . import _lib
from ._lib import Workspace, call, lib, ptr, require_float, stream_of
from .pointnet2_utils import furthest_point_sample, furthest_point_sample_counts, gather_operation, grouping_operation


def _knn(q, p, k, pad=0, want_dist=False):
    """K nearest of p for every row of q; q (B,S,C), p (B,N,C) fp32 on the GPU."""
    q = q.float().contiguous()  # distances are evaluated in fp32 (also under autocast)
    p = p.float().contiguous()
    require_float(q, "new_xyz")
    require_float(p, "xyz")
    B, S, C = q.shape
    N = p.shape[1]
    if p.shape[0] != B or p.shape[2] != C:
        raise RuntimeError(f"knn: shape mismatch {tuple(q.shape)} vs {tuple(p.shape)}")
    if k + pad > N:
        raise RuntimeError(f"selected index k out of range (k={k + pad}, N={N})")
    idx = torch.empty(B, S, k, dtype=torch.int32, device=q.device)
    dist = torch.empty(B, S, k, dtype=torch.float32, device=q.device) if want_dist else None
    with torch.cuda.device(q.device):
        wsb = lib().pcops_knn_workspace_bytes(B, S, N, C, k + pad) if _KNN_SORTED else 0
        # with scratch: C >= 32 by the streamed, candidate-split form (knnC3_kernel + merge),
        # the index-order scan's result bit for bit
        if wsb:
            ws = Workspace.get(q.device, wsb)
            call("knn", lib().pcops_knn_ws, ptr(q), ptr(p), B, S, N, C, k, pad, ptr(idx), ptr(dist), ptr(ws), wsb,
                 stream_of(q))
        else:
            call("knn", lib().pcops_knn, ptr(q), ptr(p), B, S, N, C, k, pad, ptr(idx), ptr(dist), stream_of(q))
    return (idx, dist) if want_dist else idx


_KNN_SORTED = os.environ.get("PCOPS_KNN_SORTED", "1") != "0"   # A/B switch: 0 = pcops_knn (no scratch)


def query_knn(nsample, xyz, new_xyz, include_self=True):
    """Find k-NN of new_xyz in xyz -> (B,S,nsample) int32 (model_utils.py:281-286)."""
    pad = 0 if include_self else 1
    return _knn(new_xyz, xyz, nsample, pad)


def query_knn_point(k, xyz, new_xyz):
    """(B,S,k) int64 like torch.topk (model_utils.py:807-810)."""
    return _knn(new_xyz, xyz, k).long()


def index_points(points, idx):
    """points (B,N,C), idx (B,S[,K]) -> (B,S[,K],C) (model_utils.py:828-845)."""
    B, N, C = points.shape
    shp = idx.shape
    idx3 = idx.reshape(B, -1, 1).to(torch.int32).contiguous()
    g = grouping_operation(points.transpose(1, 2).contiguous(), idx3)  # (B,C,S*K,1)
    return g.reshape(B, C, *shp[1:]).movedim(1, -1)


def group_local(xyz, k=20, return_idx=False):
    """xyz (B,C,N) -> (B,C,N,k) neighbour features (model_utils.py:812-826)."""
    xyz = xyz.contiguous()
    pts = xyz.transpose(2, 1).contiguous()
    idx32 = _knn(pts, pts, k)
    group_xyz = grouping_operation(xyz, idx32)
    if return_idx:
        return group_xyz, idx32.long()
    return group_xyz


def fps_subsample(pcd, n_points=2048):
    """pcd (B,N,3) -> (B,n_points,3) (model_utils.py:489-499)."""
    new_pcd = gather_operation(pcd.permute(0, 2, 1).contiguous(), furthest_point_sample(pcd.contiguous(), n_points))
    return new_pcd.permute(0, 2, 1).contiguous()


def fps_subsample_counts(pcd, counts, n_points=2048):
    """fps_subsample of zero-padded clouds whose valid rows are counts (B,) int32: the FPS sweep
    stops at each cloud's count (pointnet2_utils.furthest_point_sample_counts); the same points
    as fps_subsample of the padded buffer."""
    idx = furthest_point_sample_counts(pcd.contiguous(), counts, n_points)
    new_pcd = gather_operation(pcd.permute(0, 2, 1).contiguous(), idx)
    return new_pcd.permute(0, 2, 1).contiguous()


class _SAGroup(torch.autograd.Function):
    """pcops_sa_group: grouped (xyz - centre, points) rows in channels_last order."""

    @staticmethod
    def forward(ctx, xyz_t, new_xyz_t, points_t, idx, out_dtype):
        B, N, _ = xyz_t.shape
        S, K = idx.shape[1], idx.shape[2]
        C = 0 if points_t is None else points_t.shape[2]
        out = torch.empty(B, S, K, 3 + C, dtype=out_dtype, device=xyz_t.device)
        with torch.cuda.device(xyz_t.device):
            call("sa_group", lib().pcops_sa_group, ptr(xyz_t), ptr(new_xyz_t), ptr(points_t), ptr(idx), B, N, S, K, C,
                 ptr(out), 1 if out_dtype == torch.bfloat16 else 0, stream_of(xyz_t))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, S, K, C)
        ctx.mark_non_differentiable(idx)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, N, S, K, C = ctx.dims
        if C == 0 or not ctx.needs_input_grad[2]:
            return None, None, None, None, None
        g = g.contiguous()
        gp = torch.empty(B, N, C, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            call("sa_group_grad", lib().pcops_sa_group_grad, ptr(g), 1 if g.dtype == torch.bfloat16 else 0, ptr(idx),
                 B, N, S, K, C, ptr(gp), stream_of(g))
        return None, None, gp, None, None


class SharedFPS:
    """Furthest-point indices of one cloud computed once for two consumers.

    FPS is greedy: the first m indices of an FPS of M >= m points ARE the FPS of m points of the
    same cloud (every round depends only on the rounds before it; the tie rule, sampling_gpu.cu:
    69-173, depends on N, not on M).  The models sample the partial input twice -- the local
    encoder (SVDFormer.py:177, PointSea.py:241, local_points) and the point encoder's first SA
    module (model_utils.py:341, 512) -- so the FPS runs once, for the larger count, on the stream
    that produced it; `take(m)` hands the first m columns to another stream after an event wait
    (graph-capturable: the origin stream waits on a side stream's event)."""

    def __init__(self, idx):
        self.idx = idx
        self.event = self.stream = None
        if idx.is_cuda:
            self.stream = torch.cuda.current_stream(idx.device)
            self.event = torch.cuda.Event()
            self.event.record(self.stream)

    def take(self, m):
        if m > self.idx.shape[1]:
            raise ValueError(f"SharedFPS holds {self.idx.shape[1]} indices, {m} requested")
        if self.event is not None:
            cur = torch.cuda.current_stream(self.idx.device)
            # never on the producing stream itself: stream order suffices there, and under graph
            # capture a side stream waiting on its own event files itself in its own list of
            # parallel capture streams (HIP 7.0) -- the end-of-capture walk never returns (_lib.fork)
            if cur != self.stream:
                _lib.guarded_wait(cur, self.stream, event=self.event)
                self.idx.record_stream(cur)
        return self.idx if m == self.idx.shape[1] else self.idx[:, :m].contiguous()


def sample_and_group_knn_cl(xyz, points_t, npoint, k, out_dtype=torch.float32, fidx=None):
    """sample_and_group_knn (model_utils.py:323-356, use_xyz) in three launches --
    FPS, kNN, and ONE fused grouping (pcops_sa_group) that writes the
    neighbourhood features straight into the channels_last memory the first
    1x1 conv reads.  xyz (B,3,N) without gradient, points_t (B,N,C) token-major
    (or None) -> new_xyz (B,3,S), features (B,3+C,S,K) channels_last, idx."""
    xyz_t = xyz.transpose(1, 2).contiguous()
    fidx = furthest_point_sample(xyz_t, npoint) if fidx is None else fidx.take(npoint)
    new_xyz = gather_operation(xyz.contiguous(), fidx)                 # (B,3,S), the reference's new_xyz
    new_xyz_t = new_xyz.transpose(1, 2).contiguous()
    idx = query_knn(k, xyz_t, new_xyz_t)
    if points_t is not None:
        points_t = points_t.float().contiguous()
    feat = _SAGroup.apply(xyz_t, new_xyz_t, points_t, idx, out_dtype)  # (B,S,K,3+C)
    return new_xyz, feat.permute(0, 3, 1, 2), idx


def sample_and_group_knn(xyz, points, npoint, k, use_xyz=True, idx=None, fidx=None):
    """model_utils.py:323-356: FPS -> gather -> kNN -> group (xyz, points)."""
    xyz_flipped = xyz.permute(0, 2, 1).contiguous()
    new_xyz = gather_operation(xyz, furthest_point_sample(xyz_flipped, npoint) if fidx is None else fidx.take(npoint))
    if idx is None:
        idx = query_knn(k, xyz_flipped, new_xyz.permute(0, 2, 1).contiguous())
    grouped_xyz = grouping_operation(xyz, idx)
    grouped_xyz -= new_xyz.unsqueeze(3).repeat(1, 1, 1, k)
    if points is not None:
        grouped_points = grouping_operation(points, idx)
        new_points = torch.cat([grouped_xyz, grouped_points], 1) if use_xyz else grouped_points
    else:
        new_points = grouped_xyz
    return new_xyz, new_points, idx, grouped_xyz


class _EdgeGroup(torch.autograd.Function):
    """pcops_edge_group: EdgeConv's (x_i - x_j, x_i) rows in channels_last order."""

    @staticmethod
    def forward(ctx, x_t, idx, out_dtype):
        B, N, C = x_t.shape
        K = idx.shape[2]
        out = torch.empty(B, N, K, 2 * C, dtype=out_dtype, device=x_t.device)
        with torch.cuda.device(x_t.device):
            call("edge_group", lib().pcops_edge_group, ptr(x_t), ptr(idx), B, N, K, C, ptr(out),
                 1 if out_dtype == torch.bfloat16 else 0, stream_of(x_t))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, K, C)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, N, K, C = ctx.dims
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = g.contiguous()
        gx = torch.empty(B, N, C, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            call("edge_group_grad", lib().pcops_edge_group_grad, ptr(g), 1 if g.dtype == torch.bfloat16 else 0,
                 ptr(idx), B, N, K, C, ptr(gx), stream_of(g))
        return gx, None, None


def edge_features(x, k, out_dtype=None):
    """EdgeConv's edge features (model_utils.py:869-877): for the k feature-space
    nearest neighbours j of every point i (group_local, :812-826), the rows
    [x_i - x_j, x_i] -> (B, 2C, N, k) in channels_last memory, out_dtype (x's dtype
    by default; bf16 under autocast is what the first 1x1 conv would cast to).
    x (B, C, N).  Two launches: the kNN on the token-major fp32 cloud, then ONE
    pass (pcops_edge_group) that gathers, subtracts, concatenates and writes the
    conv's input layout -- in place of the grouping launch, repeat, subtract, cat
    and channels_last copy."""
    B, C, N = x.shape
    if out_dtype is None:
        out_dtype = x.dtype
    pts = x.float().transpose(1, 2).contiguous()   # (B, N, C) fp32: the kNN's operand and the gather source
    idx = _knn(pts.detach(), pts.detach(), k)
    return _EdgeGroup.apply(pts, idx, out_dtype).permute(0, 3, 1, 2)


# ------------------------------------------------------------------ PointNet++ SA / FP (radius path)
# PCOPS_PN2_FUSED=0: the SA / FP modules run the unfused chain of the existing ops (ball_query,
# grouping_operation, three_nn, three_interpolate, torch glue) -- A/B runs and the parity tests
_PN2_FUSED = os.environ.get("PCOPS_PN2_FUSED", "1") != "0"
BALL_GROUP_MAX_K = 1024   # pcops_ball_group's index slots per wave


def _cm(a, a_t):
    """The channel-major (B,C,N) form of a tensor given channel-major or token-major (or neither)."""
    return a if a is not None else (None if a_t is None else a_t.transpose(1, 2))


def _rows_dtype():
    return torch.bfloat16 if torch.is_autocast_enabled("cuda") else torch.float32


class _BallGroup(torch.autograd.Function):
    """pcops_ball_group: ball query and the grouped (xyz - centre, points) rows in one launch."""

    @staticmethod
    def forward(ctx, xyz_t, new_xyz_t, points_t, radius, K, out_dtype):
        B, N, _ = xyz_t.shape
        S = new_xyz_t.shape[1]
        C = 0 if points_t is None else points_t.shape[2]
        out = torch.empty(B, S, K, 3 + C, dtype=out_dtype, device=xyz_t.device)
        idx = torch.empty(B, S, K, dtype=torch.int32, device=xyz_t.device)
        with torch.cuda.device(xyz_t.device):
            call("ball_group", lib().pcops_ball_group, ptr(xyz_t), ptr(new_xyz_t), ptr(points_t), B, N, S, K, C,
                 float(radius), ptr(idx), ptr(out), 1 if out_dtype == torch.bfloat16 else 0, stream_of(xyz_t))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, S, K, C)
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, g, _gidx):
        (idx,) = ctx.saved_tensors
        B, N, S, K, C = ctx.dims
        if C == 0 or not ctx.needs_input_grad[2]:
            return None, None, None, None, None, None
        g = g.contiguous()
        gp = torch.empty(B, N, C, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            call("sa_group_grad", lib().pcops_sa_group_grad, ptr(g), 1 if g.dtype == torch.bfloat16 else 0, ptr(idx),
                 B, N, S, K, C, ptr(gp), stream_of(g))
        return None, None, gp, None, None, None


def ball_group_rows(xyz_t, new_xyz_t, points_t, radius, nsample, out_dtype=torch.float32):
    """Ball query around new_xyz_t (B,S,3) in xyz_t (B,N,3) and the grouped rows
    [xyz[idx] - centre, points_t[idx]] -> rows (B,S,K,3+C) in out_dtype, idx (B,S,K) int32: ONE
    launch (pcops_ball_group); an nsample beyond BALL_GROUP_MAX_K runs ball_query + pcops_sa_group,
    the same rows.  Coordinates carry no gradient (as sample_and_group_knn_cl); points_t does."""
    from .pointnet2_utils import ball_query

    xyz_t = xyz_t.detach().float().contiguous()
    new_xyz_t = new_xyz_t.detach().float().contiguous()
    require_float(xyz_t, "xyz")
    require_float(new_xyz_t, "new_xyz")
    if points_t is not None:
        points_t = points_t.float().contiguous()
    nsample = int(nsample)
    if nsample > BALL_GROUP_MAX_K:
        idx = ball_query(radius, nsample, xyz_t, new_xyz_t)
        return _SAGroup.apply(xyz_t, new_xyz_t, points_t, idx, out_dtype), idx
    return _BallGroup.apply(xyz_t, new_xyz_t, points_t, radius, nsample, out_dtype)


def ball_group_cl(xyz, points_t, npoint, nsample, radius, out_dtype=torch.float32, fidx=None):
    """sample_and_group (model_utils.py:97-130, use_xyz) in two launches after the FPS gather's --
    FPS, gather, and ONE pcops_ball_group that searches the ball and writes the neighbourhood rows
    into the channels_last memory the first 1x1 conv reads.  xyz (B,3,N) without gradient,
    points_t (B,N,C) token-major (or None) -> new_xyz (B,3,S), features (B,3+C,S,K) channels_last,
    idx (B,S,K).  The radius twin of sample_and_group_knn_cl."""
    xyz_t = xyz.transpose(1, 2).contiguous()
    fidx = furthest_point_sample(xyz_t, npoint) if fidx is None else fidx.take(npoint)
    new_xyz = gather_operation(xyz.contiguous(), fidx)                 # (B,3,S), the reference's new_xyz
    rows, idx = ball_group_rows(xyz_t, new_xyz.transpose(1, 2), points_t, radius, nsample, out_dtype)
    return new_xyz, rows.permute(0, 3, 1, 2), idx


def sample_and_group(xyz, points, npoint, nsample, radius, use_xyz=True):
    """model_utils.py:97-130: FPS -> gather -> ball query -> group (xyz, points); the unfused chain.
    xyz (B,3,N), points (B,f,N) -> new_xyz (B,3,npoint), new_points (B, 3 | f+3 | f, npoint, nsample),
    idx (B,npoint,nsample), grouped_xyz (B,3,npoint,nsample)."""
    from .pointnet2_utils import ball_query

    xyz_flipped = xyz.permute(0, 2, 1).contiguous()
    new_xyz = gather_operation(xyz, furthest_point_sample(xyz_flipped, npoint))
    idx = ball_query(radius, nsample, xyz_flipped, new_xyz.permute(0, 2, 1).contiguous())
    grouped_xyz = grouping_operation(xyz, idx)
    grouped_xyz -= new_xyz.unsqueeze(3).repeat(1, 1, 1, nsample)
    if points is not None:
        grouped_points = grouping_operation(points, idx)
        new_points = torch.cat([grouped_xyz, grouped_points], 1) if use_xyz else grouped_points
    else:
        new_points = grouped_xyz
    return new_xyz, new_points, idx, grouped_xyz


class _FPInterp(torch.autograd.Function):
    """pcops_fp_interp_forward / _backward: three-NN, weights, interpolation and the skip concat."""

    @staticmethod
    def forward(ctx, unknown_t, known_t, points2_t, points1_t, mode, out_dtype):
        B, N, _ = unknown_t.shape
        M, C2 = known_t.shape[1], points2_t.shape[2]
        C1 = 0 if points1_t is None else points1_t.shape[2]
        dev = unknown_t.device
        out = torch.empty(B, N, C2 + C1, dtype=out_dtype, device=dev)
        idx = torch.empty(B, N, 3, dtype=torch.int32, device=dev)
        weight = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("fp_interp_forward", lib().pcops_fp_interp_forward, ptr(unknown_t), ptr(known_t), ptr(points2_t),
                 ptr(points1_t), B, N, M, C2, C1, int(mode), ptr(idx), ptr(weight), ptr(out),
                 1 if out_dtype == torch.bfloat16 else 0, stream_of(unknown_t))
        ctx.save_for_backward(idx, weight)
        ctx.dims = (B, N, M, C2, C1)
        ctx.mark_non_differentiable(idx, weight)
        return out, idx, weight

    @staticmethod
    def backward(ctx, g, _gidx, _gweight):
        idx, weight = ctx.saved_tensors
        B, N, M, C2, C1 = ctx.dims
        g = g.contiguous()
        gp2 = gp1 = None
        if ctx.needs_input_grad[2]:
            gp2 = torch.empty(B, M, C2, dtype=torch.float32, device=g.device)
            with torch.cuda.device(g.device):
                call("fp_interp_backward", lib().pcops_fp_interp_backward, ptr(g), 1 if g.dtype == torch.bfloat16 else 0,
                     ptr(idx), ptr(weight), B, N, M, C2, C2 + C1, ptr(gp2), stream_of(g))
        if C1 and ctx.needs_input_grad[3]:
            gp1 = g[..., C2:].float()   # the skip gradient: the trailing column slice
        return None, None, gp2, gp1, None, None


def fp_interp_cl(unknown_t, known_t, points1_t, points2_t, mode=0, out_dtype=torch.float32, return_weights=False):
    """Feature propagation up to the MLP in ONE launch (pcops_fp_interp_forward): the three nearest
    known points of every unknown point, the inverse-distance weights (mode 0: model_utils.py:244-247,
    mode 1: pointnet2_modules.py:187-189), the interpolated points2_t rows and the skip features
    points1_t, token-major.  unknown_t (B,N,3), known_t (B,M,3) without gradient, points2_t (B,M,C2),
    points1_t (B,N,C1) or None -> (B,N,C2+C1) in out_dtype (with return_weights: also idx, weight)."""
    unknown_t = unknown_t.detach().float().contiguous()
    known_t = known_t.detach().float().contiguous()
    require_float(unknown_t, "unknowns")
    require_float(known_t, "knows")
    points2_t = points2_t.float().contiguous()
    if points1_t is not None:
        points1_t = points1_t.float().contiguous()
    out, idx, weight = _FPInterp.apply(unknown_t, known_t, points2_t, points1_t, mode, out_dtype)
    return (out, idx, weight) if return_weights else out


def fp_interp_chain(unknown_t, known_t, points1, points2, mode=0):
    """The same rows by the existing ops: three_nn, the weight arithmetic in torch, three_interpolate,
    torch.cat and the token-major copy.  points1 (B,C1,N) or None, points2 (B,C2,M) channel-major."""
    from .pointnet2_utils import three_interpolate, three_nn

    dist, idx = three_nn(unknown_t.contiguous(), known_t.contiguous())
    if mode == 0:
        recip = 1.0 / torch.clamp_min(dist, 1e-10)
        weight = recip / torch.sum(recip, 2, keepdim=True).repeat((1, 1, 3))
    else:
        recip = 1.0 / (dist + 1e-8)
        weight = recip / torch.sum(recip, dim=2, keepdim=True)
    new_points = three_interpolate(points2.contiguous(), idx, weight)
    if points1 is not None:
        new_points = torch.cat([new_points, points1], 1)
    return new_points.transpose(1, 2).contiguous()


def _fp_fused(unknown_t, known_t):
    return (_PN2_FUSED and unknown_t.is_cuda and not unknown_t.requires_grad and known_t is not None
            and not known_t.requires_grad and known_t.shape[1] >= 1)


class Conv1d(nn.Module):
    """model_utils.py:9-25: Conv1d -> BatchNorm1d -> activation on (B,C,N).  forward_tokens runs the
    same layer on token-major (B,N,C) rows: the kernel-size-1 conv as a GEMM, the BatchNorm over the
    (B*N, C) rows; forward is forward_tokens between two transposes."""

    def __init__(self, in_channel, out_channel, kernel_size=1, stride=1, if_bn=True, activation_fn=torch.relu):
        super().__init__()
        self.conv = nn.Conv1d(in_channel, out_channel, kernel_size, stride=stride)
        self.if_bn = if_bn
        self.bn = nn.BatchNorm1d(out_channel)
        self.activation_fn = activation_fn

    def _pointwise(self):
        return self.conv.kernel_size == (1,) and self.conv.stride == (1,)

    def forward_tokens(self, x):
        from .attention import linear

        if not self._pointwise():
            return self.forward(x.transpose(1, 2)).transpose(1, 2)
        out = linear(x, self.conv.weight.view(self.conv.out_channels, -1), self.conv.bias)
        if self.if_bn:
            out = self.bn(out.reshape(-1, out.shape[-1])).view(out.shape)
        if self.activation_fn is not None:
            out = self.activation_fn(out)
        return out

    def forward(self, x):
        if self._pointwise():
            return self.forward_tokens(x.transpose(1, 2)).transpose(1, 2)
        out = self.conv(x)
        if self.if_bn:
            out = self.bn(out)
        if self.activation_fn is not None:
            out = self.activation_fn(out)
        return out


class PointNet_SA_Module(nn.Module):
    """model_utils.py:161-207: FPS -> ball query -> group -> shared MLP -> max over the ball.
    forward keeps the reference's layouts; forward_tokens takes and returns token-major tensors
    (xyz_t (B,N,3), points_t (B,N,f) -> new_xyz_t (B,S,3), features (B,S,mlp[-1])).  On the GPU,
    with use_xyz and coordinates that need no gradient, the grouping is one pcops_ball_group launch
    (ball_group_cl); PCOPS_PN2_FUSED=0, or any other case, runs sample_and_group.  Both feed the
    same MLP and max code."""

    def __init__(self, npoint, nsample, radius, in_channel, mlp, if_bn=True, group_all=False, use_xyz=True):
        super().__init__()
        from .svdformer import Conv2d

        self.npoint, self.nsample, self.radius, self.mlp = npoint, nsample, radius, mlp
        self.group_all, self.use_xyz = group_all, use_xyz
        if use_xyz:
            in_channel += 3
        last = in_channel
        convs = []
        for out_channel in mlp:
            convs.append(Conv2d(last, out_channel, if_bn=if_bn))
            last = out_channel
        self.mlp_conv = nn.Sequential(*convs)

    def _run(self, xyz, xyz_t, points, points_t):
        from .svdformer import max_over_neighbours_tokens, sample_and_group_all

        xyz = _cm(xyz, xyz_t)
        if self.group_all:
            new_xyz, new_points, _, _ = sample_and_group_all(xyz, _cm(points, points_t), self.use_xyz)
        elif _PN2_FUSED and self.use_xyz and xyz.is_cuda and not xyz.requires_grad:
            if points_t is None and points is not None:
                points_t = points.transpose(1, 2)
            new_xyz, new_points, _ = ball_group_cl(xyz, points_t, self.npoint, self.nsample, self.radius,
                                                   _rows_dtype())
        else:
            points = _cm(points, points_t)
            new_xyz, new_points, _, _ = sample_and_group(xyz.contiguous(), None if points is None else points.contiguous(),
                                                         self.npoint, self.nsample, self.radius, self.use_xyz)
        new_points = self.mlp_conv(new_points.contiguous(memory_format=torch.channels_last))
        return new_xyz, max_over_neighbours_tokens(new_points)

    def forward(self, xyz, points):
        """xyz (B,3,N), points (B,f,N) -> new_xyz (B,3,npoint), new_points (B,mlp[-1],npoint)."""
        new_xyz, tok = self._run(xyz, None, points, None)
        return new_xyz, tok.transpose(1, 2).contiguous()

    def forward_tokens(self, xyz_t, points_t):
        new_xyz, tok = self._run(None, xyz_t, None, points_t)
        return new_xyz.transpose(1, 2).contiguous(), tok


class PointNet_FP_Module(nn.Module):
    """model_utils.py:209-256: three-NN inverse-distance interpolation of points2 onto xyz1, concat
    with points1, shared MLP.  forward keeps the reference's (B,C,N) layouts; forward_tokens takes
    xyz1_t (B,N,3), xyz2_t (B,M,3), points1_t (B,N,C1), points2_t (B,M,C2) and returns (B,N,mlp[-1]).
    On the GPU the interpolation and the concat are one pcops_fp_interp_forward launch
    (fp_interp_cl); PCOPS_PN2_FUSED=0, or coordinates that need a gradient, run fp_interp_chain."""

    def __init__(self, in_channel, mlp, use_points1=False, in_channel_points1=None, if_bn=True):
        super().__init__()
        self.use_points1 = use_points1
        if use_points1:
            in_channel += in_channel_points1
        last = in_channel
        convs = []
        for out_channel in mlp:
            convs.append(Conv1d(last, out_channel, if_bn=if_bn))
            last = out_channel
        self.mlp_conv = nn.Sequential(*convs)

    def _run(self, xyz1_t, xyz2_t, points1, points1_t, points2, points2_t):
        if not self.use_points1:
            points1 = points1_t = None
        if _fp_fused(xyz1_t, xyz2_t):
            p1 = points1_t if points1_t is not None or points1 is None else points1.transpose(1, 2)
            p2 = points2_t if points2_t is not None else points2.transpose(1, 2)
            tok = fp_interp_cl(xyz1_t, xyz2_t, p1, p2, 0, _rows_dtype())
        else:
            tok = fp_interp_chain(xyz1_t, xyz2_t, _cm(points1, points1_t), _cm(points2, points2_t), 0)
        for layer in self.mlp_conv:
            tok = layer.forward_tokens(tok)
        return tok

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 (B,3,N), xyz2 (B,3,M), points1 (B,C1,N), points2 (B,C2,M) -> (B,mlp[-1],N)."""
        tok = self._run(xyz1.permute(0, 2, 1).contiguous(), xyz2.permute(0, 2, 1).contiguous(), points1, None,
                        points2, None)
        return tok.transpose(1, 2).contiguous()

    def forward_tokens(self, xyz1_t, xyz2_t, points1_t, points2_t):
        return self._run(xyz1_t, xyz2_t, None, points1_t, None, points2_t)


# ---------------------------------------------------------------- point <-> pixel feature exchange
_COORD_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}


def batched_index_select(inp, dim, index):
    """models/model_utils.py:1119-1131: inp (B, *, ..., *), 0 < dim, index (B, M) -> inp gathered along
    `dim` with the same M indices for every other axis."""
    views = [inp.shape[0]] + [1 if i != dim else -1 for i in range(1, len(inp.shape))]
    expanse = list(inp.shape)
    expanse[0] = -1
    expanse[dim] = -1
    return torch.gather(inp, dim, index.view(views).expand(expanse))


def _coord_mask(coord, P):
    """The reference's mask (:1145-1146, :1167-1168) and the integer pixels with the rejected ones at 0."""
    mask = (coord >= 0) * (coord <= P - 1)
    return mask, torch.where(mask, coord, torch.zeros_like(coord)).long()


def point_fea_img_fea_chain(point_fea, point_coo, h, w):
    """The reference's expression (:1145-1152) without its in-place writes; torch ops, any device."""
    mask, pix = _coord_mask(point_coo, h * w)
    fea = torch.where(mask.unsqueeze(-1), point_fea, torch.zeros_like(point_fea))
    bs, _, fs = fea.shape
    return torch.zeros([bs, h * w, fs], device=fea.device, dtype=fea.dtype).scatter_add(
        1, pix.unsqueeze(2).repeat([1, 1, fs]), fea)


def distribute_img_fea_points_chain(img_fea, point_coord):
    """The reference's expression (:1164-1175); torch ops, any device."""
    B, C, H, W = list(img_fea.size())
    rows = img_fea.permute(0, 2, 3, 1).reshape([B, H * W, C])
    mask, pix = _coord_mask(point_coord, H * W)
    fea = batched_index_select(inp=rows, dim=1, index=pix)
    return torch.where(mask.unsqueeze(-1), fea, torch.zeros_like(fea))


def _image_strides(t):
    """(B,C,H,W) dense in NCHW or channels_last -> element strides (batch, pixel, channel), else None."""
    B, C, H, W = t.shape
    if t.is_contiguous():
        return C * H * W, 1, H * W
    if t.is_contiguous(memory_format=torch.channels_last):
        return C * H * W, C, 1
    return None


def pixel_gather(img, strides, C, coord, P, out=None):
    """pcops_pixel_gather: image side `img` of C channels addressed by element `strides` (batch, pixel,
    channel), coord (B,N) -> (B,N,C)."""
    B, N = coord.shape
    out = torch.empty(B, N, C, device=coord.device) if out is None else out
    with torch.cuda.device(coord.device):
        call("pixel_gather", lib().pcops_pixel_gather, ptr(img), ptr(coord), _COORD_DTYPES[coord.dtype], B, N, C, P,
             strides[0], strides[1], strides[2], ptr(out), stream_of(coord))
    return out


def pixel_splat(fea, coord, P, strides, out):
    """pcops_pixel_splat: fea (B,N,C) contiguous, coord (B,N) -> `out`, whose image side is addressed by
    element `strides` (batch, pixel, channel); the ordered (bitwise reproducible) scatter-sum."""
    B, N, C = fea.shape
    wsb = lib().pcops_pixel_splat_workspace_bytes(B, N, P)
    ws = Workspace.get(fea.device, wsb)
    with torch.cuda.device(fea.device):
        call("pixel_splat", lib().pcops_pixel_splat, ptr(fea), ptr(coord), _COORD_DTYPES[coord.dtype], B, N, C, P,
             ptr(out), strides[0], strides[1], strides[2], ptr(ws), wsb, stream_of(fea))
    return out


class _PixelSplat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fea, coord, P):
        B, N, C = fea.shape
        ctx.save_for_backward(coord)
        ctx.P = P
        return pixel_splat(fea.contiguous(), coord, P, (P * C, C, 1), torch.empty(B, P, C, device=fea.device))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (coord,) = ctx.saved_tensors
        g = g.contiguous()
        C = g.shape[2]
        return pixel_gather(g, (ctx.P * C, C, 1), C, coord, ctx.P), None, None


class _PixelGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, coord):
        B, C, H, W = img.shape
        ctx.save_for_backward(coord)
        ctx.cl = not img.is_contiguous()
        ctx.shape = img.shape
        return pixel_gather(img, _image_strides(img), C, coord, H * W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (coord,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        # the gradient in the input's memory format, written in place by the splat's sum pass
        gi = torch.empty(ctx.shape, device=g.device,
                         memory_format=torch.channels_last if ctx.cl else torch.contiguous_format)
        pixel_splat(g.contiguous(), coord, H * W, _image_strides(gi), gi)
        return gi, None


def _exchange_fused(fea, coord):
    from .render import viewops_fused

    return (viewops_fused() and fea.is_cuda and coord.is_cuda and fea.dtype == torch.float32
            and coord.dtype in _COORD_DTYPES)


def point_fea_img_fea(point_fea, point_coo, h, w):
    """models/model_utils.py:1134-1154: splat per-point features into an h x w plane.
    point_fea (B,N,C), point_coo (B,N), each coordinate x*w + y -> (B, h*w, C); differentiable in point_fea.

    A coordinate c takes part iff 0 <= c <= h*w - 1 and lands on the pixel trunc(c); negative values,
    >= h*w, NaN and +-inf contribute nothing.  On fp32 GPU tensors this is one ordered libpcops scatter-sum
    (pcops_pixel_splat): each output element is the fp32 sum of its terms in ascending point index, bitwise
    reproducible and equal to the reference's scatter_add run sequentially.  Other dtypes, CPU tensors and
    PCOPS_VIEWOPS_FUSED=0 run the reference's torch chain.

    Deliberate deviations from the reference: the inputs are NOT modified (the reference zeroes the rejected
    entries of the caller's point_fea and point_coo in place); a rejected point adds nothing (the reference
    adds 0 * fea to pixel 0, which differs only for a non-finite fea); integer coordinate dtypes are accepted
    (the reference's in-place `*= mask.float()` raises on them)."""
    assert len(point_fea.shape) == 3
    assert len(point_coo.shape) == 2
    assert point_fea.shape[0:2] == point_coo.shape
    if not _exchange_fused(point_fea, point_coo):
        return point_fea_img_fea_chain(point_fea, point_coo, h, w)
    return _PixelSplat.apply(point_fea, point_coo.detach().contiguous(), h * w)


def distribute_img_fea_points(img_fea, point_coord):
    """models/model_utils.py:1157-1176: read image features back at the points.
    img_fea (B,C,H,W), point_coord (B,N), each coordinate x*W + y -> (B,N,C), 0 for a point whose
    coordinate is outside the image; differentiable in img_fea.

    The index rule is point_fea_img_fea's.  On fp32 GPU tensors this is one libpcops row gather
    (pcops_pixel_gather) that reads an NCHW or channels_last map in place, and its gradient is the ordered
    scatter-sum written directly in the map's memory format.  Other dtypes, CPU tensors, maps dense in
    neither format and PCOPS_VIEWOPS_FUSED=0 run the reference's torch chain.

    Deliberate deviation from the reference: a rejected point reads 0 (the reference reads
    0 * img[pixel 0], which differs only when that pixel is non-finite); the inputs are not modified."""
    if not _exchange_fused(img_fea, point_coord) or _image_strides(img_fea) is None:
        return distribute_img_fea_points_chain(img_fea, point_coord)
    return _PixelGather.apply(img_fea, point_coord.detach().contiguous())
