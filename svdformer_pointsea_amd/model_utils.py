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
  nearest_distances(x, y)                               :288-297
  self_nearest_distances(x)                             :299-307
  self_nearest_distances_K(x, k=3)                      :309-321
  get_nearest_index(target, source, k=1, return_dis=False)   :501-521
  indexing_neighbor(x, index)                           :523-540
  nn_dist_raw (the fused scan's distances and indices, no autograd)   :288-321, 501-521
  square_distance / knn / get_graph_feature             :258-279, 911-943
  MLP / MLP_Res / PointNetFeatureExtractor              :45-60, 79-95, 631-805
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


# ---------------------------------------------------------------- neighbour distances
# PCOPS_NEIGHBOURS_FUSED=0: the reference's torch expressions (the *_chain functions) everywhere --
# A/B runs and the parity tests.  With the switch on, a call still takes the chain when its operands
# are not fp32 CUDA tensors, when C != 3, when K > NN_DIST_MAX_K or when B > NN_DIST_MAX_B.
_NEIGHBOURS_FUSED = os.environ.get("PCOPS_NEIGHBOURS_FUSED", "1") != "0"
NN_DIST_MAX_K = 64   # pcops_knn's list limit
NN_DIST_MAX_B = 65535   # the batch is the scan's grid.y


def _nn_check(q, p, k):
    if q.dim() != 3 or p.dim() != 3 or q.shape[0] != p.shape[0] or q.shape[1] != p.shape[1]:
        raise RuntimeError(f"neighbour distances: shape mismatch {tuple(q.shape)} vs {tuple(p.shape)}")
    if k > p.shape[2]:
        raise RuntimeError(f"selected index k out of range (k={k}, N={p.shape[2]})")


def _nn_fused(q, p, k):
    return (_NEIGHBOURS_FUSED and q.is_cuda and p.is_cuda and q.dtype == torch.float32 and p.dtype == torch.float32
            and q.shape[1] == 3 and 1 <= k <= NN_DIST_MAX_K and q.shape[0] <= NN_DIST_MAX_B)


def _nn_forward(q, p, k, form, self_diag, root):
    """pcops_nn_dist_forward on contiguous fp32 q (B,3,S), p (B,3,N) -> val (B,S) | (B,S,k), idx int32."""
    B, _, S = q.shape
    N = p.shape[2]
    if self_diag and S != N:
        raise RuntimeError(f"self_diag needs one cloud, got {S} and {N} points")
    val = torch.empty((B, S) if root else (B, S, k), dtype=torch.float32, device=q.device)
    idx = torch.empty(B, S, k, dtype=torch.int32, device=q.device)
    with torch.cuda.device(q.device):
        call("nn_dist_forward", lib().pcops_nn_dist_forward, ptr(q), ptr(p), B, S, N, k, 1 if form == "B" else 0,
             int(bool(self_diag)), int(bool(root)), ptr(idx), ptr(val), stream_of(q))
    return val, idx


def nn_dist_raw(q, p, k, form="A", self_diag=False):
    """The k smallest squared distances of every query, no autograd: q (B,3,S), p (B,3,N) fp32 on the GPU
    -> (distances (B,S,k) fp32, idx (B,S,k) int32) in ascending (distance, index) order.
    form "A": ((-2 dot) + |q|^2) + |p|^2 (nearest_distances, square_distance); "B": (|p|^2 + |q|^2) - 2 dot
    (get_nearest_index); self_diag adds 2 to the candidate whose index is the query's (S == N)."""
    if form not in ("A", "B"):
        raise ValueError(f"form must be 'A' or 'B', got {form!r}")
    _nn_check(q, p, k)
    q, p = q.detach().contiguous(), p.detach().contiguous()
    require_float(q, "q")
    require_float(p, "p")
    if q.shape[1] != 3 or k > NN_DIST_MAX_K:
        raise RuntimeError(f"nn_dist_raw: C == 3 and k <= {NN_DIST_MAX_K} only (C={q.shape[1]}, k={k})")
    return _nn_forward(q, p, k, form, self_diag, False)


class _NNDist(torch.autograd.Function):
    """pcops_nn_dist_forward / _backward.  p None: the cloud against itself (one gradient)."""

    @staticmethod
    def forward(ctx, q, p, k, form, self_diag, root):
        same = p is None
        q = q.contiguous()
        pc = q if same else p.contiguous()
        val, idx = _nn_forward(q, pc, k, form, self_diag, root)
        ctx.save_for_backward(q, pc, idx, val if root else None)
        ctx.cfg = (k, bool(self_diag), bool(root), same)
        ctx.mark_non_differentiable(idx)
        return val, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gidx):
        q, p, idx, val = ctx.saved_tensors
        k, self_diag, root, same = ctx.cfg
        B, _, S = q.shape
        N = p.shape[2]
        want_q = ctx.needs_input_grad[0] and not same
        want_p = ctx.needs_input_grad[0] if same else ctx.needs_input_grad[1]
        if not (want_q or want_p):
            return None, None, None, None, None, None
        g = g.float().contiguous()
        gq = torch.empty_like(q) if want_q else None
        gp = torch.empty_like(p) if want_p else None
        with torch.cuda.device(q.device):
            wsb = lib().pcops_nn_dist_backward_workspace_bytes(B, S, N, k, int(same)) if want_p else 0
            ws = Workspace.get(q.device, wsb) if wsb else None
            call("nn_dist_backward", lib().pcops_nn_dist_backward, ptr(q), ptr(p), ptr(idx), ptr(val), ptr(g), B, S, N,
                 k, int(self_diag), int(root), int(same), ptr(gq), ptr(gp), ptr(ws), wsb, stream_of(q))
        return (gp if same else gq), (None if same else gp), None, None, None, None


def square_distance(src, dst):
    """models/model_utils.py:258-279: src (B,N,C), dst (B,M,C) -> the (B,N,M) squared distances
    ((-2 src.dst) + |src|^2) + |dst|^2; the torch expression (a full matrix is what it returns)."""
    B, N, _ = src.shape
    _, M, _ = dst.shape
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist += torch.sum(src ** 2, -1).view(B, N, 1)
    dist += torch.sum(dst ** 2, -1).view(B, 1, M)
    return dist


def nearest_distances_chain(x, y):
    """models/model_utils.py:288-297, line for line."""
    inner = -2 * torch.matmul(x.transpose(2, 1), y)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    yy = torch.sum(y ** 2, dim=1, keepdim=True)
    pairwise_distance = xx.transpose(2, 1) + inner + yy
    return torch.sqrt(torch.min(pairwise_distance, dim=2, keepdim=True).values)


def self_nearest_distances_chain(x):
    """models/model_utils.py:299-307, line for line."""
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pairwise_distance = xx.transpose(2, 1) + inner + xx
    pairwise_distance += torch.eye(x.shape[2]).to(pairwise_distance.device) * 2
    return torch.sqrt(torch.min(pairwise_distance, dim=2, keepdim=True).values)


def self_nearest_distances_K_chain(x, k=3):
    """models/model_utils.py:309-321, line for line."""
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pairwise_distance = xx.transpose(2, 1) + inner + xx
    pairwise_distance += torch.eye(x.shape[2]).to(pairwise_distance.device) * 2
    pairwise_distance *= -1
    k_nearest_distance = pairwise_distance.topk(k=k, dim=2)[0]
    k_nearest_distance *= -1
    return torch.sqrt(torch.mean(k_nearest_distance, dim=2, keepdim=True))


def get_nearest_index_chain(target, source, k=1, return_dis=False):
    """models/model_utils.py:501-521, line for line."""
    inner = torch.bmm(target.transpose(1, 2), source)
    s_norm_2 = torch.sum(source ** 2, dim=1)
    t_norm_2 = torch.sum(target ** 2, dim=1)
    d_norm_2 = s_norm_2.unsqueeze(1) + t_norm_2.unsqueeze(2) - 2 * inner
    nearest_dis, nearest_index = torch.topk(d_norm_2, k=k, dim=-1, largest=False)
    if not return_dis:
        return nearest_index
    return nearest_index, nearest_dis


def indexing_neighbor_chain(x, index):
    """models/model_utils.py:523-540, line for line (the batch index on x's device)."""
    batch_size, num_points, k = index.size()
    id_0 = torch.arange(batch_size, device=x.device).view(-1, 1, 1)
    x = x.transpose(2, 1).contiguous()
    feature = x[id_0, index]
    return feature.permute(0, 3, 1, 2).contiguous()


def nearest_distances(x, y):
    """models/model_utils.py:288-297: x (B,3,N) queries, y (B,3,M) targets -> (B,N,1), the distance of every
    x point to its nearest y point: sqrt(min_j d_ij), d = ((-2 x.y) + |x|^2) + |y|^2 in torch's fp32 order.
    Differentiable in x and y.  On fp32 GPU clouds one libpcops scan (pcops_nn_dist_forward) without the
    (B,N,M) matrix: the minimum is the reference's bit for bit, the square root the correctly rounded one
    (torch's CPU sqrt is within 1 ulp of it), NaN where the minimum is negative; the gradient is
    deterministic (pcops_nn_dist_backward).  Anything else runs nearest_distances_chain."""
    _nn_check(x, y, 1)
    if not _nn_fused(x, y, 1):
        return nearest_distances_chain(x, y)
    return _NNDist.apply(x, y, 1, "A", False, True)[0].unsqueeze(2)


def self_nearest_distances(x):
    """models/model_utils.py:299-307: x (B,3,N) -> (B,N,1), sqrt of the row minimum of the cloud's own
    distance matrix with 2 ADDED on the diagonal (a point farther than sqrt(2) from every other keeps its
    own d_ii + 2, with gradient 0).  Fused path and fallbacks as nearest_distances."""
    _nn_check(x, x, 1)
    if not _nn_fused(x, x, 1):
        return self_nearest_distances_chain(x)
    return _NNDist.apply(x, None, 1, "A", True, True)[0].unsqueeze(2)


def self_nearest_distances_K(x, k=3):
    """models/model_utils.py:309-321: x (B,3,N) -> (B,N,1), sqrt(mean of the k smallest) of the same matrix.
    The fused path adds the k distances in rank order (torch.mean's order varies with k: within
    (k + 3) * 2^-24 relative of it on rows of positive terms)."""
    _nn_check(x, x, k)
    if not _nn_fused(x, x, k):
        return self_nearest_distances_K_chain(x, k)
    return _NNDist.apply(x, None, k, "A", True, True)[0].unsqueeze(2)


def get_nearest_index(target, source, k=1, return_dis=False):
    """models/model_utils.py:501-521: target (B,3,v1), source (B,3,v2) -> the k nearest source points of
    every target point, int64 (B,v1,k) (with return_dis: also their squared distances (B,v1,k),
    differentiable in both clouds).  d = (|s|^2 + |t|^2) - 2 t.s in torch's fp32 order; ascending
    (distance, index) -- torch.topk leaves the order of exact ties unspecified."""
    _nn_check(target, source, k)
    if not _nn_fused(target, source, k):
        return get_nearest_index_chain(target, source, k, return_dis)
    dis, idx = _NNDist.apply(target, source, k, "B", False, False)
    return (idx.long(), dis) if return_dis else idx.long()


def indexing_neighbor(x, index):
    """models/model_utils.py:523-540: x (B,C,N0), index (B,N,k) -> (B,C,N,k), x[b, :, index[b, n, j]].
    fp32 GPU features: grouping_operation; otherwise the reference's indexing."""
    if _NEIGHBOURS_FUSED and x.is_cuda and index.is_cuda and x.dtype == torch.float32:
        return grouping_operation(x.contiguous(), index.to(torch.int32).contiguous())
    return indexing_neighbor_chain(x, index)


def knn_chain(x, k):
    """models/model_utils.py:911-917, line for line."""
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pairwise_distance = -xx - inner - xx.transpose(2, 1)
    return pairwise_distance.topk(k=k, dim=-1)[1]


def knn(x, k):
    """models/model_utils.py:911-917: x (B,C,N) -> the k nearest points of every point (itself included),
    int64 (B,N,k).  On fp32 GPU features the libpcops search (_knn), which ranks by
    ((-2 dot) + |x_i|^2) + |x_j|^2 where the reference ranks by (inner + |x_j|^2) + |x_i|^2: the order can
    differ between candidates closer than an ulp of the distance, an order torch.topk leaves unspecified
    for exact ties anyway."""
    if not (_NEIGHBOURS_FUSED and x.is_cuda and x.dtype == torch.float32 and k <= NN_DIST_MAX_K):
        return knn_chain(x, k)
    pts = x.detach().transpose(1, 2).contiguous()
    return _knn(pts, pts, k).long()


def get_graph_feature(x, k=20, idx=None):
    """models/model_utils.py:919-943: the DGCNN graph feature [x_j - x_i, x_i] of the k nearest neighbours,
    x (B,C,N) -> (B,2C,N,k); on x's device (the reference hard-codes 'cuda')."""
    batch_size = x.size(0)
    num_points = x.size(2)
    x = x.view(batch_size, -1, num_points)
    if idx is None:
        idx = knn(x, k=k)
    k = idx.shape[2]
    feature = indexing_neighbor(x, idx)                       # (B,C,N,k): x_j
    centre = x.unsqueeze(3).repeat(1, 1, 1, k)
    return torch.cat((feature - centre, centre), dim=1).contiguous()


class MLP(nn.Module):
    """models/model_utils.py:45-60."""

    def __init__(self, in_channel, layer_dims, bn=None):
        super().__init__()
        layers = []
        last_channel = in_channel
        for out_channel in layer_dims[:-1]:
            layers.append(nn.Linear(last_channel, out_channel))
            if bn:
                layers.append(nn.BatchNorm1d(out_channel))
            layers.append(nn.ReLU())
            last_channel = out_channel
        layers.append(nn.Linear(last_channel, layer_dims[-1]))
        self.mlp = nn.Sequential(*layers)

    def forward(self, inputs):
        return self.mlp(inputs)


class MLP_Res(nn.Module):
    """models/model_utils.py:79-95: x (B,in_dim,n) -> (B,out_dim,n)."""

    def __init__(self, in_dim=128, hidden_dim=None, out_dim=128):
        super().__init__()
        if hidden_dim is None:
            hidden_dim = in_dim
        self.conv_1 = nn.Conv1d(in_dim, hidden_dim, 1)
        self.conv_2 = nn.Conv1d(hidden_dim, out_dim, 1)
        self.conv_shortcut = nn.Conv1d(in_dim, out_dim, 1)

    def forward(self, x):
        shortcut = self.conv_shortcut(x)
        return self.conv_2(torch.relu(self.conv_1(x))) + shortcut


class PointNetFeatureExtractor(nn.Module):
    """models/model_utils.py:631-805: the PointNet feature extractor (global, or per-point with the
    global feature repeated); x (B,N,D), or (B,D,N) with transposed_input."""

    def __init__(self, in_channels=3, feat_size=1024, layer_dims=[64, 128], global_feat=True,
                 activation=torch.nn.functional.relu, batchnorm=True, transposed_input=False):
        super().__init__()
        if not isinstance(in_channels, int):
            raise TypeError(f"Argument in_channels expected to be of type int. Got {type(in_channels)} instead.")
        if not isinstance(feat_size, int):
            raise TypeError(f"Argument feat_size expected to be of type int. Got {type(feat_size)} instead.")
        if not hasattr(layer_dims, "__iter__"):
            raise TypeError("Argument layer_dims is not iterable.")
        for i, layer_dim in enumerate(layer_dims):
            if not isinstance(layer_dim, int):
                raise TypeError(f"Elements of layer_dims must be of type int. Found type {type(layer_dim)} at index {i}.")
        if not isinstance(global_feat, bool):
            raise TypeError(f"Argument global_feat expected to be of type bool. Got {type(global_feat)} instead.")
        self.feat_size = feat_size
        self.activation = activation
        self.global_feat = global_feat
        dims = [in_channels] + list(layer_dims) + [feat_size]   # the caller's list is left as it is
        self.conv_layers = nn.ModuleList()
        if batchnorm:
            self.bn_layers = nn.ModuleList()
        for i in range(len(dims) - 1):
            self.conv_layers.append(nn.Conv1d(dims[i], dims[i + 1], 1))
            if batchnorm:
                self.bn_layers.append(nn.BatchNorm1d(dims[i + 1]))
        self.batchnorm = batchnorm
        self.transposed_input = transposed_input

    def _layer(self, i, x):
        x = self.conv_layers[i](x)
        return self.bn_layers[i](x) if self.batchnorm else x

    def forward(self, x):
        if not self.transposed_input:
            x = x.transpose(1, 2)
        num_points = x.shape[2]
        x = self.activation(self._layer(0, x))
        local_features = x if self.global_feat is False else None
        for i in range(1, len(self.conv_layers) - 1):
            x = self.activation(self._layer(i, x))
        x = self._layer(len(self.conv_layers) - 1, x)     # the last layer: no nonlinearity
        x = torch.max(x, 2, keepdim=True)[0]
        x = x.view(-1, self.feat_size)
        if self.global_feat:
            return x
        x = x.view(-1, self.feat_size, 1).repeat(1, 1, num_points)
        return torch.cat((x, local_features), dim=1)
