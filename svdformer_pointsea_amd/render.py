"""Depth renderers on libpcops.so.

PCViews       <- models/model_utils.py:1179-1234 (SVDFormer; harmonic-mean depth splat)
PCViews_Real  <- models_PointSea/mv_utils_zs.py:136-195 (PointSea; voxel scatter-max,
                 7x7 max-pool, 3x3 Gaussian, max over depth, normalise)
The view rotation matrices are built exactly as the reference builds them
(euler2mat in torch float32, transposed); they are computed on the host CPU so
the product path does not depend on the device's sin/cos.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, lib, ptr, require_float, stream_of

# PCOPS_VIEWOPS_FUSED=0: the differentiable get_img and the point/pixel exchange ops of model_utils run the
# reference's op chain in torch instead of the libpcops kernels (A/B runs, parity tests)
_FUSED_ENV = "PCOPS_VIEWOPS_FUSED"


def viewops_fused():
    return os.environ.get(_FUSED_ENV, "1") != "0"


def euler2mat(angle):
    """models/model_utils.py:952-1001 (also mv_utils_zs.py:46-94): [b,3] -> [b,3,3]."""
    x, y, z = angle[:, 0], angle[:, 1], angle[:, 2]
    b = angle.shape[0]
    cosz, sinz = torch.cos(z), torch.sin(z)
    zero = z.detach() * 0
    one = zero.detach() + 1
    zmat = torch.stack([cosz, -sinz, zero, sinz, cosz, zero, zero, zero, one], dim=1).reshape(b, 3, 3)
    cosy, siny = torch.cos(y), torch.sin(y)
    ymat = torch.stack([cosy, zero, siny, zero, one, zero, -siny, zero, cosy], dim=1).reshape(b, 3, 3)
    cosx, sinx = torch.cos(x), torch.sin(x)
    xmat = torch.stack([one, zero, zero, zero, cosx, -sinx, zero, sinx, cosx], dim=1).reshape(b, 3, 3)
    return xmat @ ymat @ zmat


class PCViews:
    """Three fixed views; get_img(points (B,N,3)) -> (B*3, R, R) depth images."""

    def __init__(self, TRANS, RESOLUTION):
        _views = np.asarray([
            [[0 * np.pi / 2, 0, np.pi / 2], [0, 0, TRANS]],
            [[1 * np.pi / 2, 0, np.pi / 2], [0, 0, TRANS]],
            [[0, -np.pi / 2, np.pi / 2], [0, 0, TRANS]]])
        self.num_views = 3
        angle = torch.tensor(_views[:, 0, :]).float()
        self.rot_mat = euler2mat(angle).transpose(1, 2).contiguous()
        self.translation = torch.tensor(_views[:, 1, :]).float().contiguous()
        self.resolution = RESOLUTION
        self._dev = {}

    def _consts(self, device):
        if device not in self._dev:
            self._dev[device] = (self.rot_mat.to(device), self.translation.to(device))
        return self._dev[device]

    def get_img(self, points):
        """Depth images of the three views.  When `points` needs a gradient the image is attached to the
        graph (the reference's get_img is differentiable through the depth; the pixel coordinates pass
        through ceil); otherwise this is the forward-only pass on the shared workspace."""
        if points.requires_grad and torch.is_grad_enabled():
            rot, trans = self._consts(points.device)
            if not (viewops_fused() and points.is_cuda and points.dtype == torch.float32):
                return points2depth_chain(points, rot, trans, self.resolution)
            return _Points2Depth.apply(points, rot, trans, self.resolution)
        points = points.detach().contiguous()
        require_float(points, "points")
        B, N, _ = points.shape
        V, R = self.num_views, self.resolution
        rot, trans = self._consts(points.device)
        img = torch.empty(B * V, R, R, device=points.device)
        wsb = lib().pcops_points2depth_workspace_bytes(B, V, R, R)
        ws = _lib.Workspace.get(points.device, wsb)
        with torch.cuda.device(points.device):
            call("points2depth", lib().pcops_points2depth, ptr(points), ptr(rot), ptr(trans), B, N, V, R, R, ptr(img),
                 ptr(ws), wsb, stream_of(points))
        return img

    def project(self, points):
        """(B,N,3) -> (B*3, N) int64: the pixel ex*R + ey get_img adds each point to in each view, -1 where
        it rejects the point (off canvas, or behind the camera).  The coordinates point_fea_img_fea and
        distribute_img_fea_points take, for these views."""
        points = points.detach().contiguous()
        if not (viewops_fused() and points.is_cuda and points.dtype == torch.float32):
            return points2pixel_chain(points, *self._consts(points.device), self.resolution)
        require_float(points, "points")
        B, N, _ = points.shape
        V, R = self.num_views, self.resolution
        rot, trans = self._consts(points.device)
        pix = torch.empty(B * V, N, dtype=torch.int64, device=points.device)
        with torch.cuda.device(points.device):
            call("points2pixel", lib().pcops_points2pixel, ptr(points), ptr(rot), ptr(trans), B, N, V, R, R, ptr(pix),
                 stream_of(points))
        return pix


def _project_chain(points, rot, trans, R):
    """point_transform (:1223-1234) and the projection of points2depth / distribute (:1093-1100, :1025-1041,
    size 1) in the reference's op order -> depth, ex, ey, mask, each (B*V, N)."""
    b, v = points.shape[0], rot.shape[0]
    p = torch.matmul(torch.repeat_interleave(points, v, dim=0), rot.repeat(b, 1, 1))
    p = p - trans.unsqueeze(1).repeat(b, 1, 1)
    eps = torch.tensor([1e-12], device=points.device)
    depth = p[:, :, 2]
    coord_x = (p[:, :, 0] / (depth + eps)) * (R / R)
    coord_y = p[:, :, 1] / (depth + eps)
    _x = ((coord_x + 1) * R) / 2
    _y = ((coord_y + 1) * R) / 2
    ex = (_x + -0.5).ceil()
    ey = (_y + -0.5).ceil()
    mask = (ex >= 0) * (ex <= R - 1) * (ey >= 0) * (ey <= R - 1) * (depth >= 0)
    return depth, ex, ey, mask


def points2depth_chain(points, rot, trans, R):
    """PCViews.get_img as the reference writes it (models/model_utils.py:1196-1234 -> points2depth
    :1080-1115 -> distribute :1004-1077 with size_x = size_y = 1), in torch ops and in its op order:
    points (B,N,3), rot (V,3,3) as stored (transposed), trans (V,3) -> (B*V, R, R).  Works on CPU and GPU
    tensors and differentiates through autograd; the baseline the kernels are compared with."""
    depth, ex, ey, mask = _project_chain(points, rot, trans, R)
    bv = depth.shape[0]
    eps = torch.tensor([1e-12], device=points.device)
    # a rejected pair adds weight 0 at pixel 0 (the reference adds 0 at its wrapped pixel, and turns a
    # non-finite pixel -- z + eps == 0 -- into an index); every kept pair is the reference's term at its pixel
    weight = torch.where(mask, 1 / (depth + eps), torch.zeros_like(depth))
    weighted = torch.where(mask, depth * weight, torch.zeros_like(depth))
    coords = torch.where(mask, ex * R + ey, torch.zeros_like(ex)).long()
    wsum = torch.zeros([bv, R * R], device=points.device).scatter_add(1, coords, weight)
    wsum = wsum + (wsum == 0.0).float()
    vsum = torch.zeros([bv, R * R], device=points.device).scatter_add(1, coords, weighted)
    return (vsum / wsum).view([bv, R, R])


def points2pixel_chain(points, rot, trans, R):
    """The pixel ex*R + ey of every (image, point) pair, -1 where the mask rejects it: (B*V, N) int64."""
    with torch.no_grad():
        _, ex, ey, mask = _project_chain(points, rot, trans, R)
        return torch.where(mask, (ex * R + ey), torch.full_like(ex, -1.0)).long()


class _Points2Depth(torch.autograd.Function):
    """pcops_points2depth with the weight-sum image kept (its `workspace` is a tensor of its own), and
    pcops_points2depth_backward, a gather over (points, img, wsum)."""

    @staticmethod
    def forward(ctx, points, rot, trans, R):
        pts = points.detach().contiguous()
        B, N, _ = pts.shape
        V = rot.shape[0]
        img = torch.empty(B * V, R, R, device=pts.device)
        wsum = torch.empty(B * V, R, R, device=pts.device)
        with torch.cuda.device(pts.device):
            call("points2depth", lib().pcops_points2depth, ptr(pts), ptr(rot), ptr(trans), B, N, V, R, R, ptr(img),
                 ptr(wsum), wsum.numel() * 4, stream_of(pts))
        ctx.save_for_backward(pts, rot, trans, img, wsum)
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pts, rot, trans, img, wsum = ctx.saved_tensors
        return points2depth_backward(pts, rot, trans, img, wsum, g), None, None, None


def points2depth_backward(points, rot, trans, img, wsum, grad_img, out=None):
    """pcops_points2depth_backward: (B,N,3) gradient of the points from the saved image and weight sums."""
    B, N, _ = points.shape
    V, R = rot.shape[0], img.shape[-1]
    g = grad_img.contiguous()
    require_float(g, "grad_img")
    gp = torch.empty_like(points) if out is None else out
    with torch.cuda.device(points.device):
        call("points2depth_backward", lib().pcops_points2depth_backward, ptr(points), ptr(rot), ptr(trans), ptr(img),
             ptr(wsum), ptr(g), B, N, V, R, R, ptr(gp), stream_of(points))
    return gp


# mv_utils_zs.py:9-14
params = {'maxpoolz': 1, 'maxpoolxy': 7, 'maxpoolpadz': 0, 'maxpoolpadxy': 3, 'convz': 1, 'convxy': 3,
          'convsigmaxy': 3, 'convsigmaz': 1, 'convpadz': 0, 'convpadxy': 1, 'imgbias': 0., 'depth_bias': 0.2,
          'obj_ratio': 0.8, 'bg_clr': 0.0, 'resolution': 224, 'depth': 8}


def get2DGaussianKernel(ksize, sigma=0):
    """mv_utils_zs.py:197-204."""
    center = ksize // 2
    xs = (np.arange(ksize, dtype=np.float32) - center)
    kernel1d = np.exp(-(xs ** 2) / (2 * sigma ** 2))
    kernel = kernel1d[..., None] @ kernel1d[None, ...]
    kernel = torch.from_numpy(kernel)
    return kernel / kernel.sum()


def get3DGaussianKernel(ksize, depth, sigma=2, zsigma=2):
    """mv_utils_zs.py:206-212."""
    kernel2d = get2DGaussianKernel(ksize, sigma)
    zs = (np.arange(depth, dtype=np.float32) - depth // 2)
    zkernel = np.exp(-(zs ** 2) / (2 * zsigma ** 2))
    kernel3d = np.repeat(kernel2d[None, :, :], depth, axis=0) * zkernel[:, None, None]
    return kernel3d / torch.sum(kernel3d)


class PCViews_Real:
    """get_img(points (B,N,3)) -> (B*3, 3, 224, 224) PointSea 'realistic' depth images.

    Forward-only: the points are detached.  A gradient would have to run through a scatter-max of clipped
    depths and the bounding-box normalisation, and nothing trains through this renderer (unlike
    PCViews.get_img, which is differentiable)."""

    def __init__(self, TRANS=-0.7):
        _views = np.asarray([
            [[0 * np.pi / 2, 0, np.pi / 2], [-0.5, -0.5, TRANS]],
            [[1 * np.pi / 2, 0, np.pi / 2], [-0.5, -0.5, TRANS]],
            [[0, -np.pi / 2, np.pi / 2], [-0.5, -0.5, TRANS]]])
        _views_bias = np.asarray([
            [[0, np.pi / 9, 0], [-0.5, 0, TRANS]],
            [[0, np.pi / 9, 0], [-0.5, 0, TRANS]],
            [[0, np.pi / 15, 0], [-0.5, 0, TRANS]]])
        self.num_views = _views.shape[0]
        self.rot_mat = euler2mat(torch.tensor(_views[:, 0, :]).float()).transpose(1, 2).contiguous()
        self.rot_mat2 = euler2mat(torch.tensor(_views_bias[:, 0, :]).float()).transpose(1, 2).contiguous()
        self.translation = torch.tensor(_views[:, 1, :]).float().contiguous()
        kern = get3DGaussianKernel(params['convxy'], params['convz'], sigma=params['convsigmaxy'],
                                   zsigma=params['convsigmaz'])
        self.kernel = torch.as_tensor(kern, dtype=torch.float32).reshape(3, 3).contiguous()
        self._dev = {}

    def _consts(self, device):
        if device not in self._dev:
            self._dev[device] = tuple(t.to(device) for t in (self.rot_mat, self.rot_mat2, self.translation,
                                                             self.kernel))
        return self._dev[device]

    def points2grid(self, points):
        """(B,N,3) -> voxel grid (B*3, 8, 224, 224), [img][z][x][y] (mv_utils_zs.py:97-133)."""
        points = points.detach().contiguous()
        require_float(points, "points")
        B, N, _ = points.shape
        R, D, V = params['resolution'], params['depth'], self.num_views
        rot, rot2, trans, _ = self._consts(points.device)
        grid = torch.empty(B * V, D, R, R, device=points.device)
        with torch.cuda.device(points.device):
            call("points2grid", lib().pcops_points2grid, ptr(points), ptr(rot), ptr(rot2), ptr(trans), B, N, V, R, D,
                 ptr(grid), stream_of(points))
        return grid

    def grid2image(self, grid):
        """Grid2Image (mv_utils_zs.py:16-43): (BV, D, R, R) -> (BV, 3, R, R)."""
        grid = grid.contiguous()
        BV, D, R, _ = grid.shape
        kern = self._consts(grid.device)[3]
        img = torch.empty(BV, 3, R, R, device=grid.device)
        wsb = lib().pcops_grid2image_workspace_bytes(BV, D, R)
        ws = _lib.Workspace.get(grid.device, wsb)
        with torch.cuda.device(grid.device):
            call("grid2image", lib().pcops_grid2image, ptr(grid), ptr(kern), BV, D, R, ptr(img), ptr(ws), wsb,
                 stream_of(grid))
        return img

    def get_img(self, points):
        return self.grid2image(self.points2grid(points))
