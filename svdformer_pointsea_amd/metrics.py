"""Training losses and evaluation metrics of the reference on libpcops:
utils/loss_utils.py:10-155 and metrics/CD/fscore.py:3-16.

  chamfer / chamfer_sqrt / chamfer_single_side(_sqrt)    Chamfer losses
  get_loss / get_loss_PM                                 train_pcn / PointSea losses
  calc_cd                                                CD-L1 (cd_p), CD-L2 (cd_t), F-score
  calc_dcd                                               density-aware Chamfer
  fscore                                                 F-score on squared distances
  completion_metrics(_raw)                               all of the last three from one Chamfer search,
                                                         in one launch (csrc/metrics.hip)
Names, arguments and return structures are the reference's.  The
nearest-neighbour search is the Chamfer kernel (csrc/chamfer.hip, both
directions in one launch); what follows it are the same reductions, in the
same floating-point order, as the reference's torch expressions.
"""
import collections
import os

import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd import Function

from . import chamfer3D
from ._lib import Workspace, call, lib, ptr, require_float, require_int, stream_of
from .model_utils import fps_subsample

_nn = chamfer3D.chamfer_3DDist()


def _means(p1, p2, root):
    d1, d2, _, _ = _nn(p1, p2)
    if root:
        d1, d2 = torch.sqrt(d1), torch.sqrt(d2)
    return torch.mean(d1), torch.mean(d2)


class _SqrtMeanChamfer(Function):
    """chamfer_sqrt (both=True: (mean(sqrt(d1)) + mean(sqrt(d2))) / 2) and chamfer_single_side_sqrt
    (both=False: mean(sqrt(d1))), loss_utils.py:10-31, as one autograd node.  The forward runs the
    same torch expressions on the Chamfer kernel's distances (same values, bit for bit); the
    backward forms autograd's distance gradient in one launch (pcops_chamfer_sqrt_mean_grad: the
    "/ 2", mean and sqrt backward steps in their order) and hands it to pcops_chamfer_backward,
    instead of ~8 scalar / elementwise launches per loss term."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, p1, p2, both):
        d1, d2, i1, i2 = chamfer3D.chamfer_forward_raw(p1, p2)
        s1 = torch.sqrt(d1)
        m1 = torch.mean(s1)
        s2 = torch.sqrt(d2) if both else None
        out = (m1 + torch.mean(s2)) / 2 if both else m1
        ctx.save_for_backward(p1, p2, i1, i2, s1, s2)
        ctx.both = both
        return out

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, g):
        p1, p2, i1, i2, s1, s2 = ctx.saved_tensors
        B, n, _ = p1.shape
        m = p2.shape[1]
        g = g.contiguous()
        gd1, gd2 = torch.empty_like(s1), torch.empty(B, m, device=p1.device)
        g1, g2 = torch.empty_like(p1), torch.empty_like(p2)
        with torch.cuda.device(p1.device):
            call("chamfer_sqrt_mean_grad", lib().pcops_chamfer_sqrt_mean_grad, ptr(g), 0.5 if ctx.both else 1.0,
                 ptr(s1), B * n, ptr(s2), B * m, ptr(gd1), ptr(gd2), stream_of(p1))
            call("chamfer_3D.backward", lib().pcops_chamfer_backward, ptr(p1), ptr(p2), B, n, m, ptr(gd1), ptr(gd2),
                 ptr(i1), ptr(i2), ptr(g1), ptr(g2), stream_of(p1))
        return (g1 if ctx.needs_input_grad[0] else None), (g2 if ctx.needs_input_grad[1] else None), None


def _fused_loss(p1, p2):
    """The one-node sqrt-mean loss applies (PCOPS_LOSS_FUSED=0 keeps the autograd chain; read per call)."""
    return (os.environ.get("PCOPS_LOSS_FUSED", "1") != "0" and p1.is_cuda and p2.is_cuda and p1.dim() == 3
            and p2.dim() == 3 and p1.shape[0] == p2.shape[0] and p1.shape[-1] == 3 and p2.shape[-1] == 3
            and p1.shape[1] > 0 and p2.shape[1] > 0)


class _CountsMeanChamfer(Function):
    """The four Chamfer losses over counted clouds as one autograd node: the mean over b of the
    reference's loss on cloud pair b cut to its counts (root: sqrt of the distances first; both: the two
    directions, "/ 2" of their sum under root, else direction 1 alone).  Forward: the counted search, one
    launch for the per-pair means (pcops_chamfer_counts_means, fixed summation order) and the mean of B
    numbers; backward: pcops_chamfer_counts_mean_grad and pcops_chamfer_backward_counts.  No count is
    read back to the host.  A pair with an empty side adds 0 and gets zero gradients."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, p1, p2, counts1, counts2, root, both):
        d1, d2, i1, i2 = chamfer3D.chamfer_forward_raw(p1, p2, counts1, counts2)
        B, n = d1.shape
        means = torch.empty(B, 4, device=p1.device)
        with torch.cuda.device(p1.device):
            call("chamfer_counts_means", lib().pcops_chamfer_counts_means, ptr(d1), ptr(d2), ptr(counts1),
                 ptr(counts2), B, n, d2.shape[1], ptr(means), stream_of(p1))
        a, c = (means[:, 0], means[:, 1]) if root else (means[:, 2], means[:, 3])
        per = a if not both else ((a + c) / 2 if root else a + c)
        ctx.save_for_backward(p1, p2, i1, i2, d1, d2, counts1, counts2)
        ctx.root, ctx.both = root, both
        return per.mean()

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, g):
        p1, p2, i1, i2, d1, d2, counts1, counts2 = ctx.saved_tensors
        B, n, _ = p1.shape
        m = p2.shape[1]
        g = g.contiguous()
        gd1, gd2 = torch.empty_like(d1), torch.empty_like(d2)
        with torch.cuda.device(p1.device):
            call("chamfer_counts_mean_grad", lib().pcops_chamfer_counts_mean_grad, ptr(g),
                 0.5 if (ctx.both and ctx.root) else 1.0, ptr(d1), ptr(d2), ptr(counts1), ptr(counts2), B, n, m,
                 int(ctx.root), int(ctx.both), ptr(gd1), ptr(gd2), stream_of(p1))
        g1, g2 = chamfer3D.chamfer_backward_counts_raw(p1, p2, counts1, counts2, gd1, gd2, i1, i2)
        return ((g1 if ctx.needs_input_grad[0] else None), (g2 if ctx.needs_input_grad[1] else None), None, None,
                None, None)


def _counts_chain(loss, p1, p2, counts1, counts2):
    """mean over b of loss(p1[b:b+1, :c1[b]], p2[b:b+1, :c2[b]]): a loop of B = 1 calls of the uniform loss
    on slices, with the counts read back to the host.  For A/B runs and tests only -- the counted node
    (_CountsMeanChamfer) replaces it."""
    B, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    c1 = [n] * B if counts1 is None else counts1.clamp(0, n).tolist()
    c2 = [m] * B if counts2 is None else counts2.clamp(0, m).tolist()
    terms = [loss(p1[b:b + 1, :c1[b]], p2[b:b + 1, :c2[b]]) if c1[b] and c2[b] else p1.new_zeros(())
             for b in range(B)]
    return torch.stack(terms).mean()


def _counted(p1, p2, counts1, counts2, root, both, chain):
    if not (p1.is_cuda and p2.is_cuda):
        raise RuntimeError("counted Chamfer losses need CUDA tensors")
    if os.environ.get("PCOPS_LOSS_FUSED", "1") == "0":
        return chain(p1, p2, counts1, counts2)
    return _CountsMeanChamfer.apply(p1.contiguous(), p2.contiguous(), counts1, counts2, root, both)


def chamfer_counts_chain(p1, p2, counts1=None, counts2=None):
    return _counts_chain(chamfer, p1, p2, counts1, counts2)


def chamfer_sqrt_counts_chain(p1, p2, counts1=None, counts2=None):
    return _counts_chain(chamfer_sqrt, p1, p2, counts1, counts2)


def chamfer_single_side_counts_chain(p1, p2, counts1=None, counts2=None):
    return _counts_chain(chamfer_single_side, p1, p2, counts1, counts2)


def chamfer_single_side_sqrt_counts_chain(p1, p2, counts1=None, counts2=None):
    return _counts_chain(chamfer_single_side_sqrt, p1, p2, counts1, counts2)


def chamfer(p1, p2, counts1=None, counts2=None):
    """counts1 / counts2 ((B,) int32 on the device, here and in the three losses below): the clouds are
    padded buffers and the value is the mean over b of the loss on pair b cut to its counts."""
    if counts1 is not None or counts2 is not None:
        return _counted(p1, p2, counts1, counts2, False, True, chamfer_counts_chain)
    m1, m2 = _means(p1, p2, False)
    return m1 + m2


def chamfer_sqrt(p1, p2, counts1=None, counts2=None):
    if counts1 is not None or counts2 is not None:
        return _counted(p1, p2, counts1, counts2, True, True, chamfer_sqrt_counts_chain)
    if _fused_loss(p1, p2):
        return _SqrtMeanChamfer.apply(p1.contiguous(), p2.contiguous(), True)
    m1, m2 = _means(p1, p2, True)
    return (m1 + m2) / 2


def chamfer_single_side(pcd1, pcd2, counts1=None, counts2=None):
    if counts1 is not None or counts2 is not None:
        return _counted(pcd1, pcd2, counts1, counts2, False, False, chamfer_single_side_counts_chain)
    return _means(pcd1, pcd2, False)[0]


def chamfer_single_side_sqrt(pcd1, pcd2, counts1=None, counts2=None):
    if counts1 is not None or counts2 is not None:
        return _counted(pcd1, pcd2, counts1, counts2, True, False, chamfer_single_side_sqrt_counts_chain)
    if _fused_loss(pcd1, pcd2):
        return _SqrtMeanChamfer.apply(pcd1.contiguous(), pcd2.contiguous(), False)
    return _means(pcd1, pcd2, True)[0]


def gt_pyramid(gt, n1, nc):
    """(gt_c, gt_1): gt FPS-subsampled to n1 points, then that to nc points
    (loss_utils.py:47-48).  It depends on gt only, so a caller may compute it
    ahead of (and beside) the forward pass and hand it to get_loss(gts=...)."""
    gt_1 = fps_subsample(gt, n1)
    return fps_subsample(gt_1, nc), gt_1


def _stage_losses(pcds_pred, gt, CD, gts=None):
    """CD of (coarse, fine1, fine2) against gt FPS-subsampled to each size."""
    Pc, P1, P2 = pcds_pred
    gt_c, gt_1 = gts if gts is not None else gt_pyramid(gt, P1.shape[1], Pc.shape[1])
    return [CD(Pc, gt_c), CD(P1, gt_1), CD(P2, gt)]


def get_loss(pcds_pred, gt, sqrt=True, alpha1=1, alpha2=1, gts=None):
    """loss_utils.py:33-58 -> (cdc + alpha1*cd1 + alpha2*cd2, [cdc, cd1, cd2]).
    `gts` (optional): gt_pyramid(gt, ...) computed earlier by the caller."""
    cdc, cd1, cd2 = _stage_losses(pcds_pred, gt, chamfer_sqrt if sqrt else chamfer, gts)
    return cdc + alpha1 * cd1 + alpha2 * cd2, [cdc, cd1, cd2]


def get_loss_PM(pcds_pred, partial, gt, sqrt=True, gts=None, partial_counts=None):
    """loss_utils.py:60-82: get_loss + single-sided partial -> fine2 matching.  partial_counts ((B,) int32
    on the device): `partial` is a padded buffer of counted clouds (data.seprate_point_cloud(...,
    return_counts=True)), and the matching term is taken against each cloud's own points."""
    cdc, cd1, cd2 = _stage_losses(pcds_pred, gt, chamfer_sqrt if sqrt else chamfer, gts)
    pm = (chamfer_single_side_sqrt if sqrt else chamfer_single_side)(partial, pcds_pred[2], counts1=partial_counts)
    return cdc + cd1 + cd2 + pm, [cdc, cd1, cd2]


def fscore(dist1, dist2, threshold=0.0001):
    """(f1, precision_1, precision_2) per sample; dist1/dist2 are SQUARED."""
    p1 = torch.mean((dist1 < threshold).float(), dim=1)
    p2 = torch.mean((dist2 < threshold).float(), dim=1)
    f1 = 2 * p1 * p2 / (p1 + p2)
    f1[torch.isnan(f1)] = 0
    return f1, p1, p2


def calc_cd(output, gt, calc_f1=False, return_raw=False, normalize=False, separate=False):
    """Per-sample [cd_p (CD-L1), cd_t (CD-L2)] (+ f1) (+ dist1, dist2, idx1, idx2).
    Distances are gt -> output first, as loss_utils.py:98-115; `normalize` is
    accepted and unused there too."""
    dist1, dist2, idx1, idx2 = chamfer3D.chamfer_3DDist()(gt, output)
    l1 = [torch.sqrt(d).mean(1) for d in (dist1, dist2)]
    l2 = [d.mean(1) for d in (dist1, dist2)]
    if separate:
        res = [torch.cat([v.unsqueeze(0) for v in l1]), torch.cat([v.unsqueeze(0) for v in l2])]
    else:
        res = [(l1[0] + l1[1]) / 2, l2[0] + l2[1]]
    if calc_f1:
        res.append(fscore(dist1, dist2)[0])
    if return_raw:
        res.extend([dist1, dist2, idx1, idx2])
    return res


def _density_term(dist, idx, n_targets, alpha, n_lambda, frac):
    """mean_i (1 - exp(-alpha d_i) / (n_hits(idx_i)^lambda + 1e-6) * frac)."""
    hits = torch.zeros(idx.shape[0], n_targets, dtype=idx.dtype, device=idx.device)
    hits.scatter_add_(1, idx.long(), torch.ones_like(idx))
    w = hits.gather(1, idx.long()).float().detach() ** n_lambda
    w = (w + 1e-6) ** (-1) * frac
    return (1 - torch.exp(-dist * alpha) * w).mean(dim=1)


def calc_dcd(x, gt, alpha=1000, n_lambda=1, return_raw=False, non_reg=False):
    """Density-aware Chamfer distance -> [dcd, cd_p, cd_t] (+ raw)."""
    x, gt = x.float(), gt.float()
    n_x, n_gt = x.shape[1], gt.shape[1]
    assert x.shape[0] == gt.shape[0]
    f12, f21 = n_x / n_gt, n_gt / n_x
    if non_reg:
        f12, f21 = max(1, f12), max(1, f21)
    cd_p, cd_t, dist1, dist2, idx1, idx2 = calc_cd(x, gt, return_raw=True)
    # dist1/idx1: every gt point's nearest x; dist2/idx2: every x's nearest gt
    loss = (_density_term(dist1, idx1, n_x, alpha, n_lambda, f21) +
            _density_term(dist2, idx2, n_gt, alpha, n_lambda, f12)) / 2
    res = [loss, cd_p, cd_t]
    if return_raw:
        res.extend([dist1, dist2, idx1, idx2])
    return res


# column layout of pcops_completion_metrics' output row (include/pcops.h PCOPS_METRICS_*)
_METRIC_COLS = ("l1a", "l1b", "l2a", "l2b", "cd_p", "cd_t", "p1", "p2", "f1", "t1", "t2", "dcd")
CompletionMetrics = collections.namedtuple("CompletionMetrics", _METRIC_COLS)
CompletionMetrics.__doc__ = """Per-sample (B,) tensors: cd_p (CD-L1), cd_t (CD-L2), f1, dcd, and their parts --
l1a / l1b = mean(sqrt(dist1 / dist2)), l2a / l2b = mean(dist1 / dist2), p1 / p2 the F-score's two
precisions, t1 / t2 the two density terms (direction 1 is gt -> output, as calc_cd)."""


def _dcd_fracs(n_x, n_gt, non_reg):
    f12, f21 = n_x / n_gt, n_gt / n_x
    return (max(1, f12), max(1, f21)) if non_reg else (f12, f21)


def completion_metrics_raw(dist1, dist2, idx1, idx2, threshold=1e-4, alpha=1000, non_reg=False, counts1=None,
                           counts2=None):
    """CompletionMetrics of one Chamfer result chamfer(gt, output) -- dist1 / idx1 (B, n_gt), dist2 / idx2
    (B, n_out), CUDA fp32 / int32 -- in one launch (pcops_completion_metrics, n_lambda == 1).  The
    fields are column views of the kernel's (B, 12) output: no torch arithmetic follows the launch.
    counts1 / counts2 ((B,) int32 on the device): the result of a counted search; every row is then
    formed from its pair's valid rows and own sizes, and a pair with an empty side gives a NaN row."""
    for t, name in ((dist1, "dist1"), (dist2, "dist2")):
        require_float(t, name)
    for t, name in ((idx1, "idx1"), (idx2, "idx2")):
        require_int(t, name)
    B, n = dist1.shape
    m = dist2.shape[1]
    if dist2.shape[0] != B or idx1.shape != dist1.shape or idx2.shape != dist2.shape:
        raise RuntimeError("completion_metrics_raw: dist1 / idx1 must be (B, n_gt) and dist2 / idx2 (B, n_out)")
    dev = dist1.device
    out = torch.empty(B, len(_METRIC_COLS), device=dev)
    if counts1 is not None or counts2 is not None:
        for t, name in ((counts1, "counts1"), (counts2, "counts2")):
            if t is not None:
                require_int(t, name)
        with torch.cuda.device(dev):
            wsb = lib().pcops_completion_metrics_workspace_bytes(B, n, m)
            ws = Workspace.get(dev, wsb)
            call("completion_metrics_counts", lib().pcops_completion_metrics_counts, ptr(dist1), ptr(idx1), ptr(dist2),
                 ptr(idx2), ptr(counts1), ptr(counts2), B, n, m, threshold, alpha, int(bool(non_reg)), ptr(out),
                 ptr(ws), wsb, stream_of(dist1))
        return CompletionMetrics(*out.unbind(1))
    f12, f21 = _dcd_fracs(m, n, non_reg)
    with torch.cuda.device(dev):
        wsb = lib().pcops_completion_metrics_workspace_bytes(B, n, m)
        ws = Workspace.get(dev, wsb)
        call("completion_metrics", lib().pcops_completion_metrics, ptr(dist1), ptr(idx1), ptr(dist2), ptr(idx2), B, n,
             m, threshold, alpha, f21, f12, ptr(out), ptr(ws), wsb, stream_of(dist1))
    return CompletionMetrics(*out.unbind(1))


def completion_metrics(output, gt, threshold=1e-4, alpha=1000, n_lambda=1, non_reg=False, output_counts=None,
                       gt_counts=None):
    """calc_cd(output, gt, calc_f1=True) and calc_dcd(output, gt, alpha, n_lambda, non_reg=non_reg) as one
    CompletionMetrics: one Chamfer search (the reference runs it twice, calc_dcd calls calc_cd again) and
    one pcops_completion_metrics launch instead of ~50 scalar / elementwise ones.  Inputs that are not
    CUDA fp32, or n_lambda != 1, compose the existing calc_cd / calc_dcd (so under oracle.cpu_path.cpu_ops()
    it runs on the CPU).  output_counts / gt_counts ((B,) int32 on the device): padded buffers of counted
    clouds, scored per pair on its valid points (CUDA fp32, n_lambda == 1 only)."""
    if output_counts is not None or gt_counts is not None:
        if not (n_lambda == 1 and output.is_cuda and gt.is_cuda and output.dtype == torch.float32
                and gt.dtype == torch.float32):
            raise RuntimeError("completion_metrics: counted clouds need CUDA fp32 tensors and n_lambda == 1")
        dist1, dist2, idx1, idx2 = chamfer3D.chamfer_forward_raw(gt.detach().contiguous(), output.detach().contiguous(),
                                                                 gt_counts, output_counts)
        return completion_metrics_raw(dist1, dist2, idx1, idx2, threshold, alpha, non_reg, gt_counts, output_counts)
    if (n_lambda == 1 and output.is_cuda and gt.is_cuda and output.dtype == torch.float32
            and gt.dtype == torch.float32):
        dist1, dist2, idx1, idx2 = chamfer3D.chamfer_forward_raw(gt.detach().contiguous(),
                                                                 output.detach().contiguous())
        return completion_metrics_raw(dist1, dist2, idx1, idx2, threshold, alpha, non_reg)
    with torch.no_grad():
        output, gt = output.float(), gt.float()
        l1, l2, dist1, dist2, idx1, idx2 = calc_cd(output, gt, return_raw=True, separate=True)
        f1, p1, p2 = fscore(dist1, dist2, threshold)
        f12, f21 = _dcd_fracs(output.shape[1], gt.shape[1], non_reg)
        t1 = _density_term(dist1.float(), idx1, output.shape[1], alpha, n_lambda, f21)
        t2 = _density_term(dist2.float(), idx2, gt.shape[1], alpha, n_lambda, f12)
        return CompletionMetrics(l1[0], l1[1], l2[0], l2[1], (l1[0] + l1[1]) / 2, l2[0] + l2[1], p1, p2, f1, t1, t2,
                                 (t1 + t2) / 2)
