"""CPU side of metrics.completion_metrics: the size query of pcops_completion_metrics (no compute
call -- there is no GPU here) and the composed path it takes for tensors that are not CUDA fp32."""
import numpy as np
import torch


def test_completion_metrics_size_query_without_gpu():
    from svdformer_pointsea_amd import _lib

    L = _lib.lib()
    assert L.pcops_completion_metrics_workspace_bytes(8, 16384, 16384) == 0   # hit counts in LDS
    assert L.pcops_completion_metrics_workspace_bytes(2, 2048, 32768) == 0
    assert L.pcops_completion_metrics_workspace_bytes(1, 40000, 33000) == 40000 * 4
    assert L.pcops_completion_metrics_workspace_bytes(3, 100, 32769) == 3 * 32769 * 4


def test_completion_metrics_cpu_path_composes_calc_cd_and_calc_dcd():
    from oracle.cpu_path import cpu_ops
    from svdformer_pointsea_amd import metrics as M

    rng = np.random.default_rng(0)
    gt = torch.from_numpy((rng.random((2, 300, 3)) - 0.5).astype(np.float32))
    x = gt[:, :200] + 0.01 * torch.from_numpy(rng.standard_normal((2, 200, 3)).astype(np.float32))
    with cpu_ops():
        for kw in ({}, {"non_reg": True}, {"n_lambda": 2}):
            r = M.completion_metrics(x, gt, **kw)
            cd_p, cd_t, f1 = M.calc_cd(x, gt, calc_f1=True)
            dcd = M.calc_dcd(x, gt, **kw)[0]
            for got, want in ((r.cd_p, cd_p), (r.cd_t, cd_t), (r.f1, f1), (r.dcd, dcd)):
                assert torch.equal(got, want)
            assert torch.equal((r.t1 + r.t2) / 2, r.dcd) and torch.equal(r.l2a + r.l2b, r.cd_t)
