"""CPU tests of the PointNet++ modules against tests/golden/pointnet2.npz (the reference's own
classes on the CPU oracle, tests/golden/make_golden_pointnet2.py): state_dict keys and shapes of
every class, the pure-torch branches (group_all, npoint=None, known=None) value for value, and the
fixture's own winner condition."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointnet2_support import CASES, build, case_inputs, golden_of, run  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from pointnet2_cases import CPU_CASES, SA_CASES  # noqa: E402

CAP = 0.02


@pytest.mark.parametrize("case", sorted(CASES))
def test_state_dict_keys_and_shapes(case):
    g = golden_of(case)
    sd = build(case).state_dict()
    keys = sorted(sd)
    assert keys == list(g["keys"])
    assert [str(tuple(sd[k].shape)) for k in keys] == list(g["shapes"])


def test_the_cases_cover_every_class():
    assert {c[1] for c in CASES.values()} == {"PointnetSAModuleMSG", "PointnetSAModule", "PointnetFPModule",
                                              "PointNet_SA_Module", "PointNet_FP_Module"}
    from svdformer_pointsea_amd import model_utils, pointnet2_modules

    seq = pointnet2_modules.build_shared_mlp([4, 8, 8], bn=False)
    assert sorted(seq.state_dict()) == ["0.bias", "0.weight", "2.bias", "2.weight"]
    blk = model_utils.Conv1d(4, 8)
    assert sorted(k for k in blk.state_dict() if not k.endswith("num_batches_tracked")) == [
        "bn.bias", "bn.running_mean", "bn.running_var", "bn.weight", "conv.bias", "conv.weight"]


@pytest.mark.parametrize("method", ["forward", "forward_tokens"])
@pytest.mark.parametrize("case", CPU_CASES)
def test_pure_torch_branches_match_the_golden_on_cpu(case, method):
    """fp32 torch against fp32 torch, the same ops: every output within 1e-5 max|out|.  Gradients are
    held to 1e-5 of the case's largest gradient entry, not of their own tensor: the bias of a conv
    that a BatchNorm follows has the exact gradient 0, and what both sides hold there is the
    rounding residue of sums whose terms have the size of the other gradients."""
    g = golden_of(case)
    res = run(case, torch.device("cpu"), method)
    gscale = max(float(np.abs(v).max()) for k, v in g.items() if k.startswith(("pgrad", "igrad")))
    for k, want in g.items():
        if k in ("keys", "shapes", "gaps", "bar"):
            continue
        got = res[k]
        if method == "forward_tokens" and got.ndim == 3 and (k.startswith(("eval", "train", "igrad"))):
            got = got.transpose(0, 2, 1)
        assert got.shape == want.shape, (k, got.shape, want.shape)
        scale = gscale if k.startswith(("pgrad", "igrad")) else float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        assert err <= 1e-5 * scale, (case, k, err, scale)


@pytest.mark.parametrize("case", SA_CASES)
def test_fixture_winner_condition(case):
    """Among the pre-max maxima with a positive top-2 gap, at most 2 % lie below the bar."""
    g = golden_of(case)
    gaps, bar = g["gaps"], float(g["bar"])
    assert gaps.size > 0 and (gaps > 0).all()
    assert int((gaps < bar).sum()) <= CAP * gaps.size


def test_fixture_inputs_are_the_fps_subset():
    ins = case_inputs()
    assert ins["known_t"].shape == (2, 16, 3)
    assert all((ins["xyz_t"][b] == ins["known_t"][b, 0]).all(1).any() for b in range(2))
