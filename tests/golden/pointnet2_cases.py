"""The PointNet++ module cases of pointnet2.npz, shared by the generator (which builds the
reference's classes from them) and the tests (which build this package's): class name,
constructor arguments, the named inputs of `forward`, and the weight seed.  Inputs come from
`inputs(seed)`; nothing here needs the reference.

Shapes: B 2, N 100 points in the unit cube, 16 FPS centres, C 5 input features, C2 8 features on
the 16 known points.  FP outputs are kept at 8 channels so the fixture stays small."""
import numpy as np

B, N, S, C, C2 = 2, 100, 16, 5, 8
SEED_IN = 7

# case -> (source module, class, kwargs, forward argument names, weight seed)
#   source "p2": pointnet2_ops.pointnet2_modules, "mu": models/model_utils.py
CASES = {
    "sa_msg": ("p2", "PointnetSAModuleMSG",
               dict(npoint=S, radii=[0.2, 0.4], nsamples=[8, 16], mlps=[[C, 16, 32], [C, 16, 32]]),
               ("xyz_t", "feat"), 17),
    "sa_all": ("p2", "PointnetSAModule", dict(mlp=[C, 16, 32], npoint=None), ("xyz_t", "feat"), 8),
    "fp": ("p2", "PointnetFPModule", dict(mlp=[C2 + C, 16, 8]), ("xyz_t", "known_t", "feat", "known_feat"), 9),
    "fp_noskip": ("p2", "PointnetFPModule", dict(mlp=[C2, 16, 8]), ("xyz_t", "known_t", None, "known_feat"), 10),
    "fp_noknown": ("p2", "PointnetFPModule", dict(mlp=[C2 + C, 16, 8]), ("xyz_t", None, "feat", "global_feat"), 11),
    "mu_sa": ("mu", "PointNet_SA_Module", dict(npoint=S, nsample=8, radius=0.3, in_channel=C, mlp=[16, 32]),
              ("xyz", "feat"), 22),
    "mu_sa_all": ("mu", "PointNet_SA_Module",
                  dict(npoint=S, nsample=8, radius=0.3, in_channel=C, mlp=[16, 32], group_all=True),
                  ("xyz", "feat"), 13),
    "mu_sa_noxyz": ("mu", "PointNet_SA_Module",
                    dict(npoint=S, nsample=8, radius=0.3, in_channel=C, mlp=[16, 32], use_xyz=False),
                    ("xyz", "feat"), 14),
    "mu_fp": ("mu", "PointNet_FP_Module", dict(in_channel=C2, mlp=[16, 8], use_points1=True, in_channel_points1=C),
              ("xyz", "known", "feat", "known_feat"), 15),
    "mu_fp_nop1": ("mu", "PointNet_FP_Module", dict(in_channel=C2, mlp=[16, 8]),
                   ("xyz", "known", None, "known_feat"), 16),
}
GRAD_INPUTS = ("feat", "known_feat", "global_feat")   # the feature inputs whose gradient is recorded
SA_CASES = ("sa_msg", "sa_all", "mu_sa", "mu_sa_all", "mu_sa_noxyz")
CPU_CASES = ("sa_all", "fp_noknown", "mu_sa_all")       # pure-torch branches


def kwargs_of(case):
    """A deep-enough copy: PointnetSAModuleMSG edits its mlps lists in place."""
    kw = dict(CASES[case][2])
    for k, v in kw.items():
        if isinstance(v, list):
            kw[k] = [list(e) if isinstance(e, list) else e for e in v]
    return kw


def inputs(fps_idx):
    """name -> fp32 array.  fps_idx (B,S): the FPS indices of xyz_t (the known points are that
    subset of the unknown ones, so zero distances are the normal case)."""
    rng = np.random.default_rng(SEED_IN)
    xyz_t = rng.uniform(0.0, 1.0, (B, N, 3)).astype(np.float32)
    feat = rng.standard_normal((B, C, N)).astype(np.float32)
    known_feat = rng.standard_normal((B, C2, S)).astype(np.float32)
    global_feat = rng.standard_normal((B, C2, 1)).astype(np.float32)
    out = dict(xyz_t=xyz_t, xyz=np.ascontiguousarray(xyz_t.transpose(0, 2, 1)), feat=feat, known_feat=known_feat,
               global_feat=global_feat)
    if fps_idx is not None:
        known_t = np.take_along_axis(xyz_t, fps_idx[..., None].astype(np.int64), 1)
        out.update(known_t=known_t, known=np.ascontiguousarray(known_t.transpose(0, 2, 1)))
    return out


def loss_weight(case, shape):
    """The fixed tensor of the loss sum(out * w)."""
    return np.random.default_rng(1000 + CASES[case][4]).standard_normal(shape).astype(np.float32)
