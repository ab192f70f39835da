"""Generate tests/golden/chamfer_counts.npz from the REFERENCE's own loss / metric code, as
make_golden_loss.py does (same stand-ins: the reference's float64 chamfer_python.distChamfer for the
Chamfer extension; run in the build container only, only the .npz is committed).

The reference has no batch of unequal clouds: what a counted call must equal is its code run at
B = 1 on every pair cut to its counts.  Case (tests/chamfer_counts_refs.py: golden_case, inputs
regenerated from the seed): B = 4, N = 600, M = 520, counts1 = [600, 257, 33, 1] (the gt / partial
side), counts2 = [1, 520, 512, 100] (the output side).  Per pair b, with x1 = xyz1[b:b+1, :c1[b]] and
x2 = xyz2[b:b+1, :c2[b]]:

  sqrt, l2            utils/loss_utils.py:10-21   chamfer_sqrt(x1, x2), chamfer(x1, x2)
  ss_sqrt, ss_l2      utils/loss_utils.py:23-31   chamfer_single_side_sqrt(x1, x2), chamfer_single_side(x1, x2)
  pm_sqrt, pm_l2      the same two against the FULL second cloud xyz2[b:b+1] (get_loss_PM's matching term
                      of a counted partial against an uncounted prediction)
  cd_p, cd_t, f1      utils/loss_utils.py:98-115  calc_cd(x2, x1, calc_f1=True)
  dcd, dcd_nonreg     utils/loss_utils.py:117-155 calc_dcd(x2, x1) / (non_reg=True): rows dcd, cd_p, cd_t

Usage:
    python tests/golden/make_golden_chamfer_counts.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main():
    from make_golden_loss import _stub_modules
    import chamfer_counts_refs as R

    torch.set_grad_enabled(False)
    lu, _ = _stub_modules()
    a, b = (torch.from_numpy(x) for x in R.golden_case())
    keys = ("sqrt", "l2", "ss_sqrt", "ss_l2", "pm_sqrt", "pm_l2", "cd_p", "cd_t", "f1")
    out = {k: np.zeros(R.GOLDEN_B, np.float64) for k in keys}
    out["dcd"], out["dcd_nonreg"] = np.zeros((3, R.GOLDEN_B), np.float32), np.zeros((3, R.GOLDEN_B), np.float32)
    for k, (c1, c2) in enumerate(zip(R.GOLDEN_COUNTS1, R.GOLDEN_COUNTS2)):
        x1, x2 = a[k:k + 1, :c1], b[k:k + 1, :c2]
        out["sqrt"][k] = float(lu.chamfer_sqrt(x1, x2))
        out["l2"][k] = float(lu.chamfer(x1, x2))
        out["ss_sqrt"][k] = float(lu.chamfer_single_side_sqrt(x1, x2))
        out["ss_l2"][k] = float(lu.chamfer_single_side(x1, x2))
        out["pm_sqrt"][k] = float(lu.chamfer_single_side_sqrt(x1, b[k:k + 1]))
        out["pm_l2"][k] = float(lu.chamfer_single_side(x1, b[k:k + 1]))
        cd_p, cd_t, f1 = lu.calc_cd(x2, x1, calc_f1=True)
        out["cd_p"][k], out["cd_t"][k], out["f1"][k] = float(cd_p), float(cd_t), float(f1)
        out["dcd"][:, k] = [float(t) for t in lu.calc_dcd(x2, x1)]
        out["dcd_nonreg"][:, k] = [float(t) for t in lu.calc_dcd(x2, x1, non_reg=True)]
    for k, v in out.items():
        print(k, v, flush=True)
    path = os.path.join(HERE, "chamfer_counts.npz")
    np.savez_compressed(path, **out)
    print("chamfer_counts.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
