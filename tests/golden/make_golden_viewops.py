"""Generate tests/golden/viewops.npz from the REFERENCE's own view-space functions (run where the
reference is available; only the .npz is committed).  Inputs are regenerated from seeds by
tests/viewops_refs.py (exchange_inputs, depth_inputs); only results are stored.

  x_<case>_splat    models/model_utils.py:1134-1154 point_fea_img_fea(fea, coord, h, w) on clones (it
                    zeroes its arguments in place)
  x_<case>_gather   :1157-1176 distribute_img_fea_points(img, coord); img is passed channels_last, the
                    only layout its permute(...).view(...) accepts
  d_<case>_grad     autograd of :1179-1234 PCViews(TRANS=-0.7, R).get_img: points.grad after
                    img.backward(g); d_<case>_img the image itself for the small resolutions (the 224 one is
                    depth.npz's)

Usage:  python tests/golden/make_golden_viewops.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, _load, _stub_modules  # noqa: E402
import viewops_refs as VR  # noqa: E402


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    mu = _load(os.path.join(REF, "models/model_utils.py"), "ref_model_utils")
    out = {}
    for name, case in VR.EXCHANGE_GOLDEN.items():
        _, B, N, C, h, w = case
        fea, coord, img = (torch.from_numpy(a) for a in VR.exchange_inputs(*case))
        with torch.no_grad():
            out[f"x_{name}_splat"] = mu.point_fea_img_fea(fea.clone(), coord.clone(), h, w).numpy()
            cl = img.contiguous(memory_format=torch.channels_last)
            if not cl.permute(0, 2, 3, 1).is_contiguous():   # C == 1 or h*w == 1: strides are ambiguous
                cl = img.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            out[f"x_{name}_gather"] = mu.distribute_img_fea_points(cl, coord.clone()).numpy()
    depth = np.load(os.path.join(HERE, "depth.npz"))
    for name, (_, B, N, R) in VR.DEPTH_GOLDEN.items():
        pts, g = VR.depth_inputs(name, depth)
        p = torch.from_numpy(pts).requires_grad_(True)
        view = mu.PCViews(TRANS=-0.7, RESOLUTION=R)
        img = view.get_img(p)
        img.backward(torch.from_numpy(g))
        assert torch.isfinite(p.grad).all() and (p.grad != 0).any()
        out[f"d_{name}_grad"] = p.grad.numpy()
        if name == "r224":
            assert np.array_equal(img.detach().numpy(), depth["img"])
        else:
            out[f"d_{name}_img"] = img.detach().numpy()
    path = os.path.join(HERE, "viewops.npz")
    np.savez_compressed(path, **out)
    print("viewops.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
