"""Regenerates tests/golden/median_depth_*.npz and seed_scalars.npz from a checkout of the reference:

    python tests/golden/make_seed_goldens.py /path/to/reference

Inputs and recorded outputs only.  The outputs come from the reference's own functions, imported and run on CPU tensors:
utils/slam_utils.get_median_depth (with and without opacity / mask / return_std, odd and even n_valid),
gaussian_splatting/utils/sh_utils.RGB2SH and gaussian_splatting/utils/general_utils.inverse_sigmoid.
create_pcd_from_image_and_depth needs Open3D and add_new_keyframe cannot be imported without the whole SLAM stack, so the
selection, the back-projection and the depth prior have no recorded reference outputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    sys.path.insert(0, ref)
    from gaussian_splatting.utils.general_utils import inverse_sigmoid
    from gaussian_splatting.utils.sh_utils import RGB2SH
    from utils.slam_utils import get_median_depth

    rng = np.random.default_rng(20261016)
    cases = {
        # name: (H, W, use_opacity, use_mask, parity of n_valid wanted)
        "plain_odd": (24, 31, False, False, 1), "plain_even": (24, 32, False, False, 0),
        "opacity_odd": (30, 40, True, False, 1), "opacity_even": (30, 40, True, False, 0),
        "mask_odd": (17, 23, False, True, 1), "both_even": (48, 64, True, True, 0), "both_odd": (48, 64, True, True, 1),
    }
    for name, (H, W, use_o, use_m, parity) in cases.items():
        depth = rng.uniform(0.2, 6.0, (1, H, W)).astype(np.float32)
        depth[rng.uniform(size=depth.shape) < 0.15] = 0.0
        depth[rng.uniform(size=depth.shape) < 0.02] = -1.0
        depth[0, 0, :4] = depth[0, 1, :4]  # repeated values around
        opacity = rng.uniform(0.8, 1.0, (1, H, W)).astype(np.float32)
        mask = rng.uniform(size=(1, H, W)) < 0.7
        o = torch.from_numpy(opacity) if use_o else torch.ones(1, H, W)
        m = torch.from_numpy(mask) if use_m else None
        # fix the parity of n_valid by invalidating one more pixel if needed
        _, _, valid = get_median_depth(torch.from_numpy(depth), o, m, return_std=True)
        if int(valid.sum()) % 2 != parity:
            idx = np.flatnonzero(valid.numpy().reshape(-1))[0]
            depth.reshape(-1)[idx] = 0.0
        med, std, valid = get_median_depth(torch.from_numpy(depth), o, m, return_std=True)
        med_only = get_median_depth(torch.from_numpy(depth), o, m)
        assert int(valid.sum()) % 2 == parity and float(med_only) == float(med)
        out = dict(depth=depth, median=np.float32(med.item()), std=np.float32(std.item()), valid=valid.numpy(),
                   n_valid=np.int64(valid.sum().item()), use_opacity=np.bool_(use_o), use_mask=np.bool_(use_m))
        if use_o:
            out["opacity"] = opacity
        if use_m:
            out["mask"] = mask
        np.savez_compressed(os.path.join(HERE, "median_depth_%s.npz" % name), **out)
        print(name, out["n_valid"], out["median"], out["std"])
    rgb = torch.arange(256, dtype=torch.float64).div(255.0).float()
    x = torch.tensor([0.5, 0.1, 0.9, 0.25], dtype=torch.float32)
    np.savez_compressed(os.path.join(HERE, "seed_scalars.npz"), rgb=rgb.numpy(), rgb2sh=RGB2SH(rgb).numpy(), x=x.numpy(),
                        inverse_sigmoid=inverse_sigmoid(x).numpy())


if __name__ == "__main__":
    main(sys.argv[1])
