#!/usr/bin/env python3
"""Recorded device outputs: the controls of tests/test_cpu_comparator_canaries.py (tests/golden/device_<scene>.npz).

Runs on the MI355X.  For each canary scene of tests/helpers.py it runs the tiled forward and backward exactly as
test_gpu_tiled.test_forward_and_backward_parity does (SH colours, background helpers.PARITY_BG, the scene's scale modifier,
seeds helpers.seeds(cam, seed=1)) and stores what the kernels returned:
  color [3,H,W], depth [1,H,W], opacity [1,H,W], n_contrib [H,W], n_touched [P], radii [P], num_rendered
  the twelve outputs of the backward, under helpers.GRAD_NAMES (an output the backward does not produce is not stored)
These are a correct fp32 evaluation of the frame: the comparators must accept them, and since a correct evaluation stays
correct, they do not go stale when the kernels change their rounding.

usage: make_device_outputs.py [OUT_DIR]   (default: this directory)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401,E402  (puts the repository and the package on sys.path)
import helpers as hp  # noqa: E402

SCENES = ["canary_97x61", "p500_100x75_sh0", "p300_behind_64x48"]


def record(name):
    from gsaj import rasterizer as C

    cam, sc, deg = hp.make(name)
    mod = hp.scale_modifier(name)
    (_, _), kw = hp.oracle_forward(cam, sc, deg, bg=hp.PARITY_BG, scale_modifier=mod)
    out, args = hp.gpu_forward(cam, sc, deg, bg=hp.PARITY_BG, kw=kw, scale_modifier=mod)
    R, color, radii, geom, binning, img, depth, opacity, n_touched = out
    P, W, H = sc["means3D"].shape[0], cam["W"], cam["H"]
    dbg = C.debug_export(P, R, W, H, geom, binning, img)
    dLc, dLd = hp.seeds(cam, seed=1)
    g = hp.gpu_backward(cam, deg, out, args, dLc, dLd)
    f = lambda x: x.detach().cpu().numpy()  # noqa: E731
    rec = dict(color=f(color), depth=f(depth), opacity=f(opacity), n_contrib=f(dbg["n_contrib"]).astype(np.uint16).reshape(H, W),
               n_touched=f(n_touched).astype(np.int32), radii=f(radii).astype(np.int32), num_rendered=np.int64(R))
    for nm, x in zip(hp.GRAD_NAMES, g):
        if x is not None:
            rec[nm] = f(x).astype(np.float32)
    return rec


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out_dir, exist_ok=True)
    for name in SCENES:
        path = os.path.join(out_dir, "device_%s.npz" % name)
        np.savez_compressed(path, **record(name))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
