#!/usr/bin/env python3
"""Golden vectors for SSIM and the colour-refinement loss (tests/golden/ssim_*.npz).

Runs ONLY in the build container (needs the reference checkout at /root/reference).  The reference's
gaussian_splatting/utils/loss_utils.py imports cv2 at module level, which is not installed here, so the file is parsed and only
the FunctionDef nodes gaussian, create_window, ssim, _ssim and l1_loss are executed (with torch, F, exp and Variable in scope).
Everything is evaluated under CPU autograd in float32, as the reference runs.  Only inputs and outputs are stored:
  img1, img2                 the inputs ([C,H,W] or [N,C,H,W], float32)
  ssim, dssim                ssim(img1, img2) (size_average=True) and its gradient w.r.t. img1
  loss, dloss                (1 - 0.2) * l1_loss + 0.2 * (1 - ssim) and its gradient w.r.t. img1 (lambda_dssim = 0.2)
  ssim_n, wn, dssim_n        4-D cases only: ssim(..., size_average=False) [N], weights wn [N], d(wn . ssim_n)/dimg1
"""
import ast
import os
from math import exp

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/gaussian_splatting/utils/loss_utils.py"
LAMBDA = 0.2


def load_reference():
    with open(REF) as fh:
        tree = ast.parse(fh.read(), REF)
    keep = {"gaussian", "create_window", "ssim", "_ssim", "l1_loss"}
    mod = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in keep], type_ignores=[])
    ns = {"torch": torch, "F": F, "exp": exp, "Variable": Variable}
    exec(compile(mod, REF, "exec"), ns)
    return ns


def cases():
    rng = np.random.default_rng(20261016)
    a = rng.uniform(0, 1, (3, 48, 64)).astype(np.float32)
    yield "random_3x48x64", a, np.clip(a + rng.normal(0, 0.15, a.shape), 0, 1).astype(np.float32)
    yy, xx = np.mgrid[0:40, 0:56].astype(np.float32)
    s = np.stack([0.5 + 0.4 * np.sin(xx / 9 + c) * np.cos(yy / 7 - c) for c in range(3)]).astype(np.float32)
    yield "smooth_3x40x56", s, (s + rng.normal(0, 1e-3, s.shape)).astype(np.float32)
    b = rng.uniform(0, 1, (3, 32, 32)).astype(np.float32)
    yield "identical_3x32x32", b, b.copy()
    c1 = np.broadcast_to(np.array([0.2, 0.5, 0.9], np.float32)[:, None, None], (3, 24, 40)).copy()
    c2 = np.broadcast_to(np.array([0.25, 0.5, 0.7], np.float32)[:, None, None], (3, 24, 40)).copy()
    yield "constant_3x24x40", c1, c2
    d = rng.uniform(0, 1, (3, 5, 7)).astype(np.float32)
    yield "small_3x5x7", d, rng.uniform(0, 1, d.shape).astype(np.float32)
    e = rng.uniform(0, 1, (2, 3, 24, 32)).astype(np.float32)
    yield "batch_2x3x24x32", e, np.clip(e + rng.normal(0, 0.2, e.shape), 0, 1).astype(np.float32)
    f = rng.uniform(0, 1, (1, 40, 36)).astype(np.float32)
    yield "gray_1x40x36", f, np.clip(0.8 * f + rng.normal(0.1, 0.1, f.shape), 0, 1).astype(np.float32)


def main():
    ref = load_reference()
    for name, img1, img2 in cases():
        out = {"img1": img1, "img2": img2}
        t2 = torch.tensor(img2)
        x = torch.tensor(img1, requires_grad=True)
        s = ref["ssim"](x, t2)
        s.backward()
        out["ssim"], out["dssim"] = np.float32(s.item()), x.grad.numpy().copy()
        x = torch.tensor(img1, requires_grad=True)
        loss = (1.0 - LAMBDA) * ref["l1_loss"](x, t2) + LAMBDA * (1.0 - ref["ssim"](x, t2))
        loss.backward()
        out["loss"], out["dloss"] = np.float32(loss.item()), x.grad.numpy().copy()
        if img1.ndim == 4:
            x = torch.tensor(img1, requires_grad=True)
            sn = ref["ssim"](x, t2, size_average=False)
            wn = np.array([0.7, -1.3], np.float32)[:img1.shape[0]]
            (sn * torch.tensor(wn)).sum().backward()
            out["ssim_n"], out["wn"], out["dssim_n"] = sn.detach().numpy(), wn, x.grad.numpy().copy()
        path = os.path.join(HERE, "ssim_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%s: ssim %.6f loss %.6f (%d bytes)" % (path, out["ssim"], out["loss"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
