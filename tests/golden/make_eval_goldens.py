#!/usr/bin/env python3
"""Golden vectors for the per-frame rendering metrics (tests/golden/eval_*.npz).

Usage: make_eval_goldens.py <path of a checkout of the reference>   (or GSAJ_REFERENCE in the environment)

Needs the reference's source, which is not part of this repository.  Its modules import cv2, evo, wandb and torchmetrics at module
level, none of which this needs, so the files are parsed and only these nodes are executed on CPU tensors in float32:
  gaussian_splatting/utils/image_utils.py   psnr
  gaussian_splatting/utils/loss_utils.py    gaussian, create_window, ssim, _ssim
  utils/eval_utils.py                       the statements of eval_rendering's loop body on lines 141-155 (clamp, the two 8-bit
                                            pictures, the mask, psnr, ssim; the render of line 140 and LPIPS of 156 are not among them)
cv2.cvtColor(a, cv2.COLOR_BGR2RGB) is replaced by the index reversal a[..., ::-1] it is (for one channel: the identity).
Only inputs and outputs are stored:
  image, gt           the render and the ground truth [C,H,W] float32
  psnr, ssim          psnr_score, ssim_score as float32 (psnr may be inf or NaN)
  n                   mask.sum()
  pred_u8, gt_u8      what the loop appended to img_pred / img_gt: [H,W,C] uint8, channels reversed
"""
import ast
import os
import sys
from math import exp

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST_LINE, LAST_LINE = 141, 155


def functions(path, keep, ns):
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    mod = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in keep], type_ignores=[])
    exec(compile(mod, path, "exec"), ns)
    return ns


class _Cv2:
    COLOR_BGR2RGB = "bgr2rgb"

    @staticmethod
    def cvtColor(a, code):
        assert code == _Cv2.COLOR_BGR2RGB
        return np.ascontiguousarray(a[..., ::-1])


def load_reference(ref):
    ns = {"torch": torch, "F": F, "exp": exp, "Variable": Variable, "np": np, "cv2": _Cv2}
    functions(os.path.join(ref, "gaussian_splatting", "utils", "image_utils.py"), {"psnr"}, ns)
    functions(os.path.join(ref, "gaussian_splatting", "utils", "loss_utils.py"), {"gaussian", "create_window", "ssim", "_ssim"}, ns)
    path = os.path.join(ref, "utils", "eval_utils.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "eval_rendering")
    loop = next(n for n in fn.body if isinstance(n, ast.For))
    body = [s for s in loop.body if FIRST_LINE <= s.lineno <= LAST_LINE]
    targets = [ast.unparse(s).split("=")[0].strip() for s in body if isinstance(s, ast.Assign)]
    assert targets == ["image", "gt", "pred", "gt", "pred", "mask", "psnr_score", "ssim_score"], targets
    return ns, compile(ast.Module(body=body, type_ignores=[]), path, "exec")


def cases():
    rng = np.random.default_rng(20261019)
    gt = rng.uniform(0.05, 1.0, (3, 40, 56)).astype(np.float32)
    gt[rng.uniform(size=gt.shape) < 0.3] = 0.0  # single channel values: the mask differs by channel at most pixels
    yield "noise_3x40x56", (gt + rng.uniform(-0.4, 0.4, gt.shape)).astype(np.float32), gt
    g = rng.uniform(0.0, 1.0, (1, 17, 15)).astype(np.float32)
    g[0, 3:6, 2:9] = 0.0
    yield "gray_1x17x15", (0.9 * g + rng.normal(0.05, 0.1, g.shape)).astype(np.float32), g
    b = rng.uniform(0.1, 0.9, (3, 16, 16)).astype(np.float32)
    yield "identical_3x16x16", b.copy(), b
    yield "black_gt_3x8x8", rng.uniform(0, 1, (3, 8, 8)).astype(np.float32), np.zeros((3, 8, 8), np.float32)
    d = rng.uniform(0, 1, (3, 5, 7)).astype(np.float32)
    d[1, 2, 3] = 0.0
    yield "tiny_3x5x7", rng.uniform(-0.2, 1.2, d.shape).astype(np.float32), d


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GSAJ_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    ns, code = load_reference(ref)
    for name, image, gt in cases():
        env = dict(ns, rendering=torch.tensor(image), gt_image=torch.tensor(gt), img_pred=[], img_gt=[])
        exec(code, env)
        out = dict(image=image, gt=gt, psnr=np.float32(env["psnr_score"].item()), ssim=np.float32(env["ssim_score"].item()),
                   n=np.int64(env["mask"].sum().item()), pred_u8=env["img_pred"][0], gt_u8=env["img_gt"][0])
        path = os.path.join(HERE, "eval_%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%s: psnr %s ssim %.6f n %d of %d (%d bytes)" % (path, out["psnr"], out["ssim"], out["n"], image.size, os.path.getsize(path)))


if __name__ == "__main__":
    main()
