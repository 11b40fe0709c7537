#!/usr/bin/env python3
"""One colour-refinement iteration (reference utils/slam_backend.py:320-352: render -> (1 - 0.2) L1 + 0.2 (1 - SSIM) ->
backward -> Adam on the Gaussian parameters) on cfg2 (synthetic scene, 640x480), three ways:
  A. drop-in render() + the reference's torch SSIM (five depthwise F.conv2d) + L1 + .backward()
  B. the same with gsaj.ssim (HIP forward + backward kernels)
  C. FrameContext.forward -> RefinementLoss (gsaj_refine_loss_seeds) -> FrameContext.backward -> parameter .grad in closed form
Each adds the same fused torch.optim.Adam step.  Prints ms per iteration (synchronised wall clock over n iterations) and the
time of the SSIM loss + seeds alone (torch autograd vs the two kernels)."""
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gaussian_splatting.gaussian_renderer import render  # noqa: E402
from gaussian_splatting.scene.gaussian_model import GaussianModel  # noqa: E402
from gsaj import losses, ssim as gssim, synthetic as syn  # noqa: E402
from gsaj.rasterizer import FrameContext  # noqa: E402
from utils.camera_utils import Camera  # noqa: E402

LAMBDA = 0.2


def torch_ssim(img1, img2):
    """SSIM as the reference computes it (gaussian_splatting/utils/loss_utils.py:42-101): 11x11 window, depthwise conv2d."""
    C = img1.shape[-3]
    g = torch.tensor([math.exp(-((x - 5) ** 2) / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).expand(C, 1, 11, 11).contiguous().to(img1)
    conv = lambda x: F.conv2d(x, w, padding=5, groups=C)  # noqa: E731
    m1, m2 = conv(img1), conv(img2)
    s1, s2, s12 = conv(img1 * img1) - m1 * m1, conv(img2 * img2) - m2 * m2, conv(img1 * img2) - m1 * m2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))).mean()


class Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device("cuda:0")
    cam, sc = syn.config_scene("cfg2")
    W, H = cam["W"], cam["H"]
    model = GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"], sh_degree=3,
                                         device=dev)
    view = Camera.from_synthetic(cam, device=dev)
    view.cam_rot_delta.requires_grad_(False)
    view.cam_trans_delta.requires_grad_(False)
    bg = torch.zeros(3, device=dev)
    gt = torch.as_tensor(np.random.default_rng(0).uniform(0, 1, (3, H, W)), dtype=torch.float32, device=dev)
    # lr 0: the timing must not depend on where the parameters drift; the fused Adam step still runs in full
    opt = torch.optim.Adam(model.parameters(), lr=0.0, fused=True)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    def dropin(ssim_fn):
        def it():
            img = render(view, model, Pipe, bg)["render"]
            loss = (1.0 - LAMBDA) * gssim.l1_loss(img, gt) + LAMBDA * (1.0 - ssim_fn(img, gt))
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return it

    P, M = sc["means3D"].shape[0], sc["shs"].shape[1]
    ctx = FrameContext(P, W, H, M, dev)
    rl = losses.RefinementLoss(W, H, dev, lambda_dssim=LAMBDA)
    tx, ty = math.tan(0.5 * view.FoVx), math.tan(0.5 * view.FoVy)

    def iter_c():
        with torch.no_grad():
            xyz, op, fe, s, r = (model.get_xyz.contiguous(), model.get_opacity.contiguous(), model.get_features.contiguous(),
                                 model.get_scaling.contiguous(), model.get_rotation.contiguous())
            ctx.forward(bg=bg, means3D=xyz, opacities=op, viewmatrix=view.world_view_transform, projmatrix=view.full_proj_transform,
                        campos=view.camera_center, tanfovx=tx, tanfovy=ty, sh_degree=3, shs=fe, scales=s, rotations=r, sync=False)
            o = rl(ctx.color, gt)
            g = ctx.backward(bg=bg, means3D=xyz, viewmatrix=view.world_view_transform, projmatrix=view.full_proj_transform,
                             projmatrix_raw=view.projection_matrix, campos=view.camera_center, tanfovx=tx, tanfovy=ty,
                             dL_dcolor=o["dL_dcolor"], dL_ddepth=zero_depth, sh_degree=3, shs=fe, scales=s, rotations=r)
            model.assign_bucket_gradients(g)
        opt.step()
        opt.zero_grad(set_to_none=True)

    zero_depth = torch.zeros((1, H, W), device=dev)
    with torch.no_grad():  # a synchronous first frame sizes the arena of the asynchronous ones
        ctx.forward(bg=bg, means3D=model.get_xyz.contiguous(), opacities=model.get_opacity.contiguous(),
                    viewmatrix=view.world_view_transform, projmatrix=view.full_proj_transform, campos=view.camera_center, tanfovx=tx,
                    tanfovy=ty, sh_degree=3, shs=model.get_features.contiguous(), scales=model.get_scaling.contiguous(),
                    rotations=model.get_rotation.contiguous())

    # the loss + pixel seeds alone, on a fixed image
    img0 = ctx.color.clone()

    def loss_torch():
        x = img0.detach().requires_grad_(True)
        ((1.0 - LAMBDA) * gssim.l1_loss(x, gt) + LAMBDA * (1.0 - torch_ssim(x, gt))).backward()

    def loss_gsaj():
        rl(img0, gt)

    ms_lt, ms_lg = timed(loss_torch), timed(loss_gsaj)
    ms_a, ms_b, ms_c = timed(dropin(torch_ssim)), timed(dropin(gssim.ssim)), timed(iter_c)
    print("refinement loss + dL/dcolor alone, 640x480x3: torch autograd (conv2d SSIM) %.3f ms | gsaj_refine_loss_seeds %.3f ms"
          % (ms_lt, ms_lg))
    print("colour-refinement iteration, cfg2 (%d Gaussians, %dx%d), incl. fused Adam: A drop-in + torch SSIM %.3f ms | "
          "B drop-in + gsaj.ssim %.3f ms | C FrameContext + RefinementLoss %.3f ms" % (P, W, H, ms_a, ms_b, ms_c))


if __name__ == "__main__":
    main()
