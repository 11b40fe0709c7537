"""Regenerates tests/golden/grad_mask_*.npz from a checkout of the reference:

    python tests/golden/make_grad_mask_goldens.py /path/to/reference

Inputs and recorded outputs only.  The outputs come from the reference's own functions, imported and run on CPU tensors:
utils/slam_utils.image_gradient and image_gradient_mask on the gray image, and utils/camera_utils.Camera.compute_grad_mask, called
unbound on a SimpleNamespace(original_image=..., grad_mask=None) with Dataset.type "replica" (the 32x32 block form) and "tum"
(the global form), edge_threshold 1.1 and 4.  The two helpers hard-code device="cuda"; torch.tensor and torch.ones are wrapped
while they run so that the constant lands on the CPU.  `intensity` is sqrt((gv mask_v)^2 + (gh mask_h)^2) of the recorded
gradients, the tensor compute_grad_mask forms before it thresholds.

The scenes are tests/grad_mask_restated.make_scene (a generator of inputs, nothing of the method under test).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

THRESHOLDS = (1.1, 4.0)
CASES = (  # name, scene, H, W
    ("noise_64x96", "noise", 64, 96), ("noise_68x100", "noise", 68, 100), ("noise_97x131", "noise", 97, 131),
    ("noise_100x170", "noise", 100, 170), ("checker_68x100", "checker", 68, 100), ("dyadic_68x100", "dyadic", 68, 100),
    ("bright_68x100", "bright", 68, 100),
)


def _on_cpu(fn):
    def wrapped(*a, **k):
        if k.get("device") == "cuda":
            k["device"] = "cpu"
        return fn(*a, **k)
    return wrapped


def main(ref):
    import grad_mask_restated as gr

    sys.path.insert(0, ref)
    from utils.camera_utils import Camera
    from utils.slam_utils import image_gradient, image_gradient_mask

    saved = torch.tensor, torch.ones
    torch.tensor, torch.ones = _on_cpu(torch.tensor), _on_cpu(torch.ones)
    try:
        for name, kind, H, W in CASES:
            image = gr.make_scene(kind, H, W)
            timg = torch.from_numpy(image)
            gray = timg.mean(dim=0, keepdim=True)
            gv, gh = image_gradient(gray)
            mv, mh = image_gradient_mask(gray)
            assert torch.equal(mv, mh)
            inten = torch.sqrt((gv * mv) ** 2 + (gh * mh) ** 2)
            out = dict(image=image, gray=gray[0].numpy(), gv=gv[0].numpy(), gh=gh[0].numpy(), valid=mv[0].numpy(),
                       intensity=inten[0].numpy(), thresholds=np.asarray(THRESHOLDS, np.float64))
            for i, thr in enumerate(THRESHOLDS):
                for mode, dtype in (("tum", torch.bool), ("replica", torch.float32)):
                    cam = SimpleNamespace(original_image=timg.clone(), grad_mask=None)
                    Camera.compute_grad_mask(cam, {"Training": {"edge_threshold": thr}, "Dataset": {"type": mode}})
                    assert cam.grad_mask.dtype == dtype and tuple(cam.grad_mask.shape) == (1, H, W)
                    out["%s_%d" % ("global" if mode == "tum" else "block", i)] = cam.grad_mask[0].numpy()
            np.savez_compressed(os.path.join(HERE, "grad_mask_%s.npz" % name), **out)
            print(name, "kept global", [int(out["global_%d" % i].sum()) for i in range(2)], "block",
                  [int((out["block_%d" % i] == 1).sum()) for i in range(2)])
    finally:
        torch.tensor, torch.ones = saved


if __name__ == "__main__":
    main(sys.argv[1])
