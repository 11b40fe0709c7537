#!/usr/bin/env python3
"""The six device loops, run on the 160x120 / 3000-Gaussian world of tests/test_gpu_track_and_map.py, with the SHA-256 of every state
buffer after each phase.  Only constructors and methods of the public classes are used, so the same file runs in two trees (a parent and
a change) on one library, one process each; the two outputs must be equal hash for hash -- the same entry points are called with the
same arguments in the same order, so there is no floating-point freedom.

    python tools/loops_same_bits.py OUT.json
    python tools/loops_same_bits.py --compare PARENT.json CHANGE.json OUT.json
"""
import math
import types

import numpy as np

from same_bits import main, sha

W, H, F, P = 160, 120, 140.0, 3000
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1e-3, position_lr_final=1e-3, position_lr_delay_mult=1.0,
                             position_lr_max_steps=30000, feature_lr=5e-3, opacity_lr=2e-2, scaling_lr=2e-3, rotation_lr=1e-3)


def world(torch):
    from gsaj import synthetic as syn
    from gsaj.rasterizer import FrameContext

    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    cams = syn.keyframe_cameras(4, radius=0.25, W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(P, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    g = dict(means3D=t(sc["means3D"]), opacities=t(sc["opacities"]), shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    bg, M = torch.zeros(3, device=dev), sc["shs"].shape[1]
    fc = FrameContext(P, W, H, M, dev)
    frames = []
    for c in cams:
        fc.forward(bg, g["means3D"], g["opacities"], t(c["viewmatrix"]), t(c["projmatrix"]), t(c["campos"]), c["tanfovx"], c["tanfovy"],
                   sh_degree=3, shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
        frames.append((fc.color.clone(), fc.depth[0].clone()))
    w2cs = [np.ascontiguousarray(c["viewmatrix"].T).astype(np.float32) for c in cams]
    gen = torch.Generator().manual_seed(3)
    masks = [(torch.rand(1, H, W, generator=gen) < 0.6).to(torch.uint8).to(dev) for _ in cams]
    return types.SimpleNamespace(dev=dev, t=t, cams=cams, g=g, bg=bg, M=M, frames=frames, w2cs=w2cs, masks=masks, praw=t(cams[0]["projmatrix_raw"]),
                                 tan=(cams[0]["tanfovx"], cams[0]["tanfovy"]))


def two_frames(w, out, tag, tr, buffers, iterate, masked):
    """Frames 1 and 2, each started at the previous frame's true pose; masked: "given" | "edge" | None."""
    for k in (1, 2):
        kw = dict(grad_mask=w.masks[k]) if masked == "given" else dict(edge_threshold=1.1) if masked == "edge" else {}
        tr.set_frame(w.frames[k][0], w.frames[k][1], w2c=w.w2cs[k - 1], **kw)
        out["%s/frame%d/set" % (tag, k)] = {n: sha(b()) for n, b in buffers.items()}
        iterate()
        out["%s/frame%d/solved" % (tag, k)] = {n: sha(b()) for n, b in buffers.items()}


def run(torch):
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj.align import RgbdAligner
    from gsaj.gauss_newton import GaussNewtonTracker, GaussNewtonWindow, PyramidGaussNewtonTracker
    from gsaj.mapping import DeviceMapper
    from gsaj.tracking import DeviceTracker

    w, out = world(torch), {}
    head = (P, W, H, w.M, w.dev)
    cam = (w.praw, w.tan[0], w.tan[1], w.bg)
    for mode, kw in (("fused", dict(fused=True)), ("unfused", dict(fused=False)), ("graph", dict(use_graph=True))):
        for masked in ("given", "edge"):
            tr = DeviceTracker(*head, w.w2cs[0], *cam, alpha=0.9, sh_degree=3, lr_rot=0.003, lr_trans=0.002, **kw, **w.g)
            two_frames(w, out, "DeviceTracker/%s/%s" % (mode, masked), tr, dict(state=lambda: tr.pose.state, packed=lambda: tr.packed),
                       lambda: tr.iterate(6), masked)
    for joint in (False, True):
        tr = GaussNewtonTracker(*head, w.w2cs[0], *cam, alpha=0.9, sh_degree=3, solve_exposure=joint, **w.g)
        two_frames(w, out, "GaussNewtonTracker/%s" % ("solve_exposure" if joint else "plain"), tr, dict(state=lambda: tr.state),
                   lambda: tr.iterate(4), None)
    # the window: one masked slot, one inactive view; then one frame from three starts
    win = GaussNewtonWindow(3, *head, np.stack(w.w2cs[:3]), *cam, alpha=0.9, sh_degree=3, **w.g)
    for k in range(3):
        win.set_view(k, w.frames[k + 1][0], w.frames[k + 1][1], grad_mask=w.masks[k] if k == 1 else None, w2c=w.w2cs[k])
    win.active[2] = 0
    win.iterate(3)
    out["GaussNewtonWindow/views"] = dict(state=sha(win.state), best=repr(win.best()))
    win.active[2] = 1
    win.set_frame(w.frames[1][0], w.frames[1][1], w2cs=np.stack([w.w2cs[0], w.w2cs[1], w.w2cs[2]]))
    out["GaussNewtonWindow/starts/set"] = dict(state=sha(win.state), gt_color=sha(win.gt_color), grad_mask=sha(win.grad_mask))
    win.iterate(3)
    out["GaussNewtonWindow/starts/solved"] = dict(state=sha(win.state), best=repr(win.best()))
    for masked in ("given", "edge"):
        pt = PyramidGaussNewtonTracker(*head, w.w2cs[0], *cam, levels=2, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5, alpha=0.9, sh_degree=3, **w.g)
        two_frames(w, out, "PyramidGaussNewtonTracker/%s" % masked, pt, dict(state=lambda: pt.state), lambda: pt.iterate([2, 2, 2]), masked)
        out["PyramidGaussNewtonTracker/%s/level_masks" % masked] = [sha(t.grad_mask) for t in pt.trackers]
    rng = np.random.default_rng(5)
    for fused in (True, False):
        shs = w.g["shs"] + w.t(rng.normal(scale=0.05, size=tuple(w.g["shs"].shape)))
        m = GaussianModel(3)
        m._set_params(w.g["means3D"] + w.t(rng.normal(scale=0.01, size=(P, 3))), shs[:, :1], shs[:, 1:],
                      torch.logit(w.g["opacities"].clamp(0.02, 0.98)), torch.log(w.g["scales"]), w.g["rotations"].clone(), w.dev)
        m.active_sh_degree = 3
        m.init_lr(1.0)
        m.training_setup(ARGS)
        mp = DeviceMapper(m, 3, W, H, w.praw, w.tan[0], w.tan[1], w.bg, w2cs=w.w2cs[:3], fused=fused, lr_rot=0.001, lr_trans=0.001,
                          lr_exposure_a=0.01, lr_exposure_b=0.01)
        for k in range(3):
            mp.set_view(k, *w.frames[k])
        mp.iterate(3)
        tag = "DeviceMapper/%s" % ("fused" if fused else "unfused")
        out[tag] = dict(poses=sha(mp.poses.state), scalars=sha(mp.scalars),
                        **{n: sha(getattr(m, "_" + n)) for n in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")})
    al = RgbdAligner(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, w.dev, levels=2)
    al.set_reference(w.frames[0][0], w.frames[0][1], w.w2cs[0])
    ran = al.align(*w.frames[1])
    out["RgbdAligner"] = dict(state=sha(al.state), row=sha(al.row), ran=ran)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    main("loops_same_bits", run, "tools/loops_same_bits.py in a tree of the parent commit and in this tree, one process each, the same library: "
         "SHA-256 of every state buffer of the six device loops after each phase", unit="phases", one_library=True)
