"""GPU: the last-workgroup hand-off (csrc/last_block.h) of its five users over a ladder of workgroup counts -- 1 (the arriver is
itself last), 2, 256 (one full trip of the last workgroup's load loop), 257 and 513 (one and two trips with a ragged end); see
tests/last_block_ladder.py for the sizes.  Every case runs input A, a clearly different input B, and A again on the SAME workspace
and context: the reading CU's cache is warm with the previous run's partials and the ticket has been used, which is where a stale
partial would show.  The third run's outputs equal the first's bit for bit, and every run is checked with the comparator the suite
already has for that entry point (tests/test_cpu_last_block.py shows that each rejects a partial left out or taken from B).

Counts other tests already produce with a single input (32x32 and 37x29 in test_gpu_loss.py: 1 and 2; P = 256, 257 of the isotropic
loss: 1 and 2; n = 257 in test_gpu_knn.py: 2) are run again here because of the A, B, A sequence."""
import numpy as np
import pytest

import last_block_ladder as lb
import loss_restated as lr

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dtype=None):
    import torch
    return None if a is None else torch.as_tensor(np.array(a), dtype=dtype or torch.float32, device=_dev())


def _np(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


def same_bits(first, third, tag):
    for k in first:
        assert first[k].tobytes() == third[k].tobytes(), "%s: %s of the third run (A after B) differs from the first" % (tag, k)


# Each runner: [A, B, A] outputs (name -> NumPy array) from ONE workspace / context.
def run_loss(W, H):
    import torch
    from gsaj import losses

    ls, f, outs = losses.LossSeeds(W, H, _dev()), torch.float32, []
    for fr in (lb.loss_frames(W, H) * 2)[:3]:
        o = ls(int(fr["flags"]), float(fr["alpha"]), float(fr["rgb_thr"]), _t(fr["image"], f), _t(fr["depth"], f), _t(fr["opacity"], f),
               _t(fr["gt"], f), _t(fr["gt_depth"], f), _t(fr["mask"], torch.uint8), _t([fr["a"]], f), _t([fr["b"]], f), want_opacity_grad=True)
        outs.append(_np({k: v for k, v in o.items() if v is not None}))
    return outs


def run_iso(P):
    from gsaj.losses import IsotropicLoss

    iso, outs = IsotropicLoss(P, _dev()), []
    for c in (lb.iso_cases(P) * 2)[:3]:
        loss, g = iso(_t(c["scales"]), weight=lr.ISO_WEIGHT)
        outs.append(_np(dict(loss=loss, dL_dscales=g)))
    return outs


def run_ssim(N, C, W, H):
    import torch
    from gsaj import _lib

    lib = _lib.load()
    ws = torch.zeros(lib.gsaj_ssim_workspace_bytes(N, C, W, H), dtype=torch.uint8, device=_dev())   # zeroed once, as the contract says
    s, outs = torch.cuda.current_stream().cuda_stream, []
    for c in (lb.ssim_pairs(N, C, W, H) * 2)[:3]:
        x, y = _t(c["x"]), _t(c["y"])
        out, smap = torch.empty(N + 1, device=_dev()), torch.empty_like(x)
        _lib.check(lib.gsaj_ssim_forward(N, C, W, H, x.data_ptr(), y.data_ptr(), out.data_ptr(), smap.data_ptr(), ws.data_ptr(), s), "fwd")
        torch.cuda.synchronize()
        outs.append(_np(dict(ssim_out=out, ssim_map=smap)))
    return outs


def run_knn(n):
    import torch
    from gsaj import _lib

    lib = _lib.load()
    ws = torch.empty(lib.gsaj_dist2_workspace_bytes(n), dtype=torch.uint8, device=_dev())
    s, outs = torch.cuda.current_stream().cuda_stream, []
    for p in (lb.knn_points(n) * 2)[:3]:
        pts, out = _t(p), torch.empty(n, dtype=torch.float32, device=_dev())
        codes, idx = torch.empty(n, dtype=torch.int32, device=_dev()), torch.empty(n, dtype=torch.int32, device=_dev())
        _lib.check(lib.gsaj_dist2(n, pts.data_ptr(), out.data_ptr(), ws.data_ptr(), s), "gsaj_dist2")
        _lib.check(lib.gsaj_debug_dist2_order(n, ws.data_ptr(), codes.data_ptr(), idx.data_ptr(), s), "gsaj_debug_dist2_order")
        outs.append(_np(dict(dist2=out, codes=codes, idx=idx)))
    return outs


def bwd_inputs(P):
    """(cam, [A, B]): two scenes of P small Gaussians in front of a 64x48 camera, each with pixel-gradient seeds of its own."""
    import helpers as hp
    from gsaj import synthetic as syn

    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=lb.BWD_W, H=lb.BWD_H, fx=56.0, fy=56.0, cx=31.5, cy=23.5)
    small = (np.log(0.002), np.log(0.02))
    return cam, [(syn.make_scene(P, seed, cam, z_range=(1.0, 5.0), log_scale_range=small, sh_coeffs=1), hp.seeds(cam, seed=seed)) for seed in (41, 42)]


def run_bwd(P):
    import torch
    from gsaj.rasterizer import FrameContext

    cam, scenes = bwd_inputs(P)
    fc = FrameContext(P, cam["W"], cam["H"], 1, _dev(), per_gaussian_tau=True)
    bg, view, proj, praw, campos = (_t(a) for a in (np.zeros(3), cam["viewmatrix"], cam["projmatrix"], cam["projmatrix_raw"], cam["campos"]))
    outs = []
    for sc, (dLc, dLd) in (scenes * 2)[:3]:
        kw = dict(shs=_t(sc["shs"]), scales=_t(sc["scales"]), rotations=_t(sc["rotations"]))
        means = _t(sc["means3D"])
        fc.forward(bg, means, _t(sc["opacities"]), view, proj, campos, cam["tanfovx"], cam["tanfovy"], sh_degree=0, **kw)
        g = fc.backward(bg, means, view, proj, praw, campos, cam["tanfovx"], cam["tanfovy"], _t(dLc), _t(dLd), sh_degree=0, **kw)
        torch.cuda.synchronize()
        outs.append(_np(dict(tau=g["tau"], tau_sum=g["tau_sum"], mean3D=g["mean3D"])))
    return outs


@pytest.mark.parametrize("W,H", lb.LOSS_SIZES)
def test_loss_seeds(W, H):
    outs, frames = run_loss(W, H), lb.loss_frames(W, H)
    for o, fr, nm in zip(outs, frames, "AB"):
        print(nm, lr.assert_loss_close(o, fr["want"], "%dx%d input %s" % (W, H, nm)))
    same_bits(outs[0], outs[2], "loss %dx%d" % (W, H))


@pytest.mark.parametrize("P", lb.ISO_P)
def test_isotropic_loss(P):
    outs, cases = run_iso(P), lb.iso_cases(P)
    for o, c, nm in zip(outs, cases, "AB"):
        print(nm, lr.assert_iso_close(o["loss"], o["dL_dscales"], c["want"], "isotropic P %d input %s" % (P, nm)))
    same_bits(outs[0], outs[2], "isotropic P %d" % P)


@pytest.mark.parametrize("N,C,W,H", lb.SSIM_CASES)
def test_ssim_forward(N, C, W, H):
    outs, cases = run_ssim(N, C, W, H), lb.ssim_pairs(N, C, W, H)
    for o, c, nm in zip(outs, cases, "AB"):
        tag = "ssim %dx%dx%dx%d input %s" % (N, C, W, H, nm)
        assert np.all(np.abs(o["ssim_map"] - c["S64"]) <= c["bound"]), tag
        lb.assert_ssim_means(o["ssim_out"], c, tag)
    same_bits(outs[0], outs[2], "ssim %dx%dx%dx%d" % (N, C, W, H))


@pytest.mark.parametrize("n", lb.KNN_N)
def test_bounding_box(n):
    outs, pts = run_knn(n), lb.knn_points(n)
    for o, p, nm in zip(outs, pts, "AB"):
        lb.assert_knn_order(o["codes"], o["idx"], p, lb.knn_box(lb.knn_box_partials(p)), "n %d input %s" % (n, nm))
    same_bits(outs[0], outs[2], "knn n %d" % n)


@pytest.mark.parametrize("P", lb.BWD_P)
def test_backward_tau_sum(P):
    outs = run_bwd(P)
    for o, nm in zip(outs, "AB"):
        assert np.abs(o["tau"]).sum() > 0, "no Gaussian of input %s reached a pixel" % nm
        lb.assert_tau_sum(o["tau_sum"], o["tau"], "P %d input %s" % (P, nm))
    same_bits(outs[0], outs[2], "backward P %d" % P)
