"""GPU: the SSIM kernels (gsaj_ssim_forward / _backward) and the colour-refinement loss (gsaj_refine_loss_seeds) against the
reference's fixtures (tests/golden/ssim_*.npz) and the fp64 restatement (tests/ssim_restated.py); negative canaries that show the
comparator rejects gradients of the wrong semantics; bit-reproducibility; gsaj.ssim under autograd, through render() and through
RefinementLoss + FrameContext.backward; a short colour refinement against one that uses a torch SSIM.

Tolerance (fp32 kernels against fp64).  Every blurred moment E[x^2], E[y^2], E[xy] of inputs in [0, 1] is at most 1 and is a sum
of 121 products accumulated as 11 + 11 fp32 additions (horizontal, then vertical), so its rounding error is at most about
22 u with u = 2^-24; the subtraction E[x^2] - mu^2 adds about 2 u more.  Round up to DELTA = 32 u ~ 1.9e-6 absolute on each of
sigma1^2, sigma2^2, sigma12.  Where the images are locally flat these are ~0 and the denominator D = sigma1^2 + sigma2^2 + C2 is
only C2 = 9e-4, so D (and B = 2 sigma12 + C2) are relatively wrong by up to 2 DELTA / C2 ~ 4.2e-3.  Hence:
  * per pixel, S moves by at most DELTA (|dS/dE[xy]| + 2 |dS/dE[x^2]|) -- evaluated with the fp64 partials at that pixel --
    plus a few u for S itself; the mean moves by at most the mean of that bound;
  * the gradient is a sum of the partials (each ~1/D or ~1/D^2 relative error 2 DELTA / C2 and 4 DELTA / C2) times blurs, so
    per pixel it is relatively wrong by at most GRAD_TOL = 4 DELTA / C2 ~ 8.5e-3, measured against max|g| (the mean divides
    every gradient by N*C*H*W, so raw values carry no scale of their own).
The negative canaries below show that this bound still rejects gradients with the wrong padding, a shifted window or a dropped
L1 term, by a factor of several at least.
"""
import glob
import math
import os

import numpy as np
import pytest

import ssim_restated as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ssim_*.npz")))
U = 2.0 ** -24
DELTA = 32 * U
GRAD_TOL = 4 * DELTA / sr.C2


def grad_err(g, ref):
    return float(np.abs(np.asarray(g, np.float64) - ref).max() / max(np.abs(ref).max(), 1.0 / ref.size))


def map_bound(partials, S):
    _, dxx, dxy = partials
    return DELTA * (np.abs(dxy) + 2 * np.abs(dxx)) + 4 * U * np.abs(S) + 4 * U


def _dev():
    import torch

    return torch.device("cuda:0")


def _t(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=_dev())


def run_kernels(a, b, dL_dssim=None):
    """[N,C,H,W] -> (ssim_out [N+1], ssim_map, dL/dimg for the upstream dL_dssim [N+1] (default: d mean)) from the C ABI."""
    import torch
    from gsaj import _lib

    lib = _lib.load()
    N, C, H, W = a.shape
    ws = torch.zeros(lib.gsaj_ssim_workspace_bytes(N, C, W, H), dtype=torch.uint8, device=_dev())
    x, y = _t(a), _t(b)
    out = torch.empty(N + 1, device=_dev())
    smap = torch.empty_like(x)
    g = torch.empty_like(x)
    up = np.zeros(N + 1, np.float32)
    up[N] = 1.0
    up = _t(up if dL_dssim is None else dL_dssim)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gsaj_ssim_forward(N, C, W, H, x.data_ptr(), y.data_ptr(), out.data_ptr(), smap.data_ptr(), ws.data_ptr(), s), "fwd")
    _lib.check(lib.gsaj_ssim_backward(N, C, W, H, x.data_ptr(), y.data_ptr(), up.data_ptr(), g.data_ptr(), ws.data_ptr(), s), "bwd")
    torch.cuda.synchronize()
    return out.cpu().numpy(), smap.cpu().numpy(), g.cpu().numpy(), ws


def run_refine(a, b, lam=0.2):
    import torch
    from gsaj import losses

    H, W = a.shape[1:]
    rl = losses.RefinementLoss(W, H, _dev(), lambda_dssim=lam)
    o = rl(_t(a), _t(b))
    torch.cuda.synchronize()
    return rl.scalars.cpu().numpy(), o["dL_dcolor"].cpu().numpy(), rl


def scene_pair(W, H, seed):
    """Rendered-looking pair: smooth shading + texture noise + a flat patch (sigma ~ 0) + a hard edge, and a perturbed copy."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([0.5 + 0.4 * np.sin(xx / (11 + 3 * c) + c) * np.cos(yy / (17 - c) - c) for c in range(3)])
    a = a + rng.normal(0, 0.05, a.shape)
    a[:, H // 4:H // 2, W // 3:W // 2] = 0.3
    a[:, :, 3 * W // 4:] *= 0.5
    a = np.clip(a, 0, 1).astype(np.float32)
    b = np.clip(a + rng.normal(0, 0.04, a.shape), 0, 1).astype(np.float32)
    b[:, H // 4:H // 2, W // 3:W // 2] = 0.32
    return a, b


# ---- 1. the reference's fixtures -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_kernels_match_reference_fixtures(path):
    z = np.load(path)
    a, b = z["img1"], z["img2"]
    a4, b4 = (a, b) if a.ndim == 4 else (a[None], b[None])
    N = a4.shape[0]
    out, smap, g, _ = run_kernels(a4, b4)
    S64, parts = sr.ssim_forward(a4, b4)
    bound = map_bound(parts, S64)
    # the fixture itself is fp32 arithmetic (2-D conv): allow both roundings
    assert abs(out[N] - z["ssim"]) <= 2 * bound.mean() + 1e-6, (out[N], z["ssim"])
    assert np.all(np.abs(smap - S64) <= bound), np.abs(smap - S64).max()
    assert grad_err(g.reshape(a.shape), z["dssim"]) < GRAD_TOL
    if a.ndim == 4:
        assert np.all(np.abs(out[:N] - z["ssim_n"]) <= 2 * bound.reshape(N, -1).mean(axis=1) + 1e-6)
        up = np.append(z["wn"], np.float32(0))
        _, _, gn, _ = run_kernels(a4, b4, up)
        assert grad_err(gn, z["dssim_n"]) < GRAD_TOL
    elif a.shape[0] == 3:  # colour refinement is defined on RGB images
        sc, dcol, _ = run_refine(a, b)
        assert abs(sc[0] - z["loss"]) <= 2 * 0.2 * bound.mean() + 1e-6, (sc, z["loss"])
        assert grad_err(dcol, z["dloss"]) < GRAD_TOL


def test_gsaj_ssim_autograd_matches_fixtures():
    import torch
    from gsaj import ssim as gssim

    for path in FIXTURES:
        z = np.load(path)
        x = _t(z["img1"]).requires_grad_(True)
        y = _t(z["img2"])
        s = gssim.ssim(x, y)
        assert s.dim() == 0
        s.backward()
        assert grad_err(x.grad.cpu().numpy(), z["dssim"]) < GRAD_TOL, path
        x.grad = None
        loss = 0.8 * gssim.l1_loss(x, y) + 0.2 * (1.0 - gssim.ssim(x, y))
        loss.backward()
        assert grad_err(x.grad.cpu().numpy(), z["dloss"]) < GRAD_TOL, path
        assert abs(float(loss) - float(z["loss"])) < 1e-4
        if x.dim() == 4:
            x.grad = None
            sn = gssim.ssim(x, y, size_average=False)
            assert tuple(sn.shape) == (x.shape[0],)
            (sn * _t(z["wn"])).sum().backward()
            assert grad_err(x.grad.cpu().numpy(), z["dssim_n"]) < GRAD_TOL, path
            np.testing.assert_allclose(sn.detach().cpu().numpy(), z["ssim_n"], atol=5e-4)
        m = gssim.ssim_map(x.detach(), y)
        assert m.shape == x.shape
        torch.cuda.synchronize()


# ---- 2. the fp64 restatement at full size --------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,seed", [(640, 480, 1), (640, 480, 2), (641, 479, 3), (1280, 720, 4), (33, 17, 5)])
def test_kernels_match_fp64_restatement(W, H, seed):
    a, b = scene_pair(W, H, seed)
    out, smap, g, _ = run_kernels(a[None], b[None])
    S64, parts = sr.ssim_forward(a[None], b[None])
    bound = map_bound(parts, S64)
    assert np.all(np.abs(smap - S64) <= bound), float(np.abs(smap - S64).max())
    assert abs(out[1] - S64.mean()) <= bound.mean() and abs(out[0] - S64.mean()) <= bound.mean()
    g64 = sr.ssim_backward(a[None], b[None], parts, 1.0 / S64.size)
    assert grad_err(g, g64) < GRAD_TOL
    sc, dcol, _ = run_refine(a, b)
    loss64, l164, s64, gl64 = sr.refine_loss(a, b)
    assert abs(sc[1] - l164) < 1e-6 and abs(sc[2] - s64) <= bound.mean() and abs(sc[0] - loss64) <= 0.2 * bound.mean() + 1e-6
    assert grad_err(dcol, gl64) < GRAD_TOL


# ---- 3. negative canaries: the same comparator rejects the wrong semantics -------------------------------------------------
def test_comparator_rejects_wrong_semantics():
    a, b = scene_pair(640, 480, 7)
    _, dcol, _ = run_refine(a, b)
    _, _, _, good = sr.refine_loss(a, b)
    assert grad_err(dcol, good) < GRAD_TOL
    for kw in (dict(pad="edge"), dict(shift=1), dict(l1_sign=False)):
        _, _, _, wrong = sr.refine_loss(a, b, **kw)
        e = grad_err(dcol, wrong)
        assert e > 3 * GRAD_TOL, (kw, e, GRAD_TOL)


# ---- 4. bit-reproducible, ticket reset ----------------------------------------------------------------------------------
def test_two_calls_identical_bits_and_ticket_reset():
    import torch
    from gsaj import _lib

    a, b = scene_pair(641, 479, 8)
    a4, b4 = np.stack([a, b]), np.stack([b, a])
    out1, m1, g1, ws = run_kernels(a4, b4)
    out2, m2, g2, _ = run_kernels(a4, b4)
    assert np.array_equal(out1, out2) and np.array_equal(m1, m2) and np.array_equal(g1, g2)
    # the ticket (first word of the 256-byte-aligned workspace) is back to zero after the launch
    base = (ws.data_ptr() + 255) & ~255
    ticket = ws[base - ws.data_ptr():base - ws.data_ptr() + 4].cpu().numpy().view(np.uint32)[0]
    assert ticket == 0
    sc1, d1, rl = run_refine(a, b)
    o = rl(_t(a), _t(b))
    torch.cuda.synchronize()
    assert np.array_equal(sc1, rl.scalars.cpu().numpy()) and np.array_equal(d1, o["dL_dcolor"].cpu().numpy())
    assert _lib.load().gsaj_version() >= 101


# ---- 5. through the renderer -------------------------------------------------------------------------------------------
def torch_ssim(img1, img2):
    """The reference's SSIM restated with plain torch ops (shifted slices, no convolution library): fp32 autograd."""
    import torch
    import torch.nn.functional as F

    g = torch.as_tensor(sr.window_1d(), device=img1.device)

    def blur(x):
        xp = F.pad(x, (5, 5, 5, 5))
        H, W = x.shape[-2:]
        h = sum(g[k] * xp[..., :, k:k + W] for k in range(11))
        return sum(g[k] * h[..., k:k + H, :] for k in range(11))

    m1, m2 = blur(img1), blur(img2)
    s1 = blur(img1 * img1) - m1 * m1
    s2 = blur(img2 * img2) - m2 * m2
    s12 = blur(img1 * img2) - m1 * m2
    S = ((2 * m1 * m2 + sr.C1) * (2 * s12 + sr.C2)) / ((m1 * m1 + m2 * m2 + sr.C1) * (s1 + s2 + sr.C2))
    return S.mean()


def _small_scene(perturb_seed=None):
    import torch
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj import synthetic as syn
    from utils.camera_utils import Camera

    W, H = 160, 120
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=W, H=H, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    sc = syn.make_scene(1500, 7, cam, z_range=(1.0, 5.0), log_scale_range=(np.log(0.01), np.log(0.08)), sh_coeffs=1)
    shs = sc["shs"].copy()
    if perturb_seed is not None:
        shs[:, 0, :] += np.random.default_rng(perturb_seed).normal(0, 0.4, shs[:, 0, :].shape).astype(np.float32)
    model = GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], shs, sh_degree=0,
                                         device=_dev())
    return model, Camera.from_synthetic(cam, device=_dev()), cam, sc


class _Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False


def test_render_gradients_gsaj_ssim_vs_torch_ssim_and_refinement_loss():
    import torch
    from gaussian_splatting.gaussian_renderer import render
    from gsaj import losses, ssim as gssim
    from gsaj.rasterizer import FrameContext

    bg = torch.zeros(3, device=_dev())
    gt_model, view, cam, sc = _small_scene()
    with torch.no_grad():
        gt = render(view, gt_model, _Pipe, bg)["render"].detach().contiguous()
    model, view, _, _ = _small_scene(perturb_seed=11)
    grads, imgs = {}, {}
    for name, fn in (("gsaj", gssim.ssim), ("torch", torch_ssim)):
        for p in model.parameters():
            p.grad = None
        img = render(view, model, _Pipe, bg)["render"]
        img.retain_grad()
        loss = 0.8 * gssim.l1_loss(img, gt) + 0.2 * (1.0 - fn(img, gt))
        loss.backward()
        grads[name] = [p.grad.detach().clone() for p in (model._xyz, model._features_dc, model._opacity, model._scaling)]
        imgs[name] = (float(loss), img.grad.detach().clone())
    assert abs(imgs["gsaj"][0] - imgs["torch"][0]) < 1e-5
    for ga, gb in zip(grads["gsaj"], grads["torch"]):
        assert float((ga - gb).abs().max() / gb.abs().max()) < GRAD_TOL

    # RefinementLoss + FrameContext.backward = the autograd path
    P, M = model.get_xyz.shape[0], 1
    ctx = FrameContext(P, cam["W"], cam["H"], M, _dev())
    with torch.no_grad():
        fa = dict(bg=bg, means3D=model.get_xyz.contiguous(), opacities=model.get_opacity.contiguous(), viewmatrix=view.world_view_transform,
                  projmatrix=view.full_proj_transform, campos=view.camera_center, tanfovx=math.tan(0.5 * view.FoVx), tanfovy=math.tan(0.5 * view.FoVy),
                  sh_degree=0, shs=model.get_features.contiguous(), scales=model.get_scaling.contiguous(),
                  rotations=model.get_rotation.contiguous())
        ctx.forward(**fa)
        rl = losses.RefinementLoss(cam["W"], cam["H"], _dev())
        o = rl(ctx.color, gt)
        assert abs(float(o["loss"]) - imgs["gsaj"][0]) < 1e-5
        seed_err = float((o["dL_dcolor"] - imgs["gsaj"][1]).abs().max() / imgs["gsaj"][1].abs().max())
        assert seed_err < 1e-5, seed_err
        fa.pop("opacities")
        g = ctx.backward(projmatrix_raw=view.projection_matrix, dL_dcolor=o["dL_dcolor"],
                         dL_ddepth=torch.zeros((1, cam["H"], cam["W"]), device=_dev()), **fa)
        dmean = g["mean3D"][:P]
        ref = grads["gsaj"][0]
        assert float((dmean - ref).abs().max() / ref.abs().max()) < 1e-4


# ---- 6. a short colour refinement --------------------------------------------------------------------------------------
def test_colour_refinement_loss_falls_and_tracks_torch_ssim():
    import torch
    from gaussian_splatting.gaussian_renderer import render
    from gsaj import ssim as gssim

    bg = torch.zeros(3, device=_dev())
    gt_model, view, _, _ = _small_scene()
    with torch.no_grad():
        gt = render(view, gt_model, _Pipe, bg)["render"].detach().contiguous()
    traj = {}
    for name, fn in (("gsaj", gssim.ssim), ("torch", torch_ssim)):
        model, view, _, _ = _small_scene(perturb_seed=12)
        opt = torch.optim.Adam([model._features_dc], lr=0.01)
        ls = []
        for _ in range(30):
            img = render(view, model, _Pipe, bg)["render"]
            loss = 0.8 * gssim.l1_loss(img, gt) + 0.2 * (1.0 - fn(img, gt))
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            ls.append(float(loss))
        traj[name] = np.array(ls)
    a, b = traj["gsaj"], traj["torch"]
    assert a[-1] < 0.7 * a[0], a
    assert np.abs(a - b).max() < 1e-3 * a[0] + 1e-6, np.abs(a - b).max()
