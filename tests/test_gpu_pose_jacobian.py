"""GPU: the per-pixel pose Jacobian of the forward-mode compositor (csrc/pose_jac.hip: k_splat_jac, k_render_jac) and the normal
equations formed from it, explicit (gsaj_rasterize_pose_jacobian) and fused with the tracking loss (gsaj_rasterize_pose_jacobian_loss).

The Jacobian is DEFINED as the transpose of the backward's linear map, so it is judged the way the backward's own dL/dtau is:
against the CPU oracle's backward under the same seeds, with the limits of tests/helpers.py.  The scene (tests/gn_restated.py:
jac_scene; 72x40, partial tiles on both edges, SH degree 3, non-zero background) was chosen on the CPU with the oracle alone so that
no pixel is borderline: the strict limit applies.  H and g are judged against the float64 restatement applied to the DEVICE's own
Jacobian, element by element within (roundings per term + reduction depth) 2^-24 sum|term| -- the counts are derived from the
kernel's arithmetic in gn_restated (G_ROUNDINGS = 12: product 1, channels 4, butterfly 6, final rounding 1; H_ROUNDINGS = 13)."""
import numpy as np
import pytest

import gn_restated as gn
import helpers as hp
import loss_restated as lr

pytestmark = pytest.mark.gpu


class Frame:
    """One forward of the scene on the device + everything the oracle says about it (computed once per record format)."""

    def __init__(self, record_bits):
        import torch
        from gsaj.rasterizer import FrameContext
        from oracle import oracle as orc

        self.dev = torch.device("cuda:0")
        self.t = t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.dev)  # noqa: E731
        self.cam, self.sc, self.planted = gn.jac_scene()
        cam, sc = self.cam, self.sc
        (self.ref, self.st), _ = gn.oracle_forward(cam, sc, record_bits=record_bits)
        self.seeds = gn.jac_seeds(0)
        self.em = orc.error_model(self.st, *self.seeds, hp.BORDER_REL, hp.BORDER_REL_T)
        P = sc["means3D"].shape[0]
        self.ctx = FrameContext(P, gn.JAC_W, gn.JAC_H, 16, self.dev, record_bits=record_bits)
        self.bg = t(gn.JAC_BG)
        self.g = dict(means3D=t(sc["means3D"]), opacities=t(sc["opacities"]))
        self.kw = dict(sh_degree=gn.JAC_DEG, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
        self.view = (t(cam["viewmatrix"]), t(cam["projmatrix"]), t(cam["campos"]))
        self.praw = t(cam["projmatrix_raw"])
        self.tan = (cam["tanfovx"], cam["tanfovy"])
        self.forward()

    def forward(self):
        return self.ctx.forward(self.bg, self.g["means3D"], self.g["opacities"], *self.view, *self.tan, **self.kw)

    def jac(self, **kw):
        return self.ctx.pose_jacobian(self.bg, self.g["means3D"], self.view[0], self.view[1], self.praw, self.view[2], *self.tan, **kw, **self.kw)

    def jac_loss(self, L, **kw):
        return self.ctx.pose_jacobian_loss(L, self.bg, self.g["means3D"], self.view[0], self.view[1], self.praw, self.view[2], *self.tan,
                                           **kw, **self.kw)

    def backward(self, s_c, s_d):
        g = self.ctx.backward(self.bg, self.g["means3D"], self.view[0], self.view[1], self.praw, self.view[2], *self.tan, self.t(s_c),
                              self.t(s_d), pose_only=True, **self.kw)
        return g["tau_sum"].cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def fr():
    f = Frame(32)
    f.out = f.jac(want_jacobian=True, want_images=True)
    f.J = f.out["jacobian"].cpu().numpy()
    return f


def test_rederived_images_are_the_forwards_bits_and_n_contrib_is_respected(fr):
    import torch

    assert torch.equal(fr.out["color"], fr.ctx.color) and torch.equal(fr.out["depth"], fr.ctx.depth)
    assert np.isfinite(fr.J).all()
    # the oracle stops every pixel at the same contributor (clean scene): the images are its images
    hp.assert_image_close(fr.out["color"].cpu().numpy(), fr.ref["color"], hp.IMG_TOL, border_mask=fr.em["border_mask"], tag="jac/color")
    hp.assert_image_close(fr.out["depth"].cpu().numpy(), fr.ref["depth"], hp.IMG_TOL, border_mask=fr.em["border_mask"], tag="jac/depth")
    x, y = fr.planted["empty_tile"][1]
    assert not fr.J[y, x].any() and not fr.J[32:, 64:].any(), "a tile no Gaussian touches: background only, J = 0"


def test_transpose_identity_against_the_oracle(fr):
    """sum s J, contracted on the host in float64 from jac_out, against the oracle's dL/dtau under the same seeds: the way smoke()
    judges the backward's own dL/dtau, strict limit (the scene has no borderline pixel)."""
    from oracle import oracle as orc

    assert not fr.em["border_mask"].any()
    g = gn.contract(fr.J, *fr.seeds)
    e = gn.assert_transpose_identity(g, fr.st, *fr.seeds, fr.cam["projmatrix_raw"], hp.GRAD_TOL, "device J")
    e_old = hp.rel_err(fr.backward(*fr.seeds), orc.backward(fr.st, *fr.seeds, fr.cam["projmatrix_raw"])["dL_dtau_sum"])
    print("transpose identity: rel err %.3e (the existing backward's: %.3e)" % (e, e_old))


def test_single_rows_against_the_oracle_under_one_hot_seeds(fr):
    """~16 pixels covering every planted case, an edge-tile pixel and a background-only pixel, all four channels: the row against the
    oracle's backward under a one-hot seed, within max(GRAD_TOL, CHAIN_K x the error of the existing device backward under the same
    seed) -- two correct fp32 evaluations in different orders differ by a small multiple of one's rounding noise."""
    from oracle import oracle as orc

    pixels = gn.row_pixels(fr.planted, fr.em["border_mask"])
    assert len(pixels) >= 14
    worst = 0.0
    for (x, y) in pixels:
        for ch in range(4):
            s_c, s_d = np.zeros((3, gn.JAC_H, gn.JAC_W), np.float32), np.zeros((1, gn.JAC_H, gn.JAC_W), np.float32)
            (s_c if ch < 3 else s_d)[ch % 3, y, x] = 1.0
            want = orc.backward(fr.st, s_c, s_d, fr.cam["projmatrix_raw"])["dL_dtau_sum"]
            if (x, y) == fr.planted["empty_tile"][1]:
                assert not want.any() and not fr.J[y, x, ch].any()
                continue
            assert np.abs(want).max() > 0, (x, y, ch)
            e_old = hp.rel_err(fr.backward(s_c, s_d), want)
            e_new = hp.rel_err(fr.J[y, x, ch], want)
            print("pixel (%2d, %2d) ch %d: row err %.3e, existing backward %.3e" % (x, y, ch, e_new, e_old))
            assert e_new <= max(hp.GRAD_TOL, hp.CHAIN_K * e_old), (x, y, ch, e_new, e_old)
            worst = max(worst, e_new)
    print("worst row err %.3e" % worst)


def test_explicit_normal_equations_against_the_restatement_on_the_devices_jacobian(fr):
    rng = np.random.default_rng(3)
    HW = gn.JAC_H * gn.JAC_W
    s_c, s_d = fr.seeds
    h_c = (np.abs(rng.normal(size=(3, gn.JAC_H, gn.JAC_W))) / (3 * HW)).astype(np.float32)
    h_d = (np.abs(rng.normal(size=(1, gn.JAC_H, gn.JAC_W))) / HW).astype(np.float32)
    o = fr.jac(seeds=(fr.t(s_c), fr.t(s_d)), curvature=(fr.t(h_c), fr.t(h_d)))
    assert o["jacobian"] is None
    want = gn.normal_equations(fr.J, np.concatenate([s_c, s_d]), np.concatenate([h_c, h_d]))
    r = gn.assert_normal_equations_close(o["H"].cpu().numpy(), o["g"].cpu().numpy(), want, "explicit")
    print("explicit H, g: worst err / bound %.3f" % r)
    assert np.linalg.eigvalsh(o["H"].cpu().numpy().astype(np.float64)).min() > -1e-6 * np.abs(want["H"]).max()
    only_g = fr.jac(seeds=(fr.t(s_c), fr.t(s_d)))
    assert only_g["H"] is None and np.array_equal(only_g["g"].cpu().numpy(), o["g"].cpu().numpy())


def _ground_truth(fr, seed=9):
    """A ground truth near the render: colour and depth off by a smooth offset + noise (residuals of both signs, most of them well
    away from 0), some pixels below the rgb boundary threshold, some without depth; a byte mask."""
    rng = np.random.default_rng(seed)
    H, W = gn.JAC_H, gn.JAC_W
    c, d = fr.ctx.color.cpu().numpy(), fr.ctx.depth.cpu().numpy()[0]
    gt = np.clip(c + rng.normal(scale=0.08, size=c.shape) + 0.05 * np.sin(np.arange(W) / 7.0)[None, None, :], 0.0, 1.5).astype(np.float32)
    gt[:, 3:6, 10:30] = 0.001                                   # below the rgb boundary threshold
    gd = (d + rng.normal(scale=0.1, size=d.shape)).astype(np.float32)
    gd[rng.uniform(size=d.shape) < 0.1] = 0.0                   # no depth measured
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint8)
    return gt, gd, mask


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_fused_normal_equations_and_loss_terms(fr, mono, masked):
    import torch

    gt, gd, mask = _ground_truth(fr)
    flags = lr.TRACKING | (lr.MONOCULAR if mono else 0)
    a, b = np.float32(0.1), np.float32(-0.02)
    L = dict(flags=flags, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=fr.t(gt), gt_depth=None if mono else fr.t(gd),
             grad_mask=torch.as_tensor(mask.reshape(-1), device=fr.dev) if masked else None, exposure_a=fr.t([a]), exposure_b=fr.t([b]),
             scalars=torch.zeros(5, device=fr.dev))
    img = dict(image=fr.ctx.color.cpu().numpy(), depth=fr.ctx.depth.cpu().numpy(), opacity=fr.ctx.opacity.cpu().numpy())
    for delta in (0.0, 0.03):
        o = fr.jac_loss(L, irls_delta=delta, want_jacobian=True)
        assert np.array_equal(o["jacobian"].cpu().numpy(), fr.J), "the fused form walks the same Jacobian"
        rows = o["partials"].cpu().numpy().astype(np.float64)
        assert rows.shape == (64, 32)
        tot = rows.sum(axis=0)
        q = gn.irls(flags, 0.9, 0.01, img["image"], img["depth"], img["opacity"], gt, None if mono else gd, mask if masked else None, a, b,
                    delta=delta)
        want = gn.normal_equations(fr.J, q["s"], q["h"], q["err_s"], q["err_h"])
        tag = "fused mono=%s masked=%s delta=%g" % (mono, masked, delta)
        r = gn.assert_normal_equations_close(gn.sym6(tot[:21]), tot[21:27], want, tag)
        ratios = lr.assert_loss_close(dict(loss=tot[27], l1_rgb=tot[28], l1_depth=tot[29]), q["loss"], tag, outputs=("loss", "l1_rgb", "l1_depth"))
        print("%s: H, g worst err / bound %.3f, loss terms %s" % (tag, r, ratios))
        if delta == 0.0:  # the seeds are the backward's, bit for bit: g is its dL/dtau
            fr.ctx.forward_loss(L, fr.bg, fr.g["means3D"], fr.g["opacities"], *fr.view, *fr.tan, **fr.kw)
            gb = fr.ctx.backward_loss(L, fr.bg, fr.g["means3D"], fr.view[0], fr.view[1], fr.praw, fr.view[2], *fr.tan, pose_only=True, **fr.kw)
            assert hp.rel_err(tot[21:27], gb["tau_sum"].cpu().numpy()) < hp.GRAD_TOL
            lr.assert_loss_close(dict(loss=L["scalars"][0], l1_rgb=L["scalars"][1], l1_depth=L["scalars"][2]), q["loss"], tag + " forward_loss",
                                 outputs=("loss", "l1_rgb", "l1_depth"))
            np.testing.assert_allclose(tot[27:30], L["scalars"][:3].cpu().numpy(), rtol=2e-6, atol=1e-12)
            fr.forward()


def test_fp16_records_transpose_identity():
    """record_bits = 16 contexts work through gsaj_load_row: the transpose identity against the oracle's fp16-record mode at the fp32
    path's limit, and against the plain fp32 oracle at the looser one half-precision storage implies (test_gpu_fp16_records.py)."""
    from oracle import oracle as orc

    f = Frame(16)
    assert not f.em["border_mask"].any()
    J = f.jac(want_jacobian=True)["jacobian"].cpu().numpy()
    g = gn.contract(J, *f.seeds)
    gn.assert_transpose_identity(g, f.st, *f.seeds, f.cam["projmatrix_raw"], hp.GRAD_TOL, "fp16 records")
    (_, st32), _ = gn.oracle_forward(f.cam, f.sc)
    assert hp.rel_err(g, orc.backward(st32, *f.seeds, f.cam["projmatrix_raw"])["dL_dtau_sum"]) < 3e-2


def test_two_runs_give_identical_bits(fr):
    import torch

    s = (fr.t(fr.seeds[0]), fr.t(fr.seeds[1]))
    h = (fr.t(np.abs(fr.seeds[0])), fr.t(np.abs(fr.seeds[1])))
    a = fr.jac(seeds=s, curvature=h, want_jacobian=True)
    fr.forward()
    b = fr.jac(seeds=s, curvature=h, want_jacobian=True)
    for k in ("jacobian", "H", "g"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["jacobian"], fr.out["jacobian"])


def test_misuse_raises_and_an_empty_view_gives_zero():
    import torch
    from gsaj import _lib
    from gsaj.rasterizer import FrameContext

    f = Frame(32)
    fresh = FrameContext(f.sc["means3D"].shape[0], gn.JAC_W, gn.JAC_H, 16, f.dev)
    args = (f.bg, f.g["means3D"], f.view[0], f.view[1], f.praw, f.view[2], *f.tan)
    with pytest.raises(_lib.GsajError, match="forward"):
        fresh.pose_jacobian(*args, **f.kw)
    with pytest.raises(_lib.GsajError, match="forward"):
        fresh.pose_jacobian_loss({}, *args, **f.kw)
    f.ctx.set_tile_band(0, 2)
    with pytest.raises(_lib.GsajError, match="band"):
        f.jac(want_jacobian=True)
    f.ctx.set_tile_band(0, 3)  # the whole frame again
    f.forward()
    assert f.jac(want_jacobian=True)["jacobian"] is not None
    # no visible Gaussian: everything behind the camera
    behind = f.g["means3D"] - 100.0 * f.t(f.cam["viewmatrix"].reshape(4, 4)[:3, 2])[None, :]
    fresh.forward(f.bg, behind, f.g["opacities"], *f.view, *f.tan, **f.kw)
    assert int(fresh.radii.max()) == 0
    s = (f.t(f.seeds[0]), f.t(f.seeds[1]))
    o = fresh.pose_jacobian(f.bg, behind, f.view[0], f.view[1], f.praw, f.view[2], *f.tan, seeds=s, curvature=s, want_jacobian=True, **f.kw)
    assert not o["H"].any() and not o["g"].any() and not o["jacobian"].any()
    assert torch.isfinite(o["H"]).all()
