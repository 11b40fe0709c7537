"""GPU: the joint form of the loss-fused Jacobian compositor (csrc/pose_jac.hip: k_render_jac8 through
gsaj_rasterize_pose_jacobian_loss8): the 8x8 normal equations over [rho, theta, a, b] on the 72x40 scene of tests/gn_restated.py.

H8 and g8 are judged against the float64 restatement (tests/gn8_restated.py) applied to the DEVICE's own Jacobian and images, element
by element within the bound derived there from the count of fp32 roundings; the pose block against the 6-form's bound; the exposure
gradient against the first-order path DeviceTracker uses (gsaj_rasterize_forward_loss / _backward_loss), which is pinned to the
reference's autograd."""
import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import loss_restated as lr
from test_gpu_pose_jacobian import Frame, _ground_truth

pytestmark = pytest.mark.gpu

A, B = np.float32(0.2), np.float32(-0.05)
TAU_SLOTS = [n for n, (k, l) in enumerate(g8.SYM8) if k < 6] + list(range(36, 42))   # every slot a pose column enters


@pytest.fixture(scope="module", params=[32, 16], ids=["fp32-records", "fp16-records"])
def fr(request):
    f = Frame(request.param)
    f.J = f.jac(want_jacobian=True)["jacobian"].cpu().numpy()
    f.img = dict(image=f.ctx.color.cpu().numpy(), depth=f.ctx.depth.cpu().numpy(), opacity=f.ctx.opacity.cpu().numpy())
    f.gt = _ground_truth(f)
    return f


def _loss(fr, mono, masked, flags_extra=0, a=A, b=B, mask=None, gd=None):
    import torch

    gt, gd0, mask0 = fr.gt
    mask = mask0 if mask is None else mask
    gd = gd0 if gd is None else gd
    flags = lr.TRACKING | (lr.MONOCULAR if mono else 0) | flags_extra
    L = dict(flags=flags, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=fr.t(gt), gt_depth=None if mono else fr.t(gd),
             grad_mask=torch.as_tensor(mask.reshape(-1), device=fr.dev) if masked else None,
             exposure_a=None if a is None else fr.t([a]), exposure_b=None if b is None else fr.t([b]), scalars=torch.zeros(5, device=fr.dev))
    return L, flags, gt, (None if mono else gd), (mask if masked else None)


def _rows8(fr, L, delta):
    o = fr.jac_loss(L, irls_delta=delta, solve_exposure=True)
    rows = o["partials"].cpu().numpy()
    assert rows.shape == (64, 64) and rows.dtype == np.float32
    assert not rows[:, 49:].any(), "slots [49:64) are written as zero"
    return rows


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_joint_rows_against_the_restatement_and_the_pose_block_against_the_6_form(fr, mono, masked):
    L, flags, gt, gd, mask = _loss(fr, mono, masked)
    for delta in (0.0, 0.03):
        rows = _rows8(fr, L, delta)
        tot = rows.astype(np.float64).sum(axis=0)
        q = gn.irls(flags, 0.9, 0.01, fr.img["image"], fr.img["depth"], fr.img["opacity"], gt, gd, mask, A, B, delta=delta)
        want = g8.normal_equations8(fr.J, fr.img["image"], A, q["s"], q["h"], q["err_s"], q["err_h"])
        tag = "joint mono=%s masked=%s delta=%g" % (mono, masked, delta)
        H8 = g8.sym8(tot[:36])
        r = gn.assert_normal_equations_close(H8, tot[36:44], want, tag)
        ratios = lr.assert_loss_close(dict(loss=tot[44], l1_rgb=tot[45], l1_depth=tot[46]), q["loss"], tag, outputs=("loss", "l1_rgb", "l1_depth"))
        assert np.linalg.eigvalsh(H8).min() > -1e-6 * np.abs(H8).max()
        # the 6-form on the same finished forward: the pose block, g8[0:6] and the loss slots within the 6-form's own bound
        rows6 = fr.jac_loss(L, irls_delta=delta)["partials"].cpu().numpy()
        tot6 = rows6.astype(np.float64).sum(axis=0)
        want6 = gn.normal_equations(fr.J, q["s"], q["h"], q["err_s"], q["err_h"])
        r6 = gn.assert_normal_equations_close(H8[:6, :6], tot[36:42], want6, tag + " pose block")
        gn.assert_normal_equations_close(gn.sym6(tot6[:21]), tot6[21:27], want6, tag + " 6-form")
        same_H = np.array_equal(H8[:6, :6].astype(np.float32), gn.sym6(tot6[:21]).astype(np.float32))
        same_g = np.array_equal(tot[36:42].astype(np.float32), tot6[21:27].astype(np.float32))
        same_l = np.array_equal(rows[:, 44:49], rows6[:, 27:32])
        print("%s: H8, g8 worst err / bound %.3f (pose block against the 6-form's bound %.3f), loss terms %s; same bits as the 6-form: "
              "H %s, g %s, loss and exposure slots %s" % (tag, r, r6, ratios, same_H, same_g, same_l))
        np.testing.assert_allclose(tot[44:49], tot6[27:32], rtol=2e-6, atol=1e-12)


@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_exposure_gradient_agrees_with_the_first_order_path(fr, mono, masked):
    """delta = 0: g8[6] = sum s C and g8[7] = sum s / e^a are dL/da and dL/db of the L1 loss, which the fused first-order path sums
    as k_rgb x its two exposure sums.  Tolerance: the loss-scalar bound of tests/loss_restated.py (SUM_K eps sum|term| + eps |value|)."""
    L, flags, gt, gd, mask = _loss(fr, mono, masked)
    rows = _rows8(fr, L, 0.0)
    tot = rows.astype(np.float64).sum(axis=0)
    fr.ctx.forward_loss(L, fr.bg, fr.g["means3D"], fr.g["opacities"], *fr.view, *fr.tan, **fr.kw)
    fr.ctx.backward_loss(L, fr.bg, fr.g["means3D"], fr.view[0], fr.view[1], fr.praw, fr.view[2], *fr.tan, pose_only=True, **fr.kw)
    first = L["scalars"].cpu().numpy().astype(np.float64)
    fr.forward()
    want = lr.restate(flags, 0.9, 0.01, fr.img["image"], fr.img["depth"], fr.img["opacity"], gt, gd, mask, A, B)
    tag = "mono=%s masked=%s" % (mono, masked)
    for name, got, ref in (("dL_dexposure_a", tot[42], first[3]), ("dL_dexposure_b", tot[43], first[4])):
        bound = lr.SUM_K * lr.EPS * want["mass"][name] + lr.EPS * abs(want["value"][name])
        print("%s %s: joint %.9e first-order %.9e restated %.9e; |joint - first-order| / bound %.3f" % (
            tag, name, got, ref, want["value"][name], abs(got - ref) / bound))
        assert abs(ref) > 0 and abs(got - ref) <= bound, (tag, name, got, ref, bound)
    lr.assert_loss_close(dict(dL_dexposure_a=tot[42], dL_dexposure_b=tot[43]), want, tag, outputs=("dL_dexposure_a", "dL_dexposure_b"))


def test_empty_tile_masked_frame_and_identical_bits(fr):
    import torch

    L, flags, gt, gd, _ = _loss(fr, False, False)
    rows = _rows8(fr, L, 0.03)
    # the tile no Gaussian touches: J = 0 AND the rendered opacity, the tracking loss's colour weight and depth gate, is 0 -- its
    # pixels add nothing to any slot, the exposure columns included.  Rows are not labelled with their tile, so: the restatement,
    # quadrant by quadrant, says which quadrants are all zero; the device has exactly as many all-zero rows, plus the grid's padding.
    x0, y0 = gn.EMPTY_TILE[0] * 16, gn.EMPTY_TILE[1] * 16
    assert x0 + 8 == gn.JAC_W and y0 + 8 == gn.JAC_H and not fr.J[y0:, x0:].any() and not fr.img["opacity"][0, y0:, x0:].any()
    q = gn.irls(flags, 0.9, 0.01, fr.img["image"], fr.img["depth"], fr.img["opacity"], gt, gd, None, A, B, delta=0.03)
    zero_quadrants = 0
    for ty in range(3):
        for tx in range(5):
            for wave in range(4):
                sel = np.zeros((gn.JAC_H, gn.JAC_W), bool)
                sel[ty * 16 + (wave >> 1) * 8:ty * 16 + (wave >> 1) * 8 + 8, tx * 16 + (wave & 1) * 8:tx * 16 + (wave & 1) * 8 + 8] = True
                part = g8.normal_equations8(fr.J, fr.img["image"], A, q["s"] * sel, q["h"] * sel)
                empty = not part["H"].any() and not part["g"].any()
                zero_quadrants += empty
                if (tx, ty) == gn.EMPTY_TILE:
                    assert empty, "the empty tile adds nothing"
                elif sel.any():
                    assert part["H"][6, 6] > 0 and part["H"][7, 7] > 0, (tx, ty, wave)
    assert zero_quadrants == 4 + 15 - 3    # the empty tile's four, the 15 quadrants outside the 72x40 image (3 of them the empty tile's)
    assert int((~rows[:, :49].any(axis=1)).sum()) == zero_quadrants + 4, "60 quadrants in a grid of 64 workgroups"
    # two runs: identical bits
    fr.forward()
    again = _rows8(fr, L, 0.03)
    assert np.array_equal(rows.view(np.uint32), again.view(np.uint32))
    # a fully masked frame: no colour term; without measured depth (or monocular) nothing is left
    zero = np.zeros((gn.JAC_H, gn.JAC_W), np.uint8)
    for mono in (True, False):
        Lm = _loss(fr, mono, True, mask=zero, gd=np.zeros((gn.JAC_H, gn.JAC_W), np.float32))[0]
        rz = _rows8(fr, Lm, 0.03)
        assert not rz[:, :44].any() and np.isfinite(rz).all(), "fully masked: H8 and g8 are all zero"
    assert torch.cuda.is_available()


def test_argument_errors_raise(fr):
    import torch
    from gsaj import _lib

    # (GSAJ_ERR_INVALID_ARGUMENT surfaces as a plain Exception carrying gsaj_last_error(): gsaj._lib.check)
    with pytest.raises(Exception, match="joint form"):   # the joint form solves for the exposure: GSAJ_LOSS_NO_EXPOSURE is an error
        fr.jac_loss(_loss(fr, False, False, flags_extra=lr.NO_EXPOSURE)[0], irls_delta=0.03, solve_exposure=True)
    with pytest.raises(Exception, match="joint form"):   # ... and so are null exposure pointers, even with the flag
        fr.jac_loss(_loss(fr, False, False, flags_extra=lr.NO_EXPOSURE, a=None, b=None)[0], irls_delta=0.03, solve_exposure=True)
    with pytest.raises(Exception, match="loss8"):
        fr.jac_loss(_loss(fr, False, False, b=None)[0], irls_delta=0.03, solve_exposure=True)
    L = _loss(fr, False, False)[0]
    with pytest.raises(Exception, match="irls_delta"):   # the 6-form's argument errors
        fr.jac_loss(L, irls_delta=-1.0, solve_exposure=True)
    with pytest.raises(Exception, match="loss8"):
        fr.jac_loss(dict(L, gt_depth=None), irls_delta=0.03, solve_exposure=True)
    with pytest.raises(_lib.GsajError, match="64"):   # a 6-form row buffer handed to the joint form
        fr.jac_loss(L, irls_delta=0.03, solve_exposure=True, partials=torch.zeros((64, 32), device=fr.dev))
    # the 6-form still accepts GSAJ_LOSS_NO_EXPOSURE
    assert fr.jac_loss(_loss(fr, False, False, flags_extra=lr.NO_EXPOSURE, a=None, b=None)[0], irls_delta=0.03)["partials"].shape == (64, 32)
