"""CPU: the joint (pose + exposure) Gauss-Newton path's restatements (tests/gn8_restated.py) checked against finite differences, against
the 6-form's restatement and against themselves; the canaries -- every mutant must be rejected by the comparator the GPU tests use;
the restated Levenberg-Marquardt loop recovering pose AND exposure where the 6-form's loop is left with a biased pose; the host side."""
import math
import re

import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import loss_restated as lr

F = np.float32
A_STAR, B_STAR = 0.2, -0.05      # the exposure of the issue's cases
DELTA = 0.03
LM = dict(nu=4.0, lambda_min=1e-7, lambda_max=1e7, threshold=1e-4)


@pytest.fixture(scope="module")
def scene():
    cam, sc, planted = gn.jac_scene()
    (out, st), _ = gn.oracle_forward(cam, sc)
    rows = gn.gaussian_rows(st, cam["projmatrix_raw"])
    J, col, dep = gn.jacobian(st, rows, gn.JAC_BG)
    rng = np.random.default_rng(9)
    H, W = gn.JAC_H, gn.JAC_W
    col, dep = col.astype(F), dep.astype(F)
    # a ground truth near the render (the recipe of tests/test_gpu_pose_jacobian.py): residuals of both signs, on both sides of DELTA
    gt = np.clip(col + rng.normal(scale=0.08, size=col.shape) + 0.05 * np.sin(np.arange(W) / 7.0)[None, None, :], 0.0, 1.5).astype(F)
    gt[:, 3:6, 10:30] = 0.001
    gd = (dep + rng.normal(scale=0.1, size=dep.shape)).astype(F)
    gd[rng.uniform(size=dep.shape) < 0.1] = 0.0
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint8)
    kw = dict(flags=lr.TRACKING, alpha=0.9, rgb_thr=0.01, image=col, depth=dep[None], opacity=out["opacity"], gt=gt, gt_depth=gd, mask=mask)
    a, b = F(A_STAR), F(B_STAR)
    q = gn.irls(a=a, b=b, delta=DELTA, **kw)
    ne8 = g8.normal_equations8(J, col, a, q["s"], q["h"], q["err_s"], q["err_h"])
    return dict(cam=cam, sc=sc, J=J, col=col, kw=kw, a=a, b=b, q=q, ne8=ne8)


def test_exposure_gradient_is_the_finite_difference_of_the_smooth_loss_and_the_block_its_gauss_newton_curvature(scene):
    """g8[6:8] against central differences of the Huberised loss in a and b.  Step 1e-5: the truncation error is step^2 |f'''| / 6 with
    |f'''| <= sum kappa (e^a C)^3 / delta-ish = O(1 / DELTA) ~ 33 -> 6e-10; fp64 round-off 2^-52 |f| / step ~ 1e-12.  Bound: 1e-8
    absolute on gradients of size ~1e-1.  The exposure block of H8 against sum w dr_i dr_j with w = kappa / max(|r|, delta), dr/da =
    m e^a C, dr/db = m, from the residuals directly: the same real number in another order -- relative 1e-12."""
    kw, a0, b0 = scene["kw"], float(scene["a"]), float(scene["b"])
    step, bound = 1e-5, 1e-8
    f = lambda a, b: g8.smooth_loss(kw["flags"], kw["alpha"], kw["rgb_thr"], kw["image"], kw["depth"], kw["opacity"], kw["gt"],  # noqa: E731
                                    kw["gt_depth"], kw["mask"], a, b, DELTA)
    fd = np.array([(f(a0 + step, b0)[0] - f(a0 - step, b0)[0]) / (2 * step), (f(a0, b0 + step)[0] - f(a0, b0 - step)[0]) / (2 * step)])
    g = scene["ne8"]["g"][6:8]
    assert np.abs(g).min() > 1e-3, g
    assert np.abs(fd - g).max() < bound, (fd, g)
    _, r, kappa, mf, c = f(a0, b0)
    w = kappa[None] / np.maximum(np.abs(r), DELTA)
    da, db = mf[None] * math.exp(a0) * c, np.broadcast_to(mf[None], c.shape)
    want = np.array([[(w * da * da).sum(), (w * da * db).sum()], [(w * da * db).sum(), (w * db * db).sum()]])
    np.testing.assert_allclose(scene["ne8"]["H"][6:8, 6:8], want, rtol=1e-12)
    assert np.linalg.eigvalsh(scene["ne8"]["H"]).min() > -1e-12 * np.abs(scene["ne8"]["H"]).max()


def test_the_pose_block_is_the_6_forms_result_exactly(scene):
    q = scene["q"]
    ne6 = gn.normal_equations(scene["J"], q["s"], q["h"], q["err_s"], q["err_h"])
    ne8 = scene["ne8"]
    for k in ("H", "H_mass", "H_bound"):
        assert np.array_equal(ne8[k][:6, :6], ne6[k]), k
    for k in ("g", "g_mass", "g_bound"):
        assert np.array_equal(ne8[k][:6], ne6[k]), k
    assert np.array_equal(ne8["H"], ne8["H"].T) and not ne8["H"][6:, 6:].min() < 0
    # the loss slots are irls's, which both forms share
    assert q["loss"]["value"]["loss"] > 0


@pytest.mark.parametrize("mutant", g8.MUTANTS[:3])
def test_column_mutants_are_rejected_by_the_normal_equation_comparator(scene, mutant):
    q, ne8 = scene["q"], scene["ne8"]
    assert gn.assert_normal_equations_close(ne8["H"].astype(F), ne8["g"].astype(F), ne8, "self") <= 1.0
    bad = g8.normal_equations8(scene["J"], scene["col"], scene["a"], q["s"], q["h"], gt=scene["kw"]["gt"], mutant=mutant)
    with pytest.raises(AssertionError, match="x bound"):
        gn.assert_normal_equations_close(bad["H"], bad["g"], ne8, mutant)


def _quadratic8(seed=0):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(50, 8))
    return (A.T @ A).astype(F).astype(np.float64), rng.normal(size=8).astype(F).astype(np.float64) * 1e-2


def test_lm8_step_solves_a_quadratic_and_the_reject_mutant_is_rejected_by_the_state_comparator():
    H, g = _quadratic8()
    st = g8.lm8_new_state(np.eye(4), 1e-12, exposure=(0.1, -0.02))
    g8.lm8_step(st, H, g, 1.0, nu=2.0, lambda_min=1e-15, lambda_max=1e6, threshold=1e-4)
    x = np.linalg.solve(H, -g)
    np.testing.assert_allclose(np.concatenate([st["tau"], st["dexposure"]]), x, rtol=1e-5)
    np.testing.assert_allclose(st["exposure"], np.array([0.1, -0.02], F).astype(np.float64) + x[6:], atol=1e-7)
    proj = np.eye(4)
    good, bad = g8.lm8_new_state(np.eye(4), 1e-3), g8.lm8_new_state(np.eye(4), 1e-3)
    for loss in (1.0, 1.5, 0.5):  # accept, reject, accept
        g8.lm8_step(good, H, g, loss, 2.0, 1e-6, 1e3, 1e-4)
        g8.lm8_step(bad, H, g, loss, 2.0, 1e-6, 1e3, 1e-4, mutant="exposure_not_restored_on_reject")
    assert (good["accepted"], good["rejected"]) == (2, 1)
    g8.assert_lm8_state_close(g8.pack_state8(good, proj), good, proj, "self")
    with pytest.raises(AssertionError, match="exposure"):
        g8.assert_lm8_state_close(g8.pack_state8(bad, proj), good, proj, "exposure_not_restored_on_reject")
    # a non-positive pivot: lambda up, neither pose nor exposure moves
    before = (good["w2c"].copy(), good["exposure"].copy(), good["lam"])
    g8.lm8_step(good, -np.eye(8), g, 0.1, 2.0, 1e-6, 1e3, 1e-4)
    assert np.array_equal(good["w2c"], before[0]) and np.array_equal(good["exposure"], before[1])
    assert good["lam"] == before[2], "the accept's lambda / nu is undone by the failed factorisation's lambda x nu"
    assert not good["converged"]


# The true frame is rendered TRUE_OFFSET away from the scene's pose (the noisy fixture pose the scene was built for: the loop's start)
# and turned into e^{a*} C + b*: 3 cm / 0.75 degrees, a few pixels at the scene's depths -- well inside the basin of a Gauss-Newton
# step, large against the criterion's 0.35.  (a*, b*) = (0.2, -0.05) already shows the bias on the CPU: no larger offset was needed.
TRUE_OFFSET = (0.03, -0.02, 0.025, 0.75)
JOINT_COUNT = 6    # the iteration at which the restated joint loop first meets both criteria (asserted below)


def _true_pose(start):
    ang = math.radians(TRUE_OFFSET[3])
    d = np.eye(4)
    d[:3, :3] = np.array([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
    d[:3, 3] = TRUE_OFFSET[:3]
    return np.linalg.inv(d) @ start


def test_restated_joint_loop_recovers_pose_and_exposure_and_the_6_form_is_left_with_a_larger_translation_error(scene):
    cam, sc = scene["cam"], scene["sc"]
    start = cam["w2c"].copy()
    true = _true_pose(start)
    (out, _), _ = gn.oracle_forward(g8.camera_at(cam, true), sc)
    gt, gd = (math.exp(A_STAR) * out["color"] + B_STAR).astype(F), out["depth"][0].astype(F)
    t0 = g8.pose_errors(start, true)[0]
    e0 = max(abs(A_STAR), abs(B_STAR))
    joint, met = g8.lm8_new_state(start, 1e-3), None
    acc = []
    for it in range(1, JOINT_COUNT + 1):
        H, g, loss = g8.restated_rows(cam, sc, joint["w2c"], joint["exposure"], gt, gd, 0.01, True)
        g8.lm8_step(joint, H, g, loss, **LM)
        acc.append(joint["acc_loss"])
        te, re_ = g8.pose_errors(joint["acc_w2c"], true)
        ee = float(np.abs(joint["acc_exposure"] - [A_STAR, B_STAR]).max())
        print("joint %d: loss %.5f translation %.4f x start, rotation %.5f, exposure %.4f x start" % (it, loss, te / t0, re_, ee / e0))
        if met is None and te < 0.35 * t0 and re_ < 0.02 and ee < 0.35 * e0:
            met = it
    assert all(b <= a for a, b in zip(acc, acc[1:])), acc
    assert met == JOINT_COUNT, (met, te / t0, re_, ee / e0)
    six = gn.lm_new_state(start, 1e-3)
    for it in range(1, JOINT_COUNT + 1):
        H, g, loss = g8.restated_rows(cam, sc, six["w2c"], (0.0, 0.0), gt, gd, 0.01, False)
        gn.lm_step(six, H, g, loss, **LM)
    te6 = g8.pose_errors(six["acc_w2c"], true)[0]
    print("6-form after %d: loss %.5f translation %.4f x start (joint: %.4f)" % (JOINT_COUNT, six["acc_loss"], te6 / t0, te / t0))
    assert te6 > te, (te6, te)
    assert six["acc_loss"] > 10 * joint["acc_loss"], "the 6-form's small, happily accepted loss is still the photometric offset"


NEW_SYMBOLS = ("gsaj_rasterize_pose_jacobian_loss8", "gsaj_gn8_state_floats", "gsaj_pose_gn8_step")


def test_header_declares_the_joint_symbols_and_the_binding_matches_their_arity():
    from gsaj import _lib

    with open(_lib.HEADER) as fh:
        text = fh.read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\);" % name, text, re.S)
        assert m, "%s is not declared in include/gsaj.h" % name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        n = 0 if args == "void" else len(args.split(","))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, (name, n)
    assert len(_lib.SIGNATURES["gsaj_rasterize_pose_jacobian_loss8"][1]) == len(_lib.SIGNATURES["gsaj_rasterize_pose_jacobian_loss"][1])
    assert re.search(r"#define GSAJ_GN8_PARTIAL_FLOATS 64\b", text) and re.search(r"#define GSAJ_GN_PARTIAL_FLOATS 32\b", text)
    lib = _lib.load()
    n8 = int(re.search(r"#define GSAJ_GN8_STATE_FLOATS (\d+)", text).group(1))
    assert lib.gsaj_gn8_state_floats() == n8 == g8.pack_state8(g8.lm8_new_state(np.eye(4), 1.0), np.eye(4)).size
    assert lib.gsaj_gn_state_floats() == 136 and lib.gsaj_version() >= 108


def test_unpack_sym8_and_the_joint_form_has_no_cpu_path():
    import torch
    import gsaj
    from gsaj import _lib
    from gsaj.rasterizer import FrameContext, unpack_sym8

    h = torch.arange(36, dtype=torch.float32)
    assert np.array_equal(unpack_sym8(h).numpy(), g8.sym8(h.numpy()))
    z = torch.zeros(3)
    with pytest.raises(_lib.GsajError, match="HIP device"):
        gsaj.GaussNewtonTracker(10, 32, 32, 16, "cpu", np.eye(4), np.eye(4), 0.5, 0.5, z, torch.zeros(10, 3), torch.zeros(10, 1),
                                solve_exposure=True)
    ctx = object.__new__(FrameContext)
    ctx.dev = torch.device("cpu")
    with pytest.raises(_lib.GsajError, match="HIP device"):
        ctx.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5, solve_exposure=True)
