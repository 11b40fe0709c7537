"""CPU: the Gauss-Newton tracking path's restatements (tests/gn_restated.py) checked against the oracle and against themselves, the
canaries -- every mutant must be rejected by the comparator the GPU tests use --, the scene of the GPU Jacobian tests (chosen here,
with the oracle alone, so that the strict limit applies there), and the host side: header, binding, no CPU path."""
import os
import re

import numpy as np
import pytest

import gn_restated as gn
import helpers as hp
import loss_restated as lr
from oracle import oracle as orc


@pytest.fixture(scope="module")
def scene():
    cam, sc, planted = gn.jac_scene()
    (out, st), _ = gn.oracle_forward(cam, sc)
    s_c, s_d = gn.jac_seeds(0)
    em = orc.error_model(st, s_c, s_d, hp.BORDER_REL, hp.BORDER_REL_T)
    rows = gn.gaussian_rows(st, cam["projmatrix_raw"])
    J, col, dep = gn.jacobian(st, rows, gn.JAC_BG)
    return dict(cam=cam, sc=sc, planted=planted, out=out, st=st, seeds=(s_c, s_d), em=em, rows=rows, J=J, color=col, depth=dep)


def test_the_scene_of_the_gpu_tests_is_clean_and_shows_every_planted_case(scene):
    st, planted, out = scene["st"], scene["planted"], scene["out"]
    assert not scene["em"]["border_mask"].any(), "JAC_SEED: a borderline pixel -- the strict limit would not apply"
    (_, st16), _ = gn.oracle_forward(scene["cam"], scene["sc"], record_bits=16)
    em16 = orc.error_model(st16, *scene["seeds"], hp.BORDER_REL, hp.BORDER_REL_T)
    assert not em16["border_mask"].any(), "JAC_SEED: a borderline pixel with fp16 records"
    assert len(gn.row_pixels(planted, scene["em"]["border_mask"])) >= 14
    nc, fT = st["n_contrib"], st["final_T"]
    at = lambda name: planted[name][1][::-1]  # noqa: E731  (y, x)
    assert 350 <= st["P"] <= 420 and (st["W"], st["H"]) == (72, 40) and st["W"] % 16 and st["H"] % 16
    assert nc[at("stack")] > 70                                   # more than two 32-entry staging chunks in one quadrant
    assert fT[at("opaque")] < 2e-4 and nc[at("opaque")] < 20      # ended early, with list entries left behind it
    tile = gn.EMPTY_TILE[1] * 5 + gn.EMPTY_TILE[0]
    assert st["ranges"][tile, 0] == st["ranges"][tile, 1] and nc[at("empty_tile")] == 0
    # the alpha cap is active: o G > 0.99 at the centre pixel of a cap splat
    i = planted["cap"][0][0]
    a, b, c, o = st["conic_opacity"][i].astype(np.float64)
    dx, dy = st["means2D"][i].astype(np.float64) - np.round(st["means2D"][i])
    assert o * np.exp(-0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy) > 0.99
    # clamp gates: the centres project beyond +-1.3 tanfov, and the Gaussians are rendered
    vm = scene["cam"]["viewmatrix"].reshape(4, 4).astype(np.float64)
    for name, axis, lim in (("clamp_x", 0, 1.3 * scene["cam"]["tanfovx"]), ("clamp_y", 1, 1.3 * scene["cam"]["tanfovy"])):
        for i in planted[name][0]:
            t = np.append(scene["sc"]["means3D"][i].astype(np.float64), 1.0) @ vm
            assert abs(t[axis] / t[2]) > lim and st["radii"][i] > 0, (name, i)
    near = [float((np.append(scene["sc"]["means3D"][i].astype(np.float64), 1.0) @ vm)[2]) for i in planted["near"][0]]
    assert near[0] > 0.2 > near[1] and st["radii"][planted["near"][0][0]] > 0 and st["radii"][planted["near"][0][1]] == 0
    assert st["clamped"][planted["sh_clamp"][0]].any()


def test_restated_jacobian_is_the_transpose_of_the_oracles_backward(scene):
    """sum s J against the oracle's dL/dtau, the comparator and limit of the GPU test; the walk re-derives the oracle's images."""
    g = gn.contract(scene["J"], *scene["seeds"])
    e = gn.assert_transpose_identity(g, scene["st"], *scene["seeds"], scene["cam"]["projmatrix_raw"], hp.GRAD_TOL, "restated")
    assert e < 1e-5
    assert np.abs(scene["color"] - scene["out"]["color"]).max() < 5e-6 and np.abs(scene["depth"] - scene["out"]["depth"][0]).max() < 5e-6
    # single rows under one-hot seeds, background-only pixel: row = 0
    x, y = scene["planted"]["empty_tile"][1]
    assert not scene["J"][y, x].any()
    x, y = scene["planted"]["cap"][1]
    for ch in range(4):
        s_c, s_d = np.zeros((3, gn.JAC_H, gn.JAC_W), np.float32), np.zeros((1, gn.JAC_H, gn.JAC_W), np.float32)
        (s_c if ch < 3 else s_d)[ch % 3, y, x] = 1.0
        want = orc.backward(scene["st"], s_c, s_d, scene["cam"]["projmatrix_raw"])["dL_dtau_sum"]
        assert hp.rel_err(scene["J"][y, x, ch], want) < hp.GRAD_TOL, ch


@pytest.mark.parametrize("mutant", ["drop_alpha_S", "no_background"])
def test_compositor_mutants_are_rejected_by_the_transpose_comparator(scene, mutant):
    Jm, _, _ = gn.jacobian(scene["st"], scene["rows"], gn.JAC_BG, mutant=mutant)
    with pytest.raises(AssertionError, match="differs from the oracle"):
        gn.assert_transpose_identity(gn.contract(Jm, *scene["seeds"]), scene["st"], *scene["seeds"], scene["cam"]["projmatrix_raw"],
                                     hp.GRAD_TOL, mutant)


def _frame(flags, masked, seed=4):
    fr = lr.make_frame(41, 25, flags, masked, seed)
    return fr, dict(flags=fr["flags"], alpha=fr["alpha"], rgb_thr=fr["rgb_thr"], image=fr["image"], depth=fr["depth"], opacity=fr["opacity"],
                    gt=fr["gt"], gt_depth=fr["gt_depth"], mask=fr["mask"], a=fr["a"], b=fr["b"])


@pytest.mark.parametrize("flags", [lr.TRACKING, lr.TRACKING | lr.MONOCULAR])
@pytest.mark.parametrize("masked", [False, True])
def test_seeds_at_delta_zero_are_the_backwards_seeds_exactly(flags, masked):
    fr, kw = _frame(flags, masked)
    q = gn.irls(delta=0.0, **kw)
    want = lr.restate_frame(fr)["value"]
    assert np.array_equal(q["s"][:3], want["dL_dcolor"]) and np.array_equal(q["s"][3:], want["dL_ddepth"].reshape(1, 25, 41))
    assert (q["h"] >= 0).all() and np.isfinite(q["h"]).all()
    assert not q["h"][q["s"] == 0].any(), "no curvature where the gate is closed or the residual is exactly 0"
    d = gn.irls(delta=0.05, **kw)
    assert (np.abs(d["s"]) <= np.abs(q["s"]) * (1 + 1e-12)).all() and (d["h"] <= q["h"] * (1 + 1e-12) + (q["h"] == 0) * 1e300).all()


def test_normal_equations_are_symmetric_positive_semidefinite_and_the_curvature_mutant_is_rejected():
    fr, kw = _frame(lr.TRACKING, True)
    rng = np.random.default_rng(2)
    J = rng.normal(size=(25, 41, 4, 6)) * 50.0
    q = gn.irls(delta=0.02, **kw)
    ne = gn.normal_equations(J, q["s"], q["h"], q["err_s"], q["err_h"])
    assert np.array_equal(ne["H"], ne["H"].T) and np.linalg.eigvalsh(ne["H"]).min() > -1e-12 * np.abs(ne["H"]).max()
    assert gn.assert_normal_equations_close(ne["H"].astype(np.float32), ne["g"].astype(np.float32), ne, "self") <= 1.0
    m = gn.irls(delta=0.02, mutant="delta_signed_r", **kw)
    bad = gn.normal_equations(J, m["s"], m["h"])
    with pytest.raises(AssertionError, match="x bound"):
        gn.assert_normal_equations_close(bad["H"], bad["g"], ne, "delta_signed_r")


def _quadratic(seed=0):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(40, 6))
    return (A.T @ A).astype(np.float32).astype(np.float64), rng.normal(size=6).astype(np.float32).astype(np.float64) * 1e-2


def test_lm_step_solves_a_quadratic_in_one_accepted_step_as_lambda_goes_to_zero():
    H, g = _quadratic()
    st = gn.lm_new_state(np.eye(4), 1e-12)
    gn.lm_step(st, H, g, 1.0, nu=2.0, lambda_min=1e-15, lambda_max=1e6, threshold=1e-4)
    assert (st["accepted"], st["rejected"]) == (1, 0)
    np.testing.assert_allclose(st["tau"], np.linalg.solve(H, -g), rtol=1e-5)
    np.testing.assert_allclose(st["w2c"], gn.se3_exp(st["tau"]), atol=1e-12)
    assert np.allclose(st["w2c"][:3, :3] @ st["w2c"][:3, :3].T, np.eye(3), atol=1e-12)


def test_lm_step_never_accepts_a_loss_increase_and_a_reject_goes_back_to_the_accepted_pose():
    H, g = _quadratic(1)
    rng = np.random.default_rng(5)
    st = gn.lm_new_state(np.eye(4), 1e-3)
    acc, lam = [], []
    for loss in [1.0, 0.8, 0.9, 0.85, 0.7, 0.7, 2.0, np.nan, 0.1] + list(rng.uniform(0.0, 1.0, size=20)):
        before = st["acc_w2c"].copy()
        was = st["acc_loss"] if st["has"] else np.inf
        gn.lm_step(st, H, g * rng.uniform(0.5, 1.5), loss, nu=3.0, lambda_min=1e-6, lambda_max=1e3, threshold=1e-4)
        acc.append(st["acc_loss"])
        lam.append(st["lam"])
        if not (float(np.float32(loss)) <= was):  # rejected: the step was taken from the accepted pose, which did not move
            assert np.array_equal(st["acc_w2c"], before)
            np.testing.assert_allclose(st["w2c"], gn.se3_exp(st["tau"]) @ before, atol=1e-12)
    assert all(b <= a for a, b in zip(acc, acc[1:]))
    assert 1e-6 <= min(lam) and max(lam) <= 1e3


def test_lm_mutant_is_rejected_by_the_state_comparator():
    H, g = _quadratic(2)
    proj = np.eye(4)
    good, bad = gn.lm_new_state(np.eye(4), 1e-3), gn.lm_new_state(np.eye(4), 1e-3)
    for loss in (1.0, 1.5, 0.5):  # accept, reject, accept
        gn.lm_step(good, H, g, loss, 2.0, 1e-6, 1e3, 1e-4)
        gn.lm_step(bad, H, g, loss, 2.0, 1e-6, 1e3, 1e-4, mutant="not_restored_on_reject")
    gn.assert_lm_state_close(gn.pack_state(good, proj), good, proj, "self")
    with pytest.raises(AssertionError):
        gn.assert_lm_state_close(gn.pack_state(bad, proj), good, proj, "not_restored_on_reject")


NEW_SYMBOLS = ("gsaj_pose_jac_workspace_bytes", "gsaj_pose_jac_partial_rows", "gsaj_rasterize_pose_jacobian",
               "gsaj_rasterize_pose_jacobian_loss", "gsaj_gn_state_floats", "gsaj_pose_gn_step")


def test_header_declares_the_new_symbols_and_the_binding_matches_their_arity():
    from gsaj import _lib

    with open(_lib.HEADER) as fh:
        text = fh.read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\);" % name, text, re.S)
        assert m, "%s is not declared in include/gsaj.h" % name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        n = 0 if args == "void" else len(args.split(","))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, (name, n)
    assert re.search(r"#define GSAJ_GN_STATE_FLOATS (\d+)", text) and re.search(r"#define GSAJ_GN_PARTIAL_FLOATS 32\b", text)
    lib = _lib.load()
    assert lib.gsaj_gn_state_floats() == int(re.search(r"#define GSAJ_GN_STATE_FLOATS (\d+)", text).group(1)) == gn.pack_state(
        gn.lm_new_state(np.eye(4), 1.0), np.eye(4)).size
    assert lib.gsaj_pose_jac_partial_rows(72, 40) == 64 and lib.gsaj_pose_jac_workspace_bytes(400, 72, 40) >= 400 * 48 * 4 + 64 * 32 * 4


def test_there_is_no_cpu_path():
    import torch
    import gsaj
    from gsaj import _lib
    from gsaj.rasterizer import FrameContext

    z = torch.zeros(3)
    with pytest.raises(_lib.GsajError, match="HIP device"):
        gsaj.GaussNewtonTracker(10, 32, 32, 16, "cpu", np.eye(4), np.eye(4), 0.5, 0.5, z, torch.zeros(10, 3), torch.zeros(10, 1))
    ctx = object.__new__(FrameContext)  # (a FrameContext cannot be made without a device: its constructor allocates on it)
    ctx.dev = torch.device("cpu")
    for call in (lambda: ctx.pose_jacobian(z, z, z, z, z, z, 0.5, 0.5), lambda: ctx.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5)):
        with pytest.raises(_lib.GsajError, match="HIP device"):
            call()
