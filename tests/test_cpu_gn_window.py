"""CPU: the batched Gauss-Newton path without a GPU -- the restated window (tests/gn_window_restated.py) and its canaries: every
mutant that reads another view's data must be rejected by the comparators the GPU tests use; the host logic of GaussNewtonWindow
and BatchContext.pose_jacobian_loss with the launch replaced; the new C-ABI symbols and their argument errors; and the premises of
the GPU behaviour tests on the restated loop."""
import math
import re

import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import gn_window_restated as gw
import loss_restated as lr

F = np.float32
DELTA = 0.03
LM = dict(nu=4.0, lambda_min=1e-7, lambda_max=1e7, converged_threshold=1e-4)
A_STAR, B_STAR = 0.2, -0.05     # the exposure of the behaviour tests (tests/test_gpu_gn8_tracker.py)
BUDGET = 8                      # ... and their iteration budget, 2 x GN8_MEASURED


@pytest.fixture(scope="module")
def window():
    """The K = 3 views restated from the oracle: state, derivative rows, Jacobian, images; each view's own ground truth."""
    cams, sc, _ = gw.window_cameras()
    views, truths = [], []
    for v, cam in enumerate(cams):
        (out, st), _ = gn.oracle_forward(cam, sc)
        rows = gn.gaussian_rows(st, cam["projmatrix_raw"])
        J, col, dep = gn.jacobian(st, rows, gn.JAC_BG)
        views.append(dict(st=st, rows=rows, J=J, image=col.astype(F), depth=dep.astype(F)[None], opacity=out["opacity"]))
        truths.append(gw.ground_truth(col, dep, v))
    return dict(cams=cams, sc=sc, views=views, truths=truths)


def test_every_view_of_the_window_differs_from_view_0(window):
    """What makes a cross-view mix-up visible: no two views share a camera, a tile list, a ground truth, a mask or an exposure."""
    v0 = window["views"][0]
    for v in (1, 2):
        view = window["views"][v]
        assert not np.array_equal(view["st"]["point_list"], v0["st"]["point_list"])
        assert np.abs(view["J"] - v0["J"]).max() > 1e-3 * np.abs(v0["J"]).max()
        for a, b in zip(window["truths"][v], window["truths"][0]):
            assert not np.array_equal(a, b)
        assert gw.EXPOSURES[v] != gw.EXPOSURES[0]
    assert gw.K == 3 and len(set(gw.EXPOSURES)) == 3


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
@pytest.mark.parametrize("mutant", gw.EQUATION_MUTANTS)
def test_a_view_that_reads_view_0s_data_is_rejected_by_the_normal_equation_comparator(window, mutant, joint):
    good = gw.window_equations(window["views"], window["truths"], gw.EXPOSURES, DELTA, joint, masked=True)
    bad = gw.window_equations(window["views"], window["truths"], gw.EXPOSURES, DELTA, joint, masked=True, mutant=mutant)
    for v in range(gw.K):
        want = good[v][0]
        assert gn.assert_normal_equations_close(want["H"].astype(F), want["g"].astype(F), want, "self") <= 1.0
        if v == 0:   # view 0 reads its own data under every mutant
            assert np.array_equal(bad[0][0]["H"], want["H"]) and np.array_equal(bad[0][0]["g"], want["g"])
            continue
        with pytest.raises(AssertionError, match="x bound"):
            gn.assert_normal_equations_close(bad[v][0]["H"], bad[v][0]["g"], want, "%s view %d" % (mutant, v))


@pytest.mark.parametrize("mutant", gw.EQUATION_MUTANTS[:3])
def test_the_loss_comparator_rejects_them_too(window, mutant):
    good = gw.window_equations(window["views"], window["truths"], gw.EXPOSURES, DELTA, False, masked=True)
    bad = gw.window_equations(window["views"], window["truths"], gw.EXPOSURES, DELTA, False, masked=True, mutant=mutant)
    for v in (1, 2):
        got = bad[v][1]["loss"]["value"]
        with pytest.raises(AssertionError):
            lr.assert_loss_close(dict(loss=got["loss"], l1_rgb=got["l1_rgb"], l1_depth=got["l1_depth"]), good[v][1]["loss"], mutant,
                                 outputs=("loss", "l1_rgb", "l1_depth"))


def _quadratics(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for v in range(gw.K):
        A = rng.normal(size=(50, n))
        out.append(((A.T @ A).astype(F).astype(np.float64), rng.normal(size=n).astype(F).astype(np.float64) * 1e-2, 1.0 + 0.1 * v))
    return out


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_window_step_honours_active_and_skip_and_the_row_mix_up_is_rejected_by_the_state_comparator(joint):
    n = 8 if joint else 6
    new = (lambda: g8.lm8_new_state(np.eye(4), 1e-3, exposure=(0.1, -0.02))) if joint else (lambda: gn.lm_new_state(np.eye(4), 1e-3))
    pack, close = (g8.pack_state8, g8.assert_lm8_state_close) if joint else (gn.pack_state, gn.assert_lm_state_close)
    sums = _quadratics(n)
    good, bad, masked = [new() for _ in range(3)], [new() for _ in range(3)], [new() for _ in range(3)]
    gw.window_step(good, sums, joint, LM)
    gw.window_step(bad, sums, joint, LM, mutant="rows_into_previous_state")
    gw.window_step(masked, sums, joint, LM, active=(1, 0, 1), skip=(0, 0, 1))
    proj = np.eye(4)
    for v in range(3):
        close(pack(good[v], proj), good[v], proj, "self %d" % v)
    for v in (0, 1):   # (the last view has no later view's rows to be handed)
        with pytest.raises(AssertionError):
            close(pack(bad[v], proj), good[v], proj, "rows_into_previous_state view %d" % v)
    close(pack(masked[0], proj), good[0], proj, "active view")
    for v in (1, 2):   # inactive / skipped: nothing of the state moved
        assert masked[v]["accepted"] == 0 and not masked[v]["has"] and np.array_equal(masked[v]["w2c"], np.eye(4))


def test_restated_select_and_its_mutant():
    inf, nan = float("inf"), float("nan")
    assert gw.select([0.5, 0.2, 0.3], [1, 1, 1]) == (1, float(F(0.2)))
    assert gw.select([0.5, 0.2, 0.3], [1, 1, 1], active=[1, 0, 1]) == (2, float(F(0.3)))
    assert gw.select([0.5, 0.2, 0.3], [1, 1, 1], active=[1, 0, 1], mutant="select_ignores_active")[0] == 1   # what the device must not do
    assert gw.select([0.3, 0.3, 0.3], [1, 1, 1])[0] == 0, "ties go to the lowest index"
    assert gw.select([0.5, 0.3, 0.3], [1, 1, 1])[0] == 1
    assert gw.select([nan, 0.4, inf], [1, 1, 1])[0] == 1
    assert gw.select([0.1, 0.4, 0.2], [0, 1, 1])[0] == 2, "a view without an accepted pose does not qualify"
    assert gw.select([0.1, 0.4, 0.2], [0, 0, 0]) == (-1, inf)
    assert gw.select([nan, 0.4, 0.2], [1, 1, 1], active=[1, 0, 0]) == (-1, inf)


# ---- premises of the GPU behaviour tests, on the restated loop -------------------------------------------------------------------
def _next_pose(w):
    """The frame-to-frame motion of tests/test_cpu_gn8.py: 3 cm / 0.75 degrees."""
    ang = math.radians(0.75)
    d = np.eye(4)
    d[:3, :3] = np.array([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
    d[:3, 3] = (0.03, -0.02, 0.025)
    return np.linalg.inv(d) @ w


def _exposed_frame(cam, sc, true):
    (out, _), _ = gn.oracle_forward(g8.camera_at(cam, true), sc)
    return (math.exp(A_STAR) * out["color"] + B_STAR).astype(F), out["depth"][0].astype(F)


def _restated_joint_loop(cam, sc, start, true, gt, gd, before):
    """-> (state, the iteration at which the accepted pose and exposure first met the criteria of tests/test_gpu_gn8_tracker.py or
    None, the accepted losses)."""
    st, met, acc = g8.lm8_new_state(start, 1e-3), None, []
    e0 = max(abs(A_STAR), abs(B_STAR))
    for it in range(1, BUDGET + 1):
        H, g, loss = g8.restated_rows(cam, sc, st["w2c"], st["exposure"], gt, gd, 0.01, True)
        g8.lm8_step(st, H, g, loss, LM["nu"], LM["lambda_min"], LM["lambda_max"], LM["converged_threshold"])
        acc.append(st["acc_loss"])
        te, re_ = g8.pose_errors(st["acc_w2c"], true)
        ee = float(np.abs(st["acc_exposure"] - [A_STAR, B_STAR]).max())
        if met is None and te < 0.35 * before and re_ < 0.02 and ee < 0.35 * e0:
            met = it
    return st, met, acc


def test_premises_every_window_start_converges_within_the_budget_and_the_best_hypothesis_is_the_right_one(window):
    """(a) The window test: slot v holds frame v + 1 and starts from frame v's true pose; every slot meets both criteria within the
    budget and its accepted loss never rises.  (b) The multi-start test: one frame, starts at the previous true pose and at that pose
    moved by +-5 x the frame-to-frame translation along x; the hypothesis of smallest accepted loss meets the pose criterion (the
    moved ones settle, with a loss they keep accepting, at a wrong pose: what best() is for)."""
    cam, sc = window["cams"][0], window["sc"]
    poses = [np.asarray(cam["w2c"], np.float64)]
    for _ in range(gw.K):
        poses.append(_next_pose(poses[-1]))
    first = None
    for v in range(gw.K):
        gt, gd = _exposed_frame(cam, sc, poses[v + 1])
        before = g8.pose_errors(poses[v], poses[v + 1])[0]
        st, met, acc = _restated_joint_loop(cam, sc, poses[v], poses[v + 1], gt, gd, before)
        print("slot %d: criteria met after %s iterations (budget %d), accepted loss %.5f -> %.6f" % (v, met, BUDGET, acc[0], acc[-1]))
        assert met is not None and met <= BUDGET, (v, met, acc)
        assert all(b <= a for a, b in zip(acc, acc[1:])), (v, acc)
        first = first or (gt, gd, before, st)
    gt, gd, before, st0 = first
    step = float(np.abs(poses[1][:3, 3] - poses[0][:3, 3]).max())
    finals = [st0]
    for sign in (5.0, -5.0):
        start = poses[0].copy()
        start[0, 3] += sign * step
        finals.append(_restated_joint_loop(cam, sc, start, poses[1], gt, gd, before)[0])
    best, loss = gw.select([s["acc_loss"] for s in finals], [s["has"] for s in finals])
    te, re_ = g8.pose_errors(finals[best]["acc_w2c"], poses[1])
    print("multi-start: accepted losses %s -> hypothesis %d, translation error %.4f x the nominal start's" % (
        ["%.5f" % s["acc_loss"] for s in finals], best, te / before))
    assert best >= 0 and te < 0.35 * before and re_ < 0.02, (best, te, before, re_)
    for h in (1, 2):
        assert finals[h]["acc_loss"] > 10 * loss and g8.pose_errors(finals[h]["acc_w2c"], poses[1])[0] > before, \
            "a moved start keeps accepting a loss at a wrong pose"


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gsaj_pose_jac_batch_workspace_bytes", "gsaj_rasterize_pose_jacobian_loss_batch", "gsaj_rasterize_pose_jacobian_loss8_batch",
               "gsaj_pose_gn_step_batch", "gsaj_pose_gn8_step_batch", "gsaj_pose_gn_select")


def test_header_declares_the_new_symbols_and_the_binding_matches_their_arity():
    from gsaj import _lib

    with open(_lib.HEADER) as fh:
        text = fh.read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\);" % name, text, re.S)
        assert m, "%s is not declared in include/gsaj.h" % name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
    S = _lib.SIGNATURES
    assert S["gsaj_rasterize_pose_jacobian_loss_batch"] == S["gsaj_rasterize_pose_jacobian_loss8_batch"]
    # the arguments of gsaj_rasterize_backward_loss_batch up to the loss group (everything before its twelve gradient outputs)
    n = len(S["gsaj_rasterize_backward_loss_batch"][1]) - 12 - 2
    assert S["gsaj_rasterize_pose_jacobian_loss_batch"][1][:n] == S["gsaj_rasterize_backward_loss_batch"][1][:n]
    assert S["gsaj_pose_gn_step_batch"] == S["gsaj_pose_gn8_step_batch"]
    lib = _lib.load()
    one = lib.gsaj_pose_jac_batch_workspace_bytes(1, 1000, 72, 40)
    assert one % 256 == 0 and one >= 48 * 4 * 1000 and lib.gsaj_pose_jac_batch_workspace_bytes(3, 1000, 72, 40) == 3 * one
    assert lib.gsaj_pose_jac_batch_workspace_bytes(0, 1000, 72, 40) == 0
    assert lib.gsaj_version() >= 109


def _jac_batch(lib, joint=False, **kw):
    """A call whose arguments are all plausible host values (no kernel is reached by the cases below)."""
    import ctypes
    buf = ctypes.create_string_buffer(4096 + 256)
    p = (ctypes.addressof(buf) + 255) & ~255
    a = dict(K=3, P=10, D=0, M=1, capacity=64, bg=p, W=32, H=32, means3D=p, shs=None, colors_precomp=p, scales=p, scale_modifier=1.0, rotations=p,
             cov3D_precomp=None, viewmatrices=p, projmatrices=p, projmatrix_raw=p, campos=None, tanfovx=0.5, tanfovy=0.5, radii=p, geom_ws=p,
             binning_ws=p, image_ws=p, loss_flags=lr.TRACKING, alpha=0.9, thr=0.01, color=p, depth=p, opacity=p, gt_color=p, gt_depth=p,
             grad_mask=None, exposure_a=p, exposure_b=p, exposure_stride=1, jac_ws=p, irls_delta=0.01, partials=p, jac_out=None, stream=None)
    a.update(kw)
    fn = lib.gsaj_rasterize_pose_jacobian_loss8_batch if joint else lib.gsaj_rasterize_pose_jacobian_loss_batch
    rc = fn(*a.values())
    return rc, lib.gsaj_last_error().decode()


def test_argument_errors_are_returned_without_a_launch():
    import ctypes
    from gsaj import _lib

    lib = _lib.load()
    for joint, who in ((False, "loss_batch"), (True, "loss8_batch")):
        for kw, text in ((dict(K=0), "K=0"), (dict(K=-2), "K=-2"), (dict(gt_color=None), "invalid loss arguments"),
                         (dict(exposure_stride=0), "exposure stride 0"), (dict(irls_delta=-1.0), "irls_delta"), (dict(partials=None), "gn_partials"),
                         (dict(color=None), "color / depth / opacity"), (dict(jac_ws=None), "invalid argument"), (dict(radii=None), "invalid argument"),
                         (dict(capacity=0), "invalid argument")):
            rc, msg = _jac_batch(lib, joint, **kw)
            assert rc == -1 and text in msg and who in msg, (joint, kw, rc, msg)
        for name in ("geom_ws", "binning_ws", "image_ws", "jac_ws"):   # misaligned blocks
            buf = ctypes.create_string_buffer(1024)
            rc, msg = _jac_batch(lib, joint, **{name: ((ctypes.addressof(buf) + 255) & ~255) + 16})
            assert rc == -1 and "256-byte aligned" in msg, (joint, name, rc, msg)
    # the joint form solves for the exposure
    for kw in (dict(loss_flags=lr.TRACKING | lr.NO_EXPOSURE), dict(loss_flags=lr.TRACKING | lr.NO_EXPOSURE, exposure_a=None, exposure_b=None)):
        rc, msg = _jac_batch(lib, True, **kw)
        assert rc == -1 and "joint form" in msg, (kw, msg)
    assert _jac_batch(lib, True, exposure_b=None)[0] == -1
    # the batched step and select
    step = lambda fn, **kw: fn(*dict(dict(K=3, partials=1, n=4, active=None, lambda_init=1e-3, nu=4.0, lambda_min=1e-7, lambda_max=1e7, thr=1e-4,  # noqa: E731
                                          proj=None, states=1, skip=None, stride=0, stream=None), **kw).values())
    for fn, who in ((lib.gsaj_pose_gn_step_batch, "gsaj_pose_gn_step_batch"), (lib.gsaj_pose_gn8_step_batch, "gsaj_pose_gn8_step_batch")):
        for kw in (dict(K=0), dict(partials=None), dict(n=0), dict(states=None), dict(nu=1.0), dict(lambda_min=0.0), dict(lambda_init=1e8)):
            assert step(fn, **kw) == -1 and who in lib.gsaj_last_error().decode() and "nu > 1" in lib.gsaj_last_error().decode(), kw
    for args in ((0, 1, 136, None, 1, 1, None), (3, None, 136, None, 1, 1, None), (3, 1, 80, None, 1, 1, None), (3, 1, 152, None, None, 1, None),
                 (3, 1, 152, None, 1, None, None)):
        assert lib.gsaj_pose_gn_select(*args) == -1 and "gsaj_pose_gn_select" in lib.gsaj_last_error().decode(), args


# ---- host logic with the launch replaced ------------------------------------------------------------------------------------------------
class _FakeContext:
    """What GaussNewtonWindow asks of its BatchContext outside an iteration."""

    def __init__(self, K, W, H):
        import torch
        self.K, self.W, self.H, self.dev = K, W, H, torch.device("cpu")
        self.aborts = 0

    def clear_aborts(self):
        n, self.aborts = self.aborts, 0
        return n


def _window(monkeypatch, K=3, W=8, H=6, solve_exposure=True, monocular=False):
    import torch
    import gsaj.gauss_newton as G

    calls = []
    monkeypatch.setattr(G, "_launch", lambda win, sync: calls.append(sync))
    w2cs = np.stack([gn.se3_exp([0.01 * k, 0, 0, 0, 0.02 * k, 0]) for k in range(K)])
    win = G.GaussNewtonWindow.__new__(G.GaussNewtonWindow)
    win._init_host(_FakeContext(K, W, H), w2cs, np.eye(4), (0.5, 0.4), torch.zeros(3), torch.zeros(5, 3), torch.zeros(5, 1), {},
                   dict(monocular=monocular, alpha=0.9, rgb_boundary_threshold=0.01, irls_delta=0.01), (1e-3, 4.0, 1e-7, 1e7, 1e-4), solve_exposure)
    return win, calls, w2cs


@pytest.mark.parametrize("solve_exposure", [False, True])
def test_window_shapes_and_initial_state(monkeypatch, solve_exposure):
    import torch
    from gsaj.gauss_newton import GaussNewtonTracker

    win, _, w2cs = _window(monkeypatch, solve_exposure=solve_exposure)
    n = 152 if solve_exposure else 136
    assert tuple(win.state.shape) == (3, n) and win.state.is_contiguous()
    assert tuple(win.gt_color.shape) == (3, 3, 6, 8) and tuple(win.gt_depth.shape) == (3, 6, 8) and win.grad_mask is None
    assert tuple(win.accepted_w2c.shape) == (3, 4, 4) and tuple(win.accepted_exposure.shape) == (3, 2) and tuple(win.loss_terms.shape) == (3, 3)
    lm = win.lm
    m = 8 if solve_exposure else 6
    assert tuple(lm["H"].shape) == (3, m, m) and tuple(lm["g"].shape) == (3, m) and all(tuple(lm[k].shape) == (3,) for k in ("lam", "accepted", "rejected", "accepted_loss"))
    assert win.active.dtype == torch.uint8 and win.active.tolist() == [1, 1, 1]
    views, projs, cps = win.matrices()
    assert tuple(views.shape) == (3, 4, 4) and tuple(projs.shape) == (3, 4, 4) and tuple(cps.shape) == (3, 3) and views.is_contiguous()
    # every row is the single tracker's initial state for that pose
    one = GaussNewtonTracker.__new__(GaussNewtonTracker)
    one.dev, one.projection, one.lm_args, one.solve_exposure = win.dev, win.projection, win.lm_args, solve_exposure
    for k in range(3):
        one.state = torch.zeros(n)
        one.reset(w2cs[k])
        assert torch.equal(win.state[k], one.state), k
    # the exposure pair is read in place: [K] views of the state with the state's row length as stride
    assert win.state[:, 33].stride(0) == n and win.state[:, 33].data_ptr() == win.state.data_ptr() + 4 * 33


def test_set_frame_broadcasts_one_frame_and_set_view_fills_one_slot(monkeypatch):
    import torch
    from gsaj import _lib

    win, calls, w2cs = _window(monkeypatch)
    with pytest.raises(_lib.GsajError, match=r"slots \[0, 1, 2\] have no frame"):
        win.iterate(1)
    g = torch.Generator().manual_seed(1)
    frames = [(torch.rand(3, 6, 8, generator=g), torch.rand(6, 8, generator=g)) for _ in range(3)]
    win.set_view(1, *frames[1], w2c=w2cs[2], exposure=(0.1, -0.2))
    assert torch.equal(win.gt_color[1], frames[1][0]) and not win.gt_color[0].any() and not win.gt_color[2].any()
    assert torch.allclose(win.w2c[1], torch.as_tensor(w2cs[2], dtype=torch.float32)) and win.state[1, 33:35].tolist() == pytest.approx([0.1, -0.2])
    assert torch.equal(win.accepted_exposure[1], win.state[1, 33:35]) and float(win.state[1, 80]) == pytest.approx(1e-3)
    with pytest.raises(_lib.GsajError, match=r"slots \[0, 2\]"):
        win.iterate(1)
    # a mask on one slot: the others get all ones, which is no mask
    mask = (torch.rand(1, 6, 8, generator=g) < 0.5).to(torch.uint8)
    win.set_view(0, *frames[0], grad_mask=mask)
    assert tuple(win.grad_mask.shape) == (3 * 48,) and torch.equal(win.grad_mask[:48], mask.view(-1)) and bool((win.grad_mask[48:] == 1).all())
    before = win.state.clone()
    starts = np.stack([gn.se3_exp([0.1 * k, 0, 0, 0, 0, 0]) for k in range(3)])
    win.set_frame(*frames[2], w2cs=starts)
    for k in range(3):
        assert torch.equal(win.gt_color[k], frames[2][0]) and torch.equal(win.gt_depth[k], frames[2][1])
        assert torch.allclose(win.w2c[k], torch.as_tensor(starts[k], dtype=torch.float32)) and not win.state[k, 33:35].any()
    assert bool((win.grad_mask == 1).all()) and not torch.equal(win.state, before)
    kept = win.state.clone()
    win.set_frame(*frames[0])       # no new starts: the poses stay
    assert torch.equal(win.state, kept)
    # the first iteration is synchronous, the rest are not; an aborted view is reported after the loop and re-sizes the next call
    assert win.iterate(3) == 3 and calls == [True, False, False] and win.iterations == 3
    win.ctx.aborts = 2
    with pytest.raises(_lib.GsajError, match="2 asynchronous forward"):
        win.iterate(2)
    assert calls[3:] == [False, False]
    assert win.iterate(1) == 1 and calls[5] is True
    # check_every: one read of the K flags; stops when every ACTIVE view has converged
    win.state[:, 77] = torch.tensor([1.0, 0.0, 1.0])
    assert win.iterate(6, check_every=2) == 6
    win.active[1] = 0
    assert win.iterate(6, check_every=2) == 2


def test_window_error_texts(monkeypatch):
    import torch
    import gsaj
    from gsaj import _lib

    z = torch.zeros(3)
    with pytest.raises(_lib.GsajError, match="HIP device"):
        gsaj.GaussNewtonWindow(2, 10, 32, 32, 16, "cpu", np.stack([np.eye(4)] * 2), np.eye(4), 0.5, 0.5, z, torch.zeros(10, 3), torch.zeros(10, 1))
    win, _, _ = _window(monkeypatch)
    c, d = torch.zeros(3, 6, 8), torch.zeros(6, 8)
    for args, kw, text in (((3, c, d), {}, "slot 3"), ((-1, c, d), {}, "slot -1"), ((0, torch.zeros(3, 8, 6), d), {}, r"gt_color must be \[3,6,8\]"),
                           ((0, c), {}, "monocular"), ((0, c, torch.zeros(5, 8)), {}, "gt_depth must have 48"),
                           ((0, c, d), dict(grad_mask=torch.zeros(47, dtype=torch.uint8)), "grad_mask must have 48")):
        with pytest.raises(_lib.GsajError, match=text):
            win.set_view(*args, **kw)
    with pytest.raises(_lib.GsajError, match=r"w2cs must be \[3,4,4\]"):
        win.set_frame(c, d, w2cs=np.stack([np.eye(4)] * 2))
    mono, _, _ = _window(monkeypatch, monocular=True)
    assert mono.gt_depth is None
    with pytest.raises(_lib.GsajError, match="monocular"):
        mono.set_view(0, c, d)
    with pytest.raises(_lib.GsajError, match=r"w2cs must be \[3,4,4\]"):
        _window(monkeypatch, K=3)[0]._init_host(_FakeContext(3, 8, 6), np.eye(4), np.eye(4), (0.5, 0.4), z, z, z, {},
                                                dict(monocular=False, alpha=0.9, rgb_boundary_threshold=0.01, irls_delta=0.01), (1e-3, 4.0, 1e-7, 1e7, 1e-4), False)


def _batch_context(K=3, P=10, W=32, H=32):
    import torch
    from gsaj import _lib
    from gsaj.rasterizer import BatchContext

    c = BatchContext.__new__(BatchContext)
    c.lib, c.K, c.P, c.W, c.H, c.M, c.dev = _lib.load(), K, P, W, H, 1, torch.device("cpu")
    c.binning = torch.empty(0, dtype=torch.uint8)
    c.groups = [(0, K, None)]
    c.bands = {}
    return c


def test_batch_pose_jacobian_loss_host_checks_come_before_the_device(monkeypatch):
    import torch
    import gsaj.rasterizer as R
    from gsaj import _lib

    launched = []
    monkeypatch.setattr(R, "_launch_groups", lambda ctx, name, calls: launched.append((name, calls)))
    c = _batch_context()
    z = torch.zeros(3)
    with pytest.raises(_lib.GsajError, match="run a forward of this context first"):
        c.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5)
    c.binning = torch.empty(16, dtype=torch.uint8)
    c.bands = {1: (0, 1)}
    with pytest.raises(_lib.GsajError, match="a tile band is set on a view"):
        c.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5)
    c.bands = {1: (0, 2)}   # (the whole frame of a 32-row image: no band)
    rows = c.lib.gsaj_pose_jac_partial_rows(32, 32)
    with pytest.raises(_lib.GsajError, match=r"partials must be a contiguous float32 \[3, %d, 64\]" % rows):
        c.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5, solve_exposure=True, partials=torch.zeros((3, rows, 32)))
    with pytest.raises(_lib.GsajError, match=r"\[3, %d, 32\]" % rows):
        c.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5, partials=torch.zeros((rows, 32)))
    with pytest.raises(_lib.GsajError, match="must be device tensors"):
        c.pose_jacobian_loss({}, z, z, z, z, z, z, 0.5, 0.5)
    assert tuple(c.gn_partials.shape) == (3, rows, 32) and c.jac_ws.numel() == 3 * c.jac_stride and c.jac_stride % 256 == 0
    assert not launched
