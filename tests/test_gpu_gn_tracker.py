"""GPU: the Levenberg-Marquardt pose step (gsaj_pose_gn_step) against its restatement, and gsaj.gauss_newton.GaussNewtonTracker on the
scene of tests/test_gpu_track_and_map.py: what is checked there is behaviour -- the accepted loss never goes up, the pose stays a
rigid transform, the tracker meets that test's own criterion within an iteration budget -- and that an aborted asynchronous frame
is reported and changes nothing."""
import numpy as np
import pytest

import gn_restated as gn
from gsaj import synthetic as syn

pytestmark = pytest.mark.gpu

LM = dict(lambda_init=1e-3, nu=4.0, lambda_min=1e-7, lambda_max=1e7, converged_threshold=1e-4)
# Iteration budget of the behaviour test: twice the count at which the tracker first met the criterion when both trackers were
# measured in one run (tools/gn_tracker_bench.py -> profiles/r15_gn_tracker_bench.json; DESIGN.md "Gauss-Newton tracking"):
# GaussNewtonTracker GN_MEASURED iterations on the slowest of the three frames, DeviceTracker ADAM_MEASURED.
GN_MEASURED, ADAM_MEASURED = 5, 11
BUDGET = 2 * GN_MEASURED


def _step(lib, torch, rows, state, proj, skip=None):
    from gsaj import _lib
    _lib.check(lib.gsaj_pose_gn_step(rows.data_ptr(), rows.shape[0], LM["lambda_init"], LM["nu"], LM["lambda_min"], LM["lambda_max"],
                                     LM["converged_threshold"], proj.data_ptr(), state.data_ptr(), None if skip is None else skip.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "gsaj_pose_gn_step")


def _rows(rng, H, g, loss, n=5):
    """n partial rows whose sum is (H, g, loss, ...): random splits, so the slot-order fp64 sum has something to add up."""
    tot = np.zeros(32)
    tot[:21] = [H[k, l] for (k, l) in gn.SYM6]
    tot[21:27] = g
    tot[27:30] = [loss, 0.7 * loss, 0.3 * loss]
    parts = rng.dirichlet(np.ones(n), size=32).T * tot[None, :]
    return np.ascontiguousarray(parts, dtype=np.float32)   # (row-major: the transpose above is a column-major view)


def test_gn_step_accept_reject_accept_against_the_restatement_and_the_skip_word():
    import torch
    from gsaj import _lib

    lib, dev = _lib.load(), torch.device("cuda:0")
    rng = np.random.default_rng(4)
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=160, H=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    w2c0 = np.ascontiguousarray(cam["viewmatrix"].T).astype(np.float32)
    proj = torch.as_tensor(cam["projmatrix_raw"].reshape(4, 4), dtype=torch.float32, device=dev).contiguous()
    state = torch.zeros(lib.gsaj_gn_state_floats(), dtype=torch.float32, device=dev)
    state[0:16] = torch.as_tensor(w2c0.reshape(16), device=dev)
    want = gn.lm_new_state(w2c0, LM["lambda_init"])
    A = rng.normal(size=(40, 6))
    H = A.T @ A
    for call, loss in enumerate((1.0, 1.5, 0.5)):  # accept, reject, accept
        g = rng.normal(size=6) * 0.05
        rows = _rows(rng, H, g, loss)
        tot = rows.astype(np.float64).sum(axis=0)
        _step(lib, torch, torch.as_tensor(rows, device=dev), state, proj)
        gn.lm_step(want, gn.sym6(tot[:21]), tot[21:27], tot[27], LM["nu"], LM["lambda_min"], LM["lambda_max"], LM["converged_threshold"])
        gn.assert_lm_state_close(state.cpu().numpy(), want, cam["projmatrix_raw"], "call %d" % call)
        np.testing.assert_allclose(state[85:88].cpu().numpy(), tot[27:30], rtol=1e-6)
    assert (want["accepted"], want["rejected"]) == (2, 1)
    r = state[0:16].view(4, 4)[:3, :3].cpu().numpy().astype(np.float64)
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-5)
    # a non-zero skip word (aborted frame): not one float of the state changes
    before = state.clone()
    skip = torch.ones(1, dtype=torch.int32, device=dev)
    _step(lib, torch, torch.as_tensor(_rows(rng, H, rng.normal(size=6), 0.1), device=dev), state, proj, skip=skip)
    assert torch.equal(state, before)
    # a factorisation that meets a non-positive pivot: lambda goes up, the pose stays, nothing is reported converged
    bad = _rows(rng, -np.eye(6), rng.normal(size=6) * 0.05, 0.01)
    tot = bad.astype(np.float64).sum(axis=0)
    _step(lib, torch, torch.as_tensor(bad, device=dev), state, proj)
    pose_before = want["w2c"].copy()
    gn.lm_step(want, gn.sym6(tot[:21]), tot[21:27], tot[27], LM["nu"], LM["lambda_min"], LM["lambda_max"], LM["converged_threshold"])
    assert np.array_equal(want["w2c"], pose_before) and not want["converged"]
    gn.assert_lm_state_close(state.cpu().numpy(), want, cam["projmatrix_raw"], "non-positive pivot")
    with pytest.raises(Exception, match="nu > 1"):
        _lib.check(lib.gsaj_pose_gn_step(state.data_ptr(), 1, 1e-3, 1.0, 1e-7, 1e7, 1e-4, None, state.data_ptr(), None, None), "gsaj_pose_gn_step")


def _tracker(world, w2c, **kw):
    import gsaj
    from test_gpu_track_and_map import H, W

    dev, t, cams, sc, g, bg, M, frames = world
    return gsaj.GaussNewtonTracker(g["means3D"].shape[0], W, H, M, dev, w2c, t(cams[0]["projmatrix_raw"]), cams[0]["tanfovx"], cams[0]["tanfovy"],
                                   bg, alpha=0.9, sh_degree=3, **LM, **kw, **g)


def test_tracking_follows_the_camera_within_the_iteration_budget():
    """Every new frame starts from the previous estimate, as tests/test_gpu_track_and_map.py tracks it with DeviceTracker; the
    criterion is that test's: translation error below 0.35 x its starting value, rotation error below 0.02."""
    from test_gpu_track_and_map import _true_world

    assert 0 < BUDGET, "the budget is twice the measured count"
    world = _true_world()
    cams, frames = world[2], world[7]
    w2c_true = [np.ascontiguousarray(c["viewmatrix"].T) for c in cams]
    tr = _tracker(world, w2c_true[0])
    est = w2c_true[0].copy()
    for k in range(1, len(cams)):
        tr.set_frame(frames[k][0], frames[k][1], w2c=est)
        before = float(np.abs(est[:3, 3] - w2c_true[k][:3, 3]).max())
        accepted, met = [], None
        for it in range(1, BUDGET + 1):
            assert tr.iterate(1) == 1
            accepted.append(float(tr.lm["accepted_loss"]))
            pose = tr.accepted_w2c.cpu().numpy().astype(np.float64)
            assert np.allclose(pose[:3, :3] @ pose[:3, :3].T, np.eye(3), atol=1e-4), (k, it)   # the pose stays a rigid transform
            after = float(np.abs(pose[:3, 3] - w2c_true[k][:3, 3]).max())
            rot_err = float(np.abs(pose[:3, :3] @ w2c_true[k][:3, :3].T - np.eye(3)).max())
            if met is None and after < 0.35 * before and rot_err < 0.02:
                met = it
        assert all(b <= a for a, b in zip(accepted, accepted[1:])), (k, accepted)               # the accepted loss never goes up
        assert met is not None, (k, before, after, rot_err, accepted)
        assert float(tr.lm["accepted"]) + float(tr.lm["rejected"]) == BUDGET
        print("frame %d: criterion met after %d iterations (budget %d); accepted %d rejected %d, loss %.5f -> %.5f" % (
            k, met, BUDGET, int(tr.lm["accepted"]), int(tr.lm["rejected"]), accepted[0], accepted[-1]))
        est = tr.accepted_w2c.cpu().numpy().astype(np.float32)


def test_aborted_frame_is_reported_changes_nothing_and_the_next_call_recovers():
    """The arena is sized by a first view that sees nothing; the next frame's pose sees the whole map: the asynchronous forward is
    aborted on the device (the library's designed early return), every kernel of the iteration returns at once and the step, handed
    the abort word, leaves the state alone."""
    import torch
    from gsaj import _lib
    from test_gpu_track_and_map import _true_world

    world = _true_world(n_frames=2)
    cams, frames = world[2], world[7]
    w2c = np.ascontiguousarray(cams[1]["viewmatrix"].T).astype(np.float32)
    away = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ w2c).astype(np.float32)   # turned half round: nothing in front of the camera
    tr = _tracker(world, away)
    tr.ctx.auto_grow = False
    tr.set_frame(frames[1][0], frames[1][1])
    assert tr.iterate(1) == 1 and tr.ctx.true_R < 64 and 0 < tr.ctx.capacity < 2048
    tr.set_frame(frames[1][0], frames[1][1], w2c=np.ascontiguousarray(cams[0]["viewmatrix"].T))
    start = tr.state.clone()
    with pytest.raises(_lib.GsajError, match="aborted"):
        tr.iterate(3)
    assert torch.equal(tr.state, start), "an aborted frame's iterations change nothing"
    assert torch.equal(tr.w2c, tr.accepted_w2c) and float(tr.lm["accepted"]) == 0.0
    assert tr.iterate(2) == 2  # re-sized by a synchronous first iteration
    assert float(tr.lm["accepted"]) >= 1.0 and float(tr.loss_terms[0]) > 0.0
