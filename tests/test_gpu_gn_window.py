"""GPU: K Levenberg-Marquardt steps in one launch (gsaj_pose_gn_step_batch / gsaj_pose_gn8_step_batch) against the restatement and,
bit for bit, against the single-view step; gsaj_pose_gn_select; and GaussNewtonWindow on the world of tests/test_gpu_track_and_map.py
-- the keyframe-window use (three frames in three slots) and the multi-start use (one frame, three start poses).  What is checked of
the window is behaviour, with the criteria and the iteration budget of tests/test_gpu_gn8_tracker.py: each view's arithmetic is the
single tracker's, so its measured count applies.  No timing is asserted."""
import inspect
import math

import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import gn_window_restated as gw
from gsaj import synthetic as syn
from test_gpu_gn8_tracker import A_STAR, B_STAR, BUDGET, _rows8
from test_gpu_gn_tracker import BUDGET as BUDGET6
from test_gpu_gn_tracker import LM, _rows

pytestmark = pytest.mark.gpu

K = gw.K
N_ROWS = 37   # partial rows per view: more than the sum has row groups


def _lm_args():
    return LM["lambda_init"], LM["nu"], LM["lambda_min"], LM["lambda_max"], LM["converged_threshold"]


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_batched_step_against_the_restatement_and_the_single_view_step_bit_for_bit(joint):
    """accept / reject / accept, differently per view; a non-positive pivot in one view only; active = (1, 0, 1); a skip word on one
    view.  After every call the whole [K, state] tensor equals K single-view steps on the same rows and states (views that are inactive
    or skipped are not stepped there, so they must be untouched bit for bit) and every view is close to lm_step / lm8_step."""
    import torch
    from gsaj import _lib

    lib, dev = _lib.load(), torch.device("cuda:0")
    rng = np.random.default_rng(4)
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=160, H=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    proj = torch.as_tensor(cam["projmatrix_raw"].reshape(4, 4), dtype=torch.float32, device=dev).contiguous()
    n, nx = (152, 8) if joint else (136, 6)
    assert (lib.gsaj_gn8_state_floats() if joint else lib.gsaj_gn_state_floats()) == n
    batch_fn, one_fn = (lib.gsaj_pose_gn8_step_batch, lib.gsaj_pose_gn8_step) if joint else (lib.gsaj_pose_gn_step_batch, lib.gsaj_pose_gn_step)
    w2c0 = np.ascontiguousarray(cam["viewmatrix"].T).astype(np.float64)
    starts = [(gn.se3_exp(tau) @ w2c0).astype(np.float32) for tau in gw.INCREMENTS]
    states = torch.zeros((K, n), device=dev)
    want = []
    for v in range(K):
        states[v, 0:16] = torch.as_tensor(starts[v].reshape(16), device=dev)
        states[v, 33:35] = torch.as_tensor(np.asarray(gw.EXPOSURES[v], np.float32), device=dev)
        want.append(g8.lm8_new_state(starts[v], LM["lambda_init"], exposure=gw.EXPOSURES[v]) if joint else gn.lm_new_state(starts[v], LM["lambda_init"]))
    single = states.clone()
    Hs = []
    for v in range(K):
        A = rng.normal(size=(50, nx))
        Hs.append(A.T @ A)
    calls = [  # (losses, the view whose H has a non-positive pivot, active, skip words)
        ((1.0, 1.1, 1.2), None, None, None),            # accept, accept, accept
        ((1.5, 0.9, 1.6), None, None, None),            # reject, accept, reject
        ((0.5, 0.4, 0.6), None, None, None),            # accept, accept, accept
        ((0.3, 0.01, 0.35), 1, None, None),             # view 1 only: no factorisation
        ((0.2, 0.2, 0.2), None, (1, 0, 1), None),       # view 1 inactive
        ((0.1, 0.1, 0.1), None, None, (0, 0, 1)),       # view 2's frame was aborted
        ((0.05, 0.3, 0.05), None, (1, 1, 0), (1, 0, 0)),  # both at once: only view 1 is stepped (a reject)
    ]
    stream = torch.cuda.current_stream().cuda_stream
    for c, (losses, pivot, active, skip) in enumerate(calls):
        rows, sums = [], []
        for v in range(K):
            H = -np.eye(nx) if pivot == v else Hs[v]
            g = rng.normal(size=nx) * 0.05
            r = (_rows8 if joint else _rows)(rng, H, g, losses[v], n=N_ROWS)
            tot = r.astype(np.float64).sum(axis=0)
            sums.append((g8.sym8(tot[:36]), tot[36:44], tot[44]) if joint else (gn.sym6(tot[:21]), tot[21:27], tot[27]))
            rows.append(r)
        rows_t = torch.as_tensor(np.stack(rows), device=dev)
        act_t = None if active is None else torch.as_tensor(np.asarray(active, np.uint8), device=dev)
        skip_t = None if skip is None else torch.as_tensor(np.asarray(skip, np.int32) * 7, device=dev)   # (any non-zero word counts)
        before = states.clone()
        _lib.check(batch_fn(K, rows_t.data_ptr(), N_ROWS, None if act_t is None else act_t.data_ptr(), *_lm_args(), proj.data_ptr(),
                            states.data_ptr(), None if skip_t is None else skip_t.data_ptr(), 4, stream), "batched step")
        for v in range(K):
            if (active is not None and not active[v]) or (skip is not None and skip[v]):
                assert torch.equal(states[v], before[v]), "call %d: view %d is inactive or skipped and must be untouched" % (c, v)
                continue
            _lib.check(one_fn(rows_t[v].data_ptr(), N_ROWS, *_lm_args(), proj.data_ptr(), single[v].data_ptr(), None, stream), "single step")
        assert torch.equal(states, single), "call %d: the batched step differs from the single-view step" % c
        gw.window_step(want, sums, joint, LM, active=active, skip=skip)
        host = states.cpu().numpy()
        for v in range(K):
            (g8.assert_lm8_state_close if joint else gn.assert_lm_state_close)(host[v], want[v], cam["projmatrix_raw"], "call %d view %d" % (c, v))
        if pivot is not None:
            assert torch.equal(states[pivot, 0:16], before[pivot, 0:16]) and float(states[pivot, 77]) == 0.0
            assert all(not torch.equal(states[v, 0:16], before[v, 0:16]) for v in range(K) if v != pivot)
    assert [(w["accepted"], w["rejected"]) for w in want] == [(5, 1), (4, 2), (4, 1)], [(w["accepted"], w["rejected"]) for w in want]
    with pytest.raises(Exception, match="nu > 1"):
        _lib.check(batch_fn(K, states.data_ptr(), 1, None, 1e-3, 1.0, 1e-7, 1e7, 1e-4, None, states.data_ptr(), None, 0, None), "batched step")
    with pytest.raises(Exception, match="K > 0"):
        _lib.check(batch_fn(0, states.data_ptr(), 1, None, *_lm_args(), None, states.data_ptr(), None, 0, None), "batched step")


@pytest.mark.parametrize("n", [136, 152])
def test_select_against_the_restatement(n):
    import torch
    from gsaj import _lib

    lib, dev = _lib.load(), torch.device("cuda:0")
    inf, nan = float("inf"), float("nan")
    big = [1.0 + 0.01 * k for k in range(70)]
    big[66] = big[67] = 0.25          # beyond one wave's first pass, and a tie there
    cases = [
        ([0.5, 0.2, 0.3], [1, 1, 1], None),
        ([0.5, 0.2, 0.3], [1, 1, 1], [1, 0, 1]),        # an inactive view, which has the smallest loss
        ([0.3, 0.3, 0.3], [1, 1, 1], None),             # a tie: the lowest index
        ([0.5, 0.3, 0.3], [1, 1, 1], [1, 1, 1]),
        ([nan, 0.4, inf], [1, 1, 1], None),             # a NaN and an infinite loss
        ([-inf, 0.4, 0.2], [1, 1, 1], None),
        ([0.1, 0.4, 0.2], [0, 1, 1], None),             # a view without an accepted pose
        ([0.1, 0.4, 0.2], [0, 0, 0], None),             # none eligible
        ([nan, 0.4, 0.2], [1, 1, 1], [1, 0, 0]),
        ([0.7], [1], None),
        (big, [1] * 70, None),
        (big, [1] * 70, [0 if k == 66 else 1 for k in range(70)]),
    ]
    out = torch.zeros(2, dtype=torch.int32, device=dev)
    for losses, has, active in cases:
        k = len(losses)
        s = torch.zeros((k, n), device=dev)
        s[:, 81] = torch.as_tensor(np.asarray(losses, np.float32), device=dev)
        s[:, 82] = torch.as_tensor(np.asarray(has, np.float32), device=dev)
        act = None if active is None else torch.as_tensor(np.asarray(active, np.uint8), device=dev)
        out.fill_(-5)
        _lib.check(lib.gsaj_pose_gn_select(k, s.data_ptr(), n, None if act is None else act.data_ptr(), out.data_ptr(), out.data_ptr() + 4,
                                           torch.cuda.current_stream().cuda_stream), "gsaj_pose_gn_select")
        h = out.cpu()
        got = (int(h[0]), float(h[1:2].view(torch.float32)[0]))
        want = gw.select(losses, has, active)
        assert got == want, (losses[:4], has[:4], active, got, want)
        if active is not None and gw.select(losses, has, active, mutant="select_ignores_active") != want:
            assert got != gw.select(losses, has, active, mutant="select_ignores_active")


def _window(world, w2cs, **kw):
    import gsaj
    from test_gpu_track_and_map import H, W

    dev, t, cams, sc, g, bg, M, frames = world
    return gsaj.GaussNewtonWindow(len(w2cs), g["means3D"].shape[0], W, H, M, dev, np.stack(w2cs), t(cams[0]["projmatrix_raw"]), cams[0]["tanfovx"],
                                  cams[0]["tanfovy"], bg, alpha=0.9, sh_degree=3, **LM, **kw, **g)


def _exposed(frame):
    return math.exp(A_STAR) * frame[0] + B_STAR, frame[1]


@pytest.fixture(scope="module")
def world():
    from test_gpu_track_and_map import _true_world
    return _true_world()


@pytest.mark.parametrize("joint", [True, False], ids=["joint", "6-form"])
def test_window_every_slot_meets_the_single_trackers_criteria_within_its_budget(world, joint):
    """The three frames are the three slots; each slot starts from the previous frame's true pose (and exposure (0, 0)).  Joint
    form, on ground truth exposed by (a*, b*): translation error below 0.35 x its starting value, rotation error below 0.02 and
    max(|a - a*|, |b - b*|) below 0.35 x its starting value within BUDGET = 2 x GN8_MEASURED iterations.  6-form, on the plain
    frames: the pose criteria within the budget of tests/test_gpu_gn_tracker.py."""
    import torch

    cams, frames = world[2], world[7]
    w2c_true = [np.ascontiguousarray(c["viewmatrix"].T) for c in cams]
    assert len(cams) == K + 1
    budget = BUDGET if joint else BUDGET6
    assert budget == (8 if joint else 10)
    win = _window(world, w2c_true[:K], solve_exposure=joint)
    for k in range(K):
        gt = _exposed(frames[k + 1]) if joint else frames[k + 1]
        win.set_view(k, gt[0], gt[1])
    before = [float(np.abs(w2c_true[k][:3, 3] - w2c_true[k + 1][:3, 3]).max()) for k in range(K)]
    e0 = max(abs(A_STAR), abs(B_STAR))
    accepted, met, last = [[] for _ in range(K)], [None] * K, [None] * K
    for it in range(1, budget + 1):
        assert win.iterate(1) == 1
        acc_loss = win.lm["accepted_loss"].cpu().numpy()
        poses = win.accepted_w2c.cpu().numpy().astype(np.float64)
        exps = win.accepted_exposure.cpu().numpy().astype(np.float64)
        for k in range(K):
            accepted[k].append(float(acc_loss[k]))
            assert np.allclose(poses[k][:3, :3] @ poses[k][:3, :3].T, np.eye(3), atol=1e-4), (k, it)   # the pose stays a rigid transform
            after, rot_err = g8.pose_errors(poses[k], w2c_true[k + 1])
            exp_err = float(np.abs(exps[k] - [A_STAR, B_STAR]).max()) if joint else 0.0
            last[k] = (after / before[k], rot_err, exp_err / e0)
            if met[k] is None and after < 0.35 * before[k] and rot_err < 0.02 and exp_err < 0.35 * e0:
                met[k] = it
    lm = win.lm
    for k in range(K):
        print("%s slot %d: criteria met after %s iterations (budget %d); accepted %d rejected %d, loss %.5f -> %.5f; translation %.4f x start, "
              "rotation %.5f, exposure %.4f x start" % ("joint" if joint else "6-form", k, met[k], budget, int(lm["accepted"][k]), int(lm["rejected"][k]),
                                                         accepted[k][0], accepted[k][-1], *last[k]))
        assert all(b <= a for a, b in zip(accepted[k], accepted[k][1:])), (k, accepted[k])          # the accepted loss never goes up
        assert met[k] is not None, (k, last[k], accepted[k])
        assert float(lm["accepted"][k]) + float(lm["rejected"][k]) == budget
    m = 8 if joint else 6
    assert tuple(lm["H"].shape) == (K, m, m) and tuple(win.loss_terms.shape) == (K, 3) and bool((win.loss_terms[:, 0] > 0).all())
    if not joint:
        assert not win.state[:, 33:35].any() and torch.equal(win.accepted_exposure, win.state[:, 33:35])
    # an inactive slot is rendered but not stepped
    win.active[1] = 0
    held = win.state.clone()
    assert win.iterate(2) == 2
    assert torch.equal(win.state[1], held[1]) and not torch.equal(win.state[0], held[0])


def test_multi_start_best_is_the_host_argmin_and_meets_the_pose_criterion(world):
    """One (exposed) frame, K = 3 starts: the previous frame's true pose, and that pose moved by +-5 x the frame-to-frame translation
    along x.  best() is the argmin recomputed on the host from the states, and the chosen hypothesis meets the pose criterion --
    measured, as the other two are, against the nominal start's error."""
    cams, frames = world[2], world[7]
    w2c_true = [np.ascontiguousarray(c["viewmatrix"].T).astype(np.float64) for c in cams]
    step = float(np.abs(w2c_true[1][:3, 3] - w2c_true[0][:3, 3]).max())
    starts = []
    for s in (0.0, 5.0, -5.0):
        w = w2c_true[0].copy()
        w[0, 3] += s * step
        starts.append(w)
    win = _window(world, starts, solve_exposure=True)
    assert win.best() == (-1, float("inf")), "before any iteration no hypothesis has an accepted pose"
    gt = _exposed(frames[1])
    win.set_frame(gt[0], gt[1], w2cs=np.stack(starts))
    assert win.iterate(BUDGET) == BUDGET
    best, loss = win.best()
    s = win.state.cpu().numpy()
    assert (best, loss) == gw.select(s[:, 81], s[:, 82] != 0, None) and best == int(np.argmin(s[:, 81])) and loss == float(s[best, 81])
    before = g8.pose_errors(starts[0], w2c_true[1])[0]
    errs = [g8.pose_errors(win.accepted_w2c[k].cpu().numpy(), w2c_true[1]) for k in range(K)]
    print("multi-start: accepted losses %s, translation errors x the nominal start's %s -> hypothesis %d" % (
        ["%.5f" % x for x in s[:, 81]], ["%.3f" % (e[0] / before) for e in errs], best))
    assert errs[best][0] < 0.35 * before and errs[best][1] < 0.02, (best, errs, before)
    # the mask enters the choice
    win.active[best] = 0
    other, _ = win.best()
    assert other != best and other == gw.select(s[:, 81], s[:, 82] != 0, win.active.cpu().numpy())[0]


def test_the_single_view_path_is_imported_untouched():
    import gsaj
    from gsaj import gauss_newton as G

    assert gsaj.GaussNewtonTracker is G.GaussNewtonTracker and gsaj.GaussNewtonWindow is G.GaussNewtonWindow
    assert not issubclass(G.GaussNewtonWindow, G.GaussNewtonTracker) and not issubclass(G.GaussNewtonTracker, G.GaussNewtonWindow)
    one, win = inspect.signature(G.GaussNewtonTracker.__init__).parameters, inspect.signature(G.GaussNewtonWindow.__init__).parameters
    assert list(one)[:7] == ["self", "P", "W", "H", "M", "device", "w2c"] and list(win)[:8] == ["self", "K", "P", "W", "H", "M", "device", "w2cs"]
    assert [p for p in one if p not in ("w2c",)] == [p for p in win if p not in ("K", "w2cs", "streams")], "the window takes the tracker's arguments"
    for p in one:
        if p not in ("self", "w2c") and one[p].default is not inspect.Parameter.empty:
            assert win[p].default == one[p].default, p
