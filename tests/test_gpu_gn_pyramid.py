"""GPU: gsaj.PyramidGaussNewtonTracker on the scene of tests/test_gpu_track_and_map.py (160x120, 3000 Gaussians) with levels=2 (80x60,
40x30).  levels=0 is GaussNewtonTracker bit for bit; from the nominal start the accepted loss never rises within a level, the pose
stays rigid and the criterion of tests/test_gpu_gn_tracker.py is met within the iteration budget; a frame aborted at a coarse level
is reported and changes nothing, and the next call recovers; monocular and masked frames reach the criterion too.
There is no wide-start test: the search it was to rest on (tests/test_cpu_pyramid.py, the premise tests) finds no start that the
single level misses and the pyramid meets -- the basin claim is not shown on this scene (DESIGN.md "Coarse-to-fine")."""
import numpy as np
import pytest

from test_gpu_gn_tracker import LM

pytestmark = pytest.mark.gpu

LEVELS = 2
# Iteration budgets, coarsest level first: twice the iteration WITHIN each level at which the accepted pose first met the criterion
# on the slowest of the three frames, every coarser level having run its own budget.  PYR_MEASURED is measured on the MI355X
# (tools/gn_tracker_bench.py --pyramid 2 -> profiles/r19_gn_pyramid_bench.json, "first_iteration_meeting_criterion_per_level").
PYR_MEASURED = (4, 1, 1)
BUDGET = tuple(2 * m for m in PYR_MEASURED)


def _pyramid_tracker(world, w2c, levels=LEVELS, **kw):
    import gsaj
    from test_gpu_track_and_map import F, H, W

    dev, t, cams, sc, g, bg, M, frames = world
    return gsaj.PyramidGaussNewtonTracker(g["means3D"].shape[0], W, H, M, dev, w2c, t(cams[0]["projmatrix_raw"]), cams[0]["tanfovx"], cams[0]["tanfovy"],
                                          bg, alpha=0.9, sh_degree=3, levels=levels, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5, **LM, **kw, **g)


def _errors(pose, true):
    pose = np.asarray(pose, np.float64)
    return float(np.abs(pose[:3, 3] - true[:3, 3]).max()), float(np.abs(pose[:3, :3] @ true[:3, :3].T - np.eye(3)).max())


@pytest.fixture(scope="module")
def world():
    from test_gpu_track_and_map import _true_world
    return _true_world()


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_levels_0_is_the_single_level_tracker_bit_for_bit(world, joint):
    import torch
    from test_gpu_gn_tracker import _tracker

    cams, frames = world[2], world[7]
    start = np.ascontiguousarray(cams[0]["viewmatrix"].T)
    one = _tracker(world, start, solve_exposure=joint)
    pyr = _pyramid_tracker(world, start, levels=0, solve_exposure=joint)
    assert torch.equal(pyr.state, one.state)
    for tr in (one, pyr):
        tr.set_frame(frames[1][0], frames[1][1], w2c=start)
    assert one.iterate(4) == 4 and pyr.iterate([4]) == [4]
    assert torch.equal(pyr.state, one.state) and float(one.lm["accepted"]) >= 1.0
    assert torch.equal(pyr.accepted_w2c, one.accepted_w2c) and torch.equal(pyr.accepted_exposure, one.accepted_exposure)


def _track_one_frame(tr, true, before, tag):
    """Level by level through BUDGET, one iteration per call -> (the iteration, counted over the frame, at which the criterion first
    held or None; the accepted losses per level)."""
    met, it, losses = None, 0, []
    for i, n in enumerate(BUDGET):
        hot = [0] * len(BUDGET)
        hot[i] = 1
        acc = []
        for _ in range(n):
            assert tr.iterate(hot) == hot
            it += 1
            acc.append(float(tr.lm["accepted_loss"]))
            pose = tr.accepted_w2c.cpu().numpy().astype(np.float64)
            assert np.allclose(pose[:3, :3] @ pose[:3, :3].T, np.eye(3), atol=1e-4), (tag, it)   # the pose stays a rigid transform
            te, re_ = _errors(pose, true)
            if met is None and te < 0.35 * before and re_ < 0.02:
                met = it
        # the accepted loss never goes up WITHIN a level (a relevel starts a new baseline: losses of two resolutions do not compare)
        assert all(b <= a for a, b in zip(acc, acc[1:])), (tag, LEVELS - i, acc)
        losses.append(acc)
    assert float(tr.lm["accepted"]) + float(tr.lm["rejected"]) == sum(BUDGET), "the counters count over the frame"
    return met, losses


def test_tracking_follows_the_camera_coarse_to_fine_within_the_budget(world):
    """Every new frame starts from the previous estimate, as tests/test_gpu_gn_tracker.py tracks it; the criterion is that test's:
    translation error below 0.35 x its starting value, rotation error below 0.02."""
    cams, frames = world[2], world[7]
    w2c_true = [np.ascontiguousarray(c["viewmatrix"].T) for c in cams]
    tr = _pyramid_tracker(world, w2c_true[0])
    assert [(t.ctx.W, t.ctx.H) for t in tr.trackers] == [(160, 120), (80, 60), (40, 30)]
    est = w2c_true[0].copy()
    for k in range(1, len(cams)):
        tr.set_frame(frames[k][0], frames[k][1], w2c=est)
        before = _errors(est, w2c_true[k])[0]
        met, losses = _track_one_frame(tr, w2c_true[k], before, "frame %d" % k)
        te, re_ = _errors(tr.accepted_w2c.cpu().numpy(), w2c_true[k])
        print("frame %d: criterion met after %s iterations (budget %r); error %.4f x the start's, accepted loss per level %s" % (
            k, met, BUDGET, te / before, [["%.5f" % x for x in a] for a in losses]))
        assert met is not None and te < 0.35 * before and re_ < 0.02, (k, met, te / before, re_, losses)
        est = tr.accepted_w2c.cpu().numpy().astype(np.float32)


def test_one_call_runs_the_whole_schedule_and_stops_a_level_on_convergence(world):
    cams, frames = world[2], world[7]
    start, true = np.ascontiguousarray(cams[0]["viewmatrix"].T), np.ascontiguousarray(cams[1]["viewmatrix"].T)
    tr = _pyramid_tracker(world, start)
    tr.set_frame(frames[1][0], frames[1][1], w2c=start)
    assert tr.iterate(BUDGET) == list(BUDGET) and tr.iterations == sum(BUDGET)
    before = _errors(start, true)[0]
    te, re_ = _errors(tr.accepted_w2c.cpu().numpy(), true)
    assert te < 0.35 * before and re_ < 0.02, (te / before, re_)
    assert float(tr.lm["accepted"]) + float(tr.lm["rejected"]) == sum(BUDGET)
    # a new frame without a new pose starts from the kept one, at the coarsest level again; check_every moves on once converged
    tr.set_frame(frames[1][0], frames[1][1])
    done = tr.iterate((40, 40, 40), check_every=2)
    assert all(0 < d <= 40 for d in done), done
    assert float(tr.converged) == 1.0 or done[-1] == 40, "a level that stopped early had converged"
    te2, re2 = _errors(tr.accepted_w2c.cpu().numpy(), true)
    assert te2 < 0.35 * before and re2 < 0.02, (te2 / before, re2)


def test_a_frame_aborted_at_a_coarse_level_is_reported_changes_nothing_and_the_next_call_recovers(world):
    """The construction of tests/test_gpu_gn_tracker.py's abort test, on every level: the arenas are sized by a view that sees nothing,
    the next frame's pose sees the whole map -- the asynchronous forwards are aborted on the device (the library's designed early
    return), the steps and the relevels, handed the abort word, leave the state alone."""
    import torch
    from gsaj import _lib

    cams, frames = world[2], world[7]
    w2c = np.ascontiguousarray(cams[1]["viewmatrix"].T).astype(np.float32)
    away = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ w2c).astype(np.float32)   # turned half round: nothing in front of the camera
    tr = _pyramid_tracker(world, away)
    for t in tr.trackers:
        t.ctx.auto_grow = False
    tr.set_frame(frames[1][0], frames[1][1])
    assert tr.iterate((1, 1, 1)) == [1, 1, 1] and all(t.ctx.true_R < 64 and 0 < t.ctx.capacity < 2048 for t in tr.trackers)
    tr.set_frame(frames[1][0], frames[1][1], w2c=np.ascontiguousarray(cams[0]["viewmatrix"].T))
    start = tr.state.clone()
    with pytest.raises(_lib.GsajError, match="level 2: .*aborted"):
        tr.iterate((3, 0, 0))
    assert torch.equal(tr.state, start), "an aborted frame's iterations change nothing"
    # the coarse level's abort word still stands: the relevel that would follow changes nothing either
    tr.relevel(1, skip=tr.trackers[2]._abort_ptr)
    assert torch.equal(tr.state, start)
    tr.relevel(2)
    with pytest.raises(_lib.GsajError, match="aborted"):
        tr.iterate((0, 2, 2))
    assert torch.equal(tr.w2c, tr.accepted_w2c) and float(tr.lm["accepted"]) == 0.0
    assert tr.iterate((2, 2, 2)) == [2, 2, 2]   # every level re-sized by a synchronous first iteration
    assert float(tr.lm["accepted"]) >= 3.0 and float(tr.loss_terms[0]) > 0.0


@pytest.mark.parametrize("kind", ["monocular", "masked"])
def test_monocular_and_masked_frames_reach_the_criterion(world, kind):
    cams, frames = world[2], world[7]
    start, true = np.ascontiguousarray(cams[0]["viewmatrix"].T), np.ascontiguousarray(cams[1]["viewmatrix"].T)
    if kind == "monocular":
        tr = _pyramid_tracker(world, start, monocular=True)
        tr.set_frame(frames[1][0], w2c=start)
        assert tr.pyramid.has_depth is False and all(t.gt_depth is None for t in tr.trackers)
    else:
        tr = _pyramid_tracker(world, start)
        tr.set_frame(frames[1][0], frames[1][1], w2c=start, edge_threshold=1.1)
        sizes = [int(t.grad_mask.numel()) for t in tr.trackers]
        assert sizes == [160 * 120, 80 * 60, 40 * 30] and tr.pyramid.has_mask is False
        assert all(0 < int(t.grad_mask.sum()) < t.grad_mask.numel() for t in tr.trackers), "every level has its own mask, at its scale"
    assert tr.iterate(BUDGET) == list(BUDGET)
    before = _errors(start, true)[0]
    te, re_ = _errors(tr.accepted_w2c.cpu().numpy(), true)
    assert te < 0.35 * before and re_ < 0.02, (kind, te / before, re_)
