#!/usr/bin/env python3
"""Second-order against first-order tracking (gsaj.gauss_newton.GaussNewtonTracker against gsaj.tracking.DeviceTracker, whose code
this change leaves as it is): ms per iteration (device events, median of `repeats` windows after a warm-up) and the iteration --
and the time -- at which each first meets tests/test_gpu_track_and_map.py's criterion (translation error below 0.35 x its starting
value and rotation error below 0.02), on that test's 160x120 scene (three consecutive frames, each started from the previous
frame's true pose) and on the cfg2 frame (640x480, 50 000 Gaussians, started 1.2 cm / 0.3 degrees off).

Finding the first iteration that meets the criterion reads the pose back after every iteration; the timings are taken in separate,
unobserved windows.  usage: gn_tracker_bench.py [--solve-exposure] [out.json] [window=50] [repeats=7]

--solve-exposure: every ground-truth frame is turned into e^a* C + b* with (a*, b*) = EXPOSURE and every tracker starts from exposure
(0, 0).  A third tracker joins the two, GaussNewtonTracker(solve_exposure=True); its criterion is the pose criterion AND max(|a - a*|,
|b - b*|) below 0.35 x its starting value.  The other two keep the pose criterion; the exposure error each ends with is reported.

--window K: another measurement altogether -- one GaussNewtonWindow iteration of K views (every kernel once, gridDim.y = K) against K
sequential GaussNewtonTracker iterations (K trackers, each with its own context, one after the other on the same stream), 6-form and
joint form, on both scenes: ms per window iteration and per view, the ratio, and whether the window is slower than the sequential
loop beyond the latter's own min-max spread.  Every slot holds the same frame from the same start, so that both sides do the same
work.  usage: gn_tracker_bench.py --window K [out.json] [window=50] [repeats=7]

--pyramid L [--schedule a,b,..]: coarse to fine -- gsaj.PyramidGaussNewtonTracker with L levels against GaussNewtonTracker, same frame,
same start, on both scenes, from the nominal start and from a wide one (the previous true pose moved by WIDE_START x the frame-to-frame
translation along x).  Observed run (the pose read back after every iteration): the error trace of both, the pyramid's through the
iteration budget of every level (--schedule, coarsest first; default 8 per level), the iteration within each level at which the criterion first
held, and the iterations each needs to bring the translation error to 1 % and to 5e-5 of its starting value.  Timed runs (unobserved):
device events around WHOLE frames -- set_frame, which builds the pyramid, and the iterations with their relevels --, median of
`repeats` after a warm-up, the two trackers alternated.  And k_pyramid alone at 640x480 and 1280x720, L = 3: time per launch over a
window of launches against the bytes it must move.  usage: gn_tracker_bench.py --pyramid L [--schedule a,b,c] [out.json] [window=50]
[repeats=7]"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"))
import torch  # noqa: E402
from gsaj import synthetic as syn  # noqa: E402
from gsaj.gauss_newton import GaussNewtonTracker, GaussNewtonWindow, PyramidGaussNewtonTracker  # noqa: E402
from gsaj.pyramid import ImagePyramid  # noqa: E402
from gsaj.rasterizer import FrameContext  # noqa: E402
from gsaj.tracking import DeviceTracker  # noqa: E402

DEV = torch.device("cuda:0")
T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)  # noqa: E731
ADAM = dict(lr_rot=0.003, lr_trans=0.002)   # the learning rates of tests/test_gpu_track_and_map.py
EXPOSURE = (0.2, -0.05)                      # --solve-exposure: (a*, b*) of the ground-truth frames
WIDE_START = 5.0                             # --pyramid: the wide start, in frame-to-frame translations along x
MARKS = (("1e-2", 1e-2), ("5e-5", 5e-5))     # --pyramid: the translation error, over its starting value, the time is taken to


def errors(w2c, true):
    w2c = np.asarray(w2c, np.float64)
    return float(np.abs(w2c[:3, 3] - true[:3, 3]).max()), float(np.abs(w2c[:3, :3] @ true[:3, :3].T - np.eye(3)).max())


def exposure_error(e, exposure):
    return float(np.abs(np.asarray(e, np.float64).reshape(2) - np.asarray(exposure)).max())


def first_hit(tr, pose, true, before, budget, exposure=None, exposure_of=None):
    """The iteration at which the criterion first holds for `pose()` (None: not within the budget), the trace of the translation
    error over its starting value through the whole budget, and the rotation error at its end.  exposure_of (with exposure = (a*, b*)):
    the criterion also asks for the exposure error of `exposure_of()` below 0.35 x its starting value, max(|a*|, |b*|)."""
    trace, hit, rot = [], None, 0.0
    for it in range(1, budget + 1):
        tr.iterate(1)
        after, rot = errors(pose().cpu().numpy(), true)
        trace.append(round(after / before, 4))
        ok = exposure_of is None or exposure_error(exposure_of().cpu().numpy(), exposure) < 0.35 * max(abs(exposure[0]), abs(exposure[1]))
        if hit is None and after < 0.35 * before and rot < 0.02 and ok:
            hit = it
    return hit, trace, rot


def ms_per_iteration(tr, reset, window, repeats):
    reset()
    tr.iterate(10)  # warm-up: code objects, the arena
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(repeats):
        reset()
        tr.iterate(1)
        ev[0].record()
        tr.iterate(window)
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) / window)
    return float(np.median(out)), float(min(out)), float(max(out))


def case(name, cam_true, w2c_start, sc, gt, window, repeats, budgets=(100, 30), gn_kw=None, exposure=None):
    P, W, H, M = sc["means3D"].shape[0], cam_true["W"], cam_true["H"], sc["shs"].shape[1]
    g = dict(means3D=T(sc["means3D"]), opacities=T(sc["opacities"]), shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]),
             sh_degree=3)
    bg = torch.zeros(3, device=DEV)
    true = np.ascontiguousarray(cam_true["viewmatrix"].T).astype(np.float64)
    before = errors(w2c_start, true)[0]
    args = (P, W, H, M, DEV, w2c_start, T(cam_true["projmatrix_raw"]), cam_true["tanfovx"], cam_true["tanfovy"], bg)
    adam = DeviceTracker(*args, alpha=0.9, **ADAM, **g)
    gnt = GaussNewtonTracker(*args, alpha=0.9, **(gn_kw or {}), **g)
    out = dict(workload=name, P=P, W=W, H=H, start_translation_error=before)
    trackers = [("adam", adam, lambda: adam.w2c, budgets[0], None), ("gauss_newton", gnt, lambda: gnt.accepted_w2c, budgets[1], None)]
    if exposure is not None:
        gt = (math.exp(exposure[0]) * gt[0] + exposure[1], gt[1])
        gn8 = GaussNewtonTracker(*args, alpha=0.9, solve_exposure=True, **(gn_kw or {}), **g)
        trackers.append(("gauss_newton_joint", gn8, lambda: gn8.accepted_w2c, budgets[1], lambda: gn8.accepted_exposure))
        out["exposure"] = list(exposure)
    for key, tr, pose, budget, exposure_of in trackers:
        reset = lambda tr=tr: tr.set_frame(gt[0], gt[1], w2c=w2c_start)  # noqa: E731
        reset()
        hit, trace, rot = first_hit(tr, pose, true, before, budget, exposure, exposure_of)
        lm = {k: float(v) for k, v in tr.lm.items() if k in ("lam", "accepted", "rejected")} if key != "adam" else {}
        if exposure is not None:   # what each tracker's exposure ends at (the 6-form's never moves)
            src = getattr(tr, "pose", tr)   # (DeviceTracker keeps its exposure in its PoseTracker)
            e = exposure_of() if exposure_of else torch.cat([src.exposure_a.reshape(1), src.exposure_b.reshape(1)])
            lm["exposure_error_at_budget"] = round(exposure_error(e.cpu().numpy(), exposure), 6)
        med, lo, hi = ms_per_iteration(tr, reset, window, repeats)
        out[key] = dict(iterations_to_criterion=hit, ms_per_iteration=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                        ms_to_criterion=None if hit is None else round(hit * med, 3), budget=budget, error_ratio_at_budget=trace[-1],
                        lowest_error_ratio=min(trace), rotation_error_at_budget=round(rot, 6), error_ratio_trace=trace)
        out[key].update(lm)   # (the damping and the counters at the end of the budget)
    return out


class Sequential:
    """K single trackers run one after the other, each for n iterations: what a caller without the window does (one blocking status
    read per tracker and call, as one per call of the window)."""

    def __init__(self, trackers):
        self.trackers = trackers

    def iterate(self, n):
        for tr in self.trackers:
            tr.iterate(n)


def window_case(name, K, cam_true, w2c_start, sc, gt, window, repeats):
    P, W, H, M = sc["means3D"].shape[0], cam_true["W"], cam_true["H"], sc["shs"].shape[1]
    g = dict(means3D=T(sc["means3D"]), opacities=T(sc["opacities"]), shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]),
             sh_degree=3)
    bg = torch.zeros(3, device=DEV)
    tail = (T(cam_true["projmatrix_raw"]), cam_true["tanfovx"], cam_true["tanfovy"], bg)
    out = dict(workload=name, K=K, P=P, W=W, H=H)
    for key, joint in (("6-form", False), ("joint", True)):
        frame = (math.exp(EXPOSURE[0]) * gt[0] + EXPOSURE[1], gt[1]) if joint else gt
        win = GaussNewtonWindow(K, P, W, H, M, DEV, np.stack([w2c_start] * K), *tail, alpha=0.9, solve_exposure=joint, **g)
        seq = Sequential([GaussNewtonTracker(P, W, H, M, DEV, w2c_start, *tail, alpha=0.9, solve_exposure=joint, **g) for _ in range(K)])

        def reset_seq():
            for tr in seq.trackers:
                tr.set_frame(frame[0], frame[1], w2c=w2c_start)

        w = ms_per_iteration(win, lambda: win.set_frame(frame[0], frame[1], w2cs=np.stack([w2c_start] * K)), window, repeats)
        q = ms_per_iteration(seq, reset_seq, window, repeats)
        # the same work must come out: every slot's accepted loss against the single trackers' after the same number of iterations
        acc_w, acc_s = win.lm["accepted_loss"].cpu().numpy(), np.array([float(tr.lm["accepted_loss"]) for tr in seq.trackers])
        out[key] = dict(window_ms_per_iteration=round(w[0], 4), window_ms_min=round(w[1], 4), window_ms_max=round(w[2], 4),
                        sequential_ms_per_iteration=round(q[0], 4), sequential_ms_min=round(q[1], 4), sequential_ms_max=round(q[2], 4),
                        window_ms_per_view=round(w[0] / K, 4), sequential_ms_per_view=round(q[0] / K, 4), speedup=round(q[0] / w[0], 3),
                        slower_beyond_spread=bool(w[0] > q[0] + (q[2] - q[1])),
                        accepted_loss_window=[float(x) for x in acc_w], accepted_loss_sequential=[float(x) for x in acc_s])
    return out


def _frame_ms(run, repeats):
    """Median (min, max) ms of run() -- one whole frame -- between device events."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(repeats):
        ev[0].record()
        run()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return [round(float(np.median(out)), 4), round(float(min(out)), 4), round(float(max(out)), 4)]


def _prefix(per_level, total):
    """The first `total` iterations of a level-by-level run as a schedule: per_level [(level, n)], coarsest first."""
    out = []
    for _, n in per_level:
        out.append(min(n, total))
        total -= out[-1]
    return out


def pyramid_case(name, L, budgets, cam, w2c_start, sc, gt, repeats, single_budget=30):
    P, W, H, M = sc["means3D"].shape[0], cam["W"], cam["H"], sc["shs"].shape[1]
    g = dict(means3D=T(sc["means3D"]), opacities=T(sc["opacities"]), shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]),
             sh_degree=3)
    bg = torch.zeros(3, device=DEV)
    true = np.ascontiguousarray(cam["viewmatrix"].T).astype(np.float64)
    before = errors(w2c_start, true)[0]
    args = (P, W, H, M, DEV, w2c_start, T(cam["projmatrix_raw"]), cam["tanfovx"], cam["tanfovy"], bg)
    one = GaussNewtonTracker(*args, alpha=0.9, **g)
    pyr = PyramidGaussNewtonTracker(*args, alpha=0.9, levels=L, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], **g)
    out = dict(workload=name, P=P, W=W, H=H, levels=L, start_translation_error=before)
    # observed: the single-level tracker
    one.set_frame(gt[0], gt[1], w2c=w2c_start)
    hit, trace, rot = first_hit(one, lambda: one.accepted_w2c, true, before, single_budget)
    s = dict(iterations_to_criterion=hit, error_ratio_trace=trace, rotation_error_at_budget=round(rot, 6), accepted_loss=float(one.lm["accepted_loss"]))
    # observed: the pyramid, every level through its budget
    pyr.set_frame(gt[0], gt[1], w2c=w2c_start)
    ptrace, hits, per_level = [], {}, []
    for i, (l, n) in enumerate(zip(range(L, -1, -1), budgets)):
        hot = [0] * (L + 1)
        hot[i] = 1
        for it in range(1, n + 1):
            pyr.iterate(hot)
            after, rot = errors(pyr.accepted_w2c.cpu().numpy(), true)
            ptrace.append(round(after / before, 6))
            if l not in hits and after < 0.35 * before and rot < 0.02:
                hits[l] = it
        per_level.append((l, n))
    q = dict(budgets=list(budgets), first_iteration_meeting_criterion_per_level={str(l): hits.get(l) for l, _ in per_level}, error_ratio_trace=ptrace,
             rotation_error_at_budget=round(rot, 6), accepted_loss=float(pyr.lm["accepted_loss"]),
             accepted=float(pyr.lm["accepted"]), rejected=float(pyr.lm["rejected"]))
    # timed: whole frames up to each mark, the two trackers alternated
    for key, mark in MARKS:
        n_one = next((i + 1 for i, r in enumerate(trace) if r <= mark), None)
        n_pyr = next((i + 1 for i, r in enumerate(ptrace) if r <= mark), None)
        sched = None if n_pyr is None else _prefix(per_level, n_pyr)

        def run_one():
            one.set_frame(gt[0], gt[1], w2c=w2c_start)
            one.iterate(n_one)

        def run_pyr():
            pyr.set_frame(gt[0], gt[1], w2c=w2c_start)
            pyr.iterate(sched)

        for fn, ok in ((run_one, n_one), (run_pyr, n_pyr)):   # warm-up
            if ok is not None:
                fn()
        t_one, t_pyr = [], []
        for _ in range(repeats):   # alternated: one frame of each, median over the repeats
            if n_one is not None:
                t_one.append(_frame_ms(run_one, 1)[0])
            if n_pyr is not None:
                t_pyr.append(_frame_ms(run_pyr, 1)[0])
        f = lambda v: None if not v else [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]  # noqa: E731
        s["to_" + key] = dict(iterations=n_one, frame_ms_median_min_max=f(t_one))
        q["to_" + key] = dict(iterations_per_level=sched, frame_ms_median_min_max=f(t_pyr))
    # timed: one iteration of every level alone (the tool's ms_per_iteration protocol), level 0 being the single-level tracker's
    def at_level(l):
        pyr.set_frame(gt[0], gt[1], w2c=w2c_start)
        pyr.relevel(l)

    q["ms_per_iteration_per_level"] = {str(l): [round(x, 4) for x in ms_per_iteration(pyr.trackers[l], lambda l=l: at_level(l), 50, repeats)]
                                       for l in range(L, -1, -1)}
    s["ms_per_iteration"] = [round(x, 4) for x in ms_per_iteration(one, lambda: one.set_frame(gt[0], gt[1], w2c=w2c_start), 50, repeats)]
    out["gauss_newton"], out["pyramid"] = s, q
    return out


def pyramid_kernel_case(W, H, L, window, repeats):
    rng = np.random.default_rng(0)
    color, depth = T(rng.random((3, H, W), dtype=np.float32)), T(1.0 + rng.random((H, W), dtype=np.float32))
    mask = torch.as_tensor((rng.random((H, W)) < 0.3).astype(np.uint8), device=DEV)
    pyr = ImagePyramid(W, H, L, DEV, has_depth=True, has_mask=True)
    for _ in range(10):
        pyr.build(color, depth, mask)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(repeats):
        ev[0].record()
        for _ in range(window):
            pyr.build(color, depth, mask)
        ev[1].record()
        torch.cuda.synchronize()
        out.append(1e3 * ev[0].elapsed_time(ev[1]) / window)
    read = (12 + 4 + 1) * W * H
    written = sum(17 * (W >> l) * (H >> l) for l in range(1, L + 1))
    us = float(np.median(out))
    return dict(W=W, H=H, levels=L, us_per_launch=round(us, 3), us_min=round(min(out), 3), us_max=round(max(out), 3), bytes_read=read,
                bytes_written=written, gb_per_s=round((read + written) / us * 1e-3, 1))


def pyramid_main(L, argv):
    budgets = [8] * (L + 1)
    if "--schedule" in argv:
        i = argv.index("--schedule")
        budgets = [int(x) for x in argv[i + 1].split(",")]
        argv = argv[:i] + argv[i + 2:]
    assert len(budgets) == L + 1, "--schedule needs %d counts, coarsest level first" % (L + 1)
    path = argv[0] if len(argv) > 0 else None
    window = int(argv[1]) if len(argv) > 1 else 50
    repeats = int(argv[2]) if len(argv) > 2 else 7
    bg = torch.zeros(3, device=DEV)

    def render(c, sc):
        fc = FrameContext(sc["means3D"].shape[0], c["W"], c["H"], 16, DEV)
        fc.forward(bg, T(sc["means3D"]), T(sc["opacities"]), T(c["viewmatrix"]), T(c["projmatrix"]), T(c["campos"]), c["tanfovx"], c["tanfovy"],
                   sh_degree=3, shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]))
        return fc.color.clone(), fc.depth[0].clone()

    def wide(start, true):
        w = np.array(start, np.float64)
        w[0, 3] += WIDE_START * float(np.abs(w[:3, 3] - true[:3, 3]).max())
        return w.astype(np.float32)

    res = []
    W, H, F = 160, 120, 140.0
    cams = syn.keyframe_cameras(4, radius=0.25, W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(3000, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    for k in range(1, 4):
        start = np.ascontiguousarray(cams[k - 1]["viewmatrix"].T).astype(np.float32)
        true = np.ascontiguousarray(cams[k]["viewmatrix"].T).astype(np.float64)
        gt = render(cams[k], sc)
        res.append(pyramid_case("160x120, 3000 Gaussians, frame %d from frame %d's pose" % (k, k - 1), L, budgets, cams[k], start, sc, gt, repeats))
        if k == 1:
            res.append(pyramid_case("160x120, 3000 Gaussians, frame 1 from frame 0's pose moved %g frame-to-frame translations along x" % WIDE_START,
                                    L, budgets, cams[k], wide(start, true), sc, gt, repeats))
    cam2, sc2 = syn.config_scene("cfg2")
    true2 = np.ascontiguousarray(cam2["viewmatrix"].T).astype(np.float64)
    a = math.radians(0.3)
    d = np.eye(4)
    d[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    d[:3, 3] = [0.012, -0.008, 0.01]
    start2 = (d @ true2).astype(np.float32)
    gt2 = render(cam2, sc2)
    res.append(pyramid_case("cfg2 (640x480, 50 000 Gaussians)", L, budgets, cam2, start2, sc2, gt2, repeats))
    res.append(pyramid_case("cfg2 (640x480, 50 000 Gaussians), start moved %g starting errors along x" % WIDE_START, L, budgets, cam2,
                            wide(start2, true2), sc2, gt2, repeats))
    kernels = [pyramid_kernel_case(640, 480, 3, window, repeats), pyramid_kernel_case(1280, 720, 3, window, repeats)]
    text = json.dumps(dict(device=torch.cuda.get_device_name(0), window=window, repeats=repeats, levels=L, budgets=budgets, cases=res,
                           k_pyramid=kernels), indent=1)
    print(text)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")


def main():
    if "--pyramid" in sys.argv:
        i = sys.argv.index("--pyramid")
        return pyramid_main(int(sys.argv[i + 1]), sys.argv[1:i] + sys.argv[i + 2:])
    if "--window" in sys.argv:
        i = sys.argv.index("--window")
        return window_main(int(sys.argv[i + 1]), sys.argv[1:i] + sys.argv[i + 2:])
    argv = [a for a in sys.argv[1:] if a != "--solve-exposure"]
    exposure = EXPOSURE if len(argv) < len(sys.argv) - 1 else None
    path = argv[0] if len(argv) > 0 else None
    window = int(argv[1]) if len(argv) > 1 else 50
    repeats = int(argv[2]) if len(argv) > 2 else 7
    res = []
    # the scene of tests/test_gpu_track_and_map.py: frame k started from frame k - 1's true pose
    W, H, F = 160, 120, 140.0
    cams = syn.keyframe_cameras(4, radius=0.25, W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(3000, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    fc = FrameContext(3000, W, H, 16, DEV)
    g = [T(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")]
    bg = torch.zeros(3, device=DEV)

    def render(fc, c, g):
        fc.forward(bg, g[0], g[1], T(c["viewmatrix"]), T(c["projmatrix"]), T(c["campos"]), c["tanfovx"], c["tanfovy"], sh_degree=3, shs=g[2],
                   scales=g[3], rotations=g[4])
        return fc.color.clone(), fc.depth[0].clone()

    for k in range(1, 4):
        res.append(case("160x120, 3000 Gaussians, frame %d from frame %d's pose" % (k, k - 1), cams[k],
                        np.ascontiguousarray(cams[k - 1]["viewmatrix"].T), sc, render(fc, cams[k], g), window, repeats, exposure=exposure))
    cam2, sc2 = syn.config_scene("cfg2")
    fc2 = FrameContext(sc2["means3D"].shape[0], cam2["W"], cam2["H"], 16, DEV)
    g2 = [T(sc2[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")]
    start = np.ascontiguousarray(cam2["viewmatrix"].T).astype(np.float64)
    a = math.radians(0.3)
    d = np.eye(4)
    d[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    d[:3, 3] = [0.012, -0.008, 0.01]
    res.append(case("cfg2 (640x480, 50 000 Gaussians)", cam2, (d @ start).astype(np.float32), sc2, render(fc2, cam2, g2), window, repeats,
                    exposure=exposure))
    text = json.dumps(dict(device=torch.cuda.get_device_name(0), window=window, repeats=repeats, solve_exposure=exposure is not None, cases=res),
                      indent=1)
    print(text)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")


def window_main(K, argv):
    path = argv[0] if len(argv) > 0 else None
    window = int(argv[1]) if len(argv) > 1 else 50
    repeats = int(argv[2]) if len(argv) > 2 else 7
    bg = torch.zeros(3, device=DEV)

    def render(c, sc):
        fc = FrameContext(sc["means3D"].shape[0], c["W"], c["H"], 16, DEV)
        fc.forward(bg, T(sc["means3D"]), T(sc["opacities"]), T(c["viewmatrix"]), T(c["projmatrix"]), T(c["campos"]), c["tanfovx"], c["tanfovy"],
                   sh_degree=3, shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]))
        return fc.color.clone(), fc.depth[0].clone()

    W, H, F = 160, 120, 140.0
    cams = syn.keyframe_cameras(4, radius=0.25, W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(3000, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    res = [window_case("160x120, 3000 Gaussians, frame 1 from frame 0's pose", K, cams[1], np.ascontiguousarray(cams[0]["viewmatrix"].T).astype(np.float32),
                       sc, render(cams[1], sc), window, repeats)]
    cam2, sc2 = syn.config_scene("cfg2")
    start = np.ascontiguousarray(cam2["viewmatrix"].T).astype(np.float64)
    a = math.radians(0.3)
    d = np.eye(4)
    d[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    d[:3, 3] = [0.012, -0.008, 0.01]
    res.append(window_case("cfg2 (640x480, 50 000 Gaussians)", K, cam2, (d @ start).astype(np.float32), sc2, render(cam2, sc2), window, repeats))
    text = json.dumps(dict(device=torch.cuda.get_device_name(0), window=window, repeats=repeats, K=K, cases=res), indent=1)
    print(text)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
