#!/usr/bin/env python3
"""Frame-to-frame RGB-D alignment (gsaj.RgbdAligner, csrc/align.hip) measured, and set against the map tracker it is meant to start.

Method of tools/gn_tracker_bench.py: device events, medians of `repeats` after a warm-up, one process.
  align        ms per WHOLE align() call -- the copy of the frame, the pyramid build, every iteration and relevel -- with the default
               schedule, and us per iteration (gsaj_rgbd_align + gsaj_pose_gn_step) at every level, on 160x120 (L = 2) and 640x480 (L = 3)
  gauss_newton GaussNewtonTracker's ms per iteration on the same two workloads, in the same session (gn_tracker_bench.ms_per_iteration)
  start        the question the aligner exists for: the iterations and milliseconds GaussNewtonTracker needs to meet the criterion of
               tests/test_gpu_gn_tracker.py (translation error below 0.35 x the previous pose's, rotation error below 0.02) from the
               previous frame's pose, and from the aligned pose with align()'s own time added; the alignment with depth and, beside it,
               photometric only (the reference depth of these worlds is a splat render, not a surface).
The reference frame is the render at the previous pose, the current frame the render at the true pose.

--exposure A B: the joint form (gsaj.JointRgbdAligner: the brightness change e^a I + b of the current frame solved with the pose) set
against the pose-only form in the same session, the current frame's colour replaced by e^A I + B:
  table        the analytic scene of tests/align_restated.py at 80x60, L = 2, default schedule, start at the reference pose: translation /
               rotation error of both forms and the recovered (a, b), for m = 1, 2, with and without depth, at (0, 0), (A, B) and
               (-0.15, 0.05)
  align        ms per whole align() and us per iteration at every level, both forms, on 160x120 (L = 2) and cfg2's 640x480 (L = 3), with
               the errors against the true pose and the recovered (a, b) at (A, B)
(the map tracker is not run.)

usage: rgbd_align_bench.py [out.json] [window=50] [repeats=7] [--exposure A B]"""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from gn_tracker_bench import DEV, T, errors, first_hit, ms_per_iteration  # noqa: E402
from gsaj import align as A  # noqa: E402
from gsaj import synthetic as syn  # noqa: E402
from gsaj.gauss_newton import GaussNewtonTracker  # noqa: E402
from gsaj.rasterizer import FrameContext  # noqa: E402


def csrc_sha1():
    d = os.path.join(ROOT, "gs-slam-analytica_jacobian_amd", "csrc")
    h = hashlib.sha1()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def render(c, sc):
    fc = FrameContext(sc["means3D"].shape[0], c["W"], c["H"], 16, DEV)
    fc.forward(torch.zeros(3, device=DEV), T(sc["means3D"]), T(sc["opacities"]), T(c["viewmatrix"]), T(c["projmatrix"]), T(c["campos"]),
               c["tanfovx"], c["tanfovy"], sh_degree=3, shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]))
    return fc.color.clone(), fc.depth[0].clone()


def events_ms(run, repeats, per=1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(repeats):
        ev[0].record()
        run()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) / per)
    return [round(float(np.median(out)), 4), round(float(min(out)), 4), round(float(max(out)), 4)]


def workload(name, cam_prev, cam, sc, levels, window, repeats, budget=30):
    P, W, H, M = sc["means3D"].shape[0], cam["W"], cam["H"], sc["shs"].shape[1]
    prev = np.ascontiguousarray(cam_prev["viewmatrix"].T).astype(np.float32)
    true = np.ascontiguousarray(cam["viewmatrix"].T).astype(np.float64)
    ref, cur = render(cam_prev, sc), render(cam, sc)
    before, before_rot = errors(prev, true)
    out = dict(workload=name, P=P, W=W, H=H, levels=levels, start_translation_error=before, start_rotation_error=before_rot)
    al = A.RgbdAligner(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], DEV, levels=levels)
    al.set_reference(ref[0], ref[1], prev)
    res = {}
    for key, depth in (("rgbd", cur[1]), ("photometric", None)):
        run = lambda depth=depth: al.align(cur[0], depth)  # noqa: E731
        for _ in range(3):
            run()
        w2c, overlap, loss, conv = al.result()
        e = errors(w2c, true)
        row = dict(schedule=al.default_schedule(), ms_per_align_median_min_max=events_ms(run, repeats), overlap=round(overlap, 4),
                   translation_error=e[0], rotation_error=e[1], error_ratio=round(e[0] / before, 4), accepted_loss=loss, converged=conv,
                   accepted=float(al.lm["accepted"]), rejected=float(al.lm["rejected"]), aligned_w2c=w2c.astype(np.float32))
        per = {}
        for l in range(levels, -1, -1):   # one level alone: `window` iterations from the reference pose, at that level's camera
            def its(l=l, depth=depth):
                for _ in range(window):
                    A._residuals(al, l, depth is not None)
                    A._step(al, l)

            al._reset(al.ref_w2c)
            A._relevel(al, l)
            its()
            per[str(l)] = [round(1e3 * x, 2) for x in events_ms(its, repeats, per=window)]
        row["us_per_iteration_per_level_median_min_max"] = per
        res[key] = row
    # the map tracker from both starts
    g = dict(means3D=T(sc["means3D"]), opacities=T(sc["opacities"]), shs=T(sc["shs"]), scales=T(sc["scales"]), rotations=T(sc["rotations"]),
             sh_degree=3)
    gnt = GaussNewtonTracker(P, W, H, M, DEV, prev, T(cam["projmatrix_raw"]), cam["tanfovx"], cam["tanfovy"], torch.zeros(3, device=DEV),
                             alpha=0.9, **g)
    med, lo, hi = ms_per_iteration(gnt, lambda: gnt.set_frame(cur[0], cur[1], w2c=prev), window, repeats)
    out["gauss_newton_ms_per_iteration_median_min_max"] = [round(med, 4), round(lo, 4), round(hi, 4)]
    starts = [("previous_pose", prev, 0.0)] + [("aligned_" + k, res[k].pop("aligned_w2c"), res[k]["ms_per_align_median_min_max"][0]) for k in res]
    out["start"] = {}
    for key, start, extra_ms in starts:
        t0, r0 = errors(start, true)
        if t0 < 0.35 * before and r0 < 0.02:
            hit, trace, rot = 0, [], r0
        else:
            gnt.set_frame(cur[0], cur[1], w2c=start)
            hit, trace, rot = first_hit(gnt, lambda: gnt.accepted_w2c, true, before, budget)
        out["start"][key] = dict(start_error_ratio=round(t0 / before, 4), start_rotation_error=r0, iterations_to_criterion=hit,
                                 ms_to_criterion=None if hit is None else round(extra_ms + hit * med, 3), align_ms_included=extra_ms,
                                 error_ratio_trace=trace[:12], rotation_error_at_end=round(rot, 6))
    out["align"] = res
    return out


def time_aligner(al, cur, depth, levels, window, repeats, true):
    """ms per whole align() and us per iteration at every level of one aligner on one frame, with where it ends."""
    run = lambda: al.align(cur, depth)  # noqa: E731
    for _ in range(3):
        run()
    w2c, overlap, loss, conv = al.result()
    e = errors(w2c, true)
    row = dict(ms_per_align_median_min_max=events_ms(run, repeats), overlap=round(overlap, 4), translation_error=e[0], rotation_error=e[1],
               accepted_loss=loss, accepted=float(al.lm["accepted"]), rejected=float(al.lm["rejected"]))
    if al.solve_exposure:
        row["recovered_a_b"] = [round(float(v), 6) for v in al.relative_exposure.cpu()]
    per = {}
    for l in range(levels, -1, -1):
        def its(l=l):
            for _ in range(window):
                A._residuals(al, l, depth is not None)
                A._step(al, l)

        al._reset(al.ref_w2c)
        A._relevel(al, l)
        its()
        per[str(l)] = [round(1e3 * x, 2) for x in events_ms(its, repeats, per=window)]
    row["us_per_iteration_per_level_median_min_max"] = per
    return row


def exposure_workload(name, cam_prev, cam, sc, levels, window, repeats, a, b):
    W, H = cam["W"], cam["H"]
    prev = np.ascontiguousarray(cam_prev["viewmatrix"].T).astype(np.float32)
    true = np.ascontiguousarray(cam["viewmatrix"].T).astype(np.float64)
    ref, cur = render(cam_prev, sc), render(cam, sc)
    bright = math.exp(a) * cur[0] + b
    before, before_rot = errors(prev, true)
    out = dict(workload=name, W=W, H=H, levels=levels, brightness_a_b=[a, b], start_translation_error=before, start_rotation_error=before_rot)
    for form, cls in (("pose_only", A.RgbdAligner), ("joint", A.JointRgbdAligner)):
        al = cls(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], DEV, levels=levels)
        al.set_reference(ref[0], ref[1], prev)
        out[form] = {key: time_aligner(al, bright, depth, levels, window, repeats, true) for key, depth in (("rgbd", cur[1]), ("photometric", None))}
    return out


def exposure_table(a, b):
    """The device's version of the restated loops' table (tests/test_cpu_align_joint.py), on the analytic scene."""
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]   # (the restatements, and the oracle package they import)
    import align_joint_restated as aj
    import align_restated as ar
    cam, rows = ar.camera(), []
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)  # noqa: E731
    for m in (1.0, 2.0):
        for ea, eb in ((0.0, 0.0), (a, b), (-0.15, 0.05)):
            for depth in (True, False):
                case = aj.behaviour_case8(m, depth, ea, eb)
                row = dict(m=m, a=ea, b=eb, term="depth" if depth else "photo", start=[round(v, 5) for v in ar.pose_error(case["w2c"], ar.motion(m))])
                for form, cls in (("pose_only", A.RgbdAligner), ("joint", A.JointRgbdAligner)):
                    al = cls(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], DEV, levels=2)
                    al.set_reference(dev(case["ref_color"]), dev(case["ref_depth"]), case["ref_w2c"])
                    al.align(dev(case["cur_color"]), dev(case["cur_depth"]))
                    row[form] = [round(v, 5) for v in ar.pose_error(al.result()[0], ar.motion(m))]
                    if al.solve_exposure:
                        row["recovered_a_b"] = [round(float(v), 4) for v in al.relative_exposure.cpu()]
                rows.append(row)
    return rows


def exposure_main(path, window, repeats, a, b):
    table = exposure_table(a, b)
    W, H, F = 160, 120, 140.0
    cams = syn.keyframe_cameras(4, radius=0.25, W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(3000, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    res = [exposure_workload("160x120, 3000 Gaussians, frame 1 from frame 0", cams[0], cams[1], sc, 2, window, repeats, a, b)]
    cam2, sc2, prev2 = cfg2_pair()
    res.append(exposure_workload("cfg2 (640x480, 50 000 Gaussians), previous pose 1.2 cm / 0.3 degrees off", prev2, cam2, sc2, 3, window, repeats, a, b))
    text = json.dumps(dict(device=torch.cuda.get_device_name(0), csrc_sha1=csrc_sha1(), window=window, repeats=repeats, table=table,
                           cases=res), indent=1)
    print(text)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")


def cfg2_pair():
    cam2, sc2 = syn.config_scene("cfg2")
    true2 = np.ascontiguousarray(cam2["viewmatrix"].T).astype(np.float64)
    a = math.radians(0.3)
    d = np.eye(4)
    d[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    d[:3, 3] = [0.012, -0.008, 0.01]
    return cam2, sc2, syn.make_camera((d @ true2), **{k: cam2[k] for k in ("W", "H", "fx", "fy", "cx", "cy")})


def main():
    argv = sys.argv[1:]
    exposure = None
    if "--exposure" in argv:
        i = argv.index("--exposure")
        exposure = (float(argv[i + 1]), float(argv[i + 2]))
        del argv[i:i + 3]
    path = argv[0] if len(argv) > 0 else None
    window = int(argv[1]) if len(argv) > 1 else 50
    repeats = int(argv[2]) if len(argv) > 2 else 7
    assert repeats >= 7, "median of at least 7"
    if exposure is not None:
        return exposure_main(path, window, repeats, *exposure)
    res = []
    W, H, F = 160, 120, 140.0
    cams = syn.keyframe_cameras(4, radius=0.25, W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(3000, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    for k in range(1, 4):
        res.append(workload("160x120, 3000 Gaussians, frame %d from frame %d" % (k, k - 1), cams[k - 1], cams[k], sc, 2, window, repeats))
    cam2, sc2, prev2 = cfg2_pair()
    res.append(workload("cfg2 (640x480, 50 000 Gaussians), previous pose 1.2 cm / 0.3 degrees off", prev2, cam2, sc2, 3, window, repeats))
    text = json.dumps(dict(device=torch.cuda.get_device_name(0), csrc_sha1=csrc_sha1(), window=window, repeats=repeats, cases=res), indent=1)
    print(text)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
