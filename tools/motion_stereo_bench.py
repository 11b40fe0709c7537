#!/usr/bin/env python3
"""Times motion stereo (csrc/sweep.hip, gsaj/motion_stereo.py) on one MI355X, one process -> profiles/r31_motion_stereo_bench.json.

    python tools/motion_stereo_bench.py --out profiles/r31_motion_stereo_bench.json

At 640 x 480 with 64 hypotheses and a 7 x 7 window (r = 3), for 4 and 8 paths, and at 160 x 120 with 16 hypotheses, on device inputs:
call:    gsaj_motion_stereo, everything, idx16 and depth -- device events around windows of --calls calls, p10 / p50 / p90 of --windows
         windows after a warm-up window
stages:  the same call restricted to one stage (GSAJ_SWEEP_STAGE_*) on the workspace the full call left: cost (gradient bytes, pixel cost,
         box), paths (the memset of S + every line), winner (argmin .. depth); and the cost stage once more at r = 0, where the box kernel
         reads one byte per entry, so that the difference is what the window's row sums cost.  The effective GB/s counts the bytes a stage
         must move once each (they are not hardware counters): cost writes pc (1 byte), reads it back and writes C (2); paths reads C once
         per direction and adds into S (4 bytes per entry and direction); winner reads S (4).
context: StereoMatcher's stages at the same W, H, D and r, measured in the same process: its paths stage walks W - D columns, motion
         stereo's W.
There is no parent baseline (the feature is new) and no time here is a pass criterion.  A run without a HIP device fails; nothing is timed
on the CPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = ((640, 480, 64, 3, 4), (640, 480, 64, 3, 8), (160, 120, 16, 3, 8))   # W, H, D, r, paths
W_RANGE = (0.0, 1.0)


def frames(W, H, rng):
    """A two-scale random texture on the plane z = 2 seen by two cameras a sideways step apart: the source image is the reference
    shifted by the plane's parallax, a whole number of pixels.  -> ref, src uint8 [H,W], intrinsics, the two poses."""
    fx = fy = 525.0 * W / 640.0
    shift = max(2, W // 80)
    coarse = np.kron(rng.random((H // 4 + 1, (W + shift) // 4 + 1)), np.ones((4, 4)))[:H, :W + shift]
    tex = (255.0 * (0.5 * coarse + 0.5 * rng.random((H, W + shift)))).astype(np.uint8)
    ref, src = tex[:, shift:], tex[:, :W]              # src(u + shift) = ref(u)
    ref_w2c, src_w2c = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    src_w2c[0, 3] = shift * 2.0 / fx                   # u_src = u_ref + fx t_x w, w = 1 / 2
    return np.ascontiguousarray(ref), np.ascontiguousarray(src), (fx, fy, W / 2.0, H / 2.0), ref_w2c, src_w2c


def windows(torch, fn, calls, n):
    """p10, p50, p90 in milliseconds per call of n windows of `calls` calls between two device events, after one warm-up window."""
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    p10, p50, p90 = np.percentile(out, (10, 50, 90))
    return dict(p10_ms=float(p10), p50_ms=float(p50), p90_ms=float(p90))


def gbps(nbytes, row):
    return nbytes / (row["p50_ms"] * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    a = ap.parse_args()
    import torch
    from gsaj import motion_stereo as ms
    from gsaj import stereo as st

    if not torch.cuda.is_available():
        raise SystemExit("motion_stereo_bench needs the MI355X: nothing is timed on the CPU")
    dev = torch.device("cuda:0")
    rows = []
    for W, H, D, r, paths in SIZES:
        ref, src, K, ref_w2c, src_w2c = frames(W, H, np.random.default_rng(0))
        d = [torch.as_tensor(x, device=dev) for x in (ref, src, ref_w2c, src_w2c)]
        m = ms.MotionStereo(W, H, dev, *K, num_hypotheses=D, block_radius=r, paths=paths)
        idx16, depth = m(*d, *W_RANGE)
        valid = idx16 >= 0
        near = float(((depth[valid] - 2.0).abs() < 0.2).float().mean()) if bool(valid.any()) else 0.0
        entries = W * H * D
        row = dict(what="MotionStereo", W=W, H=H, D=D, r=r, paths=paths, valid_share=float(valid.float().mean()), within_10_percent_of_the_plane=near,
                   workspace_bytes=m.workspace.numel(), call=windows(torch, lambda: m(*d, *W_RANGE), a.calls, a.windows))
        for name, stage in (("stage_cost", ms.STAGE_COST), ("stage_paths", ms.STAGE_PATHS), ("stage_winner", ms.STAGE_WINNER)):
            row[name] = windows(torch, lambda: m(*d, *W_RANGE, stages=stage), a.calls, a.windows)
        m0 = ms.MotionStereo(W, H, dev, *K, num_hypotheses=D, block_radius=0, paths=paths)
        m0(*d, *W_RANGE)
        row["stage_cost_r0"] = windows(torch, lambda: m0(*d, *W_RANGE, stages=ms.STAGE_COST), a.calls, a.windows)
        row["stage_cost"].update(pc_bytes_written=entries, pc_bytes_read_once=entries, C_bytes_written=2 * entries,
                                 effective_GBps=gbps(4 * entries, row["stage_cost"]))
        row["stage_paths"].update(C_bytes_read=2 * entries * paths, effective_GBps_on_C=gbps(2 * entries * paths, row["stage_paths"]),
                                  S_atomic_bytes=4 * entries * paths, atomic_GBps_on_S=gbps(4 * entries * paths, row["stage_paths"]))
        row["stage_winner"].update(S_bytes_read=4 * entries, effective_GBps_on_S=gbps(4 * entries, row["stage_winner"]))
        rows.append(row)
        # context: the rectified matcher at the same W, H, D and window, in the same process
        sm = st.StereoMatcher(W, H, dev, num_disparities=D, block_radius=r, paths=paths)
        sm(d[0], d[1], bf=1.0)
        ctx = dict(what="StereoMatcher (context)", W=W, H=H, D=D, r=r, paths=paths, valid_columns=W - D,
                   call=windows(torch, lambda: sm(d[0], d[1], bf=1.0), a.calls, a.windows))
        for name, stage in (("stage_cost", st.STAGE_COST), ("stage_paths", st.STAGE_PATHS), ("stage_winner", st.STAGE_WINNER)):
            ctx[name] = windows(torch, lambda: sm(d[0], d[1], bf=1.0, stages=stage), a.calls, a.windows)
        rows.append(ctx)
        del m, m0, sm
    doc = dict(method="one MI355X, one process; windows of %d calls between two device events, p10 / p50 / p90 of %d windows after a warm-up "
                      "window; device inputs.  A stage row is the call restricted to that stage on the workspace the full call left.  The "
                      "effective GB/s are the bytes a stage must move once each over its p50, not hardware counters.  No parent baseline: "
                      "the feature is new; the StereoMatcher rows are context, measured in the same process." % (a.calls, a.windows),
               device=torch.cuda.get_device_name(0), rows=rows)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
