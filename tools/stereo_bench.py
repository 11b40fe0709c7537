#!/usr/bin/env python3
"""Times the stereo matcher (csrc/stereo.hip, gsaj/stereo.py) on one MI355X, one process -> profiles/r21_stereo_bench.json.

    python tools/stereo_bench.py --out profiles/r21_stereo_bench.json

At EuRoC's 752 x 480 with 64 disparities and a 21 x 21 window (r = 10), for 4 and 8 paths, on device inputs:
pair:    gsaj_stereo_match, everything, disparity and depth -- device events around windows of --calls calls, p10 / p50 / p90 of
         --windows windows after a warm-up window
stages:  the same call restricted to one stage (GSAJ_STEREO_STAGE_*) on the workspace the full call left: cost volume (prefilter + block
         cost), paths (the memset of S + every line), winner (argmin .. depth).  The effective GB/s counts the bytes of C a stage must
         move once each: the cost stage writes C for the valid columns, the paths stage reads it once per direction; the paths stage's
         atomic adds into S (4 bytes per entry and direction) are reported beside it.
whole:   StereoIngest from host arrays through two rectifying maps, uploads included, and FrameIngest of one grey image at the same
         size -- what the frame costs next to the step that was already on the device.
No OpenCV time can be measured here and the parent has no stereo path: there is no baseline row.  A run without a HIP device fails;
nothing is timed on the CPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H, D, R = 752, 480, 64, 10
BF = 47.90639384423901
EUROC_K = (458.654, 457.296, 367.215, 248.375)                      # cam0 of the EuRoC rig: fx fy cx cy
EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)


def pair(rng):
    """A two-scale random texture and its shift by a disparity that ramps from 4 to 40 pixels down the image."""
    coarse = np.kron(rng.random((H // 4 + 1, (W + 64) // 4 + 1)), np.ones((4, 4)))[:H, :W + 64]
    tex = (255.0 * (0.5 * coarse + 0.5 * rng.random((H, W + 64)))).astype(np.uint8)
    right = tex[:, 48:48 + W]
    shift = (4 + 36 * np.arange(H) // H).astype(np.int64)
    left = np.stack([tex[y, 48 - shift[y]:48 - shift[y] + W] for y in range(H)])
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    a = ap.parse_args()
    import torch
    from gsaj.ingest import FrameIngest, UndistortMap
    from gsaj.stereo import STAGE_COST, STAGE_PATHS, STAGE_WINNER, StereoIngest, StereoMatcher

    if not torch.cuda.is_available():
        raise SystemExit("stereo_bench needs the MI355X: nothing is timed on the CPU")
    dev = torch.device("cuda:0")
    left, right = pair(np.random.default_rng(0))
    d_left, d_right = torch.as_tensor(left, device=dev), torch.as_tensor(right, device=dev)
    entries = (W - D) * H * D
    rows = []
    for paths in (4, 8):
        m = StereoMatcher(W, H, dev, num_disparities=D, block_radius=R, paths=paths)
        disp16, _ = m(d_left, d_right, bf=BF)
        valid = float((disp16[:, D:] >= 0).float().mean())
        row = dict(W=W, H=H, D=D, r=R, paths=paths, valid_share=valid, workspace_bytes=m.workspace.numel(),
                   pair=windows(torch, lambda: m(d_left, d_right, bf=BF), a.calls, a.windows))
        for name, stage in (("stage_cost", STAGE_COST), ("stage_paths", STAGE_PATHS), ("stage_winner", STAGE_WINNER)):
            row[name] = windows(torch, lambda: m(d_left, d_right, bf=BF, stages=stage), a.calls, a.windows)
        row["stage_cost"]["C_bytes_written"] = 2 * entries
        row["stage_cost"]["effective_GBps_on_C"] = 2 * entries / (row["stage_cost"]["p50_ms"] * 1e-3) / 1e9
        row["stage_paths"]["C_bytes_read"] = 2 * entries * paths
        row["stage_paths"]["effective_GBps_on_C"] = 2 * entries * paths / (row["stage_paths"]["p50_ms"] * 1e-3) / 1e9
        row["stage_paths"]["S_atomic_bytes"] = 4 * entries * paths
        row["stage_paths"]["atomic_GBps_on_S"] = 4 * entries * paths / (row["stage_paths"]["p50_ms"] * 1e-3) / 1e9
        row["stage_winner"]["S_bytes_read"] = 4 * entries
        row["stage_winner"]["effective_GBps_on_S"] = 4 * entries / (row["stage_winner"]["p50_ms"] * 1e-3) / 1e9
        rows.append(row)
    ul = UndistortMap(W, H, EUROC_K, EUROC_DIST, dev)
    ur = UndistortMap(W, H, EUROC_K, EUROC_DIST, dev)
    whole = StereoIngest(W, H, dev, BF, undistort_left=ul, undistort_right=ur, num_disparities=D, block_radius=R, paths=8)
    rows.append(dict(W=W, H=H, what="StereoIngest from host arrays: two uploads, two remaps, the 8-path match, depth and colour",
                     **windows(torch, lambda: whole(left, right), a.calls, a.windows)))
    grey = FrameIngest(W, H, dev, channels=1, undistort=ul, round_u8=True)
    rows.append(dict(W=W, H=H, what="FrameIngest of the left grey image from a host array through the same map",
                     **windows(torch, lambda: grey(left), a.calls, a.windows)))
    doc = dict(method="one MI355X, one process; windows of %d calls between two device events, p10 / p50 / p90 of %d windows after a warm-up "
                      "window; device inputs for pair and stages, host arrays (uploads included) for the two whole-frame rows.  A stage row is "
                      "gsaj_stereo_match restricted to that stage.  effective_GBps_on_C / _on_S: the bytes the stage must move once each over "
                      "its p50; they are not hardware counters." % (a.calls, a.windows),
               device=torch.cuda.get_device_name(0), rows=rows)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
