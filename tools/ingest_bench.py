#!/usr/bin/env python3
"""Times the frame ingest (csrc/ingest.hip, gsaj/ingest.py) on one MI355X, one process -> profiles/r20_ingest_bench.json.

    python tools/ingest_bench.py --out profiles/r20_ingest_bench.json

kernel:  k_frame_ingest alone on device inputs -- direct and remapped, with and without depth -- device events around windows of
         --calls calls, the median of --windows windows after a warm-up window; the apparent GB/s counts the bytes the call must move
         (source bytes, map floats, depth words, output floats) once each.
whole:   FrameIngest.__call__ from host arrays, the upload of the bytes included, against the reference's host statements without
         the remap (image / 255.0, from_numpy, clamp, permute, .to(device, float32), contiguous; depth / depth_scale and its upload):
         both wall-clock around a window with a synchronise at each end.  cv2 is not available, so the host remap of a distorted
         camera is NOT in the baseline: for such a camera the baseline is a lower bound of what the host path costs.
A run without a HIP device fails; nothing is timed on the CPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = ((640, 480), (1280, 720))
FR1_K = (517.306408, 516.469215, 318.643040, 255.313989)        # the TUM fr1 calibration at 640 x 480
FR1_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)


def call_bytes(W, H, remap, depth):
    n = W * H
    return 3 * n + 12 * n + (8 * n if remap else 0) + (6 * n if depth else 0)


def device_windows(torch, fn, calls, windows):
    """Median and spread, in microseconds per call, of `windows` windows of `calls` calls between two device events."""
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / calls)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out))


def wall_windows(torch, fn, calls, windows):
    for _ in range(calls):
        fn()
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / calls)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    import torch
    from gsaj.ingest import FrameIngest, UndistortMap

    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs the MI355X: nothing is timed on the CPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rows = []
    for (W, H) in SIZES:
        image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        depth = rng.integers(0, 65536, (H, W), dtype=np.uint16)
        d_image, d_depth = torch.as_tensor(image, device=dev), torch.as_tensor(depth, device=dev)
        um = UndistortMap(W, H, tuple(k * W / 640.0 for k in FR1_K), FR1_DIST, dev)
        for remap in (False, True):
            for with_depth in (False, True):
                ing = FrameIngest(W, H, dev, undistort=um if remap else None, depth_scale=5000.0 if with_depth else None)
                dargs = (d_image, d_depth) if with_depth else (d_image,)
                hargs = (image, depth) if with_depth else (image,)
                color, d = ing(*dargs)   # (allocates the outputs; the timed calls below are the bare C call, arguments ready)
                cargs = (W, H, W, H, 3, 3 * W, d_image.data_ptr(), um.map_x.data_ptr() if remap else None, um.map_y.data_ptr() if remap else None,
                         d_depth.data_ptr() if with_depth else None, 2 * W if with_depth else 0, 5000.0, 0, color.data_ptr(),
                         d.data_ptr() if with_depth else None, torch.cuda.current_stream(dev).cuda_stream)
                kern = device_windows(torch, lambda: ing.lib.gsaj_frame_ingest(*cargs), a.calls, a.windows)
                whole_ev = device_windows(torch, lambda: ing(*hargs), a.calls, a.windows)
                whole_wall = wall_windows(torch, lambda: ing(*hargs), a.calls, a.windows)
                nbytes = call_bytes(W, H, remap, with_depth)
                rows.append(dict(W=W, H=H, remap=remap, depth=with_depth, bytes_per_call=nbytes,
                                 kernel=dict(kern, apparent_GBps=nbytes / (kern["median_us"] * 1e-6) / 1e9),
                                 whole_ingest_device_events=whole_ev, whole_ingest_wall=whole_wall))

        def host_path(with_depth):
            color = torch.from_numpy(image / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).to(device=dev, dtype=torch.float32).contiguous()
            d = torch.from_numpy(depth / 5000.0).to(device=dev, dtype=torch.float32) if with_depth else None
            return color, d

        for with_depth in (False, True):
            rows.append(dict(W=W, H=H, remap=False, depth=with_depth, host_statements_wall=wall_windows(torch, lambda: host_path(with_depth), a.calls, a.windows)))
    doc = dict(method="one MI355X, one process; windows of %d calls, median of %d after a warm-up window.  kernel: gsaj_frame_ingest on device inputs "
                      "(one k_frame_ingest launch per call, called back to back), device events.  whole_ingest_*: FrameIngest from host arrays, the upload of the "
                      "bytes included, by device events and wall-clock with a synchronise at each end.  host_statements_wall: the reference's "
                      "host statements WITHOUT the remap (cv2 is not available; for a distorted camera this baseline lacks its remap), "
                      "wall-clock with a synchronise at each end.  apparent_GBps: bytes_per_call once each over the kernel's median."
                      % (a.calls, a.windows),
               device=torch.cuda.get_device_name(0), rows=rows)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
