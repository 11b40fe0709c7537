"""Device time of the keyframe seeding path (csrc/seed.hip): the per-frame median_depth, and selection + initialisation of the
new Gaussians of a keyframe, with gsaj_dist2's share shown separately.  HIP events around `reps` back-to-back calls after a
warm-up (the calls enqueue without host synchronisation, except the 8-byte count read of the seeding).  For context only, a plain
torch-op composition of the same steps on the same device is timed the same way; nothing depends on the ratio.

    python tools/seed_bench.py --reps 200 --out profiles/seed_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/seed_bench.py --trace-once     # launch counts per call
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    sys.path.insert(0, p)

# launches per call, from the call sequences in csrc/seed.hip / csrc/knn.hip (checked against a kernel trace: --trace-once)
LAUNCHES = {"median_depth": "1 memset + 8 kernels (4 x histogram + pick)",
            "seed_select": "1 memset + 11 kernels (4 x histogram + pick, count, scan, compact)",
            "seed_gaussians": "points + gsaj_dist2 (1 memset + 16 kernels) + scales (+ 1 memset of f_rest; adaptive: + 2 x (1 memset + 8))"}


def keyframe(W, H, seed=0):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    depth = (2.0 + 0.5 * np.sin(u / 50.0) + 0.3 * np.cos(v / 35.0) + rng.normal(0, 0.01, (H, W))).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.2] = 0
    return depth, rng.uniform(0.9, 1.0, (H, W)).astype(np.float32), rng.uniform(0, 1, (3, H, W)).astype(np.float32)


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-once", action="store_true", help="one call of each entry point at 640x480, factor 32 (for a kernel trace)")
    a = ap.parse_args()
    import torch

    from gsaj import seeding, synthetic as syn
    from simple_knn._C import distCUDA2

    assert torch.cuda.is_available(), "seed_bench needs the GPU: there is no CPU path to time"
    dev = "cuda:0"
    T = lambda x: torch.as_tensor(x, device=dev)  # noqa: E731
    rows = []
    for (W, H), factors in (((640, 480), (32, 64, 128)), ((1280, 720), (32,))):
        depth, opacity, image = (T(x) for x in keyframe(W, H))
        cam = syn.fixture_camera(noisy=True, orthonormal=True, W=W, H=H, fx=0.9 * W, fy=0.9 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
        w2c = T(cam["w2c"].astype(np.float32))
        K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        if a.trace_once:
            seeding.median_depth(depth, opacity)
            seeding.seed_from_keyframe(image, depth, w2c, *K, 32, 0.01)
            torch.cuda.synchronize()
            return

        def torch_median():
            valid = (depth > 0) & (opacity > 0.95)
            d = depth[valid]
            return d.median(), d.std()

        rows.append(dict(what="median_depth", W=W, H=H, ms=timed(torch, lambda: seeding.median_depth(depth, opacity), a.reps, a.warmup),
                         torch_ops_ms=timed(torch, torch_median, a.reps, a.warmup), launches=LAUNCHES["median_depth"]))
        rows.append(dict(what="keyframe_depth_prior", W=W, H=H, launches="median_depth + 1 kernel",
                         ms=timed(torch, lambda: seeding.keyframe_depth_prior(depth, opacity, image, 0.01, depth), a.reps, a.warmup)))
        lib, ws = seeding._lib.load(), seeding._workspace(seeding._lib.load(), torch.device(dev), H, W)
        st = torch.cuda.current_stream().cuda_stream
        for factor in factors:
            xyz = seeding.seed_from_keyframe(image, depth, w2c, *K, factor, 0.01)[0]
            m = xyz.shape[0]
            c2w = torch.linalg.inv(w2c)

            def torch_seed():
                idx = torch.nonzero(((depth > 0) & (depth < 100.0)).reshape(-1))[:, 0]
                idx = idx[torch.randperm(idx.numel(), device=dev)[: int(idx.numel() * (1.0 / factor))]]
                z = depth.reshape(-1)[idx]
                pc = torch.stack([((idx % W) - K[2]) * z / K[0], ((idx // W) - K[3]) * z / K[1], z, torch.ones_like(z)], dim=1)
                pts = (pc @ c2w.T)[:, :3].contiguous()
                rgb = (image.reshape(3, -1)[:, idx].T.clamp(0, 1) * 255).byte().float() / 255
                return pts, (rgb - 0.5) / 0.28209479177387814, torch.log(torch.sqrt(distCUDA2(pts).clamp_min(1e-7) * 0.01))

            sel = lambda: lib.gsaj_seed_select(W, H, depth.data_ptr(), None, 0.0, 100.0, float(factor), 0, ws.data_ptr(), st)  # noqa: E731
            rows.append(dict(what="select + seed", W=W, H=H, factor=factor, m=m,
                             ms=timed(torch, lambda: seeding.seed_from_keyframe(image, depth, w2c, *K, factor, 0.01), a.reps, a.warmup),
                             of_which_select_ms=timed(torch, sel, a.reps, a.warmup),
                             of_which_dist2_ms=timed(torch, lambda: distCUDA2(xyz), a.reps, a.warmup),
                             torch_ops_ms=timed(torch, torch_seed, a.reps, a.warmup),
                             launches=LAUNCHES["seed_select"] + "; " + LAUNCHES["seed_gaussians"],
                             note="ms includes the blocking 8-byte count read and the allocation of the outputs and of the kNN workspace"))
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, rows=rows)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
