#!/usr/bin/env python3
"""Time of one mapping iteration through gsaj.mapping.DeviceMapper, loss fused into the batched compositors (fused=True) next to the
unfused sequence forward -> LossSeedsBatch -> backward (fused=False: the kernels of the parent of the change), alternating in one
process: cfg2 and cfg5, windows of 8 keyframes.  HIP events around blocks of 200 iterations after a warm-up, each block three times,
so that the spread of the unfused blocks is known before the two forms are compared.

The ground truth is the map's own render plus noise and every learning rate is 0: the kernels do all their work, the map and the
poses stay where they are, and both mappers see the same scene in every block.

    python tools/mapper_iter_bench.py --out profiles/r14_device_mapper.json
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    sys.path.insert(0, p)

K = 8
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.0, position_lr_final=0.0, position_lr_delay_mult=1.0,
                             position_lr_max_steps=30000, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0, rotation_lr=0.0)
# C-ABI launches of an iteration that are not rasteriser stages (gsaj_profile_begin / _end counts only those), by construction
OTHER = {True: dict(loss_finalize=1, isotropic=1, densification_stats=1, pose_step=1, map_step=1),
         False: dict(loss_seeds_batch=1, isotropic=1, densification_stats=1, pose_step=1, map_step=1, torch_copies_of_exposure_and_dexposure=3)}


def workload(torch, wl, iters, warmup, repeats):
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj import synthetic as syn
    from gsaj.mapping import DeviceMapper
    from gsaj.rasterizer import profile_stages

    dev = torch.device("cuda:0")
    cam, sc = syn.config_scene(wl)
    cams = syn.keyframe_cameras(K, W=cam["W"], H=cam["H"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])
    P, W, H, M = sc["means3D"].shape[0], cam["W"], cam["H"], sc["shs"].shape[1]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    praw, bg = t(cams[0]["projmatrix_raw"]), torch.zeros(3, device=dev)
    w2cs = [np.ascontiguousarray(c["viewmatrix"].T).astype(np.float32) for c in cams]
    mappers = {}
    for fused in (False, True):
        model = GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"],
                                             sh_degree=int(round(M ** 0.5)) - 1, device=dev)
        model.init_lr(1.0)
        model.training_setup(ARGS)
        mp = DeviceMapper(model, K, W, H, praw, cam["tanfovx"], cam["tanfovy"], bg, w2cs=w2cs, fused=fused, lr_rot=0.0, lr_trans=0.0,
                          lr_exposure_a=0.0, lr_exposure_b=0.0)
        mappers[fused] = mp
    # ground truth: what the map renders, disturbed
    first = mappers[False]
    first.iterate(1)
    gen = torch.Generator(device=dev).manual_seed(0)
    gt_c = first.ctx.color + 0.05 * torch.randn(first.ctx.color.shape, generator=gen, device=dev)
    gt_d = first.ctx.depth[:, 0] + 0.05 * torch.randn(first.ctx.depth[:, 0].shape, generator=gen, device=dev)
    launches = {}
    for fused, mp in mappers.items():
        for k in range(K):
            mp.set_view(k, gt_c[k], gt_d[k])
        mp.iterate(warmup)
        with profile_stages() as ps:
            mp.iterate(1)
            torch.cuda.synchronize()
        stages = {k: v for k, v in ps.launches.items() if v}
        launches[fused] = dict(rasteriser_stages=stages, others=OTHER[fused], total=sum(stages.values()) + sum(OTHER[fused].values()))
    ms = {False: [], True: []}
    for _ in range(repeats):
        for fused in (False, True):
            mp = mappers[fused]
            mp.iterate(5)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            mp.iterate(iters)
            b.record()
            b.synchronize()
            ms[fused].append(a.elapsed_time(b) / iters)
    spread = max(ms[False]) - min(ms[False])
    med = {f: float(np.median(v)) for f, v in ms.items()}
    out = dict(workload=wl, keyframes=K, P=P, W=W, H=H, iterations_per_block=iters, blocks=repeats,
               unfused_ms_per_iteration=[round(x, 4) for x in ms[False]], fused_ms_per_iteration=[round(x, 4) for x in ms[True]],
               unfused_median_ms=round(med[False], 4), fused_median_ms=round(med[True], 4), unfused_spread_ms=round(spread, 4),
               fused_minus_unfused_ms=round(med[True] - med[False], 4), fused_slower_than_the_unfused_spread=bool(med[True] - med[False] > spread),
               launches_per_iteration={"fused": launches[True], "unfused": launches[False]},
               seed_image_bytes_not_allocated=K * 4 * H * W * 4,
               window_loss=dict(fused=float(mappers[True].window_loss), unfused=float(mappers[False].window_loss)))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--workloads", default="cfg2,cfg5")
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("mapper_iter_bench: no GPU; a time is measured on the device or not at all")
    doc = dict(what="DeviceMapper.iterate: ms per mapping iteration (steps 1-8 of gsaj/mapping.py), fused=True against fused=False "
                    "alternating in one process, HIP events around blocks of iterations; spread = max - min of the unfused blocks",
               device=torch.cuda.get_device_name(0), results=[workload(torch, wl, a.iterations, a.warmup, a.blocks) for wl in a.workloads.split(",")])
    doc["default_fused"] = not any(r["fused_slower_than_the_unfused_spread"] for r in doc["results"])
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
