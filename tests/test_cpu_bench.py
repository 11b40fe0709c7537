"""CPU: bench.py's command line (a plain run reports the headline only, --full adds the rest) and --dump-outputs on host tensors
shaped like the cfg2 window (8 keyframes, 50 000 Gaussians SH-3, 640x480): float32 files, bounded in size, the same seeded
sample every time."""
import os
import types

import numpy as np
import torch

import bench
from gsaj.keyframe_shard import bucket_numel, bucket_views

NAMES = ["alpha", "color", "dL_dmean2D", "dL_dmeans3D", "dL_dopacity", "dL_drotations", "dL_dscales", "dL_dshs", "dL_dtau", "depth",
         "radii"]


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out", "--no-cpu-baseline", "--skip-single"])
    assert a.full and a.dump_outputs == "out" and a.no_cpu_baseline and a.skip_single


def _window(K=8, P=50_000, M=16, H=480, W=640, seed=0):
    gen = torch.Generator().manual_seed(seed)
    bucket = torch.randn(bucket_numel(P, M, True, K), generator=gen)
    v = bucket_views(bucket, P, M, True, K)
    g = dict(mean2D=torch.randn(K, P, 3, generator=gen), opacity=v["opacity"], mean3D=v["mean3D"], sh=v["sh"].view(P, M, 3),
             scale=v["scale"], rot=v["rot"], tau_all=v["tau_all"], tau_every_window=None)
    return types.SimpleNamespace(color=torch.randn(K, 3, H, W, generator=gen), depth=torch.randn(K, 1, H, W, generator=gen),
                                 opacity=torch.rand(K, 1, H, W, generator=gen),
                                 radii=torch.randint(0, 60, (K, P), generator=gen, dtype=torch.int32), slots=[g])


def test_dump_outputs_are_float32_bounded_and_repeatable(tmp_path):
    ctx = _window()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, ctx, 0)
    bench.dump_outputs(b, ctx, 0)
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in NAMES)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 2 ** 20
    for n in NAMES:
        x = np.load(os.path.join(a, n + ".npy"))
        assert x.dtype == np.float32 and x.size <= bench.DUMP_CAP, n
        assert np.array_equal(x, np.load(os.path.join(b, n + ".npy"))), n
    g = ctx.slots[0]
    # arrays within the cap: whole, in their own shape
    assert np.array_equal(np.load(os.path.join(a, "dL_dtau.npy")), g["tau_all"].numpy())
    assert np.array_equal(np.load(os.path.join(a, "dL_dmeans3D.npy")), g["mean3D"].numpy())
    assert np.array_equal(np.load(os.path.join(a, "radii.npy")), ctx.radii.numpy().astype(np.float32))
    # larger ones: the values at the seeded, sorted flat indices
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(ctx.color.numel(), bench.DUMP_CAP, replace=False))
    assert np.array_equal(np.load(os.path.join(a, "color.npy")), ctx.color.reshape(-1).numpy()[idx])
