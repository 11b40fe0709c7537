"""Time of the step on the Gaussian map: GaussianModel.map_step (one launch, csrc/map_step.hip) next to the path it replaces,
assign_bucket_gradients + optimizer.step() + zero_grad(set_to_none=True), on the same device, the same model and the same bucket.

At cfg2's map size (P = 50 000) and cfg5's (P = 1 000 000), SH degree 3 (M = 16), three scale columns, the reference's learning
rates, Adam attached and stepped once.  Each call sits between two HIP events on the stream, so a call's time includes the
gaps the host leaves between its kernels; the two paths alternate in rounds, each with its own warm-up, and every figure is taken
over all timed calls of all rounds (at least 200 per path): median, 10th and 90th percentile, minimum.  Bytes: a step reads and
writes the parameter and the two moments and reads the gradient, 59 floats x 7 x 4 B = 1652 B per Gaussian; bytes / median time
is the achieved rate of the whole call, not of a kernel.  No GPU: the script fails.  No time is a pass criterion of any test.

    python tools/bench_map_step.py --out profiles/r12_map_step_bench.json
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    sys.path.insert(0, p)

SIZES = (50_000, 1_000_000)
M = 16
BYTES_PER_GAUSSIAN = (3 + 3 * M + 1 + 3 + 4) * 7 * 4
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                             position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001)


def make_model(torch, P, dev, seed):
    from gaussian_splatting.scene.gaussian_model import GaussianModel

    gen = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    m = GaussianModel(3)
    m._set_params(r(P, 3), 0.5 * r(P, 1, 3), 0.1 * r(P, M - 1, 3), r(P, 1), r(P, 3) - 4.0, torch.nn.functional.normalize(r(P, 4)), dev)
    m.init_lr(1.0)
    m.training_setup(ARGS)
    return m


def make_slot(torch, P, dev, seed):
    from gsaj.keyframe_shard import bucket_numel, bucket_views

    gen = torch.Generator(device=dev).manual_seed(seed)
    bucket = 1e-3 * torch.randn(bucket_numel(P, M), generator=gen, device=dev)
    g = bucket_views(bucket, P, M)
    g["sh"] = g["sh"].view(P, M, 3)
    return g


def timed(torch, fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]


def stats(ms, P):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    med = q(0.5)
    return dict(calls=len(s), median_ms=med, p10_ms=q(0.1), p90_ms=q(0.9), min_ms=s[0],
                bytes=BYTES_PER_GAUSSIAN * P, tbytes_per_s_at_median=BYTES_PER_GAUSSIAN * P / (med * 1e-3) / 1e12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="timed calls per path and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_map_step: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), M=M, bytes_per_gaussian=BYTES_PER_GAUSSIAN, rounds=a.rounds,
                  calls_per_round=a.calls, sizes={})
    for P in a.sizes:
        ours, theirs = make_model(torch, P, dev, 1), make_model(torch, P, dev, 1)
        g = make_slot(torch, P, dev, 2)

        def new_path():
            ours.map_step(g)

        def parent_path():
            theirs.assign_bucket_gradients(g)
            theirs.optimizer.step()
            theirs.optimizer.zero_grad(set_to_none=True)

        new_path()
        parent_path()
        t_new, t_parent = [], []
        for _ in range(a.rounds):
            t_parent += timed(torch, parent_path, a.calls, a.warmup)
            t_new += timed(torch, new_path, a.calls, a.warmup)
        # the two models took the same steps from the same state: the largest difference between them, for the record
        diff = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(ours.parameters(), theirs.parameters()))
        r = dict(parent=stats(t_parent, P), map_step=stats(t_new, P), max_parameter_difference=diff)
        r["parent_over_map_step"] = r["parent"]["median_ms"] / r["map_step"]["median_ms"]
        result["sizes"][str(P)] = r
        print("P=%d: parent %.4f ms (p10 %.4f, p90 %.4f), map_step %.4f ms (p10 %.4f, p90 %.4f, %.2f TB/s), ratio %.2f, max |dp| %.3g"
              % (P, r["parent"]["median_ms"], r["parent"]["p10_ms"], r["parent"]["p90_ms"], r["map_step"]["median_ms"],
                 r["map_step"]["p10_ms"], r["map_step"]["p90_ms"], r["map_step"]["tbytes_per_s_at_median"], r["parent_over_map_step"], diff),
              flush=True)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
