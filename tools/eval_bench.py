"""Time of the per-frame rendering metrics: gsaj.evaluation.FrameEvaluator.add (csrc/eval.hip: three launches, nothing read back)
next to the reference's statement written in torch on the same device (utils/eval_utils.py:141-160, LPIPS left out),

    image = clamp(render, 0, 1); mask = gt > 0
    psnr(image[mask][None], gt[mask][None]).item(); ssim(image[None], gt[None]).item()

with gsaj.ssim in that statement, so that only the new part differs.  At 640 x 480 and 1200 x 680, C = 3.  Two clocks:
  device   each call between two HIP events on the stream, 200 calls per path after a warm-up: median, 10th / 90th percentile, minimum.
           A call's time includes the gaps the host leaves between its kernels (and, for the statement, its host reads).
  host     eval_rendering's per-frame metric part: wall time of `frames` consecutive frames divided by `frames`, the evaluator's one
           rows() read included for the device path; the statement reads twice per frame by itself.
Launches are listed, not traced: the device path is k_eval_pixels, k_ssim_fwd, k_eval_finalize; the statement is one launch or more
per tensor operation (OPS below).  Host reads are the synchronising calls torch reports in its sync debug mode over one call.
No GPU: the script fails.  No time is a pass criterion of any test.

    python tools/eval_bench.py --out profiles/r13_eval_bench.json
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd")):
    sys.path.insert(0, p)

SIZES = ((640, 480), (1200, 680))
# the statement's tensor operations, each at least one launch: clamp, gt > 0, two boolean-index gathers (nonzero + index each),
# two unsqueeze (none), sub, pow, mean, sqrt, reciprocal-divide, log10, mul, the SSIM kernel
OPS = dict(device_path=["k_eval_pixels", "k_ssim_fwd", "k_eval_finalize"],
           statement=["clamp", "gt", "nonzero", "index", "nonzero", "index", "sub", "pow", "mean", "sqrt", "rdiv", "log10", "mul", "k_ssim_fwd"])


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


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return dict(calls=len(s), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=s[0])


def host_reads(torch, fn):
    """Synchronising calls of one fn(), as torch's sync debug mode reports them; None where the mode is not available."""
    try:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return len([x for x in w if "synchroniz" in str(x.message)])
    except Exception:  # noqa: BLE001
        return None
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=50, help="frames per host-clock measurement")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("eval_bench: no GPU; a time is measured on the device or not at all")
    from gaussian_splatting.utils.image_utils import psnr
    from gsaj import ssim as gssim
    from gsaj.evaluation import FrameEvaluator

    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), C=3, calls=a.calls, frames_per_host_measurement=a.frames, launches=OPS,
                  launch_count=dict(device_path=len(OPS["device_path"]), statement_at_least=len(OPS["statement"])), sizes={})
    for W, H in SIZES:
        gen = torch.Generator(device=dev).manual_seed(W)
        gt = torch.rand(3, H, W, generator=gen, device=dev)
        gt[torch.rand(3, H, W, generator=gen, device=dev) < 0.1] = 0.0
        render = gt + 0.2 * torch.randn(3, H, W, generator=gen, device=dev)
        ev = FrameEvaluator(W, H, dev, capacity=4096)
        got = {}

        def device_path():
            ev.add(render, gt)

        def statement():
            image = torch.clamp(render, 0.0, 1.0)
            mask = gt > 0
            got["psnr"] = psnr(image[mask].unsqueeze(0), gt[mask].unsqueeze(0)).item()
            got["ssim"] = gssim.ssim(image.unsqueeze(0), gt.unsqueeze(0)).item()

        r = dict(device_path=stats(timed(torch, device_path, a.calls, a.warmup)), statement=stats(timed(torch, statement, a.calls, a.warmup)))
        r["device_path"]["host_reads_per_frame"] = host_reads(torch, device_path)
        r["statement"]["host_reads_per_frame"] = host_reads(torch, statement)
        for name, fn, tail in (("device_path", device_path, ev.rows), ("statement", statement, lambda: None)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.frames):
                fn()
            tail()
            torch.cuda.synchronize()
            r[name]["host_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / a.frames
        t, _ = ev.rows()
        r["psnr"] = dict(device_path=float(t[-1, 0]), statement=got["psnr"])
        r["ssim"] = dict(device_path=float(t[-1, 1]), statement=got["ssim"])
        r["statement_over_device_path"] = dict(device=r["statement"]["median_ms"] / r["device_path"]["median_ms"],
                                               host=r["statement"]["host_ms_per_frame"] / r["device_path"]["host_ms_per_frame"])
        result["sizes"]["%dx%d" % (W, H)] = r
        print("%dx%d: add %.4f ms (p10 %.4f, p90 %.4f), statement %.4f ms (p10 %.4f, p90 %.4f); host per frame %.4f / %.4f ms; host reads %s / %s"
              % (W, H, r["device_path"]["median_ms"], r["device_path"]["p10_ms"], r["device_path"]["p90_ms"], r["statement"]["median_ms"],
                 r["statement"]["p10_ms"], r["statement"]["p90_ms"], r["device_path"]["host_ms_per_frame"], r["statement"]["host_ms_per_frame"],
                 r["device_path"]["host_reads_per_frame"], r["statement"]["host_reads_per_frame"]), flush=True)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
