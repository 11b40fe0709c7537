"""Device time of the tracking gradient mask (csrc/frame.hip) and its parity figures.

Timing: HIP events around `reps` back-to-back calls after a warm-up, at 640x480, 1200x680 (Replica's frames) and 1280x720, both
modes.  For context only, the same steps as plain torch ops on the same device (utils.slam_utils.image_gradient /
image_gradient_mask, then the global median form, or the loop over 32 x 32 blocks with a median and two masked assignments each)
are timed the same way in the same process, alternating with the kernels round by round; each figure is the range over the
rounds.  Nothing depends on the ratio.

Parity: the worst ratios of the device against the NumPy restatement (tests/grad_mask_restated.py) at the sizes of
tests/test_gpu_grad_mask.py: intensity error over its bound, the margin |I - t| of differing mask pixels over its bound.

    python tools/grad_mask_bench.py --reps 200 --out profiles/grad_mask.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/grad_mask_bench.py --trace-once device   # launches per call
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/grad_mask_bench.py --trace-once torch
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

# launches per call, from the call sequences in csrc/frame.hip / csrc/seed.hip (checked against a kernel trace: --trace-once)
LAUNCHES = {False: "intensity + 1 memset + 8 kernels (4 x histogram + pick) + threshold: 10 kernels", True: "1 kernel"}
PARITY_SIZES = ((64, 96), (68, 100), (97, 131), (100, 170), (480, 640), (720, 1280))  # H, W


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


def torch_grad_mask(torch, image, edge_threshold, blocks):
    """The reference's steps as torch ops on the image's device (timing baseline only)."""
    from utils.slam_utils import image_gradient, image_gradient_mask

    gray = image.mean(dim=0, keepdim=True)
    gv, gh = image_gradient(gray)
    mv, mh = image_gradient_mask(gray)
    inten = torch.sqrt((gv * mv) ** 2 + (gh * mh) ** 2)
    if not blocks:
        return inten > inten.median() * edge_threshold
    _, h, w = image.shape
    bh, bw = int(h / 32), int(w / 32)
    for r in range(32):
        for c in range(32):
            blk = inten[:, r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
            t = blk.median() * edge_threshold
            blk[blk > t] = 1
            blk[blk <= t] = 0
    return inten


def spread(v):
    v = sorted(v)
    return dict(min=round(v[0], 5), median=round(v[len(v) // 2], 5), max=round(v[-1], 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--torch-block-reps", type=int, default=5, help="calls per round of the torch 32 x 32 block loop (thousands of launches each)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-once", choices=("device", "torch"), default=None,
                    help="one call of each mode at 640x480, of the kernels or of the torch ops (for a kernel trace)")
    a = ap.parse_args()
    import torch

    import grad_mask_restated as gr
    from gsaj.grad_mask import GradMask

    assert torch.cuda.is_available(), "grad_mask_bench needs the GPU: there is no CPU path to time"
    dev = "cuda:0"
    if a.trace_once:
        img = torch.as_tensor(gr.make_scene("noise", 480, 640), device=dev)
        op = GradMask(640, 480, dev)
        for blocks in (False, True):
            if a.trace_once == "device":
                op(img, 1.1, blocks=blocks)
            else:
                torch_grad_mask(torch, img, 1.1, blocks)
        torch.cuda.synchronize()
        return

    rows = []
    for W, H in ((640, 480), (1200, 680), (1280, 720)):
        img = torch.as_tensor(gr.make_scene("noise", H, W), device=dev)
        op = GradMask(W, H, dev)
        for blocks in (False, True):
            ours, theirs = [], []
            treps = a.torch_block_reps if blocks else a.reps
            for _ in range(a.rounds):  # alternate, so that a drift of the box hits both alike
                ours.append(timed(torch, lambda: op(img, 1.1, blocks=blocks), a.reps, a.warmup))
                theirs.append(timed(torch, lambda: torch_grad_mask(torch, img, 1.1, blocks), treps, 2 if blocks else a.warmup))
            rows.append(dict(what="grad_mask", mode="blocks" if blocks else "global", W=W, H=H, ms=spread(ours), torch_ops_ms=spread(theirs),
                             reps=a.reps, torch_reps=treps, rounds=a.rounds, launches=LAUNCHES[blocks]))
        rows.append(dict(what="grad_intensity", W=W, H=H, launches="1 kernel",
                         ms=spread([timed(torch, lambda: op.intensity(img), a.reps, a.warmup) for _ in range(a.rounds)]),
                         note="includes the allocation of the output tensor"))

    parity = []
    for H, W in PARITY_SIZES:
        scene = gr.make_scene("noise", H, W)
        img = torch.as_tensor(scene, device=dev)
        op = GradMask(W, H, dev)
        I_dev = op.intensity(img)[0].cpu().numpy()
        for blocks in (False, True):
            for thr in (1.1, 4.0):
                want = gr.grad_mask(scene, thr, blocks)
                op(img, thr, blocks=blocks)
                got = op.reference_tensor()[0].cpu().numpy().astype(np.float32)
                vis = want["visited"]
                differ = (got != want["value"].astype(np.float32)) & vis
                margin = np.abs(want["I"].astype(np.float64) - want["t"].astype(np.float64))
                parity.append(dict(
                    H=H, W=W, mode="blocks" if blocks else "global", edge_threshold=thr,
                    intensity_err_over_bound=float(np.abs(I_dev.astype(np.float64) - want["I"]).max() / gr.tolerance(0.0, want["max_gray"])),
                    intensities_not_bit_equal=int((I_dev != want["I"]).sum()), mask_pixels_differing=int(differ.sum()),
                    worst_margin_over_bound=float((margin[differ] / gr.tolerance(thr, want["max_gray"])).max()) if differ.any() else 0.0,
                    strip_err_over_bound=float(np.abs(got[~vis].astype(np.float64) - want["value"][~vis]).max()
                                               / gr.tolerance(0.0, want["max_gray"])) if (~vis).any() else 0.0))
    out = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, rows=rows, parity_against_restatement=parity)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
