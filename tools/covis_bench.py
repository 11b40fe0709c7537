"""Time of the per-frame covisibility question (csrc/covis.hip, gsaj.covisibility) next to the reference's statement of it.

Ours: CovisibilityWindow.query(cur_n_touched) -- one memset of 65 integers and one kernel that reads 8 bytes per Gaussian -- timed
with HIP events around `reps` back-to-back calls; and CovisibilityWindow.counts(...), the same plus the one device-to-host copy of
the 65 integers, timed with the host clock (every call ends in that copy, so the host waits for the device each time).
The reference's statement, on the same device and the same data: curr_visibility = (n_touched > 0).long(), then for the last
keyframe logical_or / logical_and + count_nonzero and the float ratio compared on the host (FrontEnd.is_keyframe,
utils/slam_frontend.py:218-225), and for every window entry from the third on logical_and + three count_nonzero, the Python
min() of two device scalars and the ratio compared on the host (FrontEnd.add_to_window, :236-255).  Timed with the host clock;
both sides alternate round by round, each figure is the range over the rounds.  The counts of both sides are compared first.

    python tools/covis_bench.py --reps 200 --out profiles/covis_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/covis_bench.py --trace-once device   # the kernel's own time
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/covis_bench.py --trace-once torch    # launches of the statement
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-slam-analytica_jacobian_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SIZES = (50_000, 1_000_000)
K = 8
N_DONT_TOUCH = 2


def event_ms(torch, fn, reps, warmup):
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


def host_ms(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def torch_statement(torch, cur_n_touched, occ, window, kf_overlap=0.9, cut_off=0.4):
    """The visibility part of one keyframe decision as the reference states it (the window is full: no window_size override)."""
    cur = (cur_n_touched > 0).long()
    last = occ[window[0]]
    union = torch.logical_or(cur, last).count_nonzero()
    intersection = torch.logical_and(cur, last).count_nonzero()
    decisions = [bool(intersection / union < kf_overlap)]
    new_window = [None] + window
    for i in range(N_DONT_TOUCH, len(new_window)):
        v = occ[new_window[i]]
        intersection = torch.logical_and(cur, v).count_nonzero()
        denom = min(cur.count_nonzero(), v.count_nonzero())
        decisions.append(bool(intersection / denom <= cut_off))
    return decisions


def spread(v):
    v = sorted(v)
    return dict(min=round(v[0], 5), median=round(v[len(v) // 2], 5), max=round(v[-1], 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-once", choices=("device", "torch"), default=None,
                    help="a few calls at every size, of the kernels or of the torch statement (for a kernel trace)")
    a = ap.parse_args()
    import torch

    import covis_restated as cr
    from gsaj.covisibility import CovisibilityWindow

    assert torch.cuda.is_available(), "covis_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    window = list(range(K * 3, 0, -3))  # newest first
    rows = []
    for P in SIZES:
        nt = torch.as_tensor(cr.make_case(P, K + 1, 0.5, 1), device=dev)
        cur = nt[K].contiguous()
        cw = CovisibilityWindow(P, dev)
        cw.set_window(window, nt[:K].contiguous())
        occ = {kf: (nt[k] > 0).long() for k, kf in enumerate(window)}
        ours = lambda: cw.query(cur_n_touched=cur)          # noqa: E731
        ours_read = lambda: cw.counts(cur_n_touched=cur)    # noqa: E731
        theirs = lambda: torch_statement(torch, cur, occ, window)  # noqa: E731
        per_kf, nq = ours_read()
        assert nq == int((cur > 0).sum())
        for kf, v in occ.items():
            assert per_kf[kf] == (int(((cur > 0) & (v > 0)).sum()), int(v.sum())), kf
        if a.trace_once:
            for _ in range(10):
                ours() if a.trace_once == "device" else theirs()
            torch.cuda.synchronize()
            continue
        q, c, t = [], [], []
        for _ in range(a.rounds):  # alternate, so that a drift of the machine hits all alike
            q.append(event_ms(torch, ours, a.reps, a.warmup))
            c.append(host_ms(torch, ours_read, a.reps, a.warmup))
            t.append(host_ms(torch, theirs, a.reps, a.warmup))
        qs = spread(q)
        rows.append(dict(P=P, K=K, reps=a.reps, rounds=a.rounds, query_device_ms=qs, counts_host_ms=spread(c), torch_statement_host_ms=spread(t),
                         bytes_read_per_query=8 * P,
                         query_GBps_over_device_ms=round(8 * P / (qs["median"] * 1e-3) / 1e9, 1),
                         note="query_device_ms is memset + kernel + launch gaps of back-to-back calls; the kernel's own time is in the trace",
                         window_bytes_kept=dict(words=4 * P, reference_int64_vectors=8 * K * P)))
    if a.trace_once:
        return
    out = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, rows=rows)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
