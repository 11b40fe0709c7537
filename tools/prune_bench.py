"""Time of removing rows from the Gaussian map (csrc/compact.hip, gsaj.pruning, GaussianModel.prune_points) next to the
reference's statement of it.

Ours: CompactPlan(mask, n_kept=...) + apply(all tensors) -- three small kernels that plan and ONE launch that moves the kept rows of
every tensor -- timed with HIP events around `reps` back-to-back calls (the count is handed in, so nothing is read); the rows launch
alone on a standing plan, the figure its bytes per second are taken from; and the whole GaussianModel.prune_points (plan, the one
4-byte read, the launch, the optimizer's book) on the host clock, the device idle before and after each call.
The reference's statement, on the same device and the same tensors: _prune_optimizer + prune_points
(gaussian_splatting/scene/gaussian_model.py:559-597), t[valid_points_mask] for each of the six parameters, their twelve Adam moments
and the five bookkeeping vectors, on the host clock in the same way.  Both sides alternate round by round; each figure is the range
over the rounds.  The model is put back between calls outside the timed region (no copy: the old tensors are kept).
SH degree 3, Adam attached after one step, unique_kfIDs / n_obs on the device on both sides.

    python tools/prune_bench.py --out profiles/r07_prune_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prune_bench.py --trace-once device   # the kernels' own times
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prune_bench.py --trace-once torch    # launches of the statement
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
KEEP = (0.5, 0.9, 0.99)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
FIELDS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
AUX = ("xyz_gradient_accum", "denom", "max_radii2D", "unique_kfIDs", "n_obs")
COPY_TBPS = 6.29  # the float4 copy of the same device (HBM3E, 79 % of the 8 TB/s specification)


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


def host_ms(torch, fn, undo, reps, warmup):
    total = 0.0
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            total += time.perf_counter() - t0
        undo()
    return total * 1e3 / reps


def make_model(torch, P, dev):
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    gen = torch.Generator(device=dev).manual_seed(P)
    m = GaussianModel(3)
    shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 15, 3), opacity=(P, 1), scaling=(P, 3), rotation=(P, 4))
    for n in NAMES:
        setattr(m, FIELDS[n], torch.randn(shapes[n], generator=gen, device=dev).requires_grad_(True))
    m._init_aux()
    m.xyz_gradient_accum.uniform_(generator=gen)
    m.unique_kfIDs = torch.randint(0, 9, (P,), generator=gen, device=dev, dtype=torch.int32)
    m.n_obs = torch.randint(0, 6, (P,), generator=gen, device=dev, dtype=torch.int32)
    m.optimizer = torch.optim.Adam([dict(params=[getattr(m, FIELDS[n])], lr=1e-3, name=n) for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        p = getattr(m, FIELDS[n])
        p.grad = torch.randn(p.shape, generator=gen, device=dev)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    return m


def snapshot(m):
    ps = {n: getattr(m, FIELDS[n]) for n in NAMES}
    return dict(params=ps, state={n: dict(m.optimizer.state[ps[n]]) for n in NAMES}, aux={a: getattr(m, a) for a in AUX})


def restore(m, snap):
    m.optimizer.state.clear()
    for group in m.optimizer.param_groups:
        n = group["name"]
        group["params"][0] = snap["params"][n]
        m.optimizer.state[snap["params"][n]] = dict(snap["state"][n])
        setattr(m, FIELDS[n], snap["params"][n])
    for a, t in snap["aux"].items():
        setattr(m, a, t)


def torch_statement(torch, m, mask):
    """gaussian_model.py:559-597 on the overlay model's tensors."""
    valid = ~mask
    new = {}
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        st = m.optimizer.state.get(p, None)
        if st is not None:
            st["exp_avg"] = st["exp_avg"][valid]
            st["exp_avg_sq"] = st["exp_avg_sq"][valid]
            del m.optimizer.state[p]
            group["params"][0] = p.detach()[valid].requires_grad_(True)
            m.optimizer.state[group["params"][0]] = st
        else:
            group["params"][0] = p.detach()[valid].requires_grad_(True)
        new[group["name"]] = group["params"][0]
    for n in NAMES:
        setattr(m, FIELDS[n], new[n])
    m.xyz_gradient_accum = m.xyz_gradient_accum[valid]
    m.denom = m.denom[valid]
    m.max_radii2D = m.max_radii2D[valid]
    m.unique_kfIDs = m.unique_kfIDs[valid]
    m.n_obs = m.n_obs[valid]


def all_tensors(m):
    ts = [getattr(m, FIELDS[n]).detach() for n in NAMES]
    for n in NAMES:
        st = m.optimizer.state[getattr(m, FIELDS[n])]
        ts += [st["exp_avg"], st["exp_avg_sq"]]
    return ts + [getattr(m, a) for a in AUX]


def spread(v):
    v = sorted(v)
    return dict(min=round(v[0], 5), median=round(v[len(v) // 2], 5), max=round(v[-1], 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="back-to-back calls between the two HIP events")
    ap.add_argument("--host-reps", type=int, default=20, help="calls on the host clock, per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-once", choices=("device", "torch"), default=None,
                    help="a few calls at every size and keep fraction, of the kernels or of the torch statement (for a kernel trace)")
    a = ap.parse_args()
    import torch

    from gsaj.pruning import CompactPlan

    assert torch.cuda.is_available(), "prune_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    rows = []
    for P in SIZES:
        m = make_model(torch, P, dev)
        snap = snapshot(m)
        tensors = all_tensors(m)
        row_bytes = sum(t[0].numel() * t.element_size() for t in tensors)
        for frac in KEEP:
            mask = torch.rand(P, generator=torch.Generator(device=dev).manual_seed(int(frac * 100)), device=dev) >= frac  # True: remove
            n_kept = P - int(mask.sum())
            # both sides give the same model
            m.prune_points(mask)
            ours = [t.clone() for t in all_tensors(m)]
            restore(m, snap)
            torch_statement(torch, m, mask)
            assert all(torch.equal(x.view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(ours, all_tensors(m)))
            restore(m, snap)
            del ours

            plan_rows = lambda: CompactPlan(mask, remove=True, n_kept=n_kept).apply(*tensors)  # noqa: E731
            standing = CompactPlan(mask, remove=True, n_kept=n_kept)
            rows_only = lambda: standing.apply(*tensors)  # noqa: E731
            whole = lambda: m.prune_points(mask)  # noqa: E731
            theirs = lambda: torch_statement(torch, m, mask)  # noqa: E731
            undo = lambda: restore(m, snap)  # noqa: E731
            if a.trace_once:
                for _ in range(5):
                    whole() if a.trace_once == "device" else theirs()
                    undo()
                torch.cuda.synchronize()
                continue
            pr, ro, wh, th = [], [], [], []
            for _ in range(a.rounds):  # alternate, so that a drift of the machine hits all alike
                pr.append(event_ms(torch, plan_rows, a.reps, a.warmup))
                ro.append(event_ms(torch, rows_only, a.reps, a.warmup))
                wh.append(host_ms(torch, whole, undo, a.host_reps, a.warmup))
                th.append(host_ms(torch, theirs, undo, a.host_reps, a.warmup))
            algorithmic = (P + n_kept) * row_bytes + P
            ros = spread(ro)
            tbps = algorithmic / (ros["median"] * 1e-3) / 1e12
            rows.append(dict(P=P, keep_fraction=frac, n_kept=n_kept, tensors=len(tensors), row_bytes_all_tensors=row_bytes,
                             reps=a.reps, host_reps=a.host_reps, rounds=a.rounds,
                             plan_rows_device_ms=spread(pr), rows_device_ms=ros, prune_points_host_ms=spread(wh),
                             torch_statement_host_ms=spread(th),
                             speedup_prune_points_over_torch=round(spread(th)["median"] / spread(wh)["median"], 2),
                             algorithmic_bytes=algorithmic, rows_TBps=round(tbps, 3), rows_fraction_of_float4_copy=round(tbps / COPY_TBPS, 3),
                             launches=dict(ours=dict(plan_kernels=3, rows_kernels=1, host_reads=1),
                                           torch_statement=dict(boolean_index_statements=len(tensors), host_reads=len(tensors),
                                                                note="each t[mask] is a nonzero (its size is read by the host) and a gather")),
                             note="the device figures are kernels + launch gaps of back-to-back calls, output allocation included; "
                                  "rows_TBps is algorithmic_bytes over rows_device_ms"))
            del standing
    if a.trace_once:
        return
    out = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, float4_copy_TBps=COPY_TBPS, rows=rows)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
