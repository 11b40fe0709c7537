"""Time of the map update (csrc/densify_prune.hip, gsaj.densify, GaussianModel.densify_and_prune) next to the reference's
statement of it.

Ours, with HIP events around `reps` back-to-back calls: the plan (classification, scan, totals; the counts are handed in, so nothing
is read), the rows launch alone on a standing plan (the figure its bytes per second are taken from: 6 parameters, 12 Adam moments,
unique_kfIDs and n_obs), and the children launch alone; and the whole GaussianModel.densify_and_prune (plan, the one 16-byte read,
the two launches, three torch.zeros, the optimizer's book) on the host clock, the device idle before and after each call.
The reference's statement, on the same device and the same tensors: densify_and_clone, densify_and_split and the final
prune_points (gaussian_splatting/scene/gaussian_model.py:599-765) in torch, the normal draws taken from a tensor, on the host
clock in the same way.  Both sides alternate round by round; each figure is the range over the rounds.  The model is put back
between calls outside the timed region.  SH degree 3, Adam attached after one step, unique_kfIDs / n_obs on the device on both
sides; about 5 % of the rows are cloned, 5 % split and 2 % pruned.  No time is a pass criterion.

    python tools/densify_bench.py --out profiles/r08_densify_bench.json
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
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
FIELDS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
AUX = ("xyz_gradient_accum", "denom", "max_radii2D", "unique_kfIDs", "n_obs")
MAX_GRAD, MIN_OPACITY, EXTENT, SCREEN = 0.25, 0.3, 5.0, 20   # t_dense = 0.05, t_big = 0.5
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
    """5 % of the rows over the gradient threshold with small scales, 5 % with large ones, 2 % faint."""
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    gen = torch.Generator(device=dev).manual_seed(P)
    u = lambda lo, hi, shape: torch.rand(shape, generator=gen, device=dev) * (hi - lo) + lo  # noqa: E731
    m = GaussianModel(3)
    shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 15, 3), rotation=(P, 4))
    for n, s in shapes.items():
        setattr(m, FIELDS[n], torch.randn(s, generator=gen, device=dev).requires_grad_(True))
    cls = torch.rand(P, generator=gen, device=dev)
    small = cls < 0.5
    top = torch.where(small, u(0.004, 0.04, (P,)), u(0.07, 0.3, (P,)))
    m._scaling = torch.log(top[:, None] * torch.cat((torch.ones(P, 1, device=dev), u(0.2, 1.0, (P, 2))), dim=1)).requires_grad_(True)  # max = top
    m._opacity = torch.where(torch.rand(P, 1, generator=gen, device=dev) < 0.02, u(-3.0, -1.2, (P, 1)), u(-0.4, 3.0, (P, 1))).requires_grad_(True)
    m._init_aux()
    m.denom = torch.randint(1, 5, (P, 1), generator=gen, device=dev).float()
    m.xyz_gradient_accum = torch.where(torch.rand(P, 1, generator=gen, device=dev) < 0.1, u(0.3, 0.9, (P, 1)), u(0.0, 0.2, (P, 1))) * m.denom
    m.unique_kfIDs = torch.randint(0, 9, (P,), generator=gen, device=dev, dtype=torch.int32)
    m.n_obs = torch.randint(0, 6, (P,), generator=gen, device=dev, dtype=torch.int32)
    m.optimizer = torch.optim.Adam([dict(params=[getattr(m, FIELDS[n])], lr=1e-6, name=n) for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        p = getattr(m, FIELDS[n])
        p.grad = torch.randn(p.shape, generator=gen, device=dev)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    return m


def snapshot(m):
    ps = {n: getattr(m, FIELDS[n]) for n in NAMES}
    return dict(params=ps, state={n: dict(m.optimizer.state[ps[n]]) for n in NAMES}, aux={a: getattr(m, a) for a in AUX}, seed=m.seed)


def restore(m, snap):
    m.optimizer.state.clear()
    for group in m.optimizer.param_groups:
        n = group["name"]
        group["params"][0] = snap["params"][n]
        m.optimizer.state[snap["params"][n]] = dict(snap["state"][n])
        setattr(m, FIELDS[n], snap["params"][n])
    for a, t in snap["aux"].items():
        setattr(m, a, t)
    m.seed = snap["seed"]


def table(m):
    """What the rows launch moves: (tensors, modes)."""
    ts, modes = [getattr(m, FIELDS[n]).detach() for n in NAMES], ["parent"] * 6
    for n in NAMES:
        st = m.optimizer.state[getattr(m, FIELDS[n])]
        ts += [st["exp_avg"], st["exp_avg_sq"]]
        modes += ["zeros", "zeros"]
    return ts + [m.unique_kfIDs, m.n_obs], modes + ["parent", "parent"]


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
    ap.add_argument("--reps", type=int, default=100, help="back-to-back calls between the two HIP events")
    ap.add_argument("--host-reps", type=int, default=10, help="calls on the host clock, per round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from gsaj.densify import DensifyPlan
    from test_gpu_densify_prune import torch_densify_and_prune  # the reference's statement in torch, as the tests compare against

    assert torch.cuda.is_available(), "densify_bench needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    rows = []
    for P in SIZES:
        m = make_model(torch, P, dev)
        snap = snapshot(m)
        noise = torch.randn(2, P, 3, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        args = (MAX_GRAD, MIN_OPACITY, EXTENT, SCREEN)
        # both sides give the same model: everything copied bit for bit, the children to fp32 rounding
        plan = m.densify_and_prune(*args, noise=noise)
        counts = plan.counts
        kinds = torch.zeros(counts[3], dtype=torch.bool, device=dev)
        kinds[counts[0] + counts[1]:] = True  # the children
        ours = [t.clone() for t in all_tensors(m)]
        restore(m, snap)
        torch_densify_and_prune(m, *args, noise)
        for k, (x, y) in enumerate(zip(ours, all_tensors(m))):
            assert x.shape == y.shape, k
            if k in (0, 4):  # xyz, scaling: the children are computed
                assert torch.equal(x[~kinds], y[~kinds]) and torch.allclose(x[kinds], y[kinds], rtol=1e-5, atol=1e-5), k
            else:
                assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), k
        restore(m, snap)
        del ours

        tensors, modes = table(m)
        row_bytes = sum(t[0].numel() * t.element_size() for t in tensors)
        mk_plan = lambda: DensifyPlan(m.xyz_gradient_accum, m.denom, m._scaling, m._opacity, *args, counts=counts)  # noqa: E731
        standing = mk_plan()
        new_xyz, new_scaling = standing.apply([tensors[0], tensors[4]])
        rows_only = lambda: standing.apply(tensors, new_rows=modes)  # noqa: E731
        children = lambda: standing.children(tensors[0], tensors[4], tensors[5], new_xyz, new_scaling, seed=1)  # noqa: E731
        whole = lambda: m.densify_and_prune(*args, seed=1)  # noqa: E731
        theirs = lambda: torch_densify_and_prune(m, *args, noise)  # noqa: E731
        undo = lambda: restore(m, snap)  # noqa: E731
        pl, ro, ch, wh, th = [], [], [], [], []
        for _ in range(a.rounds):  # alternate, so that a drift of the machine hits all alike
            pl.append(event_ms(torch, mk_plan, a.reps, a.warmup))
            ro.append(event_ms(torch, rows_only, a.reps, a.warmup))
            ch.append(event_ms(torch, children, a.reps, a.warmup))
            wh.append(host_ms(torch, whole, undo, a.host_reps, a.warmup))
            th.append(host_ms(torch, theirs, undo, a.host_reps, a.warmup))
        algorithmic = P * (row_bytes + 9) + counts[3] * row_bytes
        ros = spread(ro)
        tbps = algorithmic / (ros["median"] * 1e-3) / 1e12
        rows.append(dict(P=P, counts=dict(originals=counts[0], clones=counts[1], children_per_copy=counts[2], P_out=counts[3]),
                         pruned=P - counts[0] - counts[2], tensors=len(tensors), row_bytes_all_tensors=row_bytes,
                         reps=a.reps, host_reps=a.host_reps, rounds=a.rounds,
                         plan_device_ms=spread(pl), rows_device_ms=ros, children_device_ms=spread(ch),
                         densify_and_prune_host_ms=spread(wh), torch_statement_host_ms=spread(th),
                         speedup_densify_and_prune_over_torch=round(spread(th)["median"] / spread(wh)["median"], 2),
                         algorithmic_bytes=algorithmic, rows_TBps=round(tbps, 3), rows_fraction_of_float4_copy=round(tbps / COPY_TBPS, 3),
                         launches=dict(ours=dict(plan_kernels=3, rows_kernels=1, children_kernels=1, zeros=3, host_reads=1),
                                       torch_statement=dict(note="two appends (torch.cat of 6 parameters and 12 moments each), two prunes "
                                                                 "(23 boolean-index statements each, a nonzero with a host read and a gather "
                                                                 "per statement), about 20 boolean-mask gathers to select")),
                         note="the device figures are kernels + launch gaps of back-to-back calls, output allocation included; "
                              "rows_TBps is algorithmic_bytes over rows_device_ms; the torch statement takes its normal draws from a tensor"))
        del standing
    out = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, float4_copy_TBps=COPY_TBPS, rows=rows)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
