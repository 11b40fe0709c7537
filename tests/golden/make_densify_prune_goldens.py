#!/usr/bin/env python3
"""Golden for the map update (build container only): runs the reference's OWN GaussianModel.densify_and_prune with everything it
calls (densify_and_clone, densify_and_split, densification_postfix, cat_tensors_to_optimizer, prune_points, _prune_optimizer and
the getters; gaussian_splatting/scene/gaussian_model.py:141-165, 559-765) and build_rotation / inverse_sigmoid of its
general_utils.py.  The `def`s are taken from the parsed files and executed in a namespace whose `torch` is a thin proxy: zeros /
ones lose their device="cuda", and normal(mean, std) returns mean + std * z with z from a seeded NumPy generator, so that the
noise can be stored.  The model holds CPU tensors of P = 150 Gaussians, SH degree 1, with a real torch.optim.Adam of the six
named groups after three steps.  Stores inputs, outputs, Adam moments and step, and z re-indexed by SOURCE row as [N,P,3].
Every decision quantity is asserted to lie at least 1e-4 (relative) from its threshold, except in the case "ties", whose marked
rows sit exactly ON the gradient threshold (0.5 / 2 = 0.25, an exact fp32 quotient) and on the clone scale (exp(0) = 1 = 0.01 * 100).

    python tests/golden/make_densify_prune_goldens.py   ->  tests/golden/densify_prune_P150.npz
"""
import ast
import os

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/gaussian_splatting/scene/gaussian_model.py"
REF_UTILS = "/root/reference/gaussian_splatting/utils/general_utils.py"
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
FIELDS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
AUX = ("xyz_gradient_accum", "denom", "max_radii2D", "unique_kfIDs", "n_obs")
METHODS = ("get_scaling", "get_opacity", "get_xyz", "densify_and_prune", "densify_and_clone", "densify_and_split",
           "densification_postfix", "cat_tensors_to_optimizer", "prune_points", "_prune_optimizer")
P, N, MARGIN = 150, 2, 1e-4


class TorchProxy:
    """torch, but on the CPU and with a recorded normal()."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.drawn = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *a, **kw):
        kw.pop("device", None)
        return torch.zeros(*a, **kw)

    def ones(self, *a, **kw):
        kw.pop("device", None)
        return torch.ones(*a, **kw)

    def normal(self, mean, std):
        z = torch.tensor(self.rng.standard_normal(tuple(mean.shape)).astype(np.float32))
        self.drawn.append(z.numpy().copy())
        return mean + std * z


def reference_class(proxy):
    ns = {"torch": proxy, "nn": nn}
    tree = ast.parse(open(REF_UTILS).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("build_rotation", "inverse_sigmoid")]
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF_UTILS, "exec"), ns)
    tree = ast.parse(open(REF).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GaussianModel"][0]
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(f.name for f in fns) == sorted(METHODS)
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF, "exec"), ns)
    return type("Bare", (), {n: ns[n] for n in METHODS})


def far(value, threshold, exact=None):
    """Every value at least MARGIN (relative) from the threshold; `exact` marks rows that may sit ON it because the value is
    exact in every implementation (an fp32 quotient; exp(0))."""
    v = np.asarray(value, np.float64)
    ok = np.abs(v - float(np.float32(threshold))) >= MARGIN * abs(float(threshold))
    if exact is not None:
        ok |= exact & (v == float(np.float32(threshold)))
    return bool(ok.all())


def make_case(isotropic, max_screen_size, max_grad, seed, scale_hi, extent=5.0, ties=False):
    rng = np.random.default_rng(seed)
    proxy = TorchProxy(seed + 1000)
    m = reference_class(proxy)()
    S = 1 if isotropic else 3
    min_opacity, percent_dense = 0.3, 0.01
    f32 = lambda shape: rng.normal(size=shape).astype(np.float32)  # noqa: E731
    init = dict(xyz=f32((P, 3)) * 2, f_dc=f32((P, 1, 3)), f_rest=f32((P, 3, 3)), opacity=f32((P, 1)) * 2,
                scaling=rng.uniform(np.log(0.0008 * extent), np.log(scale_hi), (P, S)).astype(np.float32), rotation=f32((P, 4)))
    params = {n: nn.Parameter(torch.tensor(init[n])) for n in NAMES}
    for n in NAMES:
        setattr(m, FIELDS[n], params[n])
    m.scaling_activation, m.scaling_inverse_activation, m.opacity_activation = torch.exp, torch.log, torch.sigmoid
    m.percent_dense = percent_dense
    m.optimizer = torch.optim.Adam([dict(params=[params[n]], lr=1e-4 * (k + 1), name=n) for k, n in enumerate(NAMES)], lr=0.0, eps=1e-15)
    for _ in range(3):
        for n in NAMES:
            params[n].grad = torch.tensor(f32(tuple(params[n].shape)))
        m.optimizer.step()
    m.xyz_gradient_accum = torch.tensor(rng.uniform(0, 1, (P, 1)).astype(np.float32))
    m.denom = torch.tensor(rng.integers(0, 4, (P, 1)).astype(np.float32))
    m.xyz_gradient_accum[m.denom == 0] = 0.0  # never seen: 0 / 0, the NaN the reference zeroes
    tie_g = tie_m = np.zeros(P, bool)
    if ties:  # rows ON a threshold where that is exact everywhere: g = 0.5 / 2 = max_grad, and exp(0) = 1 = percent_dense * extent
        assert max_grad == 0.25 and percent_dense * extent == 1.0
        tie_g, tie_m = np.arange(P) % 9 == 1, np.arange(P) % 9 == 4
        with torch.no_grad():
            m.xyz_gradient_accum[torch.tensor(tie_g)] = 0.5
            m.denom[torch.tensor(tie_g)] = 2.0
            params["scaling"][torch.tensor(tie_m)] = 0.0
            m.xyz_gradient_accum[torch.tensor(tie_m)] = 0.9
            m.denom[torch.tensor(tie_m)] = 1.0
    m.max_radii2D = torch.tensor(rng.integers(0, 30, (P,)).astype(np.float32))
    m.unique_kfIDs = torch.tensor(rng.integers(0, 9, (P,)).astype(np.int32))
    m.n_obs = torch.tensor(rng.integers(0, 6, (P,)).astype(np.int32))

    rec = dict(max_grad=np.float64(max_grad), min_opacity=np.float64(min_opacity), extent=np.float64(extent),
               max_screen_size=np.float64(max_screen_size or 0.0), percent_dense=np.float64(percent_dense))

    def snapshot(tag):
        for n in NAMES:
            p = getattr(m, FIELDS[n])
            st = m.optimizer.state[p]
            rec["%s_%s" % (tag, n)] = p.detach().numpy().copy()
            rec["%s_exp_avg_%s" % (tag, n)] = st["exp_avg"].numpy().copy()
            rec["%s_exp_avg_sq_%s" % (tag, n)] = st["exp_avg_sq"].numpy().copy()
            rec["%s_step_%s" % (tag, n)] = np.asarray(float(st["step"]))
            assert m.optimizer.param_groups[NAMES.index(n)]["params"][0] is p
        for a in AUX:
            rec["%s_%s" % (tag, a)] = getattr(m, a).numpy().copy()

    snapshot("in")
    # the decision quantities, as the reference forms them, and their distance from the thresholds
    with torch.no_grad():
        g = (m.xyz_gradient_accum / m.denom).squeeze(1)
        g[g.isnan()] = 0.0
        big = m.get_scaling.max(dim=1).values
        child = torch.exp(torch.log(m.get_scaling / (0.8 * N))).max(dim=1).values
        o = m.get_opacity.squeeze(1)
        sel = ((g >= max_grad) & (big > percent_dense * extent)).numpy()
        n_clone = int(((g >= max_grad) & (big <= percent_dense * extent)).sum())
    assert far(g, max_grad, tie_g) and far(big, percent_dense * extent, tie_m) and far(big, 0.1 * extent) and far(child, 0.1 * extent) and far(o, min_opacity)

    with torch.no_grad():
        m.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)  # gaussian_model.py:750-765
    snapshot("out")
    z = np.zeros((N, P, 3), np.float32)
    assert len(proxy.drawn) == 1 and proxy.drawn[0].shape == (N * int(sel.sum()), 3)
    z[:, sel] = proxy.drawn[0].reshape(N, int(sel.sum()), 3)  # repeat(N, 1): copy-major
    rec["z"] = z
    assert all(float(rec["out_step_" + n]) == 3.0 for n in NAMES)
    children_pruned = bool(((child.numpy() > np.float32(0.1 * extent)) & sel).any()) and bool(max_screen_size)
    if ties:
        assert (g.numpy()[tie_g] == np.float32(max_grad)).all() and (big.numpy()[tie_m] == 1.0).all() and not sel[tie_m].any()
    return rec, int(sel.sum()), n_clone, children_pruned


def main():
    out, seen = {}, {}
    for case, iso, size, thr, seed, hi in (("aniso", False, None, 0.25, 41, 1.5), ("iso", True, None, 0.25, 42, 1.5),
                                           ("aniso_size", False, 20, 0.25, 43, 1.5), ("iso_size", True, 20, 0.25, 44, 1.5),
                                           ("children_pruned", False, 20, 0.2, 45, 3.0), ("nothing", False, None, 10.0, 46, 1.5), ("ties", False, None, 0.25, 47, 30.0)):
        rec, n_split, n_clone, kids_gone = make_case(iso, size, thr, seed, hi, **(dict(extent=100.0, ties=True) if case == "ties" else {}))
        seen[case] = (n_split, n_clone, kids_gone, rec["out_xyz"].shape[0])
        for k, v in rec.items():
            out["%s/%s" % (case, k)] = v
    print(seen)
    assert seen["nothing"][:2] == (0, 0) and seen["children_pruned"][2] and seen["aniso_size"][2] and seen["iso_size"][2]
    assert all(seen[c][0] > 5 and seen[c][1] > 3 for c in seen if c != "nothing")
    path = os.path.join(HERE, "densify_prune_P150.npz")
    np.savez_compressed(path, **out)
    print("ok", os.path.getsize(path))


if __name__ == "__main__":
    main()
