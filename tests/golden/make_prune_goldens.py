#!/usr/bin/env python3
"""Golden for map pruning (build container only): runs the reference's OWN GaussianModel.prune_points and _prune_optimizer
(gaussian_splatting/scene/gaussian_model.py:559-597; the methods' `def`s are taken from the parsed file and bound to a bare
object holding CPU tensors -- the module itself needs open3d / plyfile / simple_knn to import) on a model of P = 120 Gaussians,
SH degree 1, with a torch.optim.Adam of the six named groups after three steps on seeded random gradients.  Two cases: an
anisotropic model (scaling [P,3]) and an isotropic one (scaling [P,1]).  Stores inputs, outputs and the optimizer's step only.

    python tests/golden/make_prune_goldens.py   ->  tests/golden/prune_P120.npz
"""
import ast
import os

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/gaussian_splatting/scene/gaussian_model.py"
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
FIELDS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
AUX = ("xyz_gradient_accum", "denom", "max_radii2D", "unique_kfIDs", "n_obs")
P = 120


def reference_methods(*names):
    tree = ast.parse(open(REF).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GaussianModel"][0]
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF, "exec"), ns)
    return type("Bare", (), {n: ns[n] for n in names})


def shapes(isotropic):
    return dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 3, 3), opacity=(P, 1), scaling=(P, 1 if isotropic else 3), rotation=(P, 4))


def make_case(Bare, isotropic, seed):
    rng = np.random.default_rng(seed)
    f32 = lambda shape: torch.tensor(rng.normal(size=shape).astype(np.float32))  # noqa: E731
    m = Bare()
    params = {n: nn.Parameter(f32(s)) for n, s in shapes(isotropic).items()}
    for n in NAMES:
        setattr(m, FIELDS[n], params[n])
    m.optimizer = torch.optim.Adam([dict(params=[params[n]], lr=1e-3 * (k + 1), name=n) for k, n in enumerate(NAMES)], lr=0.0, eps=1e-15)
    for _ in range(3):
        for n in NAMES:
            params[n].grad = f32(params[n].shape)
        m.optimizer.step()
    m.xyz_gradient_accum = torch.tensor(rng.uniform(0, 1, (P, 1)).astype(np.float32))
    m.denom = torch.tensor(rng.integers(0, 5, (P, 1)).astype(np.float32))
    m.max_radii2D = torch.tensor(rng.integers(0, 30, (P,)).astype(np.float32))
    m.unique_kfIDs = torch.tensor(rng.integers(0, 9, (P,)).astype(np.int32))
    m.n_obs = torch.tensor(rng.integers(0, 6, (P,)).astype(np.int32))
    mask = rng.uniform(size=P) < 0.3
    mask[0] = mask[P - 1] = True
    mask[1] = False

    rec = {"mask": mask}

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
    m.prune_points(torch.tensor(mask))  # gaussian_model.py:581-597, which calls _prune_optimizer :559-579
    snapshot("out")
    assert rec["out_xyz"].shape[0] == int((~mask).sum()) and 0.6 * P < rec["out_xyz"].shape[0] < 0.8 * P
    return rec


def main():
    Bare = reference_methods("prune_points", "_prune_optimizer")
    out = {}
    for case, iso, seed in (("aniso", False, 31), ("iso", True, 32)):
        for k, v in make_case(Bare, iso, seed).items():
            out["%s/%s" % (case, k)] = v
    path = os.path.join(HERE, "prune_P120.npz")
    np.savez_compressed(path, **out)
    print("ok", os.path.getsize(path))


if __name__ == "__main__":
    main()
