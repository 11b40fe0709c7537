"""CPU: the NumPy restatement of the reference's densify_and_prune (tests/densify_restated.py) against the outcome recorded from
the reference's own statements (tests/golden/densify_prune_P150.npz, written by tests/golden/make_densify_prune_goldens.py); the
counter-based generator against the Random123 known answers and for the quality of its normals; the mutants the golden must
reject; the C-ABI symbols of csrc/densify_prune.hip and the argument errors that need no GPU; training_setup.  No kernel is
launched."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

import densify_restated as dr

CASES = ("aniso", "iso", "aniso_size", "iso_size", "children_pruned", "nothing", "ties")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "densify_prune_P150.npz"))


def test_fixture_is_small_and_holds_the_cases(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "densify_prune_P150.npz")) < 1024 * 1024
    assert tuple(dr.cases(golden)) == tuple(sorted(CASES))
    seen = {}
    for name in CASES:
        rec = dr.case(golden, name)
        assert rec["in_xyz"].shape == (150, 3) and rec["in_f_rest"].shape == (150, 3, 3) and rec["z"].shape == (2, 150, 3)
        assert rec["in_scaling"].shape == (150, 1 if name.startswith("iso") else 3)
        assert all(float(rec["in_step_" + n]) == 3.0 == float(rec["out_step_" + n]) for n in dr.NAMES)
        assert all(np.abs(rec["in_exp_avg_sq_" + n]).min() > 0 for n in dr.NAMES)  # three real steps: no moment is zero
        assert bool(rec["max_screen_size"]) == name.endswith("_size") or name == "children_pruned"
        out = dr.densify(rec)
        seen[name] = np.bincount(out["kind"], minlength=4)
        # the margins the fixtures promise: no decision sits where the last place of exp / sigmoid matters
        th = dr.thresholds(float(rec["max_grad"]), float(rec["min_opacity"]), float(rec["extent"]), float(rec["max_screen_size"]),
                           float(rec["percent_dense"]), 2)
        g, m, mc, o = dr.quantities(rec["in_xyz_gradient_accum"], rec["in_denom"], rec["in_scaling"], rec["in_opacity"], 2)
        far = lambda v, t, exact=False: (np.abs(v - float(t)) >= 0.99e-4 * float(t)) | (exact & (v == float(t)))  # noqa: E731
        tie = name == "ties"
        assert far(g.astype(np.float64), th["thr"], tie).all() and far(m, th["t_d"], tie & (rec["in_scaling"] == 0).all(axis=1)).all()
        assert far(m, th["t_b"]).all() and far(mc, th["t_b"]).all() and far(o, th["min_o"]).all()
    assert seen["nothing"][1:].sum() == 0 and all(seen[c][1] >= 3 and seen[c][2] >= 10 for c in CASES if c != "nothing")
    rec = dr.case(golden, "children_pruned")  # parents above 0.16 extent lose their children to the size rule
    code = dr.densify(rec)["code"]
    e = np.exp(rec["in_scaling"].astype(np.float64)).max(axis=1)
    assert ((code == 0) & (e > 0.16 * float(rec["extent"])) & (rec["in_xyz_gradient_accum"] / np.maximum(rec["in_denom"], 1e-9) > 0.2)[:, 0]).sum() >= 3
    ties = dr.case(golden, "ties")
    g = dr.quantities(ties["in_xyz_gradient_accum"], ties["in_denom"], ties["in_scaling"], ties["in_opacity"], 2)[0]
    assert (g == np.float32(0.25)).sum() >= 10 and (ties["in_scaling"] == 0).all(axis=1).sum() >= 10


@pytest.mark.parametrize("name", CASES)
def test_restated_densify_reproduces_the_reference(golden, name):
    """Every shape, every row's origin, all copied tensors, moments, zeros and ids exactly; the reference's own fp32 children within
    the bounds of the fp64 restatement (so the bounds are not narrower than fp32 arithmetic needs)."""
    rec = dr.case(golden, name)
    out = dr.densify(rec)
    want = sorted(k for k in rec if k.startswith("out_"))
    assert len(want) == 6 * 4 + 5 and all(k in out for k in want)
    n = len(out["src"])
    copied = out["kind"] < 2
    for k in want:
        assert out[k].shape == rec[k].shape, k
        if "_step_" in k:
            assert float(out[k]) == float(rec[k]) == 3.0
            continue
        assert out[k].shape[0] == n, k
        if k in ("out_xyz", "out_scaling"):
            b = out["bound_" + k[4:]]
            assert np.array_equal(dr.bits(out[k].astype(np.float32))[copied], dr.bits(rec[k])[copied]), k
            err = np.abs(out[k] - rec[k].astype(np.float64))[~copied]
            assert (err <= b[~copied]).all(), (k, float((err / b[~copied]).max()))
        else:
            assert out[k].dtype == rec[k].dtype and np.array_equal(dr.bits(out[k]), dr.bits(rec[k])), k
    assert dr.mismatches(out, rec) == []
    # origin of every row: an original carries its source's xyz bits, so the order can be read back from the golden
    assert np.array_equal(dr.bits(rec["out_rotation"]), dr.bits(rec["in_rotation"][out["src"]]))
    for a in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert not rec["out_" + a].any()
    for nme in dr.NAMES:
        assert not rec["out_exp_avg_" + nme][out["kind"] > 0].any() and not rec["out_exp_avg_sq_" + nme][out["kind"] > 0].any()


@pytest.mark.parametrize("mutant", dr.MUTANTS)
def test_golden_rejects_the_mutant(golden, mutant):
    rejected = [c for c in CASES if dr.mismatches(dr.densify(dr.case(golden, c), mutant=mutant), dr.case(golden, c))]
    assert rejected, mutant
    if mutant in ("grad_gt", "clone_lt"):
        assert rejected == ["ties"]  # only a row ON the threshold tells > from >=
    if mutant == "size_rule_always":
        assert set(rejected) >= {"aniso", "iso"}  # max_screen_size None: no size rule


def test_philox_known_answers():
    k = lambda *a: np.array(a, np.uint64)  # noqa: E731
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in dr.philox4x32(k(*ctr), k(*key))) == want
    # vectorised == one at a time; the draws of row i depend on (seed, i, n) only
    z, _ = dr.normals(40, 3, 0x123456789abcdef)
    z2, _ = dr.normals(7, 3, 0x123456789abcdef, rows=[33, 34, 35, 36, 37, 38, 39])
    assert np.array_equal(z[:, 33:], z2) and not np.array_equal(z, dr.normals(40, 3, 0x123456789abcdee)[0])


def test_restated_normals_are_normal():
    """Seed 1, 131 072 draws: mean, variance, the correlation between components and the Kolmogorov distance to Phi, each within
    5 standard errors."""
    n = 131072
    z, r = dr.normals(n // 4, 4, 1)  # 4 copies x 32768 rows x 3 components: the first 131 072 of them
    v = z.reshape(-1)[:n]
    assert np.isfinite(z).all() and (r > 0).all()
    assert abs(v.mean()) < 5 / math.sqrt(n)
    assert abs(v.var() - 1.0) < 5 * math.sqrt(2.0 / n)
    a = z.reshape(-1, 3)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert abs(np.corrcoef(a[:, i], a[:, j])[0, 1]) < 5 / math.sqrt(len(a))
    assert abs(np.corrcoef(z[0].reshape(-1), z[1].reshape(-1))[0, 1]) < 5 / math.sqrt(z[0].size)  # copies of one row
    xs = np.sort(v)
    F = 0.5 * (1.0 + np.vectorize(math.erf)(xs / math.sqrt(2.0)))
    k = np.arange(1, n + 1) / n
    D = max(np.abs(F - k).max(), np.abs(F - (k - 1.0 / n)).max())
    assert D * math.sqrt(n) < 0.8687 + 5 * 0.2603  # mean and standard deviation of the Kolmogorov distribution


def test_new_symbols_exported_and_argument_errors():
    from gsaj import _lib

    lib = _lib.load()
    assert lib.gsaj_version() >= 105
    for name in ("gsaj_densify_workspace_bytes", "gsaj_densify_plan", "gsaj_densify_counts", "gsaj_densify_rows",
                 "gsaj_densify_children", "gsaj_densify_noise"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    nb = lambda P: (P + 255) // 256  # noqa: E731
    for P in (1, 256, 257, 70001, 10 ** 6):
        for N in (1, 2, 4):
            need = 4 * ((2 + N) * nb(P) + 1 + 4)
            assert need <= lib.gsaj_densify_workspace_bytes(P, N) <= need + 512
    assert [lib.gsaj_densify_workspace_bytes(*a) for a in ((0, 2), (-3, 2), (10, 0), (10, 5), (2 ** 30, 2))] == [0] * 5

    fake = 4096  # never dereferenced: every call below is rejected before anything is launched
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)  # noqa: E731
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    c = ints(-7, -7, -7, -7)

    def plan(P=10, S=3, N=2, stages=7, accum=fake, denom=fake, n_grads=10, scaling=fake, opacity=fake, thr=0.1, code=fake, ws=fake):
        return lib.gsaj_densify_plan(P, S, N, stages, accum, denom, n_grads, scaling, opacity, thr, 0.05, 0.5, 0.3, 0, 0, code, ws, None)

    def rows(P=10, N=2, n=1, src=ptrs(fake), dst=ptrs(2 * fake), rb=ints(4), zn=ints(0), code=fake, ws=fake):
        return lib.gsaj_densify_rows(P, N, n, src, dst, rb, zn, code, ws, None)

    def children(P=10, S=3, N=2, xyz=fake, scaling=2 * fake, rot=3 * fake, code=fake, ws=fake, dx=4 * fake, ds=5 * fake):
        return lib.gsaj_densify_children(P, S, N, xyz, scaling, rot, None, 1, code, ws, dx, ds, None)

    bad = [plan(P=0), plan(P=-1), plan(S=2), plan(S=0), plan(S=4), plan(N=0), plan(N=5), plan(stages=8), plan(stages=-1),
           plan(thr=0.0), plan(thr=-1.0), plan(thr=float("nan")), plan(accum=None), plan(scaling=None), plan(opacity=None),
           plan(code=None), plan(ws=None), plan(denom=None, n_grads=11), plan(denom=None, n_grads=-1), plan(P=2 ** 30)]
    assert bad == [-1] * len(bad), bad
    assert b"gsaj_densify_plan" in lib.gsaj_last_error()
    bad = [lib.gsaj_densify_counts(None, None, c), lib.gsaj_densify_counts(fake, None, None)]
    assert bad == [-1, -1] and b"gsaj_densify_counts" in lib.gsaj_last_error() and list(c) == [-7] * 4
    bad = [rows(P=0), rows(N=0), rows(N=5), rows(n=0), rows(n=33, src=ptrs(*[fake] * 33), dst=ptrs(*[2 * fake] * 33), rb=ints(*[4] * 33), zn=ints(*[0] * 33)),
           rows(src=None), rows(dst=None), rows(rb=None), rows(zn=None), rows(code=None), rows(ws=None), rows(src=ptrs(None)),
           rows(dst=ptrs(None)), rows(rb=ints(0)), rows(rb=ints(-4)), rows(rb=ints(6)), rows(rb=ints(2)), rows(rb=ints(4100)),
           rows(n=2, src=ptrs(fake, 3 * fake), dst=ptrs(2 * fake, 3 * fake), rb=ints(4, 4), zn=ints(0, 0))]
    assert bad == [-1] * len(bad), bad
    assert b"gsaj_densify_rows" in lib.gsaj_last_error()
    bad = [children(P=0), children(S=2), children(N=0), children(N=5), children(xyz=None), children(scaling=None), children(rot=None),
           children(code=None), children(ws=None), children(dx=None), children(ds=None), children(dx=fake), children(ds=2 * fake)]
    assert bad == [-1] * len(bad), bad
    assert b"gsaj_densify_children" in lib.gsaj_last_error()
    bad = [lib.gsaj_densify_noise(0, 2, 1, fake, None), lib.gsaj_densify_noise(10, 0, 1, fake, None), lib.gsaj_densify_noise(10, 5, 1, fake, None),
           lib.gsaj_densify_noise(10, 2, 1, None, None)]
    assert bad == [-1] * len(bad) and b"gsaj_densify_noise" in lib.gsaj_last_error()


def test_plan_refuses_host_tensors_and_bad_arguments():
    import torch
    from gsaj import _lib
    from gsaj.densify import DensifyPlan, densify_noise

    z = torch.zeros(10, 1)
    for args in ((z, z, torch.zeros(10, 3), z, 0.1, 0.3, 5.0, None), (z, z, np.zeros((10, 3), np.float32), z, 0.1, 0.3, 5.0, None),
                 (z, z, None, z, 0.1, 0.3, 5.0, None)):
        with pytest.raises(_lib.GsajError):
            DensifyPlan(*args)
    with pytest.raises(_lib.GsajError):
        densify_noise(10, 2, 1, device="cpu")


def test_host_thresholds_are_rounded_once():
    from gsaj.densify import thresholds

    thr, t_d, t_b, min_o, rule, size_all = thresholds(0.0002, 0.7, 6.3, None, 0.01)
    assert (thr, t_d, t_b, min_o) == (float(np.float32(0.0002)), float(np.float32(0.01 * 6.3)), float(np.float32(0.1 * 6.3)), float(np.float32(0.7)))
    assert (rule, size_all) == (False, False)
    assert thresholds(0.1, 0.7, 6.3, 20, 0.01)[4:] == (True, False) and thresholds(0.1, 0.7, 6.3, 0, 0.01)[4:] == (False, False)
    assert thresholds(0.1, 0.7, 6.3, -1, 0.01)[4:] == (True, True)  # the reference's max_radii2D (zeros) > max_screen_size


def test_model_has_the_reference_methods():
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj.covisibility import CovisibilityWindow

    for name in ("densify_and_prune", "densify_and_clone", "densify_and_split", "training_setup"):
        assert callable(getattr(GaussianModel, name, None)), name
    assert callable(getattr(CovisibilityWindow, "densify_plan", None))
    assert GaussianModel(1).percent_dense == 0.01


def test_training_setup_on_cpu_tensors():
    """Group names, order, learning rates and eps of the reference's training_setup (:321-370)."""
    import torch
    from gaussian_splatting.scene.gaussian_model import GaussianModel

    m = GaussianModel(1)
    P = 12
    m._set_params(np.zeros((P, 3)), np.zeros((P, 1, 3)), np.zeros((P, 3, 3)), np.zeros((P, 1)), np.zeros((P, 3)), np.ones((P, 4)), "cpu")
    m.xyz_gradient_accum += 1
    m.init_lr(6.0)
    a = types.SimpleNamespace(percent_dense=0.02, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                              position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001)
    m.training_setup(a)
    assert m.percent_dense == 0.02 and isinstance(m.optimizer, torch.optim.Adam)
    want = [("xyz", 0.00016 * 6.0, m._xyz), ("f_dc", 0.0025, m._features_dc), ("f_rest", 0.0025 / 20.0, m._features_rest),
            ("opacity", 0.05, m._opacity), ("scaling", 0.001 * 6.0, m._scaling), ("rotation", 0.001, m._rotation)]
    got = [(g["name"], g["lr"], g["params"][0]) for g in m.optimizer.param_groups]
    assert [(n, lr) for n, lr, _ in got] == [(n, lr) for n, lr, _ in want]
    assert all(len(g["params"]) == 1 and g["params"][0] is w[2] and g["eps"] == 1e-15 for g, w in zip(m.optimizer.param_groups, want))
    assert tuple(m.xyz_gradient_accum.shape) == (P, 1) == tuple(m.denom.shape) and not m.xyz_gradient_accum.any() and not m.denom.any()
    assert (m.lr_init, m.lr_final, m.lr_delay_mult, m.max_steps) == (0.00016 * 6.0, 0.0000016 * 6.0, 0.01, 30000)
