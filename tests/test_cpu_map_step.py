"""The map step without a GPU: tests/map_step_restated.py is pinned to the reference's semantics (CPU autograd through the
reference's activations, torch.optim.Adam(lr=0.0, eps=...) and a restated replace_tensor_to_optimizer, one step from a given
state), its comparator rejects every mutant, the learning-rate schedule returns the reference's recorded numbers, and the host
logic of GaussianModel.map_step / reset_opacity* is checked with the launch replaced by the restatement.  No kernel runs here:
tests/test_gpu_map_step.py checks the device against the same restatement."""
import os
import types

import numpy as np
import pytest
import torch

import map_step_restated as R
from map_step_restated import NAMES, RESET_ALL, RESET_KEEP_VISIBLE, RESET_NONVISIBLE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = R.CASES()
IDS = ["P%d_M%d_S%d_t%d_f%d_K%d_%s" % (c["P"], c["M"], c["S"], c["t"], c["flags"], c["K_vis"], "".join(map(str, c["skip"]))) for c in CASES]


def _inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def _logit32(x):
    """log(x / (1 - x)) with the quotient in fp32 and the logarithm correctly rounded to fp32; torch's own fp32 log is within an ulp."""
    x = np.float32(x)
    v = float(np.float32(np.log(np.float64(x / (np.float32(1) - x)))))
    assert abs(v - float(_inverse_sigmoid(torch.ones(1) * float(x)))) <= 2.0 ** -23 * abs(v)
    return v


def _replace_tensor_to_optimizer(opt, tensor, name):
    """What the reference's replace_tensor_to_optimizer (gaussian_model.py:544-557) does to the group `name`."""
    for group in opt.param_groups:
        if group["name"] == name:
            old = group["params"][0]
            state = opt.state.get(old, None)
            state["exp_avg"] = torch.zeros_like(tensor)
            state["exp_avg_sq"] = torch.zeros_like(tensor)
            del opt.state[old]
            group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
            opt.state[group["params"][0]] = state
            return group["params"][0]


def _torch_reference(c):
    """One iteration's tail as the reference runs it, on CPU fp32 tensors: backward through the activations with the bucket
    gradients upstream, then the opacity reset, then optimizer.step().  Returns (the 18 tensors, the six steps, reset_value)."""
    t = lambda k: torch.from_numpy(c[k].copy())  # noqa: E731
    prm = {n: t(n).requires_grad_(True) for n in NAMES}
    groups = [{"params": [prm[n]], "lr": c["lr"][i], "name": n} for i, n in enumerate(NAMES)]
    opt = torch.optim.Adam(groups, lr=0.0, eps=c["eps"], betas=(c["beta1"], c["beta2"]))
    for i, n in enumerate(NAMES):
        opt.state[prm[n]] = {"step": torch.tensor(c["steps"][i]), "exp_avg": t("m_" + n), "exp_avg_sq": t("v_" + n)}
    # activations (gaussian_model.py:41-56, 141-165; an isotropic model's one scale is repeated for the rasteriser)
    opacity = torch.sigmoid(prm["opacity"])
    scaling = torch.exp(prm["scaling"])
    scaling = scaling if c["S"] == 3 else scaling.repeat(1, 3)
    rotation = torch.nn.functional.normalize(prm["rotation"])
    features = torch.cat((prm["f_dc"], prm["f_rest"]), dim=1)
    xyz = prm["xyz"] * 1.0
    torch.autograd.backward([xyz, features, opacity, scaling, rotation],
                            [t("g_mean3D"), t("g_sh"), t("g_opacity").view(-1, 1), t("g_scale"), t("g_rot")])
    for i, n in enumerate(NAMES):
        if c["skip"][i]:
            prm[n].grad = None
    value = None
    flags = c["flags"]
    if flags & (RESET_ALL | RESET_NONVISIBLE):
        with torch.no_grad():
            get_opacity = torch.sigmoid(prm["opacity"])
            new = _inverse_sigmoid(torch.ones_like(get_opacity) * (0.01 if flags & RESET_ALL else 0.4))
            value = float(new.reshape(-1)[0])
            if not flags & RESET_ALL:
                for filt in [torch.from_numpy(r > 0) for r in c["radii"]]:
                    new[filt] = (prm["opacity"] if flags & RESET_KEEP_VISIBLE else get_opacity)[filt]
        prm["opacity"] = _replace_tensor_to_optimizer(opt, new, "opacity")
    opt.step()
    got = {}
    for n in NAMES:
        st = opt.state[prm[n]]
        got[n], got["m_" + n], got["v_" + n] = prm[n].detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    return got, [float(opt.state[prm[n]]["step"]) for n in NAMES], value


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_agrees_with_the_reference_semantics(c):
    """Every element of the 18 tensors within the restatement's own bound plus the same bound once more for torch's fp32 (its
    kernels round in other places: lerp for exp_avg, autograd's formula for normalize), and the step counts equal."""
    c = dict(c)
    got, steps, value = _torch_reference(c)
    if value is not None:
        c["reset_value"] = value  # (the reference forms it with torch's fp32 log; the restatement takes it as an input)
    bad = R.compare(got, steps, c, factor=2.0)
    print("worst error / bound: %.3f" % R.worst_ratio(got, c))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_comparator_rejects_the_mutant(mutant):
    """At the widest tolerance any test uses (twice the bound), on every case that can tell the mutant apart; and every mutant
    meets at least one such case."""
    n = 0
    for c, cid in zip(CASES, IDS):
        if not R.applies(mutant, c):
            continue
        n += 1
        out, _, steps = R.restate(c, mutant)
        assert R.compare(out, steps, c, factor=2.0), "%s passes for %s on %s" % (mutant, "the restatement", cid)
    assert n > 0, mutant


def test_comparator_accepts_the_restatement_rounded_to_fp32():
    for c in CASES:
        out, _, steps = R.restate(c)
        assert not R.compare({k: v.astype(np.float32) for k, v in out.items()}, steps, c)


def test_planted_rows_are_in_the_cases():
    """Each plant is met, and a row without gradient and without moments comes back bit for bit."""
    seen = set()
    for c in CASES:
        seen |= set(c["plants"].values())
        out, _, _ = R.restate(c)
        for row, plant in c["plants"].items():
            if plant == "zero_grad_zero_moments":
                for i, n in enumerate(NAMES):
                    if c["flags"] & (RESET_ALL | RESET_NONVISIBLE) and n == "opacity":
                        continue
                    for k in ("", "m_", "v_"):
                        assert np.array_equal(out[k + n][row].astype(np.float32).view(np.int32), c[k + n][row].view(np.int32)), (n, k)
    assert seen == set(R.PLANTS)


# ---- the learning-rate schedule ---------------------------------------------------------------------------------------------
def test_lr_schedule_returns_the_reference_numbers():
    """helper against tests/golden/lr_schedule.npz (make_goldens_lr.py).  Both sides are the same double-precision expression, so
    the numbers are compared to 4 ulp of the result times (1 + |log lr_init| + |log lr_final|): an exp of an argument of that
    size amplifies one ulp of the argument that much, should the two runs' libm differ in the last place."""
    from gaussian_splatting.utils.general_utils import get_expon_lr_func, helper

    z = np.load(os.path.join(GOLDEN, "lr_schedule.npz"))
    assert get_expon_lr_func(1.0, 0.1) is helper
    branches = set()
    for (step, lr_init, lr_final, delay_steps, delay_mult, max_steps), want in zip(z["args"], z["lr"]):
        got = helper(int(step), lr_init=lr_init, lr_final=lr_final, lr_delay_steps=int(delay_steps), lr_delay_mult=delay_mult,
                     max_steps=int(max_steps))
        amp = 1.0 if lr_init == 0 else 1 + abs(np.log(lr_init)) + abs(np.log(lr_final))
        assert abs(got - want) <= 4 * 2.0 ** -52 * amp * abs(want), (step, lr_init, got, want)
        branches.add("off" if step < 0 or lr_init == 0 else "delay" if delay_steps > 0 else "plain")
    assert branches == {"off", "delay", "plain"}
    assert {-1.0, 0.0, 1.0, 15000.0, 30000.0, 30001.0} <= set(z["args"][:, 0])


def test_update_learning_rate_sets_and_returns_the_xyz_rate():
    z = np.load(os.path.join(GOLDEN, "lr_schedule.npz"))
    m = _model(8, 4, 3, spatial_lr_scale=6.5)
    rows = [(a, lr) for a, lr in zip(z["args"], z["lr"]) if a[3] == 0 and a[1] == 0.00016 * 6.5]
    assert len(rows) == 6
    for a, want in rows:
        got = m.update_learning_rate(int(a[0]))
        assert got == m.optimizer.param_groups[0]["lr"] and abs(got - want) <= 1e-13 * abs(want)
    assert [g["lr"] for g in m.optimizer.param_groups[1:]] == [0.0025, 0.0025 / 20.0, 0.05, 0.001 * 6.5, 0.001]


# ---- host logic, with the launch replaced by the restatement -------------------------------------------------------------------
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                             position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001)


def _model(P, M, S, spatial_lr_scale=1.0, seed=0, setup=True):
    from gaussian_splatting.scene.gaussian_model import GaussianModel

    c = R.make_case(P, M, S, seed)
    m = GaussianModel(3)
    m._set_params(*[c[n] for n in NAMES], "cpu")
    m.init_lr(spatial_lr_scale)
    if setup:
        m.training_setup(ARGS)
    return m


def _grads(P, M, seed=1):
    c = R.make_case(P, M, 3, seed)
    return dict(mean3D=torch.from_numpy(c["g_mean3D"]), sh=torch.from_numpy(c["g_sh"]), opacity=torch.from_numpy(c["g_opacity"]).view(P, 1),
                scale=torch.from_numpy(c["g_scale"]), rot=torch.from_numpy(c["g_rot"]))


@pytest.fixture
def launches(monkeypatch):
    """gsaj.map_step._launch replaced: records its arguments and applies the restatement to the CPU tensors in place."""
    import gsaj.map_step as ms

    calls = []

    def fake(P, M, S, prm, m, v, grads, step_size, bc2_sqrt, skip, beta1, beta2, eps, flags, radii, value):
        calls.append(dict(P=P, M=M, S=S, prm=prm, m=m, v=v, grads=grads, step_size=list(step_size), bc2_sqrt=list(bc2_sqrt),
                          skip=list(skip), betas=(beta1, beta2), eps=eps, flags=flags, radii=radii, value=value))
        if flags & (RESET_ALL | RESET_NONVISIBLE):
            with torch.no_grad():
                prm[3].fill_(value)
                m[3].zero_()
                v[3].zero_()

    monkeypatch.setattr(ms, "_launch", fake)
    return calls


def test_map_step_creates_state_as_torch_does_and_counts_steps_per_group(launches):
    from gsaj.map_step import adam_scalars

    m = _model(9, 4, 3)
    g = _grads(9, 4)
    assert len(m.optimizer.state) == 0
    m.map_step(g, freeze=("rotation",))
    st = m.optimizer.state
    for n, p in zip(NAMES, m.parameters()):
        if n == "rotation":
            assert p not in st  # like a parameter whose .grad is None: no state, no step
            continue
        s = st[p]
        assert set(s) == {"step", "exp_avg", "exp_avg_sq"} and s["step"].dtype == torch.float32 and s["step"].device.type == "cpu"
        assert float(s["step"]) == 1.0 and s["exp_avg"].shape == p.shape and not s["exp_avg"].any() and not s["exp_avg_sq"].any()
        assert p.grad is None
    call = launches[0]
    assert call["skip"] == [False] * 5 + [True] and call["prm"][5] is None and call["grads"][4] is None
    assert call["betas"] == (0.9, 0.999) and call["eps"] == 1e-15 and call["flags"] == 0 and call["radii"] is None
    m.map_step(g)
    m.optimizer.param_groups[1]["lr"] = 0.01  # read at every call
    m.map_step(g)
    assert [float(st[p]["step"]) for p in m.parameters()] == [3.0] * 5 + [2.0]
    call = launches[2]
    for i, n in enumerate(NAMES):
        lr = m.optimizer.param_groups[i]["lr"]
        assert (call["step_size"][i], call["bc2_sqrt"][i]) == adam_scalars(lr, 0.9, 0.999, 2.0 if n == "rotation" else 3.0)
    assert call["step_size"][1] == 0.01 / (1 - 0.9 ** 3)
    # the launch got the optimizer's own tensors, not copies
    assert call["m"][0].data_ptr() == st[m._xyz]["exp_avg"].data_ptr() and call["prm"][0].data_ptr() == m._xyz.data_ptr()
    assert call["grads"][1].data_ptr() == g["sh"].data_ptr()


def test_map_step_and_optimizer_step_alternate(launches):
    m = _model(9, 4, 3)
    g = _grads(9, 4)
    m.map_step(g)
    m.assign_bucket_gradients(g)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.map_step(g)
    assert [float(m.optimizer.state[p]["step"]) for p in m.parameters()] == [3.0] * 6
    assert launches[1]["step_size"][0] == m.optimizer.param_groups[0]["lr"] / (1 - 0.9 ** 3)


@pytest.mark.parametrize("how", ["fused", "alone_all", "alone_nonvisible"])
def test_reset_rekeys_the_opacity_group_and_does_not_count_a_step(launches, how):
    m = _model(9, 4, 3)
    g = _grads(9, 4)
    m.map_step(g)
    old = m._opacity
    state = m.optimizer.state[old]
    filters = [torch.arange(9) % 2 == 0, torch.arange(9) % 3 == 0]
    if how == "fused":
        m.map_step(g, reset="nonvisible", radii=filters)
    elif how == "alone_all":
        m.reset_opacity()
    else:
        m.reset_opacity_nonvisible(filters)
    new = m._opacity
    assert new is not old and new.is_leaf and new.requires_grad and new.data_ptr() == old.data_ptr()
    assert m.optimizer.param_groups[3]["params"][0] is new and old not in m.optimizer.state
    assert m.optimizer.state[new] is state and float(state["step"]) == 1.0
    others = [float(m.optimizer.state[p]["step"]) for n, p in zip(NAMES, m.parameters()) if n != "opacity"]
    assert others == ([2.0] * 5 if how == "fused" else [1.0] * 5)
    call = launches[-1]
    assert call["skip"] == ([False] * 6 if how == "fused" else [True] * 6)
    if how == "alone_all":
        assert call["flags"] == RESET_ALL and call["radii"] is None
        assert call["value"] == _logit32(0.01) and bool((new == call["value"]).all())
    else:
        assert call["flags"] == RESET_NONVISIBLE and call["radii"].dtype == torch.int32 and tuple(call["radii"].shape) == (2, 9)
        assert call["radii"].tolist() == [[int(b) for b in f] for f in filters]
        assert call["value"] == _logit32(0.4)
    assert call["prm"][3].data_ptr() == old.data_ptr() and (how == "fused" or call["prm"][0] is None)
    # the model still steps, with the re-keyed state
    m.map_step(g)
    assert float(m.optimizer.state[m._opacity]["step"]) == 2.0


def test_radii_tensor_is_taken_as_it_is(launches):
    m = _model(9, 4, 3)
    r = torch.zeros((3, 9), dtype=torch.int32)
    m.reset_opacity_nonvisible(r)
    assert launches[0]["radii"].data_ptr() == r.data_ptr()
    from gsaj._lib import GsajError
    with pytest.raises(GsajError, match="columns"):
        m.reset_opacity_nonvisible(torch.zeros((3, 8), dtype=torch.int32))
    with pytest.raises(GsajError, match="needs radii"):
        m.map_step(_grads(9, 4), reset="nonvisible")


def test_moments_follow_their_rows_through_extend_from_pcd(launches):
    m = _model(9, 4, 3)
    g = _grads(9, 4)
    m.map_step(g)
    with torch.no_grad():
        m.optimizer.state[m._xyz]["exp_avg"].copy_(torch.arange(27.0).view(9, 3))
    k = 4
    m.extend_from_pcd(torch.ones(k, 3), torch.zeros(k, 3, 4), torch.zeros(k, 3), torch.ones(k, 4), torch.zeros(k, 1), kf_id=2)
    st = m.optimizer.state[m._xyz]
    assert tuple(st["exp_avg"].shape) == (13, 3) and st["exp_avg"][:9].reshape(-1).tolist() == list(range(27)) and not st["exp_avg"][9:].any()
    g2 = _grads(13, 4)
    m.map_step(g2)
    assert launches[-1]["P"] == 13 and [float(m.optimizer.state[p]["step"]) for p in m.parameters()] == [2.0] * 6
    from gsaj._lib import GsajError
    with pytest.raises(GsajError, match="gradient mean3D"):
        m.map_step(g)  # a slot sized for the map before it grew


def test_optimizers_the_kernel_cannot_reproduce_are_refused(launches):
    from gsaj._lib import GsajError

    g = _grads(9, 4)

    def model_with(opt_cls=torch.optim.Adam, **kw):
        m = _model(9, 4, 3, setup=False)
        groups = [{"params": [p], "lr": 1e-3, "name": n} for n, p in zip(NAMES, m.parameters())]
        m.optimizer = opt_cls(groups, lr=0.0, eps=1e-15, **kw)
        return m

    for kw, why in ((dict(amsgrad=True), "amsgrad"), (dict(weight_decay=0.1), "weight decay"), (dict(maximize=True), "maximize"),
                    (dict(capturable=True), "capturable"), (dict(differentiable=True), "differentiable")):
        with pytest.raises(GsajError, match=why):
            model_with(**kw).map_step(g)
    with pytest.raises(GsajError, match="torch.optim.Adam"):
        model_with(torch.optim.AdamW).map_step(g)
    m = _model(9, 4, 3, setup=False)
    with pytest.raises(GsajError, match="no optimizer"):
        m.map_step(g)
    m.optimizer = torch.optim.Adam([{"params": [m._xyz, m._features_dc], "lr": 1e-3, "name": "xyz"}], lr=0.0)
    with pytest.raises(GsajError, match="holds 2 parameters"):
        m.map_step(g)
    m = model_with()
    m.optimizer.param_groups[2]["betas"] = (0.8, 0.999)
    with pytest.raises(GsajError, match="betas and eps"):
        m.map_step(g)
    m = model_with()
    m._xyz = m._xyz.detach().clone().requires_grad_(True)  # replaced behind the optimizer's back
    with pytest.raises(GsajError, match="does not hold the model's parameter"):
        m.map_step(g)
    m = model_with()
    with pytest.raises(GsajError, match="freeze"):
        m.map_step(g, freeze=("colour",))
    m = model_with()
    m.map_step(g)
    m.optimizer.state[m._xyz]["exp_avg"] = m.optimizer.state[m._xyz]["exp_avg"].double()
    with pytest.raises(GsajError, match="exp_avg of xyz"):
        m.map_step(g)
    assert len(launches) == 1


def test_the_reference_map_tail_reads_the_same_against_the_overlay(launches):
    """slam_backend.py:299-311, line for line: densify or reset, step, schedule."""
    m = _model(9, 4, 3)
    g = _grads(9, 4)
    filters = [torch.arange(9) % 2 == 0]
    for iteration, reset in ((1, False), (2, True)):
        if reset:
            m.reset_opacity_nonvisible(filters)
        m.map_step(g)
        lr = m.update_learning_rate(iteration)
    assert lr == m.optimizer.param_groups[0]["lr"] and float(m.optimizer.state[m._opacity]["step"]) == 2.0


# ---- the C ABI's argument errors need no GPU ----------------------------------------------------------------------------------
def test_argument_errors_and_the_empty_map_without_a_gpu():
    import ctypes
    from gsaj import _lib
    from gsaj.map_step import MapStepArgs

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    a = MapStepArgs()
    assert lib.gsaj_map_step(0, 4, 3, 0, ctypes.byref(a), None) == 0  # P = 0: success, nothing launched, nothing read
    for P, M, S, flags, msg in ((5, 0, 3, 0, b"M >= 1"), (5, 4, 2, 0, b"scale_cols"), (-1, 4, 3, 0, b"P >= 0"), (5, 4, 3, 8, b"flags"),
                                (5, 4, 3, RESET_NONVISIBLE, b"needs radii"), (5, 4, 3, 0, b"group xyz"),
                                (5, 4, 3, RESET_ALL, b"group xyz"), (2 ** 30, 16, 3, 0, b"INT_MAX")):
        a = MapStepArgs()
        a.flags = flags
        assert lib.gsaj_map_step(P, M, S, 0, ctypes.byref(a), None) == -1, (P, M, S, flags)
        assert msg in lib.gsaj_last_error(), (msg, lib.gsaj_last_error())
    assert lib.gsaj_map_step(5, 4, 3, 0, None, None) == -1
    a = MapStepArgs()
    a.flags = RESET_ALL
    for i in range(6):
        a.skip[i] = 1
    assert lib.gsaj_map_step(5, 4, 3, 0, ctypes.byref(a), None) == -1 and b"group opacity" in lib.gsaj_last_error()
