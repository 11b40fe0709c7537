"""fp64 NumPy restatement of the map step (include/gsaj.h "map step"; csrc/map_step.hip): (a) the chain rule through the
activations, (b) torch.optim.Adam's update, (c) the opacity resets -- on fp32 inputs, with fp64 arithmetic, and beside every output
element a bound on what an fp32 evaluation of the same formulas may differ by.  Shared by tests/test_cpu_map_step.py, which pins the
restatement to the reference's semantics (CPU autograd through the reference's activations + torch.optim.Adam + a restated
replace_tensor_to_optimizer), and tests/test_gpu_map_step.py, which checks the device against it.  MUTANTS lists deliberate
mistakes the comparator must reject.

The bound (derived, not tuned).  u = 2^-24 is the unit round-off of fp32: one correctly rounded operation has relative error <= u;
an operation whose result is subnormal has absolute error <= ETA = 2^-149 instead.  First-order terms are written out below; the
whole bound is then multiplied by FACTOR = 2, which covers the second-order terms and nothing else.
  device functions (csrc/map_step.hip, compiled without contraction): + - * are IEEE; `/` and sqrtf are correctly rounded (hipcc's
    default for fp32 division and square root), taken as 1 u each; expf is the device library's __ocml_exp_f32, documented in
    the HIP math API table at 1 ulp, taken as relative 2 u (an ulp is up to 2 u of the value).  No ROCm document with the ulp
    figures ships with the toolchain the suite runs on, so tests/test_gpu_map_step.py::test_device_exp_and_sigmoid_error_is_within_the_figure_taken
    measures expf and 1 / (1 + expf(-o)) through the kernel itself against fp64 over the test's inputs, and asserts the figures
    taken here (EXP_REL = 2 u, SIGMOID_REL = 4 u).  Measured on MI355X: expf 1.249 u, the sigmoid 1.867 u.
  gradient g of a raw element, error dg:
    xyz, f_dc, f_rest: copies, dg = 0.
    opacity g s (1 - s), s = 1 / (1 + e), e = expf(-o): e has 2 u, 1 + e has 3 u (2 u e + u (1 + e) <= 3 u (1 + e)), the quotient
      4 u: ds = 4 u s.  1 - s: d1 = ds + u (1 - s).  g s: |g| ds + u |g s|.  (g s)(1 - s): that times (1 - s) + |g s| d1 + u |result|.
    scaling g_j expf(s_j): 3 u |t_j| (2 u + the product); isotropic: the three products and two additions, 5 u sum |t_j|.
    rotation (g_i - h_i (g . h)) / n, h = q / n, n = sqrtf(sum q_j^2): the sum of four squares has 4 u (a product and three
      additions of non-negative terms), its root 2 u + u = 3 u = dn / n; h_i has 4 u; each g_j h_j has 5 u and the three additions
      3 u more: ddot = 8 u sum |g_j h_j|; h_i dot: |h_i| ddot + 5 u |h_i dot|; the difference r_i: + u |r_i|; the quotient:
      that / n + 4 u |r_i / n|.
  Adam, per element, from m0, v0, p0 and g +- dg, with the fp32 factors b = (float)beta, c = (float)(1.0 - beta) as inputs:
    m = b1 m0 + c1 g: three roundings (two products, the sum): dm = 3 u (|m0| + |g| + dg) + c1 dg + 3 ETA.
    v = b2 v0 + (c2 g) g: non-negative terms, four roundings: dv = 4 u / (1 - 4 u) v + c2 (2 |g| dg + dg^2) + 4 ETA.
    r = sqrtf(v) and d = r / bc2_sqrt + eps by interval, because dv may reach v itself (a row without moments whose gradient is
      mostly rounding, e.g. the opacity gradient at logit +15, where 1 - s keeps two bits): r in [sqrt(max(v - dv, 0)) (1 - u),
      sqrt(v + dv) (1 + u)], d in [(r_lo / bc2_sqrt (1 - u) + eps) (1 - u), (r_hi / bc2_sqrt (1 + u) + eps) (1 + u)]; d_lo >= eps (1 - u) > 0.
    q = m / d: |q| in [max(|m| - dm, 0) / d_hi, (|m| + dm) / d_lo]: dq = the farther end's distance from |q|, e, plus the
      quotient's rounding u (|q| + e) + ETA.   D = step_size q: dD = step_size dq + u (|D| + step_size dq) + ETA.
    p = p0 - D: dp = dD + u (|p0| + |D| + dD).
  resets: zeros and reset_value are written exactly (bound 0); a visible row's s = sigmoid(o) has 4 u s; KEEP_VISIBLE rows are exact."""
import numpy as np

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
GRADS = ("g_mean3D", "g_sh", "g_opacity", "g_scale", "g_rot")
OP = 3
RESET_ALL, RESET_NONVISIBLE, RESET_KEEP_VISIBLE = 1, 2, 4
U = 2.0 ** -24
ETA = 2.0 ** -149
FACTOR = 2.0
EXP_REL = 2 * U
SIGMOID_REL = 4 * U
MUTANTS = ("no_bias_correction", "eps_inside_root", "g2_after_moment", "zero_grad_rows_skipped", "reset_opacity_stepped",
           "reset_step_advanced", "reset_moments_kept", "visible_gets_logit", "keep_visible_gets_sigmoid", "visible_from_view0",
           "isotropic_not_summed", "quaternion_not_projected", "sh_split_off_by_one")
PLANTS = ("zero_grad", "zero_grad_zero_moments", "grad_1e-20", "grad_1e+6", "quat_1e-3", "quat_10", "logit_+15", "logit_-15",
          "logscale_-12", "logscale_+3")


def f32(x):
    return np.asarray(x, dtype=np.float32)


def make_case(P, M, S, seed, t=1, flags=0, K_vis=0, skip=(0, 0, 0, 0, 0, 0), eps=1e-15, blank_view=None):
    """fp32 inputs of one launch.  Row i < min(P, 10) carries plant (i + seed) % 10 of PLANTS (case["plants"]: row -> name), so that
    P = 1 still meets each plant under some seed.  t: the step count AFTER this step (the state holds t - 1).  With K_vis > 0:
    radii [K_vis,P] with negative, zero and positive entries; rows P // 2 ... are visible in the last view only; blank_view: a view
    whose radii are all zero."""
    rng = np.random.default_rng(seed)
    shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, M - 1, 3), opacity=(P, 1), scaling=(P, S), rotation=(P, 4))
    c = dict(P=P, M=M, S=S, t=t, flags=flags, K_vis=K_vis, skip=tuple(int(s) for s in skip), seed=seed)
    c["xyz"] = f32(rng.normal(scale=2.0, size=shapes["xyz"]))
    c["f_dc"] = f32(rng.normal(scale=0.5, size=shapes["f_dc"]))
    c["f_rest"] = f32(rng.normal(scale=0.1, size=shapes["f_rest"]))
    c["opacity"] = f32(rng.normal(scale=2.0, size=shapes["opacity"]))
    c["scaling"] = f32(rng.normal(loc=-4.0, scale=1.0, size=shapes["scaling"]))
    q = rng.normal(size=shapes["rotation"])
    c["rotation"] = f32(q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.8, 1.25, size=(P, 1)))
    for n in NAMES:
        c["m_" + n] = f32(rng.normal(size=shapes[n]) * 10.0 ** rng.uniform(-6, -2, size=shapes[n]))
        c["v_" + n] = f32((rng.normal(size=shapes[n]) * 10.0 ** rng.uniform(-6, -2, size=shapes[n])) ** 2)
    gshapes = dict(g_mean3D=(P, 3), g_sh=(P, M, 3), g_opacity=(P,), g_scale=(P, 3), g_rot=(P, 4))
    for k in GRADS:
        c[k] = f32(rng.normal(size=gshapes[k]) * 10.0 ** rng.uniform(-6, 0, size=gshapes[k]))
    plants = {}
    for i in range(min(P, len(PLANTS))):
        name = PLANTS[(i + seed) % len(PLANTS)]
        plants[i] = name
        if name in ("zero_grad", "zero_grad_zero_moments"):
            for k in GRADS:
                c[k][i] = 0.0
            if name == "zero_grad_zero_moments":
                for n in NAMES:
                    c["m_" + n][i] = 0.0
                    c["v_" + n][i] = 0.0
        elif name in ("grad_1e-20", "grad_1e+6"):
            for k in GRADS:
                c[k][i] = np.float32(1e-20 if name == "grad_1e-20" else 1e6) * np.where(rng.random(c[k][i].shape) < 0.5, -1, 1)
        elif name in ("quat_1e-3", "quat_10"):
            c["rotation"][i] *= np.float32(1e-3 if name == "quat_1e-3" else 10.0) / np.linalg.norm(c["rotation"][i].astype(np.float64))
        elif name in ("logit_+15", "logit_-15"):
            c["opacity"][i] = 15.0 if name == "logit_+15" else -15.0
        else:
            c["scaling"][i] = -12.0 if name == "logscale_-12" else 3.0
    c["plants"] = plants
    c["lr"] = (1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 1e-3, 1e-3)
    c["beta1"], c["beta2"], c["eps"] = 0.9, 0.999, eps
    c["steps"] = tuple(float(t - 1) for _ in NAMES)
    x = np.float32(0.01 if flags & RESET_ALL else 0.4)
    c["reset_value"] = float(np.float32(np.log(np.float64(x / (np.float32(1) - x)))))
    c["radii"] = None
    if K_vis:
        r = rng.integers(-2, 40, size=(K_vis, P)).astype(np.int32)
        r[rng.random((K_vis, P)) < 0.75] = 0
        last = np.arange(P // 2, min(P, P // 2 + 5))
        r[:, last] = 0
        r[K_vis - 1, last] = 7
        if blank_view is not None:
            r[blank_view] = 0
        c["radii"] = r
        c["last_only"] = last
    return c


def host_scalars(lr, beta1, beta2, step):
    """step_size and bc2_sqrt as the host forms them (torch/optim/adam.py::_single_tensor_adam, Python floats), rounded to fp32 once."""
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return np.float32(lr / bc1), np.float32(bc2 ** 0.5)


def activation_grads(c, mutant=None):
    """(gradient, bound dg) w.r.t. each raw parameter, fp64."""
    P, M, S = c["P"], c["M"], c["S"]
    d = lambda k: c[k].astype(np.float64)  # noqa: E731
    out = {}
    out["xyz"] = (d("g_mean3D"), np.zeros((P, 3)))
    sh = d("g_sh")
    out["f_dc"] = (sh[:, :1, :], np.zeros((P, 1, 3)))
    rest = sh[:, 0:M - 1, :] if mutant == "sh_split_off_by_one" else sh[:, 1:, :]
    out["f_rest"] = (rest, np.zeros((P, M - 1, 3)))
    # opacity
    g, o = d("g_opacity").reshape(P, 1), d("opacity")
    s = 1.0 / (1.0 + np.exp(-o))
    ds = SIGMOID_REL * s
    d1 = ds + U * (1 - s)
    gs = g * s
    e_gs = np.abs(g) * ds + U * np.abs(gs)
    res = gs * (1 - s)
    out["opacity"] = (res, e_gs * (1 - s) + np.abs(gs) * d1 + U * np.abs(res) + ETA)
    # scaling
    ex = np.exp(d("scaling"))
    if S == 3:
        t = d("g_scale") * ex
        out["scaling"] = (t, (EXP_REL + U) * np.abs(t) + ETA)
    else:
        t = d("g_scale") * ex
        tot = t[:, :1] if mutant == "isotropic_not_summed" else t.sum(axis=1, keepdims=True)
        out["scaling"] = (tot, (EXP_REL + U + 2 * U) * np.abs(t).sum(axis=1, keepdims=True) + ETA)
    # rotation
    q, gq = d("rotation"), d("g_rot")
    n = np.maximum(np.sqrt((q * q).sum(axis=1, keepdims=True)), 1e-12)
    h = q / n
    dot = (gq * h).sum(axis=1, keepdims=True)
    ddot = 8 * U * np.abs(gq * h).sum(axis=1, keepdims=True)
    hd = h * dot
    r = gq - (0.0 if mutant == "quaternion_not_projected" else hd)
    e_r = np.abs(h) * ddot + 5 * U * np.abs(hd) + U * np.abs(r)
    out["rotation"] = (r / n, e_r / n + 4 * U * np.abs(r / n) + ETA)
    return out


def adam(p0, m0, v0, g, dg, step_size, bc2_sqrt, beta1, beta2, eps, mutant=None):
    """One Adam update in fp64 from fp32 scalars; returns (p, m, v) and their bounds (before FACTOR)."""
    b1, b2, eps = float(np.float32(beta1)), float(np.float32(beta2)), float(np.float32(eps))
    c1, c2 = float(np.float32(1.0 - beta1)), float(np.float32(1.0 - beta2))
    ss, bs = float(step_size), float(bc2_sqrt)
    m = b1 * m0 + c1 * g
    g2 = m * m if mutant == "g2_after_moment" else g * g
    v = b2 * v0 + c2 * g2
    r = np.sqrt(v)
    d = np.sqrt(v + eps) / bs if mutant == "eps_inside_root" else r / bs + eps
    q = m / d
    D = ss * q
    p = p0 - D
    dm = 3 * U * (np.abs(m0) + np.abs(g) + dg) + c1 * dg + 3 * ETA
    dv = 4 * U / (1 - 4 * U) * v + c2 * (2 * np.abs(g) * dg + dg * dg) + 4 * ETA
    r_lo, r_hi = np.sqrt(np.maximum(v - dv, 0.0)) * (1 - U), np.sqrt(v + dv) * (1 + U)
    d_lo, d_hi = (r_lo / bs * (1 - U) + eps) * (1 - U), (r_hi / bs * (1 + U) + eps) * (1 + U)
    am = np.abs(m)
    e = np.maximum((am + dm) / d_lo - np.abs(q), np.abs(q) - np.maximum(am - dm, 0.0) / d_hi)
    dq = e + U * (np.abs(q) + e) + ETA
    dD = ss * dq + U * (np.abs(D) + ss * dq) + ETA
    dp = dD + U * (np.abs(p0) + np.abs(D) + dD)
    if mutant == "zero_grad_rows_skipped":
        z = g == 0
        p, m, v = np.where(z, p0, p), np.where(z, m0, m), np.where(z, v0, v)
    return (p, m, v), (dp, dm, dv)


def visible_rows(c, mutant=None):
    r = c["radii"][:1] if mutant == "visible_from_view0" else c["radii"]
    return (r > 0).any(axis=0)


def restate(c, mutant=None):
    """-> (out, bound, steps): out / bound map every one of the 18 tensors (name, "m_" + name, "v_" + name) to its fp64 value and
    to the bound on an fp32 evaluation (FACTOR included); steps: the six step counts after the call."""
    flags = c["flags"]
    resets = bool(flags & (RESET_ALL | RESET_NONVISIBLE))
    grads = activation_grads(c, mutant)
    out, bound, steps = {}, {}, list(c["steps"])
    for i, n in enumerate(NAMES):
        p0, m0, v0 = (c[k + n].astype(np.float64) for k in ("", "m_", "v_"))
        zero = np.zeros_like(p0)
        reset_here = resets and i == OP
        res, bnd = (p0, m0, v0), (zero, zero, zero)
        if (not c["skip"][i] and not reset_here) or (reset_here and mutant == "reset_opacity_stepped" and not c["skip"][i]):
            steps[i] += 1
            step = steps[i]
            if mutant == "no_bias_correction":
                ss, bs = np.float32(c["lr"][i]), np.float32(1.0)
            else:
                ss, bs = host_scalars(c["lr"][i], c["beta1"], c["beta2"], step)
            g, dg = grads[n]
            res, bnd = adam(p0, m0, v0, g, dg, ss, bs, c["beta1"], c["beta2"], c["eps"], mutant)
        if reset_here:
            if mutant == "reset_step_advanced":
                steps[i] += 1
            p_in = res[0]
            value = float(np.float32(c["reset_value"]))
            if flags & RESET_ALL:
                p, dp = np.full_like(p0, value), zero
            else:
                vis = visible_rows(c, mutant).reshape(p0.shape)
                s = 1.0 / (1.0 + np.exp(-p_in))
                keep = bool(flags & RESET_KEEP_VISIBLE)
                if mutant == "visible_gets_logit" and not keep:
                    keep = True
                elif mutant == "keep_visible_gets_sigmoid" and keep:
                    keep = False
                p = np.where(vis, p_in if keep else s, value)
                dp = np.where(vis, zero if keep else SIGMOID_REL * s, zero)
            mv = (res[1], res[2]) if mutant == "reset_moments_kept" else (zero, zero)
            res, bnd = (p, mv[0], mv[1]), (dp, zero, zero)
        for k, r, b in zip(("", "m_", "v_"), res, bnd):
            out[k + n], bound[k + n] = r, FACTOR * b
    return out, bound, tuple(steps)


def applies(mutant, c):
    """Whether the case can tell the mutant from the restatement at all."""
    resets = bool(c["flags"] & (RESET_ALL | RESET_NONVISIBLE))
    by_view = resets and not c["flags"] & RESET_ALL
    stepped = [not s and not (resets and i == OP) for i, s in enumerate(c["skip"])]
    keep = bool(c["flags"] & RESET_KEEP_VISIBLE)
    some_visible = by_view and bool(visible_rows(c).any())
    has = lambda plant: plant in c["plants"].values()  # noqa: E731
    return {
        "no_bias_correction": any(stepped),
        "eps_inside_root": any(stepped) and c["eps"] >= 1e-8,
        "g2_after_moment": any(stepped),
        "zero_grad_rows_skipped": any(stepped) and has("zero_grad"),
        "reset_opacity_stepped": resets and not c["skip"][OP],
        "reset_step_advanced": resets,
        "reset_moments_kept": resets,
        "visible_gets_logit": some_visible and not keep,
        "keep_visible_gets_sigmoid": some_visible and keep,
        "visible_from_view0": by_view and bool((visible_rows(c) != visible_rows(c, "visible_from_view0")).any()),
        "isotropic_not_summed": c["S"] == 1 and stepped[4],
        "quaternion_not_projected": stepped[5],
        "sh_split_off_by_one": c["M"] >= 2 and stepped[2],
    }[mutant]


def compare(got, got_steps, c, factor=1.0, ref=None):
    """got: the 18 tensors by name (any float dtype), got_steps: six step counts.  Returns the list of complaints (empty: accepted):
    every element of every tensor must lie within factor x bound of the restatement, the steps must be equal."""
    out, bound, steps = ref if ref is not None else restate(c)
    bad = []
    if tuple(float(s) for s in got_steps) != tuple(float(s) for s in steps):
        bad.append("steps %s != %s" % (tuple(got_steps), steps))
    for k in out:
        x = np.asarray(got[k], dtype=np.float64).reshape(out[k].shape)
        err = np.abs(x - out[k])
        over = ~(err <= factor * bound[k])  # (NaN counts as over)
        if over.any():
            j = np.unravel_index(np.argmax(np.where(over, err / np.maximum(factor * bound[k], 1e-300), 0)), err.shape)
            bad.append("%s%s: |%.9g - %.9g| = %.3g > %.3g (%d of %d elements)" % (k, list(j), x[j], out[k][j], err[j], factor * bound[k][j], int(over.sum()), over.size))
    return bad


def worst_ratio(got, c, ref=None):
    """max over all elements of error / bound (elements with zero bound and zero error count as 0): what a test prints."""
    out, bound, _ = ref if ref is not None else restate(c)
    w = 0.0
    for k in out:
        if out[k].size == 0:
            continue
        err = np.abs(np.asarray(got[k], dtype=np.float64).reshape(out[k].shape) - out[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound[k])
        w = max(w, float(np.max(ratio)))
    return w


def CASES():
    """The cases of the CPU test (small P: the semantics do not depend on it) -- every flag combination, both scale layouts, M = 1, 4
    and 16, t = 1, 2 and 1000, both eps, frozen groups, the stand-alone reset."""
    cs = []
    seed = 0
    for t in (1, 2, 1000):
        for M, S in ((16, 3), (4, 1), (1, 3)):
            seed += 1
            cs.append(make_case(23, M, S, seed, t=t, eps=1e-15 if seed % 2 else 1e-8))
    for flags in (RESET_ALL, RESET_NONVISIBLE, RESET_NONVISIBLE | RESET_KEEP_VISIBLE, RESET_ALL | RESET_NONVISIBLE,
                  RESET_ALL | RESET_KEEP_VISIBLE, RESET_ALL | RESET_NONVISIBLE | RESET_KEEP_VISIBLE, RESET_KEEP_VISIBLE):
        for K in (1, 3):
            seed += 1
            cs.append(make_case(23, 4, 3 if seed % 2 else 1, seed, t=2, flags=flags, K_vis=K, blank_view=(1 if K > 1 else None)))
    seed += 1
    cs.append(make_case(23, 4, 3, seed, t=3, flags=RESET_NONVISIBLE, K_vis=3, skip=(1,) * 6))  # the stand-alone reset
    seed += 1
    cs.append(make_case(23, 4, 3, seed, t=3, flags=RESET_NONVISIBLE, K_vis=1, blank_view=0))  # nothing is visible
    seed += 1
    cs.append(make_case(23, 16, 3, seed, t=5, skip=(1, 0, 0, 0, 1, 1)))  # a colour refinement
    seed += 1
    cs.append(make_case(23, 4, 1, seed, t=5, flags=RESET_NONVISIBLE | RESET_KEEP_VISIBLE, K_vis=9, skip=(0, 0, 0, 1, 0, 0)))
    return cs
