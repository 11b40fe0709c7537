"""NumPy float64 restatement of the dense analytic path (csrc/dense.hip behind gsaj.dense.compute_gradients_2D / render_projected),
written from SURVEY.md Appendix A.4 and the docstring of oracle/dense_oracle.py::dense_backward, with a per-Gaussian error model
and a `mutant=` switch.  TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_dense.py and tests/test_gpu_dense.py.

The operation (depth-sorted Gaussians i = 0 .. N-1, pixel p, D = p - mu_i, fp32 inputs taken as they are):
    Sigma^-1 = [[d, -b], [-c, a]] / (a d - b c)                         q = Sigma^-1 D,  r = D^T Sigma^-1
    alpha_i  = clip(o_i exp(-1/2 r.D), 0, 1)                            T_i = prod_{j<i} (1 - alpha_j)
    after_i  = sum_{j>i} val_j alpha_j T_j  (val = colour r, g, b, depth z; g = the pixel's seeds dL/dC, dL/dD)
    dL/dalpha_i = sum_ch g_ch (val_i T_i - after_i / den_i),            den = 1 - alpha if alpha < 0.999 else 1
        naive guards: the suffix part is DROPPED where alpha >= 0.999, and an entry with |alpha| < 1e-8 adds nothing to mu / Sigma
    w = dL/dalpha alpha;  dL/dmu = sum_p w q;  dL/dSigma[a][b] = 1/2 sum_p w q_a r_b;  dL/dz = sum_p alpha T g_D;  dL/dc = sum_p alpha T g_C
    render: colour / depth of pixel p = sum_i val_i alpha_i T_i
The pixel of the normalised-coordinate variant is ((col - cx) / fx, (row - cy) / fy) formed in fp64 and rounded to fp32, as in the kernel.

Error model -- that of oracle.error_model / helpers.assert_grads_close layer (A) without cut-off flips.  Per Gaussian and component
    |fp32 evaluation - value| <= MASS_TOL * mass + COND_K * cond + 1e-37          (exactly 0 where mass == 0)
  mass = sum_p |term|: a different fp32 summation order and the roundings of the term's own products move the sum by a small multiple
         of eps * mass.  dL/dalpha enters as the sum of the absolute values of its parts, A = sum_ch |g_ch| (|val| T + |after| / den),
         not as their net: the parts cancel, and an fp32 evaluation rounds them at the size of the parts.
  cond = sum_p (what ANY fp32 evaluation of that term is uncertain by), eps = 2^-23, built from
    k_alpha = eps (1 + mag + cdet |e|): the relative uncertainty of alpha = o exp(e).  e = -1/2 (i00 dx^2 + (i01 + i10) dx dy + i11 dy^2)
         is a sum of three products that cancel for elongated, rotated Gaussians, so its absolute error is a few eps of
         mag = 1/2 (|i00| dx^2 + |i11| dy^2) + 1/2 |i01 + i10| |dx dy| (as helpers.borderline_pixel); the "1" is the rounding of D, of exp
         and of the product with o; cdet = (|a d| + |b c|) / |a d - b c| is the relative error, in eps, of the fp32 determinant every
         element of Sigma^-1 is divided by: a factor common to the three products, so it moves e by cdet |e|, not cdet mag.  0 where the
         clip makes alpha exactly 1 (or the exponential underflows to exactly 0): every evaluation is on the same side (the margins).
    k_T(i) = sum_{j<i} (eps + k_alpha_j alpha_j / (1 - alpha_j)): T_i is a product of (1 - alpha_j); each factor carries alpha_j's
         uncertainty amplified by alpha / (1 - alpha), each multiplication a rounding.
    k_q = eps (1 + cdet) (|i_a0 dx| + |i_a1 dy|): the rounding of Sigma^-1 itself, and of the two products of q_a (r_b alike), taken on
         the products' absolute values since they too cancel for rotated needles.
    the terms alpha T g:  |term| (k_alpha + k_T + eps)
    the terms w q (..r):  alpha |q| (U + A k_alpha) + alpha A k_q, with U the uncertainty of dL/dalpha:
         U = sum_ch |g| (|val| T (k_T + eps) + [sum_{j>i} |val_j| alpha_j T_j (k_alpha_j + k_T(j) + eps)] / den
                         + |after|_abs / den (k_alpha alpha / (1 - alpha) + 2 eps))      (the last: den = 1 - alpha and the division)
  The render has the same two quantities per pixel and channel: mass = sum_i |val_i| alpha_i T_i, cond = sum_i |.| (k_alpha + k_T + eps).

The guard decisions (alpha < 0.999, the clip of o G at 1, |alpha| < 1e-8) are NOT priced by a flip budget: restate() reports the
smallest relative distance of any (Gaussian, pixel) entry to each guard, make_case() asserts a margin (MARGIN, and four times the
entry's own k_alpha) and the seeds are chosen to have it.  An entry with o G == 1 exactly (opacity 1.0, mean on an integer pixel of
the plain grid: e == 0 in every evaluation) is on one side for everyone and is not near the clip in this sense.
"""
import functools
import json
import os

import numpy as np

import helpers as hp

EPS = 2.0 ** -23
MARGIN = 1e-4
# constants of the comparator: helpers.MASS_TOL / COND_K (the dense kernel shares reduce10 and the exponential with the tiled reverse
# compositor); profiles/r09_dense_parity.json holds the measured worst err / bound next to them
MASS_TOL = hp.MASS_TOL
COND_K = hp.COND_K
CONSTANTS_WHY = ("those of tests/helpers.py, unchanged: the device's worst err / bound is 0.18 (render of the recorded 640x480 input), 0.083 "
                 "(dL/dc) and 0.029 (dL/dmu, dL/dSigma), the fp32 oracle's 0.083 / 0.017 -- not below 0.03 on every tensor, so they are "
                 "not looser than the 10-30x practice for this kernel")
COMPONENTS = ("dL/dmu[0]", "dL/dmu[1]", "dL/dSigma[0][0]", "dL/dSigma[0][1]", "dL/dSigma[1][0]", "dL/dSigma[1][1]", "dL/dz",
              "dL/dc[0]", "dL/dc[1]", "dL/dc[2]")
TENSORS = (("mu", slice(0, 2)), ("Sigma", slice(2, 6)), ("depth", slice(6, 7)), ("color", slice(7, 10)))
MUTANTS = ("suffix_with_self", "guard_099", "totals_skip_128", "skip_ragged_block", "T_stalls_at_chunk", "sigma_swapped",
           "sigma_symmetrised", "suffix_total_minus_prefix")
DCHUNK = 128   # Gaussians per LDS chunk of k_dense_bwd
WG = 256       # pixels per workgroup


def to10(mu, S, z, c):
    """(grad_mu [N,2], grad_Sigma [N,2,2], grad_depth [N], grad_color [N,3]) -> [N,10] float64 in COMPONENTS order."""
    f = lambda a: (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).astype(np.float64)  # noqa: E731
    mu, S, z, c = f(mu), f(S), f(z), f(c)
    N = mu.shape[0]
    return np.concatenate([mu.reshape(N, 2), S.reshape(N, 4), z.reshape(N, 1), c.reshape(N, 3)], axis=1)


def pixel_grid(W, H, normalised_intrinsics=None):
    v, u = np.mgrid[0:H, 0:W]
    u, v = u.reshape(-1).astype(np.float64), v.reshape(-1).astype(np.float64)
    if normalised_intrinsics is not None:
        fx, fy, cx, cy = (float(x) for x in normalised_intrinsics)
        u, v = ((u - cx) / fx).astype(np.float32).astype(np.float64), ((v - cy) / fy).astype(np.float32).astype(np.float64)
    return u, v


def _excl_cumsum(a):
    out = np.zeros_like(a)
    np.cumsum(a[:-1], axis=0, out=out[1:])
    return out


def _suffix(a):
    """sum over j > i along axis 0."""
    return np.flip(np.cumsum(np.flip(a, axis=0), axis=0), axis=0) - a


def restate(means2D, covs2D, colors, depths, opac, grad_color, grad_depth, naive_guards=False, normalised_intrinsics=None,
            mutant=None, block=16384):
    """-> dict(value, mass, cond [N,10] float64 (COMPONENTS order); render_value, render_mass, render_cond [H*W,4] (r, g, b, depth);
    margins = dict(guard -> smallest relative distance of any entry, "scaled" -> smallest distance / (MARGIN + 4 k_alpha))).
    Inputs are the fp32 arrays the device gets (fp32 -> fp64 is exact)."""
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    H, W = np.asarray(grad_depth).shape
    HW = H * W
    mu, S = f32(means2D), f32(covs2D)
    N = mu.shape[0]
    val = np.concatenate([f32(colors).reshape(N, 3), f32(depths).reshape(N, 1)], axis=1)  # [N,4]
    o = f32(opac).reshape(N)
    g = np.concatenate([f32(grad_color).reshape(HW, 3), f32(grad_depth).reshape(HW, 1)], axis=1)  # [HW,4]
    if mutant == "skip_ragged_block":
        g = g.copy()
        g[(HW // WG) * WG:] = 0.0   # every one of the ten sums is linear in the pixel's seeds
    a, b, c, d = S[:, 0, 0], S[:, 0, 1], S[:, 1, 0], S[:, 1, 1]
    det = a * d - b * c
    cdet = ((np.abs(a * d) + np.abs(b * c)) / np.abs(det))[:, None]
    i00, i01, i10, i11 = (x[:, None] for x in (d / det, -b / det, -c / det, a / det))
    U_, V_ = pixel_grid(W, H, normalised_intrinsics)
    thr = 0.99 if mutant == "guard_099" else 0.999
    out = dict(value=np.zeros((N, 10)), mass=np.zeros((N, 10)), cond=np.zeros((N, 10)), render_value=np.zeros((HW, 4)),
               render_mass=np.zeros((HW, 4)), render_cond=np.zeros((HW, 4)))
    dist = {"0.999": np.inf, "clip": np.inf, "1e-8": np.inf}
    scaled = dict(dist)
    for p0 in range(0, HW, block):
        sl = slice(p0, min(HW, p0 + block))
        dx, dy = U_[None, sl] - mu[:, 0:1], V_[None, sl] - mu[:, 1:2]
        qx, qy = i00 * dx + i01 * dy, i10 * dx + i11 * dy
        rx, ry = dx * i00 + dy * i10, dx * i01 + dy * i11
        qxa, qya = np.abs(i00 * dx) + np.abs(i01 * dy), np.abs(i10 * dx) + np.abs(i11 * dy)
        rxa, rya = np.abs(dx * i00) + np.abs(dy * i10), np.abs(dx * i01) + np.abs(dy * i11)
        e = -0.5 * (rx * dx + ry * dy)
        mag = 0.5 * (np.abs(i00) * dx * dx + np.abs(i11) * dy * dy) + 0.5 * np.abs(i01 + i10) * np.abs(dx * dy)
        with np.errstate(over="ignore", under="ignore"):
            og = o[:, None] * np.exp(e)
        alpha = np.clip(og, 0.0, 1.0)
        k_a = np.where((og >= 1.0) | (alpha == 0.0), 0.0, EPS * (1.0 + mag + cdet * np.abs(e)))
        # ---- distances to the guards
        for key, guard, dd in (("0.999", 0.999, np.abs(alpha - 0.999) / 0.999),
                               ("clip", 1.0, np.where((og == 1.0) & (e == 0.0), np.inf, np.abs(og - 1.0))),
                               ("1e-8", 1e-8, np.abs(np.abs(alpha) - 1e-8) / 1e-8)):
            dist[key] = min(dist[key], float(dd.min()))
            # (k_a is relative to the entry's own o G: next to the guard's value it weighs o G / guard)
            scaled[key] = min(scaled[key], float((dd / (MARGIN + 4.0 * k_a * np.abs(og) / guard)).min()))
        one_m = 1.0 - alpha
        step = one_m.copy()
        if mutant == "T_stalls_at_chunk":
            step[DCHUNK - 1::DCHUNK] = 1.0
        T = np.ones_like(alpha)
        np.cumprod(step[:-1], axis=0, out=T[1:])
        with np.errstate(divide="ignore", invalid="ignore"):
            amp = np.where(alpha < 1.0, alpha / one_m, 0.0)
        k_T = _excl_cumsum(np.where(alpha < 1.0, EPS + k_a * amp, 0.0))
        aT = alpha * T
        k_aT = k_a + k_T + EPS
        lt = alpha < thr
        den = np.where(lt, one_m, 1.0)
        keep = np.where(naive_guards and mutant != "guard_099", lt, True).astype(np.float64)
        k_den = np.where(lt, k_a * amp, 0.0) + 2.0 * EPS
        dLda, A, Uq = np.zeros_like(alpha), np.zeros_like(alpha), np.zeros_like(alpha)
        for ch in range(4):
            contrib = val[:, ch:ch + 1] * aT
            gch, ag, av = g[None, sl, ch], np.abs(g[None, sl, ch]), np.abs(val[:, ch:ch + 1])
            out["render_value"][sl, ch] = contrib.sum(axis=0)
            out["render_mass"][sl, ch] = np.abs(contrib).sum(axis=0)
            out["render_cond"][sl, ch] = (np.abs(contrib) * k_aT).sum(axis=0)
            after = _suffix(contrib)
            if mutant == "suffix_with_self":
                after = after + contrib
            if mutant == "totals_skip_128" and N > DCHUNK:
                after = after - contrib[DCHUNK:DCHUNK + 1]
            if mutant == "suffix_total_minus_prefix":   # the kernel before this restatement existed: fp64 total - fp64 prefix
                c32 = (val[:, ch:ch + 1].astype(np.float32) * aT.astype(np.float32)).astype(np.float64)
                pre = np.cumsum(c32, axis=0)
                after = (pre[-1:] - pre).astype(np.float32).astype(np.float64)
            after_abs = _suffix(np.abs(contrib))
            after_unc = _suffix(np.abs(contrib) * k_aT)
            dLda += gch * (val[:, ch:ch + 1] * T - keep * after / den)
            A += ag * (av * T + keep * after_abs / den)
            Uq += ag * (av * T * (k_T + EPS) + keep * (after_unc / den + after_abs / den * k_den))
        skip = (np.abs(alpha) < 1e-8) if naive_guards else np.zeros_like(alpha, bool)
        w = np.where(skip, 0.0, dLda * alpha)
        wA = np.where(skip, 0.0, A * alpha)
        wU = np.where(skip, 0.0, alpha * (Uq + A * k_a))
        k_q = EPS * (1.0 + cdet)
        terms = [(w * qx, wA * np.abs(qx), wU * np.abs(qx) + wA * k_q * qxa),
                 (w * qy, wA * np.abs(qy), wU * np.abs(qy) + wA * k_q * qya)]
        for q_, qa_ in ((qx, qxa), (qy, qya)):
            for r_, ra_ in ((rx, rxa), (ry, rya)):
                terms.append((0.5 * w * q_ * r_, 0.5 * wA * np.abs(q_ * r_),
                              0.5 * (wU * np.abs(q_ * r_) + wA * k_q * (qa_ * np.abs(r_) + np.abs(q_) * ra_))))
        for ch in (3, 0, 1, 2):
            t = aT * g[None, sl, ch]
            terms.append((t, np.abs(t), np.abs(t) * k_aT))
        for k, (tv, tm, tc) in enumerate(terms):
            out["value"][:, k] += tv.sum(axis=1)
            out["mass"][:, k] += tm.sum(axis=1)
            out["cond"][:, k] += tc.sum(axis=1)
    if mutant == "sigma_swapped":
        out["value"][:, [3, 4]] = out["value"][:, [4, 3]]
    if mutant == "sigma_symmetrised":
        out["value"][:, 3] = out["value"][:, 4] = 0.5 * (out["value"][:, 3] + out["value"][:, 4])
    out["margins"] = dict(dist, scaled=scaled)
    return out


def bound(r, key="", mass_tol=None, cond_k=None):
    mass_tol = MASS_TOL if mass_tol is None else mass_tol
    cond_k = COND_K if cond_k is None else cond_k
    return mass_tol * r[key + "mass"] + cond_k * r[key + "cond"] + 1e-37


def assert_dense_close(got, restated, tag, mass_tol=None, cond_k=None):
    """got: (grad_mu, grad_Sigma, grad_depth, grad_color) or an [N,10] array.  Every row and component within its own bound, exactly
    zero where no term contributes.  -> dict(tensor -> worst err / bound)."""
    have = to10(*got) if isinstance(got, (tuple, list)) else np.asarray(got, np.float64)
    want, mass = restated["value"], restated["mass"]
    assert have.shape == want.shape, (tag, have.shape, want.shape)
    assert np.isfinite(have).all(), (tag, "non-finite gradient in row %d" % int(np.nonzero(~np.isfinite(have).all(axis=1))[0][0]))
    ratio = np.abs(have - want) / bound(restated, "", mass_tol, cond_k)
    i, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[i, k] <= 1.0, "%s: %s of Gaussian %d (of %d): got %.9e want %.9e, error %.3e = %.3g x bound (sum|terms| %.3e, cond %.3e)" % (
        tag, COMPONENTS[k], i, have.shape[0], have[i, k], want[i, k], abs(have[i, k] - want[i, k]), ratio[i, k], mass[i, k],
        restated["cond"][i, k])
    stray = (mass == 0) & (have != 0)
    if stray.any():
        i, k = (int(x[0]) for x in np.nonzero(stray))
        raise AssertionError("%s: %s of Gaussian %d is %.3e where no pixel contributes" % (tag, COMPONENTS[k], i, have[i, k]))
    return {nm: float(ratio[:, s].max()) for nm, s in TENSORS}


def assert_render_close(img, dep, restated, tag, mass_tol=None, cond_k=None):
    """Dense render (colour [H,W,3], depth [H,W]) against the per-pixel bound.  -> dict(color, depth -> worst err / bound)."""
    f = lambda a: (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).astype(np.float64)  # noqa: E731
    HW = restated["render_value"].shape[0]
    have = np.concatenate([f(img).reshape(HW, 3), f(dep).reshape(HW, 1)], axis=1)
    assert np.isfinite(have).all(), (tag, "non-finite pixel")
    ratio = np.abs(have - restated["render_value"]) / bound(restated, "render_", mass_tol, cond_k)
    p, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[p, k] <= 1.0, "%s: channel %d of pixel %d: got %.9e want %.9e = %.3g x bound" % (
        tag, k, p, have[p, k], restated["render_value"][p, k], ratio[p, k])
    assert not ((restated["render_mass"] == 0) & (have != 0)).any(), (tag, "non-zero pixel where nothing contributes")
    return dict(color=float(ratio[:, :3].max()), depth=float(ratio[:, 3].max()))


def tau_bound(order, restated, dmu_all, dcov_all, xyz_world, w2c, mass_tol=None, cond_k=None):
    """The per-row bounds carried through assemble_dL_dtau in fp64: the chain rule is linear in the four gradient arrays, so
    sum_i |coefficient| x bound is what the end-to-end dL/dtau of two evaluations inside the bounds may differ by -- for the mu,
    Sigma and depth parts; the SH part is returned by sh_tau_bound()."""
    bd = bound(restated, "", mass_tol, cond_k)
    w2c = np.asarray(w2c, np.float64)
    tau = np.zeros(6)
    for i, idx in enumerate(np.asarray(order)):
        tau += bd[i, 0:2] @ np.abs(np.asarray(dmu_all, np.float64)[idx]) + bd[i, 2:6] @ np.abs(np.asarray(dcov_all, np.float64)[idx])
        pc = w2c @ np.append(np.asarray(xyz_world, np.float64)[idx], 1.0)
        tau += bd[i, 6] * np.abs(np.array([0, 0, 1, pc[1], -pc[0], 0.0]))
    return tau


def sh_tau_bound(order, restated, xyz_world, campos, sh, deg, mass_tol=None, cond_k=None):
    """|d tau / d g_c| x bound of dL/dc, one unit colour gradient at a time (the SH part is linear in dL/dc; clamped channels are
    masked inside it)."""
    from oracle import dense_oracle as dor

    bd = bound(restated, "", mass_tol, cond_k)
    xyz, cp = np.asarray(xyz_world, np.float64), np.asarray(campos, np.float64)
    _, raw = dor.colors_from_sh(np.asarray(sh, np.float64), dor.view_dirs(xyz, cp), deg)
    tau = np.zeros(6)
    for i, idx in enumerate(np.asarray(order)):
        dorig = xyz[idx] - cp
        dn = dorig / (np.linalg.norm(dorig) + 1e-8)
        for ch in range(3):
            if raw[idx, ch] < 0.0:
                continue
            unit = np.zeros(3)
            unit[ch] = 1.0
            tau[:3] += bd[i, 7 + ch] * np.abs(dor.dnormvdv(dorig, dor.sh_dcolor_ddir(np.asarray(sh, np.float64)[idx], dn, unit, deg)))
    return tau


# ---- generated cases -------------------------------------------------------------------------------------------------------------
KINDS = ("stack", "saturated", "needles", "offscreen")
NAIVE_KINDS = ("saturated", "offscreen")   # run with naive_guards on and off: their 1e-8 margin is asserted too
# (kind, N, W, H, seed, seeds): every N in {1, 2, 127, 128, 129, 255, 256, 257, 300} at least once on an image with H W % 256 != 0
# (17x15 = 255 pixels, fewer than one workgroup; 33x17 = 561), every kind at N = 129 and N = 300, every image size at least once
CASES = (
    ("stack", 1, 17, 15, 1, "normal"), ("stack", 2, 33, 17, 2, "sign"), ("stack", 127, 16, 16, 3, "sign"),
    ("stack", 128, 33, 17, 4, "normal"), ("stack", 129, 17, 15, 5, "sign"), ("stack", 255, 33, 17, 6, "sign"),
    ("stack", 256, 64, 48, 7, "normal"), ("stack", 257, 33, 17, 8, "sign"), ("stack", 300, 64, 48, 9, "sign"),
    ("saturated", 2, 16, 16, 11, "sign"), ("saturated", 127, 17, 15, 12, "normal"), ("saturated", 129, 33, 17, 13, "sign"),
    ("saturated", 300, 33, 17, 14, "sign"),
    ("needles", 128, 16, 16, 21, "sign"), ("needles", 129, 64, 48, 22, "sign"), ("needles", 256, 33, 17, 23, "normal"),
    ("needles", 300, 17, 15, 24, "sign"),
    ("offscreen", 1, 33, 17, 31, "sign"), ("offscreen", 129, 16, 16, 32, "sign"), ("offscreen", 255, 64, 48, 73, "normal"),
    ("offscreen", 257, 17, 15, 74, "sign"), ("offscreen", 300, 33, 17, 115, "sign"),
)
NORMALISED_CASE = ("needles", 129, 64, 48, 22, "sign")   # run once more in the normalised-coordinate variant


def case_id(case):
    return "%s-%d-%dx%d" % case[:4]


def _covs(rng, N, s_major, ratio):
    th = rng.uniform(0, np.pi, N)
    s1, s2 = s_major, s_major / ratio
    c, s = np.cos(th), np.sin(th)
    S = np.empty((N, 2, 2))
    S[:, 0, 0] = c * c * s1 ** 2 + s * s * s2 ** 2
    S[:, 1, 1] = s * s * s1 ** 2 + c * c * s2 ** 2
    S[:, 0, 1] = S[:, 1, 0] = c * s * (s1 ** 2 - s2 ** 2)
    return S


def make_inputs(kind, N, W, H, seed, seeds="sign"):
    """The fp32 arrays of one case (no assertion): dict(means2D, covs2D, colors, depths, opac, grad_color, grad_depth)."""
    assert kind in KINDS, kind
    rng = np.random.default_rng(1000 * seed + N)
    size = float(max(W, H))
    centre = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    if kind == "stack":      # every Gaussian covers the whole image: T falls through 1e-20 at the back
        mu = centre + rng.normal(0, 0.75, (N, 2))
        S = _covs(rng, N, rng.uniform(1.5, 3.0, N) * size, rng.uniform(1.0, 2.0, N))
        o = rng.uniform(0.3, 0.9, N)
    elif kind == "saturated":
        mu = np.stack([rng.uniform(0, W - 1, N), rng.uniform(0, H - 1, N)], axis=1)
        S = _covs(rng, N, rng.uniform(0.8, 2.5, N), rng.uniform(1.0, 1.5, N))
        o = rng.uniform(0.05, 0.6, N)
        cls = rng.integers(0, 6, N) if N > 2 else np.arange(N)
        on_grid = cls <= 2
        mu[on_grid] = np.round(mu[on_grid])
        o[cls == 0] = 1.0                                           # alpha == 1 exactly at the centre: T -> 0, den = 1
        o[cls == 1] = rng.uniform(0.9993, 0.9998, (cls == 1).sum())    # alpha >= 0.999 at the centre pixel only
        o[cls == 2] = rng.uniform(0.99, 0.9987, (cls == 2).sum())       # ... and just below it
        o[cls == 3] = 1.5                                           # clipped over a disc
    elif kind == "needles":  # covariance condition numbers up to 1e4 (axis ratio up to 100), rotated, means off the grid
        mu = np.stack([rng.uniform(0, W - 1, N), rng.uniform(0, H - 1, N)], axis=1) + 0.37
        S = _covs(rng, N, rng.uniform(3.0, 12.0, N), 10.0 ** rng.uniform(0.0, 2.0, N))
        o = rng.uniform(0.2, 0.9, N)
    else:                    # offscreen: means up to several sigma outside, alphas below 1e-8, exponents that underflow
        s = rng.uniform(1.5, 5.0, N)
        ratio = rng.uniform(1.0, 2.0, N)
        mu = np.stack([rng.uniform(-3 * s, W - 1 + 3 * s), rng.uniform(-3 * s, H - 1 + 3 * s)], axis=1)
        o = np.where(rng.integers(0, 3, N) == 0, 10.0 ** rng.uniform(-10, -6, N), rng.uniform(0.05, 0.8, N))
        tiny = rng.integers(0, 8, N) == 0
        s = np.where(tiny, rng.uniform(0.15, 0.4, N), s)            # exp underflows a few pixels from the mean
        if N > 2:
            s[N // 2], mu[N // 2] = 0.2, (W + 20.0, H + 20.0)       # no pixel contributes at all: the row is exactly zero
        S = _covs(rng, N, s, ratio)
    col = rng.uniform(0.0, 1.0, (N, 3))
    z = np.sort(rng.uniform(1.0, 4.0, N))
    if seeds == "sign":
        gc, gd = rng.choice([-1.0, 0.0, 1.0], size=(H, W, 3)), rng.choice([-1.0, 0.0, 1.0], size=(H, W))
    else:
        gc, gd = rng.normal(size=(H, W, 3)), rng.normal(size=(H, W))
    f = np.float32
    return dict(means2D=mu.astype(f), covs2D=S.astype(f), colors=col.astype(f), depths=z.astype(f), opac=o.astype(f),
                grad_color=gc.astype(f), grad_depth=gd.astype(f))


def normalised(inp, W, H):
    """The same Gaussians in normalised image coordinates -> (inputs, (fx, fy, cx, cy))."""
    fx = fy = 0.9 * W
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    out = dict(inp)
    out["means2D"] = ((inp["means2D"].astype(np.float64) - [cx, cy]) / [fx, fy]).astype(np.float32)
    out["covs2D"] = (inp["covs2D"].astype(np.float64) / np.array([[fx * fx, fx * fy], [fy * fx, fy * fy]])).astype(np.float32)
    return out, (fx, fy, cx, cy)


def args_of(inp):
    return tuple(inp[k] for k in ("means2D", "covs2D", "colors", "depths", "opac", "grad_color", "grad_depth"))


def check_margins(margins, naive, tag):
    keys = ("0.999", "clip") + (("1e-8",) if naive else ())
    for k in keys:
        assert margins[k] >= MARGIN and margins["scaled"][k] >= 1.0, "%s: an entry is within %.2e (%.2f of its margin) of the %s guard" % (
            tag, margins[k], margins["scaled"][k], k)


@functools.lru_cache(maxsize=None)
def make_case(kind, N, W, H, seed, seeds="sign", naive=False, variant="pixel"):
    """-> (inputs, intrinsics or None, restatement), margins and reach asserted.  Cached: the arrays are shared, leave them unchanged."""
    inp = make_inputs(kind, N, W, H, seed, seeds)
    intr = None
    if variant == "normalised":
        inp, intr = normalised(inp, W, H)
    r = restate(*args_of(inp), naive_guards=naive, normalised_intrinsics=intr)
    tag = "%s-%d-%dx%d" % (kind, N, W, H)
    check_margins(r["margins"], naive or kind in NAIVE_KINDS, tag)
    if kind == "stack" and N >= 127:   # the rows a tensor-wide tolerance cannot see
        for nm, s in TENSORS:
            v, m = np.abs(r["value"][:, s]), r["mass"][:, s]
            hidden = (v.max(axis=1) < 1e-6 * v.max()) & (m.min(axis=1) > 1e-30)
            assert hidden.sum() >= 8, (tag, nm, "only %d rows six orders below the tensor's maximum" % hidden.sum())
    for a in inp.values():
        a.setflags(write=False)
    return inp, intr, r


def runs():
    """Every (case, naive, variant) the GPU tests and the CPU feasibility test go through."""
    out = []
    for case in CASES:
        out.append((case, False, "pixel"))
        if case[0] in NAIVE_KINDS:
            out.append((case, True, "pixel"))
    out.append((NORMALISED_CASE, False, "normalised"))
    return out


def run_id(run):
    case, naive, variant = run
    return case_id(case) + ("-naive" if naive else "") + ("-normalised" if variant == "normalised" else "")


# ---- measured worst err / bound (profiles/r09_dense_parity.json, written when GSAJ_WRITE_PARITY is set) ---------------------------
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r09_dense_parity.json")
WORST = {}


def note(who, test, ratios):
    """who: "oracle_fp32_cpu" or "device_mi355x"; ratios: dict(tensor -> err / bound of one case); the worst per test is kept."""
    slot = WORST.setdefault(who, {}).setdefault(test, {})
    for k, v in ratios.items():
        slot[k] = max(slot.get(k, 0.0), float(v))
    if os.environ.get("GSAJ_WRITE_PARITY"):
        doc = {}
        if os.path.exists(PARITY):
            with open(PARITY) as fh:
                doc = json.load(fh)
        doc["what"] = ("worst |evaluation - fp64 restatement| / bound per tensor and test (tests/dense_restated.py): the fp32 NumPy oracle "
                       "from tests/test_cpu_dense.py, the device from tests/test_gpu_dense.py")
        doc["constants"] = dict(MASS_TOL=MASS_TOL, COND_K=COND_K, helpers_MASS_TOL=hp.MASS_TOL, helpers_COND_K=hp.COND_K, why=CONSTANTS_WHY)
        doc.setdefault("worst_err_over_bound", {})[who] = WORST[who]
        with open(PARITY, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
