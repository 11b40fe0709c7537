"""NumPy restatements (float64) of the Gauss-Newton tracking path -- csrc/pose_jac.hip: k_splat_jac, k_render_jac, k_gn_reduce,
k_gn_step; csrc/loss_terms.h: loss_pixel_gn -- with the comparators the GPU tests use and a `mutant=` switch for the canaries.
TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_gn.py, tests/test_gpu_pose_jacobian.py and tests/test_gpu_gn_tracker.py.

  gaussian_rows      d(mean2D, conic, depth, colour)/dtau per Gaussian [P,9,6]: the oracle's fp64 chain applied to unit sums
  jacobian           the forward-mode compositor over the oracle's binned state -> J [H,W,4,6]
  irls               (i) seeds s and curvatures h [4,H,W] of the tracking loss from images, ground truth and masks, with the error an
                     fp32 evaluation of each may carry
  normal_equations   (ii) H = sum h J^T J, g = sum s J from a Jacobian array, with sum|term| and an error bound per element
  lm_step            (iii) accept / reject, damping, Cholesky, Exp(tau) W2C
  jac_scene          the 72x40 scene of the GPU Jacobian tests, every planted case named

Mutants: "drop_alpha_S" (the -alpha S term of the recurrence), "no_background" (the -bg T_final S_final term), "delta_signed_r"
(the curvature's max(|r|, delta) taken on r instead of |r|), "not_restored_on_reject" (a rejected step solves from the rejected pose).
"""
import math

import numpy as np

import loss_restated as lr
from gsaj import synthetic as syn
from oracle import oracle as orc

EPS = 2.0 ** -24   # one fp32 rounding, relative
F = np.float32
MUTANTS = ("drop_alpha_S", "no_background", "delta_signed_r", "not_restored_on_reject")
SYM6 = [(k, l) for k in range(6) for l in range(k, 6)]

# Roundings between a pixel's (s, h, J) and an element of the kernel's H / g (k_render_jac's epilogue, k_gn_reduce / k_gn_step):
#   g: the product s J 1 + four channels added 4 + the 64-lane butterfly 6 + fp64 sum over rows rounded to fp32 once 1 = 12
#   H: the products (h J_k) J_l 2 + 4 + 6 + 1 = 13
G_ROUNDINGS = 12
H_ROUNDINGS = 13


# ---- per-Gaussian derivative rows -----------------------------------------------------------------------------------------------
def gaussian_rows(st, projmatrix_raw):
    """[P,9,6] float64: rows 0..8 = d(mean2D x, y (NDC-scaled as the backward carries them), conic a, b, c, depth, colour r, g, b)/dtau:
    the chain is linear in its sums, so the row of sum j is the dL/dtau it returns for sum j = 1, all others 0."""
    P = st["P"]
    rows = np.zeros((P, 9, 6))
    for j in range(9):
        m2, cn, dc, dd = np.zeros((P, 3), F), np.zeros((P, 4), F), np.zeros((P, 3), F), np.zeros((P, 1), F)
        if j < 2:
            m2[:, j] = 1
        elif j < 5:
            cn[:, (0, 1, 3)[j - 2]] = 1   # dL_dconic is stored (a, b, -, c)
        elif j == 5:
            dd[:] = 1
        else:
            dc[:, j - 6] = 1
        rows[:, j] = orc.chain(st, m2, cn, dc, dd, projmatrix_raw, f64=True)["dL_dtau"]
    return rows


# ---- forward-mode compositor ----------------------------------------------------------------------------------------------------
def jacobian(st, rows, bg, mutant=None):
    """J [H,W,4,6] float64 (rows r, g, b, depth) and the re-derived colour [3,H,W] / depth [H,W]: every pixel walks its tile's list
    front to back up to its n_contrib, with the gates of the compositor (power > 0 and alpha < 1/255 skipped, alpha capped at 0.99
    WITHOUT gating the derivative):  J_ch += T (alpha dc + c (dalpha - alpha S)),  S += dalpha / (1 - alpha),  T *= 1 - alpha,
    then J_ch -= bg T_final S_final for the colour rows."""
    assert mutant in (None, "drop_alpha_S", "no_background"), mutant
    W, H = st["W"], st["H"]
    gx = (W + 15) // 16
    m2d, co = st["means2D"].astype(np.float64), st["conic_opacity"].astype(np.float64)
    feat, dep = st["features"].astype(np.float64), st["depths"].astype(np.float64)
    pl, ranges, ncon = st["point_list"], st["ranges"], st["n_contrib"]
    bg = np.asarray(bg, np.float64)
    J = np.zeros((H, W, 4, 6))
    img = np.zeros((4, H, W))
    for tile in range(ranges.shape[0]):
        ty, tx = divmod(tile, gx)
        ys, xs = np.mgrid[ty * 16:min(H, ty * 16 + 16), tx * 16:min(W, tx * 16 + 16)]
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        n = ys.size
        last = ncon[ys, xs].astype(np.int64)
        T, S, Jt, C = np.ones(n), np.zeros((n, 6)), np.zeros((n, 4, 6)), np.zeros((n, 4))
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        for pos in range(r0, min(r1, r0 + int(last.max(initial=0)))):
            i = int(pl[pos])
            dx, dy = m2d[i, 0] - xs, m2d[i, 1] - ys
            a, b, c, o = co[i]
            power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
            oG = o * np.exp(np.minimum(power, 0.0))
            valid = (pos - r0 + 1 <= last) & (power <= 0) & (np.minimum(0.99, oG) >= 1.0 / 255.0)
            oG = np.where(valid, oG, 0.0)
            alpha = np.minimum(0.99, oG)
            f = np.stack([-(a * dx + b * dy) * 0.5 * W, -(c * dy + b * dx) * 0.5 * H, -0.5 * dx * dx, -0.5 * dx * dy, -0.5 * dy * dy], 1)
            dA = (oG[:, None] * f) @ rows[i, :5]                                  # [n,6]
            cv = np.array([feat[i, 0], feat[i, 1], feat[i, 2], dep[i]])
            e = T[:, None] * (dA - (0.0 if mutant == "drop_alpha_S" else alpha[:, None] * S))
            Jt += cv[None, :, None] * e[:, None, :]
            w = alpha * T
            Jt[:, :3] += w[:, None, None] * rows[i, 6:9][None]
            Jt[:, 3] += w[:, None] * rows[i, 5][None]
            C += w[:, None] * cv[None]
            S += dA / (1.0 - alpha)[:, None]
            T = T * (1.0 - alpha)
        if mutant != "no_background":
            Jt[:, :3] -= bg[None, :, None] * (T[:, None] * S)[:, None, :]
        J[ys, xs] = Jt
        img[:3, ys, xs] = (C[:, :3] + T[:, None] * bg[None]).T
        img[3, ys, xs] = C[:, 3]
    return J, img[:3], img[3]


def contract(J, s_color, s_depth):
    """sum_p sum_ch s[ch,p] J_p[ch,:] in float64 -> [6]."""
    s = np.concatenate([np.asarray(s_color, np.float64).reshape(3, -1), np.asarray(s_depth, np.float64).reshape(1, -1)])
    return np.einsum("cp,pck->k", s, np.asarray(J, np.float64).reshape(-1, 4, 6))


# ---- (i) seeds and curvatures of the tracking loss ------------------------------------------------------------------------------
def irls(flags, alpha, rgb_thr, image, depth, opacity, gt, gt_depth=None, mask=None, a=None, b=None, delta=0.0, mutant=None):
    """-> dict(s, h [4,H,W] float64 (r, g, b, depth), err_s, err_h: what an fp32 evaluation may be off by, per element).
    r_ch = m (e^a C_ch + b - gt_ch), r_d = dm (D - gt_d); kappa_rgb = k_rgb w_rgb, kappa_d = k_d (loss_restated's gates and constants):
        s = kappa (dr/dC) clamp(r / delta, -1, 1)      (delta == 0: kappa (dr/dC) sgn(r), loss_restated's seed exactly)
        h = kappa (dr/dC)^2 / max(|r|, delta)          (0 where the gate is closed, or r == 0 with delta == 0)
    Error model (EPS = 2^-24 per rounding).  The colour residual is a DIFFERENCE rounded at the size of its parts, part = |e^a C| +
    |b| + |gt| (loss_restated): |dr| <= 6 EPS part (expf 2 ulp = 4, the fma 1, the subtraction 1).  It enters s where |r| < delta
    (s = kappa' r / delta) and h where |r| > delta (h = kappa' / |r|), or flips a sign outright where delta == 0 and |r| <= 64 EPS
    part.  On top: 8 roundings on the way to s, 10 to h (k_rgb's division, expf, the products, the division).  Depth: d - gt_d is one
    subtraction of two inputs, relative: 6 roundings in all for s, 5 for h."""
    assert mutant in (None, "delta_signed_r"), mutant
    w = lr.restate(flags, alpha, rgb_thr, image, depth, opacity, gt, gt_depth, mask, a, b)
    tracking, mono = bool(flags & lr.TRACKING), bool(flags & lr.MONOCULAR)
    noexp = bool(flags & lr.NO_EXPOSURE)
    _, H, W = np.shape(image)
    HW = H * W
    c, g = np.asarray(image, F).reshape(3, HW).astype(np.float64), np.asarray(gt, F).reshape(3, HW).astype(np.float64)
    op = np.asarray(opacity, F).reshape(HW).astype(np.float64)
    ea = 1.0 if noexp else float(np.exp(np.float64(F(a))))
    eb = 0.0 if noexp else float(F(b))
    al = np.float64(F(alpha))
    k_rgb = (1.0 if mono else al) / (3.0 * HW)
    k_d = (1.0 - al) / HW
    # the gates, as loss_restated decides them (on fp32): recovered from its seeds' masses
    gsum = (np.asarray(gt, F).reshape(3, HW)[0] + np.asarray(gt, F).reshape(3, HW)[1]) + np.asarray(gt, F).reshape(3, HW)[2]
    m = gsum > F(rgb_thr)
    if tracking:
        m = m & (np.ones(HW, bool) if mask is None else np.asarray(mask).reshape(HW) != 0)
    mf = m.astype(np.float64)
    wgt = op if tracking else np.ones(HW)
    r = (ea * c + eb - g) * mf
    part = (np.abs(ea * c) + abs(eb) + np.abs(g)) * mf
    d = float(delta)
    clip = np.sign(r) if d == 0 else np.clip(r / d, -1.0, 1.0)
    s_rgb = k_rgb * ea * wgt * (clip * mf)
    den = np.maximum(r if mutant == "delta_signed_r" else np.abs(r), d)
    kw = k_rgb * ea * wgt * mf
    with np.errstate(divide="ignore", invalid="ignore"):
        h_rgb = np.where(den > 0, kw * ea / np.where(den > 0, den, 1.0), 0.0)
    in_lin = (np.abs(r) <= d * (1 + 1e-3)) & (d > 0)          # s is linear in r here
    in_inv = np.abs(r) >= d * (1 - 1e-3)                      # h is 1 / |r| here
    flip = (d == 0) & (np.abs(r) <= 64 * EPS * part) & (mf > 0)
    err_s = EPS * (8 * np.abs(s_rgb) + np.where(in_lin, 6 * kw * part / (d if d > 0 else 1.0), 0.0)) + np.where(flip, 2 * kw, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        err_h = EPS * np.abs(h_rgb) * (10 + np.where(in_inv & (np.abs(r) > 0), 6 * part / np.where(np.abs(r) > 0, np.abs(r), 1.0), 0.0))
    s, h, es, eh = np.zeros((4, HW)), np.zeros((4, HW)), np.zeros((4, HW)), np.zeros((4, HW))
    s[:3], h[:3], es[:3], eh[:3] = s_rgb, h_rgb, err_s, err_h
    if not mono:
        dd, gd = np.asarray(depth, F).reshape(HW), np.asarray(gt_depth, F).reshape(HW)
        dm = gd > F(0.01)
        if tracking:
            dm = dm & (np.asarray(opacity, F).reshape(HW) > F(0.95))
        dmf = dm.astype(np.float64)
        rd = (dd.astype(np.float64) - gd.astype(np.float64)) * dmf
        clipd = np.sign(rd) if d == 0 else np.clip(rd / d, -1.0, 1.0)
        s[3] = k_d * dmf * clipd * dmf
        dend = np.maximum(rd if mutant == "delta_signed_r" else np.abs(rd), d)
        h[3] = np.where(dend > 0, k_d * dmf / np.where(dend > 0, dend, 1.0), 0.0)
        es[3], eh[3] = 6 * EPS * np.abs(s[3]), 5 * EPS * np.abs(h[3])
    assert d > 0 or np.array_equal(s[:3].reshape(3, H, W), w["value"]["dL_dcolor"]), "delta == 0: the seed is the backward's"
    return dict(s=s.reshape(4, H, W), h=h.reshape(4, H, W), err_s=es.reshape(4, H, W), err_h=eh.reshape(4, H, W), loss=w)


# ---- (ii) normal equations --------------------------------------------------------------------------------------------------------
def normal_equations(J, s=None, h=None, err_s=None, err_h=None):
    """J [H,W,4,6]; s, h [4,H,W] -> dict(g [6], H [6,6], g_mass, H_mass = sum|term| per element, g_bound, H_bound = what an fp32
    evaluation in k_render_jac's order may be off by per element: (roundings per term + reduction depth) EPS sum|term|, plus the
    seeds' / curvatures' own errors carried through |J|)."""
    Jp = np.asarray(J, np.float64).reshape(-1, 4, 6)
    out = {}
    if s is not None:
        sp = np.asarray(s, np.float64).reshape(4, -1).T                       # [p,4]
        out["g"] = np.einsum("pc,pck->k", sp, Jp)
        out["g_mass"] = np.einsum("pc,pck->k", np.abs(sp), np.abs(Jp))
        out["g_bound"] = G_ROUNDINGS * EPS * out["g_mass"]
        if err_s is not None:
            out["g_bound"] = out["g_bound"] + np.einsum("pc,pck->k", np.asarray(err_s, np.float64).reshape(4, -1).T, np.abs(Jp))
    if h is not None:
        hp_ = np.asarray(h, np.float64).reshape(4, -1).T
        out["H"] = np.einsum("pc,pck,pcl->kl", hp_, Jp, Jp)
        out["H_mass"] = np.einsum("pc,pck,pcl->kl", np.abs(hp_), np.abs(Jp), np.abs(Jp))
        for k in ("H", "H_mass"):   # the 21 stored elements, mirrored (the kernel forms the upper triangle only)
            out[k] = np.triu(out[k]) + np.triu(out[k], 1).T
        out["H_bound"] = H_ROUNDINGS * EPS * out["H_mass"]
        if err_h is not None:
            eh = np.einsum("pc,pck,pcl->kl", np.asarray(err_h, np.float64).reshape(4, -1).T, np.abs(Jp), np.abs(Jp))
            out["H_bound"] = out["H_bound"] + np.triu(eh) + np.triu(eh, 1).T
    return out


def assert_normal_equations_close(got_H, got_g, want, tag):
    """Element by element within want's bounds; -> worst err / bound."""
    worst = 0.0
    for name, got in (("H", got_H), ("g", got_g)):
        if got is None:
            continue
        have, v, bd = np.asarray(got, np.float64), want[name], want[name + "_bound"]
        assert have.shape == v.shape and np.isfinite(have).all(), (tag, name, have)
        if name == "H":
            assert np.array_equal(have, have.T), "%s: H is not symmetric" % tag
        err = np.abs(have - v)
        bad = err > bd
        assert not bad.any(), "%s: %s element %s: got %.9e want %.9e, error %.3e = %.3g x bound (sum|term| %.3e)" % (
            tag, name, np.argwhere(bad)[0], have[bad][0], v[bad][0], err[bad][0], (err[bad] / np.maximum(bd[bad], 1e-300))[0], want[name + "_mass"][bad][0])
        worst = max(worst, float((err / np.maximum(bd, 1e-300))[bd > 0].max(initial=0.0)))
    return worst


def assert_transpose_identity(g_from_J, st, s_color, s_depth, projmatrix_raw, tol, tag):
    """sum s J against the oracle's backward under the same seeds: rel_err (tests/helpers.py) below tol.  -> the error."""
    import helpers as hp
    want = orc.backward(st, s_color, s_depth, projmatrix_raw)["dL_dtau_sum"]
    e = hp.rel_err(g_from_J, want)
    assert e < tol, "%s: sum s J differs from the oracle's dL/dtau: rel err %.3e (limit %.1e)\n got %s\nwant %s" % (tag, e, tol, g_from_J, want)
    return e


# ---- (iii) the Levenberg-Marquardt step -------------------------------------------------------------------------------------------
def se3_exp(tau):
    """Exp of [rho, theta] -> 4x4 (reference utils/pose_utils.py:25-73, small-angle branches at 1e-5), float64."""
    rho, th = np.asarray(tau[:3], np.float64), np.asarray(tau[3:], np.float64)
    Wm = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]])
    W2 = Wm @ Wm
    ang = float(np.sqrt((th * th).sum()))
    if ang < 1e-5:
        R, V = np.eye(3) + Wm + 0.5 * W2, np.eye(3) + 0.5 * Wm + W2 / 6.0
    else:
        R = np.eye(3) + math.sin(ang) / ang * Wm + (1 - math.cos(ang)) / ang ** 2 * W2
        V = np.eye(3) + (1 - math.cos(ang)) / ang ** 2 * Wm + (ang - math.sin(ang)) / ang ** 3 * W2
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ rho
    return T


def sym6(h21):
    out = np.zeros((6, 6))
    for n, (k, l) in enumerate(SYM6):
        out[k, l] = out[l, k] = h21[n]
    return out


def fold_rows(rows, groups):
    """The step kernels' sum of the partial rows [n, ROW] (csrc/gn_state.h gn_sum_rows) in its stated order, in float64: row group r
    of `groups` (1024 threads / ROW: 32 for the 32-float row, 16 for the joint form's 64) adds rows r, r + groups, ... in order, then
    the groups are added in order -> [ROW] float64.  Float64 addition in a fixed order is reproducible, so the float32 cast of this is
    the device's value bit for bit."""
    rows = np.asarray(rows, F).astype(np.float64)
    acc = np.zeros((groups, rows.shape[1]))
    for i in range(rows.shape[0]):
        acc[i % groups] += rows[i]
    total = acc[0].copy()
    for q in range(1, groups):
        total += acc[q]
    return total


def lm_new_state(w2c, lambda_init):
    w = np.array(w2c, np.float64).reshape(4, 4)
    return dict(w2c=w.copy(), lam=float(lambda_init), has=False, acc_loss=0.0, acc_w2c=w.copy(), H=np.zeros((6, 6)), g=np.zeros(6),
                accepted=0, rejected=0, tau=np.zeros(6), converged=False)


def lm_step(state, H, g, loss, nu, lambda_min, lambda_max, threshold, mutant=None):
    """One gsaj_pose_gn_step on (H [6,6], g [6], loss) rendered at state["w2c"]; `state` is updated in place and returned.
    H, g are kept as the fp32 values the kernel stores; everything else is float64."""
    assert mutant in (None, "not_restored_on_reject"), mutant
    st = state
    loss = float(F(loss))
    if not st["has"] or loss <= st["acc_loss"]:
        st["acc_loss"], st["acc_w2c"] = loss, st["w2c"].copy()
        st["H"], st["g"] = np.asarray(H, F).astype(np.float64), np.asarray(g, F).astype(np.float64)
        st["lam"] = max(float(F(st["lam"]) / F(nu)), lambda_min)
        st["has"] = True
        st["accepted"] += 1
    else:
        if mutant != "not_restored_on_reject":
            st["w2c"] = st["acc_w2c"].copy()
        st["lam"] = min(float(F(st["lam"]) * F(nu)), lambda_max)
        st["rejected"] += 1
    Hs, gs = st["H"], st["g"]
    A = Hs + st["lam"] * np.diag(np.diag(Hs)) + (1e-9 * np.trace(Hs) / 6.0 + 1e-30) * np.eye(6)
    ok = True
    try:
        Lc = np.linalg.cholesky(A)
        tau = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -gs))
        ok = bool(np.isfinite(tau).all())
    except np.linalg.LinAlgError:
        ok = False
    if not ok:
        tau = np.zeros(6)
        st["lam"] = min(float(F(st["lam"]) * F(nu)), lambda_max)
    tau = np.asarray(tau, F).astype(np.float64)
    new = se3_exp(tau) @ st["w2c"]
    new[3] = [0, 0, 0, 1]
    st["w2c"], st["tau"] = new, tau
    st["converged"] = ok and bool(np.sqrt((tau * tau).sum()) < threshold)
    return st


def pack_state(st, projection):
    """A restated state as the GSAJ_GN_STATE_FLOATS floats the device would hold (float64 values; H, g are not compared)."""
    s = np.zeros(136)
    w = st["w2c"]
    s[0:16] = w.reshape(16)
    s[35:51] = w.T.reshape(16)
    s[51:67] = (w.T @ np.asarray(projection, np.float64).reshape(4, 4)).reshape(16)
    s[67:70] = -np.linalg.inv(w[:3, :3]) @ w[:3, 3]
    s[70:76] = st["tau"]
    s[76] = np.sqrt((st["tau"] ** 2).sum())
    s[77] = 1.0 if st["converged"] else 0.0
    s[80], s[81], s[82], s[83], s[84] = st["lam"], st["acc_loss"], float(st["has"]), st["accepted"], st["rejected"]
    s[88:104] = st["acc_w2c"].reshape(16)
    return s


def assert_lm_state_close(dev_state, want, projection, tag):
    """dev_state: the GSAJ_GN_STATE_FLOATS floats of the device (NumPy); want: lm_step's state.  Matrices to the absolute tolerances
    tests/test_gpu_pose_step.py applies to w2c and the camera matrices; lambda and tau relative; counters and flags exactly."""
    s = np.asarray(dev_state, np.float64)
    w = s[0:16].reshape(4, 4)
    np.testing.assert_allclose(w, want["w2c"], rtol=0, atol=5e-6, err_msg="%s: w2c" % tag)
    np.testing.assert_allclose(s[88:104].reshape(4, 4), want["acc_w2c"], rtol=0, atol=5e-6, err_msg="%s: accepted w2c" % tag)
    np.testing.assert_allclose(s[35:51].reshape(4, 4), w.T, atol=0, err_msg="%s: viewmatrix" % tag)
    np.testing.assert_allclose(s[51:67].reshape(4, 4), w.T @ np.asarray(projection, np.float64).reshape(4, 4), atol=3e-5, err_msg="%s: projmatrix" % tag)
    np.testing.assert_allclose(s[67:70], -np.linalg.inv(w[:3, :3]) @ w[:3, 3], atol=2e-5, err_msg="%s: campos" % tag)
    np.testing.assert_allclose(s[70:76], want["tau"], rtol=3e-5, atol=1e-9, err_msg="%s: tau" % tag)
    np.testing.assert_allclose(s[80], want["lam"], rtol=1e-6, err_msg="%s: lambda" % tag)
    np.testing.assert_allclose(s[81], want["acc_loss"], rtol=1e-7, err_msg="%s: accepted loss" % tag)
    assert (int(s[83]), int(s[84])) == (want["accepted"], want["rejected"]), (tag, s[83], s[84], want["accepted"], want["rejected"])
    assert bool(s[77] > 0.5) == want["converged"], (tag, s[77], s[76], want["converged"])
    np.testing.assert_allclose(s[76], np.sqrt((want["tau"] ** 2).sum()), rtol=3e-5, atol=1e-9, err_msg="%s: |tau|" % tag)


# ---- the scene of the GPU Jacobian tests ------------------------------------------------------------------------------------------
JAC_W, JAC_H, JAC_BG, JAC_DEG = 72, 40, (0.1, 0.2, 0.3), 3
JAC_SEED = 3          # chosen on the CPU with the oracle alone (tests/test_cpu_gn.py asserts it): no borderline pixel for the seeds below
EMPTY_TILE = (4, 2)   # (tx, ty): no Gaussian touches it


def jac_scene(seed=JAC_SEED):
    """-> (cam, sc, planted): 72x40 (partial tiles on both edges), SH degree 3, ~400 Gaussians: a random scene plus
      stack     75 faint Gaussians over tile (1, 0): the taken list of its quadrants spans more than two 32-entry staging chunks
      cap       three opacity-0.999 splats wide enough that o G > 0.99 around their centres (the alpha cap)
      opaque    a stack of opacity-0.95 splats that ends pixels early (T < 1e-4) with Gaussians left behind it
      clamp_x / clamp_y   centres projecting beyond +-1.3 tanfov on each axis, wide enough to reach the image (cov2D clamp gates)
      near      z_c just above and just below 0.2 at the image centre
      sh_clamp  colours driven below 0 (clamp flags set)
    and tile EMPTY_TILE cleared of every Gaussian.  planted: name -> (Gaussian ids, a pixel (x, y) the case shows at)."""
    W, H = JAC_W, JAC_H
    f = 0.9 * W
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=W, H=H, fx=f, fy=f, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(300, seed, cam, z_range=(0.8, 3.0), log_scale_range=(math.log(0.01), math.log(0.06)), sh_sigma=0.3)
    rng = np.random.default_rng(1000 + seed)
    c2w = np.linalg.inv(cam["w2c"])
    extra = dict(means3D=[], scales=[], rotations=[], opacities=[], shs=[])
    planted = {}
    count = [300]

    def add(name, uvz, scale, opacity, pixel, dc=None):
        ids = []
        for (u, v, z) in uvz:
            pc = np.array([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z, 1.0])
            extra["means3D"].append((c2w @ pc)[:3])
            extra["scales"].append(np.full(3, scale) * rng.uniform(0.8, 1.25, size=3))
            extra["rotations"].append(syn.random_unit_quaternions(rng, 1)[0])
            extra["opacities"].append([opacity])
            sh = rng.normal(0.0, 0.3, size=(16, 3))
            sh[0] = rng.uniform(-1.0, 1.0, size=3) if dc is None else dc
            extra["shs"].append(sh)
            ids.append(count[0])
            count[0] += 1
        planted[name] = (ids, pixel)

    add("stack", [(rng.uniform(19, 29), rng.uniform(3, 12), 1.0 + 0.02 * k) for k in range(75)], 0.12, 0.07, (24, 7))
    add("cap", [(38.6, 22.45, 1.2), (30.4, 12.6, 1.25), (26.55, 26.4, 1.3)], 0.12, 0.999, (38, 22))   # (pixel = u - 0.5: a tenth of a pixel off pixel centres -- power = 0 is itself a borderline gate -- and apart:
    # two capped alphas in a row leave T = 1e-4, the termination threshold itself)
    add("opaque", [(61 + 0.3 * k, 9 + 0.2 * k, 0.9 + 0.03 * k) for k in range(10)], 0.05, 0.95, (61, 9))
    add("clamp_x", [(W + 12.0, 8.0, 1.5), (-13.0, 22.0, 1.6)], 0.13, 0.8, (71, 8))
    add("clamp_y", [(30.0, H + 8.0, 1.5), (40.0, -9.0, 1.6)], 0.13, 0.8, (30, 39))
    add("near", [(35.6, 19.7, 0.2004), (36.4, 20.3, 0.1996)], 0.002, 0.9, (36, 20))
    add("sh_clamp", [(8 + 3 * k, 30 + k, 1.1 + 0.1 * k) for k in range(3)], 0.06, 0.8, (8, 30), dc=np.array([-3.0, 0.4, -2.5]))
    sc = {k: np.concatenate([sc[k], np.asarray(extra[k], np.float32).reshape((-1,) + sc[k].shape[1:])]).astype(np.float32) for k in sc}
    # clear EMPTY_TILE: drop (opacity 0 would still bin them) every Gaussian whose tile rectangle reaches it
    tile = EMPTY_TILE[1] * ((W + 15) // 16) + EMPTY_TILE[0]
    for _ in range(4):
        (_, st), _ = oracle_forward(cam, sc)
        r0, r1 = st["ranges"][tile]
        if r1 <= r0:
            break
        drop = np.unique(st["point_list"][r0:r1])
        assert all(i < 300 for i in drop), "a planted Gaussian reaches the tile that must stay empty"
        keep = np.ones(sc["means3D"].shape[0], bool)
        keep[drop] = False
        newid = np.cumsum(keep) - 1
        sc = {k: v[keep] for k, v in sc.items()}
        planted = {k: ([int(newid[i]) for i in ids], px) for k, (ids, px) in planted.items()}
    else:
        raise AssertionError("tile %r could not be cleared" % (EMPTY_TILE,))
    planted["empty_tile"] = ([], (EMPTY_TILE[0] * 16 + 3, EMPTY_TILE[1] * 16 + 4))
    planted["edge_tile"] = ([], (W - 1, 20))
    return cam, sc, planted


def oracle_forward(cam, sc, record_bits=32):
    kw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"], sh_degree=JAC_DEG)
    return orc.forward(sc["means3D"], sc["opacities"], cam["viewmatrix"], cam["projmatrix"], cam["campos"], cam["tanfovx"], cam["tanfovy"],
                       cam["W"], cam["H"], np.asarray(JAC_BG, np.float32), record_bits=record_bits, **kw), kw


def jac_seeds(seed=0):
    """randn / 3HW and randn / HW, as smoke() seeds the backward."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(3, JAC_H, JAC_W)).astype(np.float32) / (3 * JAC_H * JAC_W),
            rng.normal(size=(1, JAC_H, JAC_W)).astype(np.float32) / (JAC_H * JAC_W))


def row_pixels(planted, border_mask, want=16, seed=7):
    """About 16 pixels (x, y) for the single-row check: one per planted case, then random ones; pixels the error model flags as
    borderline are left out -- at most 2 may be."""
    rng = np.random.default_rng(seed)
    px = [p for (_, p) in planted.values()]
    while len(px) < want:
        p = (int(rng.integers(0, JAC_W)), int(rng.integers(0, JAC_H)))
        if p not in px:
            px.append(p)
    keep = [p for p in px if not border_mask[p[1], p[0]]]
    assert len(px) - len(keep) <= 2, "more than 2 of the %d row pixels are borderline" % len(px)
    return keep
