"""NumPy restatements (float64) of the JOINT Gauss-Newton tracking path -- csrc/pose_jac.hip: k_render_jac<true, true>, k_gn_step<8> -- built on
tests/gn_restated.py, with the comparators the GPU tests use and a `mutant=` switch for the canaries.  TEST INFRASTRUCTURE ONLY;
shared by tests/test_cpu_gn8.py, tests/test_gpu_pose_jacobian8.py and tests/test_gpu_gn8_tracker.py.

The unknowns are x = [rho(3), theta(3), a, b].  With r_ch = m (e^a C_ch + b - gt_ch): dr_ch = m e^a (dC_ch + C_ch da + db / e^a), so
relative to the rendered colour the exposure parameters are two more Jacobian columns under gn_restated.irls's seeds and curvatures:

  J8                 [H,W,4,8] = [J, C_ch, 1 / e^a] in the colour rows, [J, 0, 0] in the depth row
  normal_equations8  H8 = sum h J8^T J8, g8 = sum s J8 with sum|term| and an error bound per element
  smooth_loss        the Huberised loss the seeds are the gradient of (for finite differences in a, b)
  lm8_step           accept / reject, damping, 8x8 Cholesky, Exp(tau) W2C, a += x[6], b += x[7]; exposure saved / restored with the pose
  restated_rows      one iteration's (H, g, loss) at a pose and an exposure: the oracle's forward + the restated Jacobian, either form

Mutants: "b_without_inv_ea" (the b column 1 instead of 1 / e^a), "a_from_ground_truth" (the a column from gt instead of the render),
"exposure_in_depth_row" (the two columns also in the depth row), "exposure_not_restored_on_reject" (a rejected step keeps the
rejected exposure).
"""
import numpy as np

import gn_restated as gn
import loss_restated as lr
from gsaj import synthetic as syn

EPS, F = gn.EPS, gn.F
MUTANTS = ("b_without_inv_ea", "a_from_ground_truth", "exposure_in_depth_row", "exposure_not_restored_on_reject")
SYM8 = [(k, l) for k in range(8) for l in range(k, 8)]

# Roundings between a pixel's (s, h, J, C, a) and an element of the kernel's H8 / g8 (the epilogue of k_render_jac<true, true>, k_gn_step<8>).
# The reduction goes through two half-wave swaps and four row rotations instead of the 6-form's six butterfly steps: the SAME depth 6,
# so the base counts are gn_restated's: g 12, H 13.  What the new columns add:
#   the a column is the forward's colour C_ch, an fp32 INPUT of both sides: its product with s (or h J) is the term's own product,
#   already among the 12 / 13 -- nothing on top;
#   the b column is 1 / e^a, computed: expf within 2 ulp = 4 roundings, the division 1 = 5 per occurrence of the column in a term
#   (once in g8[7] and in the H8 elements (k, 7), twice in (7, 7)).
A_COLUMN_ROUNDINGS = 0
B_COLUMN_ROUNDINGS = 5
G8_ROUNDINGS = np.array([gn.G_ROUNDINGS] * 6 + [gn.G_ROUNDINGS + A_COLUMN_ROUNDINGS, gn.G_ROUNDINGS + B_COLUMN_ROUNDINGS], np.float64)
_COL = np.array([0] * 6 + [A_COLUMN_ROUNDINGS, B_COLUMN_ROUNDINGS], np.float64)
H8_ROUNDINGS = gn.H_ROUNDINGS + _COL[:, None] + _COL[None, :]


def sym8(h36):
    out = np.zeros((8, 8))
    for n, (k, l) in enumerate(SYM8):
        out[k, l] = out[l, k] = h36[n]
    return out


def J8(J, image, a, gt=None, mutant=None):
    """J [H,W,4,6], image [3,H,W] (the forward's colour, fp32), a (fp32 scalar) -> [H,W,4,8] float64."""
    assert mutant in (None, "b_without_inv_ea", "a_from_ground_truth", "exposure_in_depth_row"), mutant
    J = np.asarray(J, np.float64)
    H, W = J.shape[:2]
    c = np.asarray(gt if mutant == "a_from_ground_truth" else image, F).astype(np.float64).reshape(3, H, W)
    iea = 1.0 if mutant == "b_without_inv_ea" else 1.0 / float(np.exp(np.float64(F(a))))
    out = np.zeros((H, W, 4, 8))
    out[..., :6] = J
    out[:, :, :3, 6] = np.moveaxis(c, 0, -1)
    out[:, :, :3, 7] = iea
    if mutant == "exposure_in_depth_row":
        out[:, :, 3, 6] = c.mean(axis=0)
        out[:, :, 3, 7] = iea
    return out


def normal_equations8(J, image, a, s, h, err_s=None, err_h=None, gt=None, mutant=None):
    """-> dict(g [8], H [8,8], g_mass, H_mass, g_bound, H_bound), the form of gn_restated.normal_equations: per element
    (roundings per term + reduction depth) EPS sum|term|, plus the seeds' / curvatures' own errors carried through |J8|."""
    Jp = J8(J, image, a, gt, mutant).reshape(-1, 4, 8)
    sp, hp_ = np.asarray(s, np.float64).reshape(4, -1).T, np.asarray(h, np.float64).reshape(4, -1).T
    out = {}
    out["g"] = np.einsum("pc,pck->k", sp, Jp)
    out["g_mass"] = np.einsum("pc,pck->k", np.abs(sp), np.abs(Jp))
    out["g_bound"] = G8_ROUNDINGS * EPS * out["g_mass"]
    if err_s is not None:
        out["g_bound"] = out["g_bound"] + np.einsum("pc,pck->k", np.asarray(err_s, np.float64).reshape(4, -1).T, np.abs(Jp))
    out["H"] = np.einsum("pc,pck,pcl->kl", hp_, Jp, Jp)
    out["H_mass"] = np.einsum("pc,pck,pcl->kl", np.abs(hp_), np.abs(Jp), np.abs(Jp))
    for k in ("H", "H_mass"):
        out[k] = np.triu(out[k]) + np.triu(out[k], 1).T
    out["H_bound"] = H8_ROUNDINGS * EPS * out["H_mass"]
    if err_h is not None:
        eh = np.einsum("pc,pck,pcl->kl", np.asarray(err_h, np.float64).reshape(4, -1).T, np.abs(Jp), np.abs(Jp))
        out["H_bound"] = out["H_bound"] + np.triu(eh) + np.triu(eh, 1).T
    return out


def smooth_loss(flags, alpha, rgb_thr, image, depth, opacity, gt, gt_depth, mask, a, b, delta):
    """The loss gn_restated.irls's seeds are the gradient of, for delta > 0 (a, b: float64, NOT rounded -- finite differences move
    them):  sum kappa rho(r),  rho(r) = r^2 / (2 delta) for |r| <= delta, |r| - delta / 2 beyond; the gates and constants are irls's.
    -> (loss, residuals r [3,HW], weights kappa [HW], colour gate m [HW], the colour c [3,HW])."""
    assert delta > 0
    tracking, mono = bool(flags & lr.TRACKING), bool(flags & lr.MONOCULAR)
    _, H, W = np.shape(image)
    HW = H * W
    c, g = np.asarray(image, F).reshape(3, HW).astype(np.float64), np.asarray(gt, F).reshape(3, HW)
    gsum = (g[0] + g[1]) + g[2]
    m = gsum > F(rgb_thr)
    if tracking:
        m = m & (np.ones(HW, bool) if mask is None else np.asarray(mask).reshape(HW) != 0)
    mf = m.astype(np.float64)
    op = np.asarray(opacity, F).reshape(HW).astype(np.float64)
    al = np.float64(F(alpha))
    kappa = (1.0 if mono else al) / (3.0 * HW) * (op if tracking else np.ones(HW))
    rho = lambda r: np.where(np.abs(r) <= delta, r * r / (2 * delta), np.abs(r) - delta / 2)  # noqa: E731
    r = (np.exp(a) * c + b - g.astype(np.float64)) * mf
    loss = float((kappa * rho(r)).sum())
    if not mono:
        dd, gd = np.asarray(depth, F).reshape(HW), np.asarray(gt_depth, F).reshape(HW)
        dm = gd > F(0.01)
        if tracking:
            dm = dm & (np.asarray(opacity, F).reshape(HW) > F(0.95))
        rd = (dd.astype(np.float64) - gd.astype(np.float64)) * dm
        loss += float(((1.0 - al) / HW * rho(rd)).sum())
    return loss, r, kappa, mf, c


# ---- the Levenberg-Marquardt step on 8 unknowns -------------------------------------------------------------------------------------
def lm8_new_state(w2c, lambda_init, exposure=(0.0, 0.0)):
    st = gn.lm_new_state(w2c, lambda_init)
    e = np.asarray(exposure, F).astype(np.float64)
    st.update(H=np.zeros((8, 8)), g=np.zeros(8), exposure=e.copy(), acc_exposure=e.copy(), dexposure=np.zeros(2))
    return st


def lm8_step(state, H, g, loss, nu, lambda_min, lambda_max, threshold, mutant=None):
    """One gsaj_pose_gn8_step on (H [8,8], g [8], loss) rendered at state["w2c"], state["exposure"]; updated in place and returned.
    H, g and the exposure are kept as the fp32 values the kernel stores; everything else is float64."""
    assert mutant in (None, "exposure_not_restored_on_reject"), mutant
    st = state
    loss = float(F(loss))
    if not st["has"] or loss <= st["acc_loss"]:
        st["acc_loss"], st["acc_w2c"], st["acc_exposure"] = loss, st["w2c"].copy(), st["exposure"].copy()
        st["H"], st["g"] = np.asarray(H, F).astype(np.float64), np.asarray(g, F).astype(np.float64)
        st["lam"] = max(float(F(st["lam"]) / F(nu)), lambda_min)
        st["has"] = True
        st["accepted"] += 1
    else:
        st["w2c"] = st["acc_w2c"].copy()
        if mutant != "exposure_not_restored_on_reject":
            st["exposure"] = st["acc_exposure"].copy()
        st["lam"] = min(float(F(st["lam"]) * F(nu)), lambda_max)
        st["rejected"] += 1
    Hs, gs = st["H"], st["g"]
    A = Hs + st["lam"] * np.diag(np.diag(Hs)) + (1e-9 * np.trace(Hs) / 8.0 + 1e-30) * np.eye(8)
    ok = True
    try:
        Lc = np.linalg.cholesky(A)
        x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -gs))
        ok = bool(np.isfinite(x).all())
    except np.linalg.LinAlgError:
        ok = False
    if not ok:
        x = np.zeros(8)
        st["lam"] = min(float(F(st["lam"]) * F(nu)), lambda_max)
    x = np.asarray(x, F).astype(np.float64)
    new = gn.se3_exp(x[:6]) @ st["w2c"]
    new[3] = [0, 0, 0, 1]
    st["w2c"], st["tau"], st["dexposure"] = new, x[:6], x[6:]
    st["exposure"] = (st["exposure"].astype(F) + x[6:].astype(F)).astype(np.float64)
    st["converged"] = ok and bool(np.sqrt((x[:6] ** 2).sum()) < threshold) and bool(np.abs(x[6:]).max() < threshold)
    return st


def pack_state8(st, projection):
    """A restated state as the GSAJ_GN8_STATE_FLOATS floats the device would hold (float64 values; H8, g8 are not compared)."""
    s = np.zeros(152)
    s[:136] = gn.pack_state(st, projection)
    s[104:136] = 0.0
    s[33:35] = st["exposure"]
    s[78:80] = st["dexposure"]
    s[148:150] = st["acc_exposure"]
    return s


def assert_lm8_state_close(dev_state, want, projection, tag):
    """gn_restated.assert_lm_state_close on the shared floats, then the exposure: a, b and their accepted copies to 2 fp32 roundings
    of their size plus the step's relative tolerance (tau's), the exposure step relative like tau."""
    s = np.asarray(dev_state, np.float64)
    assert s.size == 152, (tag, s.size)
    gn.assert_lm_state_close(s[:136], want, projection, tag)
    np.testing.assert_allclose(s[78:80], want["dexposure"], rtol=3e-5, atol=1e-9, err_msg="%s: exposure step" % tag)
    tol = 2 * EPS * np.abs(want["exposure"]).max() + 3e-5 * np.abs(want["dexposure"]).max() + 1e-9
    np.testing.assert_allclose(s[33:35], want["exposure"], rtol=0, atol=tol, err_msg="%s: exposure" % tag)
    np.testing.assert_allclose(s[148:150], want["acc_exposure"], rtol=0, atol=tol, err_msg="%s: accepted exposure" % tag)


# ---- one restated iteration at a pose and an exposure ---------------------------------------------------------------------------------
def camera_at(cam, w2c):
    return syn.make_camera(np.asarray(w2c, np.float64), W=cam["W"], H=cam["H"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])


def restated_rows(cam, sc, w2c, exposure, gt, gt_depth, delta, joint, flags=lr.TRACKING, alpha=0.9, rgb_thr=0.01):
    """(H, g, loss) of one iteration at (w2c, exposure): the oracle's forward there, the restated Jacobian, irls, the normal equations
    of the chosen form.  loss: the tracking loss's own value (L1: what the step compares)."""
    c = camera_at(cam, w2c)
    (out, st), _ = gn.oracle_forward(c, sc)
    rows = gn.gaussian_rows(st, c["projmatrix_raw"])
    J, col, dep = gn.jacobian(st, rows, gn.JAC_BG)
    a, b = F(exposure[0]), F(exposure[1])
    q = gn.irls(flags, alpha, rgb_thr, col.astype(F), dep.astype(F)[None], out["opacity"], gt, gt_depth, None, a, b, delta=delta)
    if joint:
        ne = normal_equations8(J, col.astype(F), a, q["s"], q["h"])
    else:
        ne = gn.normal_equations(J, q["s"], q["h"])
    return ne["H"], ne["g"], q["loss"]["value"]["loss"]


def pose_errors(w2c, true):
    w2c, true = np.asarray(w2c, np.float64), np.asarray(true, np.float64)
    return float(np.abs(w2c[:3, 3] - true[:3, 3]).max()), float(np.abs(w2c[:3, :3] @ true[:3, :3].T - np.eye(3)).max())

