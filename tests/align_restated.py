"""NumPy restatements of the frame-to-frame RGB-D alignment -- csrc/align.hip: k_rgbd_align, k_rgbd_align_fold -- with the analytic
scene, the comparators the GPU tests use, the borderline classifier and a `mutant=` switch for the canaries.  TEST INFRASTRUCTURE
ONLY; shared by tests/test_cpu_align.py and tests/test_gpu_align.py.

  scene_frame        the analytic two-plane scene, ray cast in float64 (no rasteriser involved)
  pixels             the per-pixel arithmetic of include/gsaj.h "frame-to-frame alignment", in the header's order of operations.  One
                     statement of it, evaluated in float64 (the restatement) or in float32 (the MIRROR: NumPy rounds every float32
                     operation once, as the kernel does without contraction; division, floor, min / max, negation included)
  RowLayout          the slots of a form's row from ROW and NX; ROW6 here, ROW8 in tests/align_joint_restated.py
  fold               k_rgbd_align_fold / k_rgbd_align8_fold: the per-pixel terms summed in float64, normalised, gated by the overlap
  borderline         pixels whose gates a float32 evaluation may legally decide either way
  assert_pixels_equal / assert_row_close   the comparators
  align_loop         the restated Levenberg-Marquardt loop over the restated pyramid: gn_restated.lm_step, gsaj_pose_gn_relevel's effect
  MUTANTS            wrong kernels the comparators must reject

Roundings of one per-pixel term from the pixel's (s, h, J) -- c_pix of the row bound:
  H_kl = (h_I J_I[k]) J_I[l] + (h_Z J_Z[k]) J_Z[l]    2 products per side, rounded one after the other (2), the sum (1):  3
  g_k  = s_I J_I[k] + s_Z J_Z[k]                      1 + 1:  2;   loss = l_I + l_Z:  1;   the counts: 0
so C_PIX = 3 covers every slot.  The row comparator takes the mirror's float32 terms as given, sums them in float64 and allows
(C_PIX + ceil(log2 256) + 1) 2^-24 sum|term|: the workgroup's tree is 6 levels in a wave and 2 across the four waves, the fold rounds
its float64 quotient once."""
import math

import numpy as np

import gn_restated as gn
import pyramid_restated as pr

F = np.float32
EPS = 2.0 ** -24
C_PIX = 3
ROW_ROUNDINGS = C_PIX + 8 + 1
PIX = 16
MUTANTS = ("pixel_centres_at_integers", "textbook_level_intrinsics", "cross_block_sign", "t_rel_wrong_side", "jz_without_dz",
           "gy_with_b", "gate_without_edge_ratio", "h_without_max")
XI = np.array([0.03, -0.02, 0.01, 0.01, -0.015, 0.008])   # the scene's motion, times m
PARAMS = dict(w_depth=1.0, delta_photo=0.01, delta_depth=0.01, ratio=0.1, min_depth=0.01, max_depth=100.0, min_overlap=0.0)
LM = dict(lambda_init=1e-3, nu=4.0, lambda_min=1e-7, lambda_max=1e7, converged_threshold=1e-4)
# The fp32 floor of the pose arithmetic: a step is W2C <- Exp(tau) W2C, each element a 4-term dot product (4 products, 3 sums: 7
# roundings) of values of magnitude <= 1 here (|t| < 0.3); the default schedule of L = 2 runs 20 steps, and T = W2C_cur inverse(W2C_ref)
# adds 12 roundings on the way to the residuals: (20 x 7 + 12) 2^-24.
POSE_FLOOR = (20 * 7 + 12) * EPS


# ---- the analytic scene ---------------------------------------------------------------------------------------------------------------
def camera(W=80, H=60):
    """The scene's camera at 80 x 60 (fx = fy = 70, cx = 40, cy = 30), scaled to other sizes."""
    return dict(W=W, H=H, fx=70.0 * W / 80.0, fy=70.0 * H / 60.0, cx=W / 2.0, cy=H / 2.0)


def motion(m):
    return gn.se3_exp(m * XI)


def scene_frame(w2c, cam):
    """-> (colour [3,H,W], depth [H,W]) float32 of the scene seen from w2c: the plane z = 3 and, in front of it for world x in
    (-0.3, 0.5), the plane z = 2; texture per channel c: 0.5 + 0.2 sin(7X + 1 + c) + 0.2 sin(9Y + 2c) + 0.1 sin(5X + 6Y - c)."""
    W, H = cam["W"], cam["H"]
    w = np.asarray(w2c, np.float64).reshape(4, 4)
    R, t = w[:3, :3], w[:3, 3]
    centre = -R.T @ t
    jj, ii = np.mgrid[0:H, 0:W]
    rays = np.stack([(ii + 0.5 - cam["cx"]) / cam["fx"], (jj + 0.5 - cam["cy"]) / cam["fy"], np.ones((H, W))], -1)   # z = 1 in the camera
    dirs = rays @ R                                            # R^T d
    lam2, lam3 = (2.0 - centre[2]) / dirs[..., 2], (3.0 - centre[2]) / dirs[..., 2]
    x2 = centre[0] + lam2 * dirs[..., 0]
    front = (x2 > -0.3) & (x2 < 0.5) & (lam2 > 0)
    lam = np.where(front, lam2, lam3)
    X, Y = centre[0] + lam * dirs[..., 0], centre[1] + lam * dirs[..., 1]
    color = np.stack([0.5 + 0.2 * np.sin(7 * X + 1 + c) + 0.2 * np.sin(9 * Y + 2 * c) + 0.1 * np.sin(5 * X + 6 * Y - c) for c in range(3)])
    return color.astype(F), lam.astype(F)


def scene_case(W, H, m_true=1.0, m_start=0.5, depth=True, ref_pose=None, **params):
    """A parity case on the scene: the reference seen from ref_pose (by default a pose that is NOT the identity: T = cur inverse(ref)
    then differs from inverse(ref) cur), the current frame m_true motions on, the state's pose m_start motions on."""
    cam = camera(W, H)
    ref = gn.se3_exp(np.array([0.05, 0.02, -0.03, 0.02, 0.03, -0.01])) if ref_pose is None else np.asarray(ref_pose, np.float64)
    rc, rd = scene_frame(ref, cam)
    cc, cd = scene_frame(motion(m_true) @ ref, cam)
    return dict(cam, ref_color=rc, ref_depth=rd, ref_w2c=ref.astype(F), cur_color=cc, cur_depth=cd if depth else None,
                w2c=(motion(m_start) @ ref).astype(F), **dict(PARAMS, **params))


# ---- the per-pixel arithmetic ---------------------------------------------------------------------------------------------------------
def _grey(c, D):
    c = np.asarray(c, F).astype(D)
    return ((c[0] + c[1]) + c[2]) * D(F(1.0 / 3.0))


def _finite(x):
    return np.abs(x) < np.inf


def rel_pose(cur, ref, D, mutant=None, exact=False):
    """T [3,4]: W2C_cur inverse(W2C_ref) with the rigid inverse, in the kernel's order of operations.  exact: cur is taken as the
    float64 matrix it is (finite differences over the pose); otherwise as the float32 matrix the device holds."""
    c = np.asarray(cur, np.float64 if exact else F).reshape(4, 4).astype(D)
    r = np.asarray(ref, F).reshape(4, 4).astype(D)
    T = np.zeros((3, 4), D)
    if mutant == "t_rel_wrong_side":   # inverse(W2C_ref) W2C_cur
        Ri, ti = r[:3, :3].T, -(r[:3, :3].T @ r[:3, 3])
        T[:, :3], T[:, 3] = Ri @ c[:3, :3], Ri @ c[:3, 3] + ti
        return T.astype(D)
    ti = [-((r[0, k] * r[0, 3] + r[1, k] * r[1, 3]) + r[2, k] * r[2, 3]) for k in range(3)]
    for a in range(3):
        for b in range(3):
            T[a, b] = (c[a, 0] * r[b, 0] + c[a, 1] * r[b, 1]) + c[a, 2] * r[b, 2]
        T[a, 3] = ((c[a, 0] * ti[0] + c[a, 1] * ti[1]) + c[a, 2] * ti[2]) + c[a, 3]
    return T


def _irls(r, kappa, delta, D, mutant):
    ar = np.abs(r)
    s = kappa * np.minimum(np.maximum(r / delta, D(-1)), D(1))
    h = kappa / (ar if mutant == "h_without_max" else np.maximum(ar, delta))
    l = kappa * np.where(ar >= delta, ar - D(0.5) * delta, (r * r) / (D(2) * delta))
    return s, h, l


def _bilinear(p00, p01, p10, p11, a, b, oma, omb, mutant=None):
    val = (p00 * oma + p01 * a) * omb + (p10 * oma + p11 * a) * b
    gx = omb * (p01 - p00) + b * (p11 - p10)
    gy = (omb * (p10 - p00) + b * (p11 - p01)) if mutant == "gy_with_b" else (oma * (p10 - p00) + a * (p11 - p01))
    return val, gx, gy


def pixels(case, dtype=np.float64, mutant=None, nudge=None):
    """nudge: dict of offsets added to the named intermediate (u, v, rI, rZ, gx, gy, hx, hy) -- the float64 restatement evaluated next
    to itself, for the bound on what float32 rounding of that intermediate can do to a term.  case["w2c_exact"], if present, is a float64
    pose used unrounded.
    -> dict(valid, gate [H,W] bool; rec [H,W,16]: the pix_out record; JI, JZ [H,W,6]; terms [H,W,32]: the pixel's contribution to
    the row's 32 slots (H 21, g 6, loss, L_photo, L_depth, 1, gate); pre [H,W,5]: u, v, X_c, Y_c, Z_c before any gate but the reference
    depth's; taps [H,W,4] the depth taps), all in `dtype`.  Inputs are the float32 arrays and float32-rounded scalars the device gets."""
    assert mutant is None or mutant in MUTANTS, mutant
    D = dtype
    W, H = case["W"], case["H"]
    fx, fy, cx, cy = (D(F(case[k])) for k in ("fx", "fy", "cx", "cy"))
    wd, dp, dd, ratio, zmin, zmax = (D(F(case[k])) for k in ("w_depth", "delta_photo", "delta_depth", "ratio", "min_depth", "max_depth"))
    with np.errstate(all="ignore"):
        nudge = nudge or {}
        if "w2c_exact" in case:
            T = rel_pose(case["w2c_exact"], case["ref_w2c"], D, mutant, exact=True)
        else:
            T = rel_pose(case["w2c"], case["ref_w2c"], D, mutant)
        Ir = _grey(case["ref_color"], D)
        Zr = np.asarray(case["ref_depth"], F).reshape(H, W).astype(D)
        ok = _finite(Ir) & _finite(Zr) & (Zr >= zmin) & (Zr <= zmax)
        jj, ii = np.mgrid[0:H, 0:W]
        xn = ((ii.astype(D) + D(0.5)) - cx) / fx
        yn = ((jj.astype(D) + D(0.5)) - cy) / fy
        Xr, Yr = xn * Zr, yn * Zr
        Xc = ((T[0, 0] * Xr + T[0, 1] * Yr) + T[0, 2] * Zr) + T[0, 3]
        Yc = ((T[1, 0] * Xr + T[1, 1] * Yr) + T[1, 2] * Zr) + T[1, 3]
        Zc = ((T[2, 0] * Xr + T[2, 1] * Yr) + T[2, 2] * Zr) + T[2, 3]
        ok = ok & _finite(Xc) & _finite(Yc) & _finite(Zc) & (Zc >= zmin)
        iz = D(1) / Zc
        fxz, fyz = fx * iz, fy * iz
        px, py = fxz * Xc, fyz * Yc
        if mutant == "pixel_centres_at_integers":
            u, v = px + cx, py + cy
        else:
            u, v = (px + cx) - D(0.5), (py + cy) - D(0.5)
        u, v = u + D(nudge.get("u", 0.0)), v + D(nudge.get("v", 0.0))
        x0f, y0f = np.floor(u), np.floor(v)
        ok = ok & (x0f >= 0) & (x0f <= D(W - 2)) & (y0f >= 0) & (y0f <= D(H - 2))
        x0 = np.where(ok, x0f, 0).astype(np.int64)
        y0 = np.where(ok, y0f, 0).astype(np.int64)
        a, b = u - x0f, v - y0f
        oma, omb = D(1) - a, D(1) - b
        Ig = _grey(case["cur_color"], D)
        I00, I01, I10, I11 = Ig[y0, x0], Ig[y0, x0 + 1], Ig[y0 + 1, x0], Ig[y0 + 1, x0 + 1]
        ok = ok & _finite(I00) & _finite(I01) & _finite(I10) & _finite(I11)
        Ic, gx, gy = _bilinear(I00, I01, I10, I11, a, b, oma, omb, mutant)
        gx, gy = gx + D(nudge.get("gx", 0.0)), gy + D(nudge.get("gy", 0.0))
        duz, dvz = -(px * iz), -(py * iz)
        rI = (Ic - Ir) + D(nudge.get("rI", 0.0)) if "rI" in nudge else Ic - Ir
        sgn = D(-1) if mutant == "cross_block_sign" else D(1)
        j0, j1, j2 = gx * fxz, gy * fyz, gx * duz + gy * dvz
        JI = np.stack([j0, j1, j2, sgn * (j2 * Yc - j1 * Zc), sgn * (j0 * Zc - j2 * Xc), sgn * (j1 * Xc - j0 * Yc)], -1)
        sI, hI, lI = _irls(rI, D(1), dp, D, mutant)
        gate = np.zeros((H, W), bool)
        zero = np.zeros((H, W), D)
        Dc = rZ = sZ = hZ = lZ = zero
        JZ = np.zeros((H, W, 6), D)
        taps = np.zeros((H, W, 4), D)
        if case.get("cur_depth") is not None:
            Dm = np.asarray(case["cur_depth"], F).reshape(H, W).astype(D)
            D00, D01, D10, D11 = Dm[y0, x0], Dm[y0, x0 + 1], Dm[y0 + 1, x0], Dm[y0 + 1, x0 + 1]
            taps = np.stack([D00, D01, D10, D11], -1)
            dmin = np.minimum(np.minimum(D00, D01), np.minimum(D10, D11))
            dmax = np.maximum(np.maximum(D00, D01), np.maximum(D10, D11))
            gate = ok & _finite(D00) & _finite(D01) & _finite(D10) & _finite(D11) & (dmin >= zmin) & (dmax <= zmax)
            if mutant != "gate_without_edge_ratio":
                gate = gate & (dmax - dmin <= ratio * dmin)
            Dc, hx, hy = _bilinear(D00, D01, D10, D11, a, b, oma, omb, mutant)
            hx, hy = hx + D(nudge.get("hx", 0.0)), hy + D(nudge.get("hy", 0.0))
            rZ = (Dc - Zc) + D(nudge.get("rZ", 0.0)) if "rZ" in nudge else Dc - Zc
            k0, k1, k2 = hx * fxz, hy * fyz, hx * duz + hy * dvz
            if mutant == "jz_without_dz":
                JZ = np.stack([k0, k1, k2, sgn * (k2 * Yc - k1 * Zc), sgn * (k0 * Zc - k2 * Xc), sgn * (k1 * Xc - k0 * Yc)], -1)
            else:
                JZ = np.stack([k0, k1, k2 - D(1), sgn * (k2 * Yc - k1 * Zc) - Yc, sgn * (k0 * Zc - k2 * Xc) + Xc, sgn * (k1 * Xc - k0 * Yc)], -1)
            sZ, hZ, lZ = _irls(rZ, wd, dd, D, mutant)
            g3 = gate[..., None]
            Dc, rZ, sZ, hZ, lZ = (np.where(gate, q, zero) for q in (Dc, rZ, sZ, hZ, lZ))
            JZ = np.where(g3, JZ, D(0))
        terms = np.zeros((H, W, 32), D)
        n = 0
        for k in range(6):
            ak, zk = hI * JI[..., k], hZ * JZ[..., k]
            for l in range(k, 6):
                terms[..., n] = ak * JI[..., l] + zk * JZ[..., l]
                n += 1
        for k in range(6):
            terms[..., 21 + k] = sI * JI[..., k] + sZ * JZ[..., k]
        terms[..., 27], terms[..., 28], terms[..., 29] = lI + lZ, lI, lZ
        terms[..., 30], terms[..., 31] = D(1), gate.astype(D)
        terms = np.where(ok[..., None], terms, D(0)).astype(D)
        rec = np.stack([u, v, Xc, Yc, Zc, Ic, gx, gy, rI, sI, hI, Dc, rZ, sZ, hZ, gate.astype(D)], -1)
        rec = np.where(ok[..., None], rec, D(0)).astype(D)
        pre = np.stack([u, v, Xc, Yc, Zc], -1).astype(D)
    return dict(valid=ok, gate=gate, rec=rec, JI=np.where(ok[..., None], JI, D(0)), JZ=np.where(ok[..., None], JZ, D(0)), terms=terms, pre=pre,
                taps=taps, Zr=Zr)


def mirror(case, mutant=None):
    """The float32 mirror of k_rgbd_align: what pix_out / valid_out must hold, bit for bit."""
    return pixels(case, np.float32, mutant)


def flags_of(px):
    return (px["valid"].astype(np.uint8) | (px["gate"].astype(np.uint8) << 1)).astype(np.uint8)


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
def need_of(case):
    """max(1, ceil(min_overlap W H)), min_overlap as the float32 the call takes."""
    return max(1.0, math.ceil(float(F(case["min_overlap"])) * case["W"] * case["H"]))


class RowLayout:
    """The slots of a form's row: H (NH, the upper triangle), g (NX), [LOSS] loss, L_photo, L_depth, [VALID] valid pixels, [GATES] open
    depth gates, [GATES + 1 : ROW) zero; ROUNDINGS: the form's ROW_ROUNDINGS.  fold, row_bound and assert_row_close take one."""

    def __init__(self, ROW, NX, ROUNDINGS):
        self.ROW, self.NX, self.ROUNDINGS = ROW, NX, ROUNDINGS
        self.NH = NX * (NX + 1) // 2
        self.LOSS = self.NH + NX
        self.VALID = self.LOSS + 3
        self.GATES = self.VALID + 1
        assert self.GATES < ROW


ROW6 = RowLayout(32, 6, ROW_ROUNDINGS)   # gn_row: [27] loss ... [30] valid, [31] gates, no padding


def fold(terms, case, lay=ROW6):
    """-> the ROW slots of gn_row (gn8_row) in float64 from per-pixel terms [H,W,ROW] (any dtype), summed in float64."""
    s = np.asarray(terms, np.float64).reshape(-1, lay.ROW).sum(0)
    out = np.zeros(lay.ROW)
    out[lay.VALID:] = s[lay.VALID:]
    if s[lay.VALID] < need_of(case):
        out[lay.LOSS:lay.VALID] = np.inf
    else:
        out[:lay.VALID] = s[:lay.VALID] / s[lay.VALID]
    return out


def row_bound(terms, case, border=None, alt_terms=None, lay=ROW6):
    """Per slot: ROW_ROUNDINGS 2^-24 sum|term| / n, plus for each borderline pixel the larger |term| of its two legal sides / n (alt_terms:
    the pixel's terms on the other side; where none is given, the pixel's own |term| -- its other side is 'invalid', a zero, or the
    other side of a gate: the larger of two terms of one size)."""
    t = np.abs(np.asarray(terms, np.float64)).reshape(-1, lay.ROW)
    n = max(t[:, lay.VALID].sum(), 1.0)
    bound = lay.ROUNDINGS * EPS * t.sum(0) / n
    if border is not None and border.any():
        extra = t[border.reshape(-1)]
        if alt_terms is not None:
            extra = np.maximum(extra, np.abs(np.asarray(alt_terms, np.float64)).reshape(-1, lay.ROW)[border.reshape(-1)])
        bound = bound + extra.sum(0) / n
    return bound


def rounding_bound(case, px64, border):
    """Per slot of the row: what a float32 evaluation of the whole per-pixel chain may differ by from the float64 one, to first order.
    Every intermediate that a rounding error reaches the terms through is nudged by its own error, one at a time, both ways, and the
    per-pixel |change of the term| summed (no cancellation assumed), doubled for the second order:
      u, v    24 roundings on the way (T 5, the ray 3, X_r 1, X_c 6, iz, fxz, px 3, u 2, and 4 spare) of values <= 2 max(W, H)
      r_I     I_c 7 + I_r 3 + the subtraction 1 = 11 roundings of greys <= 1;   r_Z: D_c 7 + Z_c 7 + 1 = 15 of depths <= Zmax
      gx, gy  4 roundings of greys <= 1;   hx, hy: 4 of depths <= Zmax
    plus 16 2^-24 sum|term| for the factors of J (fxz, duz, the cross block: <= 6 relative roundings in J, twice in H, and the IRLS
    quotients) and the row's own ROW_ROUNDINGS."""
    zs = np.concatenate([np.asarray(case[k], np.float64).reshape(-1) for k in ("ref_depth", "cur_depth") if case.get(k) is not None])
    zmax = float(np.abs(zs[np.isfinite(zs)]).max(initial=1.0))
    size = {"u": 24 * 2 * max(case["W"], case["H"]), "v": 24 * 2 * max(case["W"], case["H"]), "rI": 11, "rZ": 15 * zmax, "gx": 4, "gy": 4,
            "hx": 4 * zmax, "hy": 4 * zmax}
    base = np.asarray(px64["terms"], np.float64)
    first = np.zeros(32)
    for name, k in size.items():
        d = np.zeros(base.shape)
        for sg in (1.0, -1.0):
            t = pixels(case, np.float64, nudge={name: sg * k * EPS})["terms"]
            d = np.maximum(d, np.abs(t - base))
        first += d[~border].sum(0)
    t = np.abs(base).reshape(-1, 32)
    n = max(t[:, 30].sum(), 1.0)
    return (2.0 * first + (16 + ROW_ROUNDINGS) * EPS * t.sum(0)) / n + (t[border.reshape(-1)].sum(0) / n if border.any() else 0.0)


# ---- borderline pixels ---------------------------------------------------------------------------------------------------------------
def borderline(case, px64=None):
    """[H,W] bool, decided in float64: u or v within 2e-4 px of an integer; Z_c, the reference depth or a depth tap within a relative
    1e-5 of a gate; the tap spread within a relative 1e-5 of depth_edge_ratio dmin.  Only pixels whose reference depth passes or nearly
    passes its own gate can be borderline (the others are invalid on every side)."""
    p = pixels(case) if px64 is None else px64
    zmin, zmax, ratio = (float(F(case[k])) for k in ("min_depth", "max_depth", "ratio"))
    near = lambda x, g: np.abs(x - g) <= 1e-5 * abs(g)   # noqa: E731
    with np.errstate(all="ignore"):
        Zr = p["Zr"]
        live = _finite(Zr) & (Zr >= zmin * (1 - 1e-5)) & (Zr <= zmax * (1 + 1e-5))
        u, v, Zc = p["pre"][..., 0], p["pre"][..., 1], p["pre"][..., 4]
        b = near(Zr, zmin) | near(Zr, zmax) | near(Zc, zmin)
        b |= (np.abs(u - np.round(u)) <= 2e-4) | (np.abs(v - np.round(v)) <= 2e-4)
        if case.get("cur_depth") is not None:
            taps = p["taps"]
            tb = (near(taps, zmin) | near(taps, zmax)).any(-1)
            dmin, dmax = taps.min(-1), taps.max(-1)
            tb |= np.abs((dmax - dmin) - ratio * dmin) <= 1e-5 * ratio * np.abs(dmin)
            b |= tb & p["valid"]
        near_image = (u >= -1) & (u <= case["W"]) & (v >= -1) & (v <= case["H"])   # (further out no rounding reaches a gate)
        return live & b & near_image


# ---- the comparators of the GPU tests -------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def assert_pixels_equal(got_pix, got_flags, mir, border, tag):
    """pix_out [H,W,16] and valid_out [H,W] against the mirror, bit for bit at every non-borderline pixel.  At a borderline pixel the
    device may have taken the other side of its gate: its flags must then be a legal side (bit 1 never without bit 0), and a valid
    record must still carry the mirror's u, v, X_c, Y_c, Z_c, which precede every gate.  -> the number of borderline pixels that
    took the other side."""
    got_pix, got_flags = np.asarray(got_pix, F), np.asarray(got_flags, np.uint8)
    want_pix, want_flags = mir["rec"].astype(F), flags_of(mir)
    assert got_pix.shape == want_pix.shape and got_flags.shape == want_flags.shape, (tag, got_pix.shape, got_flags.shape)
    same = (bits(got_pix) == bits(want_pix)).all(-1) & (got_flags == want_flags)
    bad = ~same & ~border
    if bad.any():
        y, x = np.argwhere(bad)[0]
        k = np.flatnonzero(bits(got_pix[y, x]) != bits(want_pix[y, x]))
        raise AssertionError("%s: %d pixel(s) differ from the mirror; first (x=%d, y=%d): flags %d want %d, fields %s got %s want %s" % (
            tag, int(bad.sum()), x, y, got_flags[y, x], want_flags[y, x], k.tolist(), got_pix[y, x][k].tolist(), want_pix[y, x][k].tolist()))
    other = ~same & border
    for y, x in np.argwhere(other):
        f = int(got_flags[y, x])
        assert f in (0, 1, 3), "%s: borderline pixel (x=%d, y=%d) has flags %d, no legal side" % (tag, x, y, f)
        if f & 1:
            assert (bits(got_pix[y, x, :5]) == bits(mir["pre"][y, x].astype(F))).all(), "%s: borderline pixel (x=%d, y=%d): the warp differs" % (tag, x, y)
        else:
            assert not got_pix[y, x].any(), "%s: invalid pixel (x=%d, y=%d) with a non-zero record" % (tag, x, y)
    return int(other.sum())


def assert_row_close(got_row, terms, case, border, tag, lay=ROW6):
    """gn_row (gn8_row) against the float64 sum of the per-pixel terms (the mirror's): every slot within row_bound; the counts exact up
    to the number of borderline pixels; the padding behind them (joint form: [49:64)) zero; below the overlap gate H and g exactly zero
    and the losses +inf.  -> worst err / bound."""
    LOSS, VALID, GATES = lay.LOSS, lay.VALID, lay.GATES
    got = np.asarray(got_row, np.float64)
    assert got.shape == (lay.ROW,), (tag, got.shape)
    want = fold(terms, case, lay)
    nb = int(border.sum()) if border is not None else 0
    assert not got[GATES + 1:].any(), "%s: the padding of the row is not zero: %s" % (tag, got[GATES + 1:])
    assert abs(got[VALID] - want[VALID]) <= nb and abs(got[GATES] - want[GATES]) <= nb, (tag, got[VALID:GATES + 1], want[VALID:GATES + 1], nb)
    need = need_of(case)
    if got[VALID] < need or want[VALID] < need:
        assert nb or (got[VALID] < need) == (want[VALID] < need), (tag, got[VALID], want[VALID])
        if got[VALID] < need:
            assert not got[:LOSS].any() and np.isposinf(got[LOSS:VALID]).all(), (tag, got)
        return 0.0
    bound = row_bound(terms, case, border, lay=lay)[:VALID]
    err = np.abs(got[:VALID] - want[:VALID])
    assert np.isfinite(got).all(), (tag, got)
    bad = err > bound
    assert not bad.any(), "%s: slot %s: got %.9e want %.9e, error %.3e = %.3g x bound" % (
        tag, np.flatnonzero(bad)[0], got[:VALID][bad][0], want[:VALID][bad][0], err[bad][0], (err[bad] / np.maximum(bound[bad], 1e-300))[0])
    return float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0))


# ---- the restated loop ---------------------------------------------------------------------------------------------------------------
def level_intrinsics(cam, l, mutant=None):
    s = float(1 << l)
    if mutant == "textbook_level_intrinsics":   # pixel centres at integer coordinates
        return dict(W=cam["W"] >> l, H=cam["H"] >> l, fx=cam["fx"] / s, fy=cam["fy"] / s, cx=(cam["cx"] + 0.5) / s - 0.5, cy=(cam["cy"] + 0.5) / s - 0.5)
    return dict(W=cam["W"] >> l, H=cam["H"] >> l, fx=cam["fx"] / s, fy=cam["fy"] / s, cx=cam["cx"] / s, cy=cam["cy"] / s)


def level_case(case, l, w2c=None, mutant=None, memo=None):
    """The case at pyramid level l (0: itself): both frames through the restated pyramid, the level's exact intrinsics."""
    out = dict(case, **level_intrinsics(case, l, mutant))
    if l:
        key = (id(case), l)
        if memo is None or key not in memo:
            lv = {}
            for name in ("ref", "cur"):
                d = case[name + "_depth"]
                d0 = np.zeros((case["H"], case["W"]), F) if d is None else d
                p = pr.pyramid(case[name + "_color"], d0, None, l, F(case["ratio"]))[l - 1]
                lv[name + "_color"], lv[name + "_depth"] = p["color"], (None if d is None else p["depth"])
            if memo is None:
                memo = {}
            memo[key] = lv
        out.update(memo[key])
    if w2c is not None:
        out["w2c"] = np.asarray(w2c, np.float64).astype(F)
    return out


def relevel(st, lambda_init):
    """gsaj_pose_gn_relevel's effect on a gn_restated.lm_new_state: back to the accepted pose, a new baseline, lambda_init."""
    if st["has"]:
        st["w2c"] = st["acc_w2c"].copy()
    st.update(lam=float(lambda_init), has=False, acc_loss=0.0, acc_w2c=st["w2c"].copy(), H=np.zeros((6, 6)), g=np.zeros(6), tau=np.zeros(6),
              converged=False)
    return st


def align_loop(case, levels, schedule=None, dtype=np.float64, lm=None):
    """The aligner's loop restated: from case["w2c"], schedule[i] iterations at level levels - i, each pixels() -> fold() ->
    gn_restated.lm_step, relevel between levels.  -> dict(w2c: the accepted pose, losses: per level the accepted loss after every
    step, st).  The state's pose is handed to every evaluation rounded to float32, as the device holds it."""
    lm = dict(LM, **(lm or {}))
    schedule = [8] + [6] * levels if schedule is None else list(schedule)
    assert len(schedule) == levels + 1
    st = gn.lm_new_state(np.asarray(case["w2c"], np.float64), lm["lambda_init"])
    losses, memo, at = [], {}, levels
    for l, n in zip(range(levels, -1, -1), schedule):
        if not n:
            continue
        if at != l:
            relevel(st, lm["lambda_init"])
            at = l
        acc = []
        for _ in range(n):
            c = level_case(case, l, st["w2c"], memo=memo)
            row = fold(pixels(c, dtype)["terms"], c)
            gn.lm_step(st, gn.sym6(row[:21]), row[21:27], row[27], lm["nu"], lm["lambda_min"], lm["lambda_max"], lm["converged_threshold"])
            acc.append(st["acc_loss"])
        losses.append((l, acc))
    return dict(w2c=st["acc_w2c"].copy(), losses=losses, st=st)


def pose_error(w2c, w2c_true):
    """(translation error [m], rotation error [rad]) of w2c against w2c_true."""
    d = np.asarray(w2c, np.float64).reshape(4, 4) @ np.linalg.inv(np.asarray(w2c_true, np.float64).reshape(4, 4))
    return float(np.linalg.norm(d[:3, 3])), float(math.acos(min(1.0, max(-1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))))


def behaviour_case(m, depth=True):
    """The behaviour scene at 80 x 60: reference pose the identity, the current frame m motions on, the start the reference pose."""
    cam = camera()
    rc, rd = scene_frame(np.eye(4), cam)
    cc, cd = scene_frame(motion(m), cam)
    return dict(cam, ref_color=rc, ref_depth=rd, ref_w2c=np.eye(4, dtype=F), cur_color=cc, cur_depth=cd if depth else None,
                w2c=np.eye(4, dtype=F), **PARAMS)


def parity_sizes():
    """The sizes of the per-pixel parity: the smallest legal, odd ones, one past a workgroup (64 x 4 pixels) in each direction, the
    scene's own and one with a partial workgroup on both edges."""
    return [(2, 2), (3, 2), (7, 5), (33, 17), (65, 4), (64, 5), (80, 60), (97, 61)]


def parity_case(W, H, mode):
    """mode: "depth", "photo" (no current depth) or "w0" (w_depth = 0).  The small frames move further: at fx of a few pixels the
    scene's own motion is a hundredth of a pixel, and every u would sit on an integer."""
    big = min(W, H) < 16
    kw = dict(m_true=8.0, m_start=3.0) if big else {}
    return scene_case(W, H, depth=mode != "photo", **kw, **({"w_depth": 0.0} if mode == "w0" else {}))


MODES = ("depth", "photo", "w0")
LONG_FOLD = (70, 260)   # 2 x 65 = 130 rows: past one trip of the fold's four-deep load loop (32 groups x 4 = 128 rows of 32 floats)


# ---- planted cases -------------------------------------------------------------------------------------------------------------------
PLANT_W, PLANT_H = 33, 17


def planted_case(sign):
    """33 x 17, fx = fy = 32, cx = 16, cy = 8, both poses pure translations, 16 tx = sign 0.375 and 16 ty = 0.25: every operation of the
    warp is exact for a power-of-two depth.  A reference depth of 2 lands at u = i + sign 0.375, v = j + 0.25; a reference depth of 0.25
    at u = i + sign 3, v = j + 2 EXACTLY -- with sign = +1 pixel (W - 4, j) lands on u = W - 1 (outside), with sign = -1 pixel (3, j) on
    u = 0 (inside, a = 0).  -> (case, planted: name -> (x, y) of a REFERENCE pixel, expect: name -> what the mirror must show there)."""
    W, H = PLANT_W, PLANT_H
    rng = np.random.default_rng(11)
    ref_w2c, cur_w2c = np.eye(4), np.eye(4)
    ref_w2c[0, 3] = 0.5
    cur_w2c[0, 3] = 0.5 + sign * 0.375 / 16.0
    cur_w2c[1, 3] = 0.25 / 16.0
    ref_color = np.full((3, H, W), 0.5, F)
    ref_depth = np.full((H, W), 2.0, F)
    cur_color = rng.uniform(0.3, 0.7, size=(3, H, W)).astype(F)
    cur_depth = (2.0 + rng.uniform(-0.02, 0.02, size=(H, W))).astype(F)
    planted = {}
    sh = 1 if sign > 0 else -1   # the landing column of a depth-2 pixel (i, j) is x0 = i (sign > 0) or i - 1 (sign < 0)
    land = lambda x: x if sign > 0 else x - 1   # noqa: E731

    def flat(x, y, value, plane):   # the four taps of reference pixel (x, y) set to one value
        x0 = land(x)
        plane[..., y:y + 2, x0:x0 + 2] = value

    # u exactly W - 1 / exactly 0: depth 0.25 -> u = i + 3 sign
    ex = (W - 4, 2) if sign > 0 else (3, 2)
    ref_depth[ex[1], ex[0]] = 0.25
    planted["u_exact"] = ex
    planted["ref_depth_zero"] = (5, 4)
    ref_depth[4, 5] = 0.0
    planted["ref_depth_nan"], planted["ref_depth_inf"] = (7, 4), (9, 4)
    ref_depth[4, 7], ref_depth[4, 9] = np.nan, np.inf
    planted["ref_color_nan"], planted["ref_color_inf"] = (11, 4), (13, 4)
    ref_color[1, 4, 11], ref_color[2, 4, 13] = np.nan, np.inf
    planted["cur_color_nan"], planted["cur_color_inf"] = (5, 7), (9, 7)
    cur_color[0, 7, land(5)], cur_color[1, 8, land(9) + 1] = np.nan, np.inf
    planted["cur_depth_nan"], planted["cur_depth_inf"] = (13, 7), (17, 7)
    cur_depth[7, land(13)], cur_depth[8, land(17) + 1] = np.nan, np.inf
    # a tap straddling the edge ratio (0.1 x dmin = 0.2) from either side
    for name, x, f in (("edge_inside", 21, 1.0 - 1e-3), ("edge_outside", 25, 1.0 + 1e-3)):
        flat(x, 7, 2.0, cur_depth)
        cur_depth[7, land(x) + 1] = F(2.0 + 0.2 * f)
        planted[name] = (x, 7)
    # |r| on either side of delta = 0.01: photometric (reference grey 0.5) and depth (Z_c = 2)
    for k, (name, r) in enumerate((("r_above", 0.011), ("r_below", 0.009), ("r_above_neg", -0.011), ("r_below_neg", -0.009))):
        x = 5 + 4 * k
        flat(x, 11, F(0.5 + r), cur_color)
        flat(x, 11, F(2.0 + r), cur_depth)
        planted[name] = (x, 11)
    case = dict(W=W, H=H, fx=32.0, fy=32.0, cx=16.0, cy=8.0, ref_color=ref_color, ref_depth=ref_depth, ref_w2c=ref_w2c.astype(F),
                cur_color=cur_color, cur_depth=cur_depth, w2c=cur_w2c.astype(F), **PARAMS)
    return case, planted, sh


def planted_near_case():
    """A general pose with a NEGATIVE z translation and min_depth = 0.5: reference depths chosen (in float64) so that Z_c lands at
    min_depth (1 -+ 1e-3) while the reference depth itself passes its gate.  -> (case, planted)."""
    case = scene_case(33, 17)
    move = gn.se3_exp(np.array([0.02, -0.01, -0.05, 0.01, -0.015, 0.008]))
    ref = np.asarray(case["ref_w2c"], np.float64)
    case["w2c"] = (move @ ref).astype(F)
    case["min_depth"] = 0.5
    T = rel_pose(case["w2c"], case["ref_w2c"], np.float64)
    planted = {}
    for name, x, f in (("zc_below", 10, 1.0 - 1e-3), ("zc_above", 14, 1.0 + 1e-3)):
        y = 8
        xn, yn = (x + 0.5 - case["cx"]) / case["fx"], (y + 0.5 - case["cy"]) / case["fy"]
        zr = (0.5 * f - T[2, 3]) / (T[2, 0] * xn + T[2, 1] * yn + T[2, 2])
        assert zr > 0.5 * (1 + 1e-3), zr
        case["ref_depth"] = case["ref_depth"].copy()
        case["ref_depth"][y, x] = F(zr)
        planted[name] = (x, y)
    return case, planted
