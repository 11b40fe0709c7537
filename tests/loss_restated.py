"""NumPy restatement of the L1 loss family (csrc/loss_terms.h: loss_pixel / loss_consts, evaluated by k_loss_seeds in csrc/loss.hip,
by the epilogue of k_render_fwd<true> and by the prologue of the loss-fused k_render_bwd; k_loss_finalize, k_count_valid) and of the
isotropic regulariser (k_isotropic), with a per-output error model, generated cases that sit ON every gate, and a `mutant=` switch.
TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_loss.py, tests/test_gpu_loss.py and tests/test_gpu_device_tracker.py.

The operation, per pixel (fp32 inputs c = rendered colour, d = rendered depth, op = rendered opacity, g = gt colour, gd = gt depth):
    m    = [cl or (g0 + g1) + g2 > rgb_thr]  x  [mask != 0  where the mode reads a mask: TRACKING, COMPUTE_LOSS]
    r_ch = (ea c_ch + eb - g_ch) m           ea = exp(a), eb = b   (1, 0 with NO_EXPOSURE and COMPUTE_LOSS)
    w    = op (TRACKING) or 1
    dL/dc_ch = k_rgb ea w m sgn(r_ch)        sgn(0) = 0           k_rgb = (1 | alpha) / 3HW   (1: MONOCULAR, COMPUTE_LOSS)
    dL/dop   = k_rgb sum_ch |r_ch|           (TRACKING only)
    dm   = [gd > 0.01 (> 0 with cl)] x [op > 0.95 (TRACKING)] x [m (cl)]
    dL/dd    = k_d dm sgn(d - gd)            k_d = (1 - alpha) / HW, or 1 / max(n_valid, 1) with cl (n_valid = #{gd > 0, mask})
  and over the image
    L_rgb = sum w |r_ch| / 3HW        L_d = sum dm |d - gd| / (HW | max(n_valid, 1))       loss = alpha L_rgb + (1 - alpha) L_d
    dL/da = k_rgb ea sum w m sgn(r_ch) c_ch        dL/db = k_rgb sum w m sgn(r_ch)         (loss = L_rgb [+ L_d]: MONOCULAR [cl])

DECISIONS are taken on the fp32 values exactly as the kernels take them -- the gt sum as (g0 + g1) + g2 in fp32 against
np.float32(rgb_thr), gd against np.float32(0.01), op against np.float32(0.95) -- so the restatement can say what is right AT a
threshold (oracle/loss_oracle.py sums gt in float64 and cannot).  ARITHMETIC after the decisions is float64 from the fp32 inputs,
ea = exp(float64(a)).  The sign of a residual is the one decision taken in float64: every generated case asserts that a residual is
either exactly 0 by construction or at least GUARD eps x scale away from 0, so no evaluation can see another sign and no pixel is
exempted anywhere.

restate(..., dtype=np.float32) is the second mode: the kernel's own operation order in fp32 (fma as one rounding via float64, sums
as 4 pixels per thread -> 64-lane butterfly -> 4 waves -> float64 over workgroups).  It stands in for a device on the CPU.

Error model (eps = 2^-23; one count = one fp32 rounding, expf allowed 2):
  seed images, every pixel:   |err| <= ROUND_K eps mass,  exactly 0 where mass == 0 (gate closed, or residual exactly 0)
  the five scalars:           |err| <= SUM_K eps sum|term| + eps |value|
mass of a term is the sum of the absolute values it is made of.  dL/dc and dL/dd are single products, mass = |value|.  A colour
residual is a DIFFERENCE, r = ea c + eb - g, which an fp32 evaluation rounds at the size of its parts (the fma's result, expf's error
on ea c), so wherever |r| enters (dL/dop, L_rgb, loss) its mass is |ea c| + |eb| + |g|, not |r|.  The depth residual d - gd is one
subtraction of two inputs: mass |d - gd|.  dL/da and dL/db are sums of signed terms that cancel: mass = sum of |term|.
"""
import functools
import json
import os

import numpy as np

TRACKING, MONOCULAR, NO_EXPOSURE, COMPUTE_LOSS = 1, 2, 4, 8
EPS = 2.0 ** -23
F = np.float32
# ROUND_K, roundings on the path of one seed value (the largest of the three images decides):
#   dL/dc:  k_rgb's division 1 + expf 2 + ke = k_rgb ea 1 + ke t 1                                     = 5   (3 HW is exact below 2^24)
#   dL/dd:  1 - alpha 1 + division 1 (x dm, x sgn are exact)                                            = 2
#   dL/dop: expf 2 + fma 1 + the subtraction of g 1 + (a0 + a1) + a2 2 + k_rgb's division 1 + product 1 = 8
ROUND_K = 8
# SUM_K, fp32 additions on one term's way into a workgroup partial + the term's own roundings (sums over workgroups are fp64):
#   k_loss_seeds: 4 pixels per thread 3 + butterfly 6 + 4 waves 3 = 12;  fused forward: butterfly 6 only
#   term of L_rgb: expf 2 + fma 1 + subtraction 1 + (a0 + a1) + a2 2 + w asum 1 = 7;  dL/da: w m 1 + t c 1 + two adds 2 + ea 1 with
#   expf 2 = 7 (+ k_rgb 1 on the total);  dL/db: 2 + 1;  L_d: 1                                         => 12 + 7 = 19
SUM_K = 19
GUARD = 64.0          # |r| >= GUARD eps scale: 16 x the worst fp32 error of fma(ea, c, eb) - g incl. 2 ulp of expf (4 eps scale)
OPACITY_ULPS = 4      # fused tests: a rendered opacity this close to 0.95 holds its pixel only to "equal to the unfused path"
LOSS_BLOCK, LOSS_PPT = 256, 4
WG = LOSS_BLOCK * LOSS_PPT
SEEDS = ("dL_dcolor", "dL_ddepth", "dL_dopacity")
SCALARS = ("loss", "l1_rgb", "l1_depth", "dL_dexposure_a", "dL_dexposure_b")
MUTANTS = ("ge_rgb", "ge_depth", "ge_opacity", "sgn0_plus", "depth_gate_without_opacity", "opacity_weight_in_mapping", "mask_in_mapping",
           "alpha_for_one_minus_alpha", "b_omitted", "ea_missing_from_da", "depth_mean_over_valid", "drop_partial", "stale_partial")
ISO_MUTANTS = ("sgn0_plus", "mean_over_P")
STALE = (7.0, 3.0, -5.0, 11.0)   # what a previous frame could have left in an unused slot of the fused forward's partials


def _wg_sum32(term):
    """[HW] fp32 -> sum as k_loss_seeds forms it: fp32 inside a workgroup (4 strided pixels per thread, xor butterfly over 64 lanes,
    the 4 waves in order), float64 over the workgroups."""
    n = -(-term.size // WG)
    x = np.zeros(n * WG, F)
    x[:term.size] = term
    x = x.reshape(n, LOSS_PPT, LOSS_BLOCK)
    s = x[:, 0]
    for q in range(1, LOSS_PPT):
        s = s + x[:, q]
    v = s.reshape(n, LOSS_BLOCK // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    red = v[..., 0]
    t = red[:, 0]
    for w in range(1, LOSS_BLOCK // 64):
        t = t + red[:, w]
    assert t.dtype == F
    return float(t.astype(np.float64).sum())


def restate(flags, alpha, rgb_thr, image, depth, opacity, gt, gt_depth=None, mask=None, a=None, b=None, dtype=np.float64, mutant=None,
            drop=-1):
    """image / gt [3,H,W], depth / opacity [1,H,W] or [H,W], gt_depth [H,W] or None, mask [H,W] bytes or None, a / b fp32 scalars.
    -> dict(value, mass: output name -> array / float; abs_r, scale [3,HW]; abs_rd, scale_d [HW]; n_valid).  dtype=np.float32: the
    kernel's operation order (value only).  mutant: one of MUTANTS; drop: the workgroup whose partial "drop_partial" loses (-1: last)."""
    assert mutant is None or mutant in MUTANTS, mutant
    mu = lambda name: mutant == name  # noqa: E731
    tracking, mono, cl = bool(flags & TRACKING), bool(flags & MONOCULAR), bool(flags & COMPUTE_LOSS)
    noexp = bool(flags & NO_EXPOSURE) or cl
    _, H, W = np.shape(image)
    HW = H * W
    c, g = np.asarray(image, F).reshape(3, HW), np.asarray(gt, F).reshape(3, HW)
    op = np.asarray(opacity, F).reshape(HW)
    mk = np.ones(HW, bool) if mask is None else np.asarray(mask).reshape(HW) != 0
    # ---- decisions, on fp32
    gsum = (g[0] + g[1]) + g[2]
    assert gsum.dtype == F
    m = np.ones(HW, bool) if cl else ((gsum >= F(rgb_thr)) if mu("ge_rgb") else (gsum > F(rgb_thr)))
    if tracking or cl or mu("mask_in_mapping"):
        m = m & mk
    weighted = tracking or mu("opacity_weight_in_mapping")
    if mono:
        d = gd = np.zeros(HW, F)
        dm = np.zeros(HW, bool)
        n_valid = 1
    else:
        d, gd = np.asarray(depth, F).reshape(HW), np.asarray(gt_depth, F).reshape(HW)
        lim = F(0.0) if cl else F(0.01)
        dm = (gd >= lim) if mu("ge_depth") else (gd > lim)
        if tracking and not mu("depth_gate_without_opacity"):
            dm = dm & ((op >= F(0.95)) if mu("ge_opacity") else (op > F(0.95)))
        if cl:
            dm = dm & m
        n_valid = max(int(((gd > F(0.0)) & mk).sum()), 1) if cl else 1   # k_count_valid
    sgn = (lambda x: np.where(x >= 0, 1.0, -1.0)) if mu("sgn0_plus") else np.sign
    al = np.float64(F(alpha))
    wgs = np.arange(HW) // WG
    keep = np.ones(HW) if not mu("drop_partial") else (wgs != (wgs.max() if drop < 0 else drop)).astype(np.float64)
    out = dict(n_valid=n_valid)

    if dtype == np.float32:   # ---- the kernel's operation order
        assert mutant is None
        ea, eb = (F(1), F(0)) if noexp else (np.exp(F(a)), F(b))
        k_rgb = (F(1) if (cl or mono) else F(alpha)) / (F(3) * F(HW))
        k_d = F(1) / F(n_valid) if cl else (F(1) - F(alpha)) / F(HW)
        mf, w = m.astype(F), (op if tracking else np.ones(HW, F))
        fma = (np.float64(ea) * c.astype(np.float64) + np.float64(eb)).astype(F)
        r = fma * mf - g * mf
        wm = w * mf
        t = wm * np.sign(r)
        asum = (np.abs(r[0]) + np.abs(r[1])) + np.abs(r[2])
        ke = k_rgb * ea
        s_rgb, s_a, s_b = w * asum, ea * (((t[0] * c[0]) + (t[1] * c[1])) + (t[2] * c[2])), (t[0] + t[1]) + t[2]
        dmf = dm.astype(F)
        rd = d * dmf - gd * dmf
        val = dict(dL_dcolor=ke * t, dL_dopacity=(k_rgb * asum) if tracking else np.zeros(HW, F), dL_ddepth=(k_d * dmf) * np.sign(rd))
        assert all(x.dtype == F for x in (s_rgb, s_a, s_b, rd, *val.values()))
        S = [_wg_sum32(x) for x in (s_rgb, np.abs(rd), s_a, s_b)]
        l_rgb, l_d = S[0] / (3.0 * HW), 0.0 if mono else S[1] / (n_valid if cl else HW)
        loss = l_rgb if mono else (l_rgb + l_d if cl else al * l_rgb + (1.0 - al) * l_d)
        val.update(loss=loss, l1_rgb=l_rgb, l1_depth=l_d, dL_dexposure_a=0.0 if noexp else np.float64(k_rgb) * S[2],
                   dL_dexposure_b=0.0 if noexp else np.float64(k_rgb) * S[3])
        for k in SCALARS:
            val[k] = float(F(val[k]))
        out["value"] = {k: (v.reshape(-1, H, W) if k in SEEDS else v) for k, v in val.items()}
        return out

    # ---- float64 from the fp32 inputs
    c64, g64, op64, mf = c.astype(np.float64), g.astype(np.float64), op.astype(np.float64), m.astype(np.float64)
    ea = 1.0 if noexp else float(np.exp(np.float64(F(a))))
    eb = 0.0 if (noexp or mu("b_omitted")) else float(F(b))
    k_rgb = (1.0 if (cl or mono) else al) / (3.0 * HW)
    depth_n = float(n_valid) if cl else (max(float(dm.sum()), 1.0) if mu("depth_mean_over_valid") else float(HW))
    k_d = 1.0 / depth_n if cl else ((al if mu("alpha_for_one_minus_alpha") else 1.0 - al) / depth_n)
    w = op64 if weighted else np.ones(HW)
    r = (ea * c64 + eb - g64) * mf
    part = (np.abs(ea * c64) + abs(eb) + np.abs(g64)) * mf        # what |r| is made of
    s = sgn(r) * mf
    dmf = dm.astype(np.float64)
    rd = (d.astype(np.float64) - gd.astype(np.float64)) * dmf
    val = dict(dL_dcolor=k_rgb * ea * w * s, dL_dopacity=k_rgb * np.abs(r).sum(axis=0) * (1.0 if tracking else 0.0),
               dL_ddepth=k_d * dmf * sgn(rd) * dmf)
    mass = dict(dL_dcolor=np.abs(val["dL_dcolor"]), dL_dopacity=k_rgb * part.sum(axis=0) * (1.0 if tracking else 0.0),
                dL_ddepth=np.abs(val["dL_ddepth"]))
    terms = [w * np.abs(r).sum(axis=0), np.abs(rd), (1.0 if mu("ea_missing_from_da") else ea) * w * (s * c64).sum(axis=0), w * s.sum(axis=0)]
    tmass = [w * part.sum(axis=0), np.abs(rd), ea * w * np.abs(s * c64).sum(axis=0), w * np.abs(s).sum(axis=0)]
    S = [float((x * keep).sum()) + (STALE[i] if mu("stale_partial") else 0.0) for i, x in enumerate(terms)]
    M = [float(x.sum()) for x in tmass]
    l_rgb, l_d = S[0] / (3.0 * HW), 0.0 if mono else S[1] / depth_n
    m_rgb, m_d = M[0] / (3.0 * HW), 0.0 if mono else M[1] / depth_n
    if mono:
        loss, m_loss = l_rgb, m_rgb
    elif cl:
        loss, m_loss = l_rgb + l_d, m_rgb + m_d
    else:
        loss, m_loss = al * l_rgb + (1.0 - al) * l_d, al * m_rgb + (1.0 - al) * m_d
    val.update(loss=loss, l1_rgb=l_rgb, l1_depth=l_d, dL_dexposure_a=0.0 if noexp else k_rgb * S[2], dL_dexposure_b=0.0 if noexp else k_rgb * S[3])
    mass.update(loss=m_loss, l1_rgb=m_rgb, l1_depth=m_d, dL_dexposure_a=0.0 if noexp else k_rgb * M[2], dL_dexposure_b=0.0 if noexp else k_rgb * M[3])
    out["value"] = {k: (v.reshape(-1, H, W) if k in SEEDS else float(v)) for k, v in val.items()}
    out["mass"] = {k: (v.reshape(-1, H, W) if k in SEEDS else float(v)) for k, v in mass.items()}
    # residual signs: |r| and the scale an fp32 evaluation rounds it at (all pixels, whatever the gates say)
    fm = ea * c64 + eb
    out.update(abs_r=np.abs(fm - g64), scale=np.maximum(np.abs(fm), np.abs(g64)), abs_rd=np.abs(d.astype(np.float64) - gd.astype(np.float64)),
               scale_d=np.maximum(np.abs(d), np.abs(gd)).astype(np.float64))
    return out


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def assert_loss_close(got, want, tag, outputs=None):
    """got: output name -> array / scalar (a LossSeeds result, torch or NumPy; None entries are skipped); want: restate(...) in float64.
    Seed images pixel by pixel, none exempted; the scalars against sum|term|.  -> dict(output -> worst err / bound)."""
    ratios = {}
    for k in outputs or (SEEDS + SCALARS):
        if got.get(k) is None:
            continue
        have = _np(got[k]).astype(np.float64)
        v, ms = want["value"][k], want["mass"][k]
        if k in SEEDS:
            v, ms, have = v.reshape(-1), ms.reshape(-1), have.reshape(-1)
            assert have.shape == v.shape, (tag, k, have.shape, v.shape)
            assert np.isfinite(have).all(), "%s: %s has a non-finite pixel" % (tag, k)
            stray = (ms == 0) & (have != 0)
            assert not stray.any(), "%s: %s is %.3e at element %d, where the gate is closed or the residual is exactly 0" % (
                tag, k, have[np.argmax(stray)], int(np.argmax(stray)))
            bound = ROUND_K * EPS * ms
            ratio = np.where(ms > 0, np.abs(have - v) / np.where(ms > 0, bound, 1.0), 0.0)
            i = int(np.argmax(ratio))
            assert ratio[i] <= 1.0, "%s: %s element %d of %d: got %.9e want %.9e, error %.3e = %.3g x bound (mass %.3e)" % (
                tag, k, i, v.size, have[i], v[i], abs(have[i] - v[i]), ratio[i], ms[i])
            ratios[k] = float(ratio[i])
        else:
            have = float(have.reshape(-1)[0])
            assert np.isfinite(have), "%s: %s is %r" % (tag, k, have)
            bound = SUM_K * EPS * ms + EPS * abs(v)
            err = abs(have - v)
            assert err <= bound, "%s: %s: got %.9e want %.9e, error %.3e = %.3g x bound (sum|term| %.3e)" % (
                tag, k, have, v, err, err / bound if bound else np.inf, ms)
            ratios[k] = err / bound if bound else 0.0
    return ratios


# ---- generated frames --------------------------------------------------------------------------------------------------------------
def ulp_up(x):
    return np.nextafter(F(x), F(np.inf))


def ulp_down(x):
    return np.nextafter(F(x), F(-np.inf))


def _gt_with_sum(target, rng):
    """Three fp32 values whose fp32 sum (g0 + g1) + g2 is exactly `target`."""
    target = F(target)
    g0, g1 = F(target * F(rng.uniform(0.2, 0.3))), F(target * F(rng.uniform(0.2, 0.3)))
    g2 = F(target - (g0 + g1))
    for _ in range(16):
        s = (g0 + g1) + g2
        if s == target:
            return g0, g1, g2
        g2 = ulp_up(g2) if s < target else ulp_down(g2)
    raise AssertionError("no fp32 triple sums to %r" % target)


def make_frame(W, H, flags, masked, seed, rgb_thr=0.01, exposure="ab", plant=True, no_valid=False):
    """One frame with every gate of loss_pixel planted on a strip of pixels (plant=True and at least 64 pixels; a 1x1 image gets the
    gt sum exactly at the threshold), guard margins asserted.  exposure: "ab" (a = -0.05, b = 0.01), "a0" (a = 0, b = 1/64: exact-zero
    colour residuals can be planted), "negb" (b = -0.5: ea c + eb < 0 on most pixels).  -> dict of fp32 arrays + the restatement."""
    tracking, mono, cl = bool(flags & TRACKING), bool(flags & MONOCULAR), bool(flags & COMPUTE_LOSS)
    noexp = bool(flags & NO_EXPOSURE) or cl
    rng = np.random.default_rng(100003 * seed + 7 * W + H)
    HW = W * H
    c = rng.uniform(0.05, 1.0, (3, HW)).astype(F)
    if exposure == "a0":
        c = (np.round(c * 256) / 256).astype(F)   # c + 1/64 is exact
    d = rng.uniform(0.5, 4.0, HW).astype(F)
    op = rng.uniform(0.6, 1.0, HW).astype(F)
    a, b = {"ab": (F(-0.05), F(0.01)), "a0": (F(0.0), F(1.0 / 64)), "negb": (F(0.1), F(-0.5))}[exposure]
    ea, eb = (1.0, 0.0) if noexp else (float(np.exp(np.float64(a))), float(b))
    alpha, thr = (F(0.0), F(0.0)) if cl else (F(0.9), F(rgb_thr))
    g = (ea * c + eb + rng.normal(0, 0.1, (3, HW))).astype(F)
    if exposure != "negb":
        g = np.clip(g, 0.0, 1.5).astype(F)
    dark = rng.uniform(size=HW) < 0.1
    g[:, dark] = (rng.uniform(0.0, 0.2, (3, int(dark.sum()))) * float(thr)).astype(F)   # colour gate closed: sum < 0.6 thr
    gd = (d + rng.normal(0, 0.05, HW)).astype(F)
    gd[rng.uniform(size=HW) < 0.1] = 0
    mask = (rng.uniform(size=HW) < 0.6).astype(np.uint8) if masked else None
    zero_c, zero_d = np.zeros((3, HW), bool), np.zeros(HW, bool)
    planted = {}
    if plant and HW >= 64:
        pos = iter(range(3, HW))
        strip = lambda name, n: planted.setdefault(name, [next(pos) for _ in range(n)])  # noqa: E731
        if not cl:
            for p, tgt in zip(strip("rgb_thr", 3), (thr, ulp_up(thr), ulp_down(thr))):
                g[:, p] = _gt_with_sum(tgt, rng)
                assert (g[0, p] + g[1, p]) + g[2, p] == tgt
                if mask is not None:
                    mask[p] = 1
            if float(thr) == 0.5:   # dyadic: the fp32 and the float64 sums agree, every evaluation sees the same three sums
                for p, g2 in zip(strip("rgb_thr_dyadic", 3), (0.125, 0.125 + 2.0 ** -24, 0.125 - 2.0 ** -25)):
                    g[:, p] = (0.25, 0.125, g2)
                    assert float((g[0, p] + g[1, p]) + g[2, p]) == float(g[:, p].astype(np.float64).sum())
                    if mask is not None:
                        mask[p] = 1
        if not mono:
            lims = (F(0.0), np.nextafter(F(0.0), F(1.0))) if cl else (F(0.01), ulp_up(0.01), ulp_down(0.01))
            for p, v in zip(strip("gt_depth", len(lims)), lims):
                gd[p] = v
                op[p] = F(0.99)
                if mask is not None:
                    mask[p] = 1
            for p in strip("zero_depth", 2):   # residual exactly 0, gates open
                gd[p], op[p], zero_d[p] = d[p], F(0.99), True
                if mask is not None:
                    mask[p] = 1
        for p, v in zip(strip("opacity", 3), (F(0.95), ulp_up(0.95), ulp_down(0.95))):
            op[p] = v
            if not mono:
                gd[p] = F(d[p] + F(0.25))
            if mask is not None:
                mask[p] = 1
        if mask is not None:
            for p, v in zip(strip("mask", 3), (0, 1, 255)):
                mask[p] = v
                g[:, p] = (ea * c[:, p] + eb + 0.125).astype(F)
                if not mono:
                    gd[p], op[p] = F(d[p] + F(0.25)), F(0.99)
        if noexp or exposure == "a0":   # colour residual exactly 0: all three channels, then one channel only
            p, q = strip("zero_color", 2)
            for pp, chans in ((p, (0, 1, 2)), (q, (1,))):
                for ch in chans:
                    g[ch, pp] = F(c[ch, pp] + F(eb))
                    zero_c[ch, pp] = True
                    assert float(g[ch, pp]) == ea * float(c[ch, pp]) + eb
                if mask is not None:
                    mask[pp] = 1
    elif plant:   # a single pixel: the gt sum exactly at the threshold (closed), or a zero depth residual in the verification loss
        if cl:
            gd[0], zero_d[0] = d[0], True
        else:
            g[:, 0] = _gt_with_sum(thr, rng)
        planted["single"] = [0]
    if no_valid:
        gd[:] = 0
        zero_d[:] = False
    # ---- guard margins: push (never skip) what is too close to a sign change or to the opacity threshold
    near = np.abs(op.astype(np.float64) - float(F(0.95))) <= OPACITY_ULPS * 2.0 ** -24
    near[planted.get("opacity", [])] = False
    op[near] = F(0.5)
    for _ in range(8):
        fm = ea * c.astype(np.float64) + eb
        bad = (np.abs(fm - g) < 2 * GUARD * EPS * np.maximum(np.abs(fm), np.abs(g))) & ~zero_c
        if not bad.any():
            break
        g[bad] = (g[bad] + F(0.01)).astype(F)
    bad_d = (np.abs(d.astype(np.float64) - gd) < 2 * GUARD * EPS * np.maximum(d, gd)) & ~zero_d
    gd[bad_d] = (gd[bad_d] + F(0.01)).astype(F)
    fr = dict(W=W, H=H, flags=flags, alpha=alpha, rgb_thr=thr, image=c.reshape(3, H, W), depth=d.reshape(1, H, W), opacity=op.reshape(1, H, W),
              gt=g.reshape(3, H, W), gt_depth=None if mono else gd.reshape(H, W), mask=None if mask is None else mask.reshape(H, W),
              a=None if noexp else a, b=None if noexp else b, planted=planted, zero_c=zero_c, zero_d=zero_d)
    for p, tgt in zip(planted.get("rgb_thr", []), (thr, ulp_up(thr), ulp_down(thr))):   # (the pushes left the planted sums alone)
        assert (g[0, p] + g[1, p]) + g[2, p] == tgt
    fr["want"] = restate_frame(fr)
    check_guards(fr, "%dx%d flags %d seed %d" % (W, H, flags, seed))
    for v in fr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fr


def restate_frame(fr, **kw):
    return restate(fr["flags"], fr["alpha"], fr["rgb_thr"], fr["image"], fr["depth"], fr["opacity"], fr["gt"], fr["gt_depth"], fr["mask"],
                   fr["a"], fr["b"], **kw)


def check_guards(fr, tag, want=None, zero_c=None, zero_d=None):
    """Every residual is exactly 0 by construction or at least GUARD eps x scale from 0 (colour and depth, every pixel)."""
    want = want or fr["want"]
    zero_c = fr["zero_c"] if zero_c is None else zero_c
    zero_d = fr["zero_d"] if zero_d is None else zero_d
    ok = np.where(zero_c, want["abs_r"] == 0, want["abs_r"] >= GUARD * EPS * want["scale"])
    assert ok.all(), "%s: colour residual %.3e at %s is within %g eps of 0 (scale %.3e)" % (
        tag, want["abs_r"][~ok][0], np.argwhere(~ok)[0], GUARD, want["scale"][~ok][0])
    if fr["gt_depth"] is not None:
        ok = np.where(zero_d, want["abs_rd"] == 0, want["abs_rd"] >= GUARD * EPS * want["scale_d"])
        assert ok.all(), "%s: depth residual %.3e at pixel %d is within %g eps of 0" % (tag, want["abs_rd"][~ok][0], np.argwhere(~ok)[0, 0], GUARD)


def gt_for_render(color, depth, flags, a, b, rgb_thr, seed):
    """Ground truth built on images a device RENDERED, so that the gates of loss_pixel occur on real rendered values: gt sums on the
    threshold and an ulp to either side, gt depths at 0.01 and its neighbours, depth residuals exactly 0, colour residuals exactly 0
    (NO_EXPOSURE: gt = colour; with exposure only where the rendered colour is exactly 0, since ea 0 + eb = eb in every arithmetic).
    -> dict(gt [3,H,W], gt_depth [H,W] or None, zero_c, zero_d, planted); guard margins pushed, to be asserted with check_guards."""
    mono, noexp = bool(flags & MONOCULAR), bool(flags & NO_EXPOSURE)
    _, H, W = color.shape
    HW = H * W
    c, d = np.asarray(color, F).reshape(3, HW), np.asarray(depth, F).reshape(HW)
    ea, eb = (1.0, 0.0) if noexp else (float(np.exp(np.float64(F(a)))), float(F(b)))
    rng = np.random.default_rng(seed)
    g = (ea * c + eb + rng.normal(0, 0.1, (3, HW))).astype(F)
    dark = rng.uniform(size=HW) < 0.1
    g[:, dark] = (rng.uniform(0.0, 0.2, (3, int(dark.sum()))) * float(rgb_thr)).astype(F)
    gd = (d + rng.normal(0, 0.05, HW)).astype(F)
    gd[rng.uniform(size=HW) < 0.1] = 0
    zero_c, zero_d, planted = np.zeros((3, HW), bool), np.zeros(HW, bool), {}
    free = list(rng.permutation(HW))
    take = lambda ok: free.pop(next((i for i, p in enumerate(free) if ok(p)), 0))  # noqa: E731
    thr = F(rgb_thr)
    for tgt in (thr, ulp_up(thr), ulp_down(thr)):
        p = take(lambda p: c[:, p].min() > 0.01)
        g[:, p] = _gt_with_sum(tgt, rng)
        planted.setdefault("rgb_thr", []).append(p)
    if not mono:
        for v in (F(0.01), ulp_up(0.01), ulp_down(0.01)):
            p = take(lambda p: d[p] > 0.1)
            gd[p] = v
            planted.setdefault("gt_depth", []).append(p)
        for _ in range(2):
            p = take(lambda p: d[p] > 0.1)
            gd[p], zero_d[p] = d[p], True
            planted.setdefault("zero_depth", []).append(p)
    empty = np.flatnonzero((c == 0).all(axis=0))
    if noexp:
        p = take(lambda p: c[:, p].sum() > 2 * float(thr))
        g[:, p], zero_c[:, p] = c[:, p], True
        planted["zero_color"] = [p]
    elif empty.size and 3 * eb > 2 * float(thr):
        p = int(empty[0])
        g[:, p], zero_c[:, p] = F(eb), True
        planted["zero_color"] = [p]
    for _ in range(8):
        fm = ea * c.astype(np.float64) + eb
        bad = (np.abs(fm - g) < 2 * GUARD * EPS * np.maximum(np.abs(fm), np.abs(g))) & ~zero_c
        if not bad.any():
            break
        g[bad] = (g[bad] + F(0.01)).astype(F)
    bad_d = (np.abs(d.astype(np.float64) - gd) < 2 * GUARD * EPS * np.maximum(np.abs(d), np.abs(gd))) & ~zero_d
    gd[bad_d] = (gd[bad_d] + F(0.01)).astype(F)
    for p, tgt in zip(planted["rgb_thr"], (thr, ulp_up(thr), ulp_down(thr))):
        assert (g[0, p] + g[1, p]) + g[2, p] == tgt
    return dict(gt=g.reshape(3, H, W), gt_depth=None if mono else gd.reshape(H, W), zero_c=zero_c, zero_d=zero_d, planted=planted)


def make_cancelling_frame(W=64, H=48, seed=5):
    """Tracking frame whose residual signs are dealt in opposite pairs, so that dL/db = k sum w sgn(r) all but cancels
    (|dL/db| < 1e-3 sum|term|, asserted) while dL/da does not (the sign follows the larger colour of the pair).  The last workgroup
    (pixels 2048 ..) holds small terms: opacity 3e-5 and residuals of 1e-3."""
    rng = np.random.default_rng(seed)
    HW = W * H
    assert HW % WG == 0 and HW // WG >= 2
    a, b = F(-0.05), F(0.01)
    ea, eb = float(np.exp(np.float64(a))), float(b)
    c = rng.uniform(0.3, 1.0, (3, HW)).astype(F)
    half = rng.uniform(0.6, 1.0, HW // 2)
    op = np.repeat(half, 2).astype(F)
    small = np.arange(HW) >= HW - WG
    op[small] = F(3e-5)
    s = np.empty((3, HW))
    s[:, 0::2] = np.where(c[:, 0::2] > c[:, 1::2], 1.0, -1.0)
    s[:, 1::2] = -s[:, 0::2]
    s[:, 5] = s[:, 4]   # one pair left unbalanced: the sum is small, not zero
    mag = rng.uniform(0.05, 0.15, (3, HW)) * np.where(small, 0.01, 1.0)
    g = (ea * c + eb - s * mag).astype(F)
    d = rng.uniform(0.5, 4.0, HW).astype(F)
    gd = (d + rng.choice([-1.0, 1.0], HW) * rng.uniform(0.02, 0.1, HW)).astype(F)
    fr = dict(W=W, H=H, flags=TRACKING, alpha=F(0.9), rgb_thr=F(0.01), image=c.reshape(3, H, W), depth=d.reshape(1, H, W), opacity=op.reshape(1, H, W),
              gt=g.reshape(3, H, W), gt_depth=gd.reshape(H, W), mask=None, a=a, b=b, planted={}, zero_c=np.zeros((3, HW), bool),
              zero_d=np.zeros(HW, bool))
    fr["want"] = w = restate_frame(fr)
    check_guards(fr, "cancelling frame")
    assert abs(w["value"]["dL_dexposure_b"]) < 1e-3 * w["mass"]["dL_dexposure_b"] and w["value"]["dL_dexposure_b"] != 0
    assert abs(w["value"]["dL_dexposure_a"]) > 0.1 * w["mass"]["dL_dexposure_a"]
    for v in fr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fr


# name -> (W, H, flags, masked, seed, kwargs).  Every flag combination with every plant at 37x29 (two workgroups, the second ragged);
# every size with a tracking and a mapping frame; 640x480 once.
SIZES = ((1, 1), (257, 1), (33, 31), (32, 32), (41, 25), (37, 29))
FLAG_NAMES = {TRACKING: "track", TRACKING | MONOCULAR: "track-mono", TRACKING | NO_EXPOSURE: "track-noexp",
              TRACKING | MONOCULAR | NO_EXPOSURE: "track-mono-noexp", 0: "map", MONOCULAR: "map-mono", NO_EXPOSURE: "map-noexp",
              MONOCULAR | NO_EXPOSURE: "map-mono-noexp"}


def _case_table():
    t = {}
    seed = 0
    for flags, nm in FLAG_NAMES.items():
        for masked in ((False, True) if flags & TRACKING else (False,)):
            seed += 1
            t["%s%s-37x29" % (nm, "-mask" if masked else "")] = (37, 29, flags, masked, seed, {})
    t["map-mask-given-37x29"] = (37, 29, 0, True, 19, {})   # mapping reads no mask: one that is passed changes nothing
    t["cl-depth-mask-37x29"] = (37, 29, COMPUTE_LOSS, True, 21, {})
    t["cl-nodepth-mask-37x29"] = (37, 29, COMPUTE_LOSS | MONOCULAR, True, 22, {})
    t["cl-no-valid-pixel-37x29"] = (37, 29, COMPUTE_LOSS, True, 23, dict(no_valid=True))
    t["cl-depth-nomask-41x25"] = (41, 25, COMPUTE_LOSS, False, 24, {})
    for W, H in SIZES[:-1]:
        seed += 1
        t["track-mask-%dx%d" % (W, H)] = (W, H, TRACKING, True, seed, {})
        t["map-%dx%d" % (W, H)] = (W, H, 0, False, seed + 50, {})
    t["cl-depth-1x1"] = (1, 1, COMPUTE_LOSS, False, 25, {})
    for nm, flags, masked in (("track-mask", TRACKING, True), ("map", 0, False)):
        t[nm + "-a0-37x29"] = (37, 29, flags, masked, 31, dict(exposure="a0"))         # exact-zero colour residuals under exposure
        t[nm + "-negb-37x29"] = (37, 29, flags, masked, 32, dict(exposure="negb"))     # ea c + eb < 0
        t[nm + "-thr0.5-37x29"] = (37, 29, flags, masked, 33, dict(rgb_thr=0.5))       # dyadic gt sums at the threshold
    t["track-mask-640x480"] = (640, 480, TRACKING, True, 41, {})
    t["cancelling-64x48"] = None
    return t


CASE_TABLE = _case_table()


def cases():
    return list(CASE_TABLE)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """Cached: the arrays are shared between tests and read-only."""
    if name == "cancelling-64x48":
        return make_cancelling_frame()
    W, H, flags, masked, seed, kw = CASE_TABLE[name]
    fr = make_frame(W, H, flags, masked, seed, **kw)
    if kw.get("exposure") == "negb":
        fm = float(np.exp(np.float64(fr["a"]))) * fr["image"].astype(np.float64) + float(fr["b"])
        assert (fm < 0).mean() > 0.3
    if kw.get("no_valid"):
        assert fr["want"]["n_valid"] == 1 and not (fr["gt_depth"] > 0).any()
    return fr


# ---- isotropic regulariser ---------------------------------------------------------------------------------------------------------
ISO_P, ISO_C = (1, 255, 256, 257, 1001), (1, 2, 3)
ISO_WEIGHT = 10.0


def iso_restate(scales, weight, grad_in=None, dtype=np.float64, mutant=None):
    """weight * mean |s_ij - mean_j s_i.| over [P,C] and its gradient (+ grad_in when accumulating).  float64 from the fp32 scales;
    dtype=np.float32: k_isotropic's own order.  -> dict(value, mass: "loss", "dL_dscales")."""
    assert mutant is None or mutant in ISO_MUTANTS
    v32 = np.asarray(scales, F)
    P, C = v32.shape
    if dtype == np.float32:
        k = F(weight) / (F(P) * F(C))
        m = np.zeros(P, F)
        for ch in range(C):
            m = m + v32[:, ch]
        m = m / F(C)
        dd = v32 - m[:, None]
        sg = np.sign(dd)
        ssum = np.zeros(P, F)
        for ch in range(C):
            ssum = ssum + sg[:, ch]
        gq = k * (sg - (ssum / F(C))[:, None])
        assert gq.dtype == F and dd.dtype == F
        grad = gq if grad_in is None else np.asarray(grad_in, F) + gq
        return dict(value=dict(loss=float(F(np.float64(k) * np.abs(dd).astype(np.float64).sum())), dL_dscales=grad))
    v = v32.astype(np.float64)
    k = float(F(weight)) / (P if mutant == "mean_over_P" else P * C)
    m = v.mean(axis=1, keepdims=True)
    dd = v - m
    sg = np.where(dd >= 0, 1.0, -1.0) if mutant == "sgn0_plus" else np.sign(dd)
    gq = k * (sg - sg.sum(axis=1, keepdims=True) / C)
    old = np.zeros_like(v) if grad_in is None else np.asarray(grad_in, F).astype(np.float64)
    # loss: per term the mean's C - 1 additions and division and the subtraction are rounded at the size of |s| + |mean|
    return dict(value=dict(loss=k * np.abs(dd).sum(), dL_dscales=old + gq),
                mass=dict(loss=k * (np.abs(v) + np.abs(m)).sum(), dL_dscales=np.abs(old) + np.abs(gq)), abs_d=np.abs(dd), mean=np.abs(m))


@functools.lru_cache(maxsize=None)
def make_iso_case(P, C, seed=0):
    """Random log-normal scales with planted rows: equal scales (a freshly seeded Gaussian; gradient exactly 0 although fp32 sees
    d = +-1 ulp where ((a + a) + a) / 3 != a) and (1/8, 2/8, 3/8) (middle d exactly 0: gradient k (-1, 0, +1) exactly).
    -> dict(scales, grad_in, equal_rows, ramp_rows, want, want_acc)."""
    rng = np.random.default_rng(977 * P + 31 * C + seed)
    s = np.exp(rng.uniform(np.log(0.01), np.log(0.2), (P, C))).astype(F)
    rows = rng.permutation(P)
    n_eq = min(P, max(1, P // 3))
    equal_rows = np.sort(rows[:n_eq])
    s[equal_rows] = s[equal_rows, :1]
    ramp_rows = np.sort(rows[n_eq:n_eq + max(1, P // 16)]) if (C == 3 and P > n_eq) else np.zeros(0, int)
    if ramp_rows.size:
        s[ramp_rows] = (0.125, 0.25, 0.375)
    grad_in = rng.normal(0, 1e-3, (P, C)).astype(F)
    want = iso_restate(s, ISO_WEIGHT)
    planted = np.zeros(P, bool)
    planted[equal_rows] = planted[ramp_rows] = True
    free = ~planted[:, None] & (C > 1)
    assert (want["abs_d"][free.repeat(C, 1)] >= GUARD * EPS * want["mean"].repeat(C, 1)[free.repeat(C, 1)]).all()
    assert (want["abs_d"][equal_rows] == 0).all() and (want["value"]["dL_dscales"][equal_rows] == 0).all()
    if C == 3:
        a = s[equal_rows, 0]
        off = ((a + a) + a) / F(3) != a
        if P >= 255:
            assert off.any(), "no equal row whose fp32 mean differs from the scale"
        k = float(F(ISO_WEIGHT)) / (P * C)
        assert (want["value"]["dL_dscales"][ramp_rows] == k * np.array([-1.0, 0.0, 1.0])).all()
    for x in (s, grad_in):
        x.setflags(write=False)
    return dict(scales=s, grad_in=grad_in, equal_rows=equal_rows, ramp_rows=ramp_rows, want=want, want_acc=iso_restate(s, ISO_WEIGHT, grad_in))


def assert_iso_close(loss, grad, want, tag):
    """-> dict(loss, dL_dscales -> worst err / bound); the gradient element by element, exactly 0 where nothing contributes."""
    have, v, ms = _np(grad).astype(np.float64), want["value"]["dL_dscales"], want["mass"]["dL_dscales"]
    assert have.shape == v.shape and np.isfinite(have).all(), (tag, have.shape)
    stray = (ms == 0) & (have != 0)
    assert not stray.any(), "%s: dL_dscales is %.3e in row %d, where it is exactly 0" % (tag, have[stray][0], np.argwhere(stray)[0, 0])
    ratio = np.where(ms > 0, np.abs(have - v) / np.where(ms > 0, ROUND_K * EPS * ms, 1.0), 0.0)
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[i, j] <= 1.0, "%s: dL_dscales[%d, %d]: got %.9e want %.9e = %.3g x bound" % (tag, i, j, have[i, j], v[i, j], ratio[i, j])
    lv, lm = want["value"]["loss"], want["mass"]["loss"]
    bound = SUM_K * EPS * lm + EPS * abs(lv)
    err = abs(float(_np(loss)) - lv)
    assert err <= bound, "%s: loss: got %.9e want %.9e, error %.3e = %.3g x bound" % (tag, float(_np(loss)), lv, err, err / bound if bound else np.inf)
    return dict(loss=err / bound if bound else 0.0, dL_dscales=float(ratio[i, j]))


# ---- measured worst err / bound (profiles/r10_loss_parity.json, written when GSAJ_WRITE_PARITY is set) ----------------------------
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10_loss_parity.json")
WORST = {}


def note(who, family, ratios):
    """who: "mirror_fp32_cpu" or "device_mi355x"; family: the case family; ratios: output -> err / bound; the worst is kept."""
    slot = WORST.setdefault(who, {}).setdefault(family, {})
    for k, v in ratios.items():
        slot[k] = max(slot.get(k, 0.0), float(v))
    if os.environ.get("GSAJ_WRITE_PARITY"):
        doc = {}
        if os.path.exists(PARITY):
            with open(PARITY) as fh:
                doc = json.load(fh)
        doc["what"] = ("worst |evaluation - float64 restatement| / bound per output and case family (tests/loss_restated.py): the fp32 "
                       "mirror from tests/test_cpu_loss.py, the device from tests/test_gpu_loss.py and tests/test_gpu_device_tracker.py")
        doc["constants"] = dict(ROUND_K=ROUND_K, SUM_K=SUM_K, GUARD=GUARD)
        doc.setdefault("worst_err_over_bound", {}).setdefault(who, {}).update(WORST[who])
        with open(PARITY, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
