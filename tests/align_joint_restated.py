"""NumPy restatements of the JOINT frame-to-frame RGB-D alignment -- csrc/align.hip: k_rgbd_align8, k_rgbd_align8_fold -- on top of
tests/align_restated.py and tests/gn8_restated.py's step.  TEST INFRASTRUCTURE ONLY; shared by
tests/test_cpu_align_joint.py and tests/test_gpu_align_joint.py.

The unknowns are x = [rho(3), theta(3), a, b]; the current frame is modelled as e^a I_r + b (include/gsaj.h, "the joint form" of the
frame-to-frame alignment).  Everything up to the photometric residual -- the warp, the gates, the bilinear taps, J_I, the depth term --
is align_restated.pixels, called as it is; what is restated here is what the joint kernel does differently:

  pixels8            g_I = ea I_r;  r_I = I_c - (g_I + b);  J8 = [J_I, -g_I, -1], the depth row [J_Z, 0, 0];  the 49 terms of a pixel.
                     One statement, evaluated in float64 (the restatement) or float32 (the MIRROR, one rounding per operation); `gain` is
                     an INPUT of both: expf is not correctly rounded, so the device reports the float it used (gain_out) and the mirror is
                     evaluated with it
  fold8, row_bound8, assert_row_close8   align_restated's fold, row_bound and assert_row_close at the joint row's layout (ROW8: 64
                     slots, NX = 8): k_rgbd_align8_fold -- the terms summed in float64, normalised by the valid count, the overlap gate
  align8_loop        the aligner's joint loop on gn8_restated.lm8_step, the relevel's effect on the exposure included
  with_brightness    a case whose current frame's colour is e^a I + b
  exposure_tolerance the tolerance of the recovered (a, b): twice the distance between the loop in float64 and the same loop on the
                     float32 mirror, plus a rounding floor -- computed here, on the CPU, from no device result
  MUTANTS            wrong kernels the finite-difference test or the comparators must reject

The row bound.  assert_row_close8 takes the mirror's float32 terms AS GIVEN (they are the kernel's own terms bit for bit wherever the
pixel parity holds: the same operations on the same floats), sums them in float64 and allows ROW_ROUNDINGS 2^-24 sum|term| per slot.
Between a term and the row's slot lie: the wave's reduce10 tree -- one half-wave swap, one row swap, four row rotations: 6 additions;
the four waves added IN ORDER, ((w0 + w1) + w2) + w3: 3 additions on the longest path (not 2: it is a chain, not a tree); the fold's
float64 sums (2^-53: nothing) and its quotient rounded to float32 once: 1.  ROW_ROUNDINGS = 6 + 3 + 1 = 10, whatever the slot: the
joint kernel's 49 partials go through five reduce10 of the same depth, none through a reduce4."""
import functools
import math

import numpy as np

import align_restated as ar
import gn8_restated as gn8
import gn_restated as gn

F = np.float32
EPS = ar.EPS
ROW_ROUNDINGS = 6 + 3 + 1
ROW8 = ar.RowLayout(64, 8, ROW_ROUNDINGS)
ROW, NH, NX = ROW8.ROW, ROW8.NH, ROW8.NX
LOSS, VALID, GATES = ROW8.LOSS, ROW8.VALID, ROW8.GATES   # [44] loss, [45] L_photo, [46] L_depth, [47] valid pixels, [48] open depth gates, [49:64) zero
assert (ROW, NH, LOSS, VALID, GATES) == (64, 36, 44, 47, 48)
MUTANTS = ("a_column_sign", "a_column_without_gain", "b_column_plus_one", "gain_on_current", "exposure_in_depth_term", "h8_by_columns",
           "a_b_swapped")
EXPOSURES = ((0.0, 0.0), (0.1, 0.03), (-0.15, 0.05))
# the floor of a recovered exposure in float32: a and b are stepped 20 times, a += x[6] (1 rounding of a value <= 1 each), and the gain
# e^a carries expf's 2 ulp: (20 + 4) 2^-24
EXPOSURE_FLOOR = 24 * EPS


def gain_of(a):
    """e^a as the restatement takes it when no device gain is given: exp in float64 of the float32 a, rounded to float32."""
    return F(np.exp(np.float64(F(a))))


def with_brightness(case, a, b, exposure=(0.0, 0.0)):
    """The case with its current frame's colour replaced by e^a I + b (float32, as a camera would hand it over) and the state's
    exposure set to `exposure`."""
    cc = (np.exp(np.float64(a)) * np.asarray(case["cur_color"], np.float64) + np.float64(b)).astype(F)
    return dict(case, cur_color=cc, exposure=(F(exposure[0]), F(exposure[1])))


# ---- the per-pixel arithmetic -----------------------------------------------------------------------------------------------------------
def pixels8(case, dtype=np.float64, gain=None, mutant=None, nudge=None):
    """case["exposure"] = (a, b) of the state (float32 on the device; case["exposure_exact"], if present, is used unrounded: finite
    differences).  gain: the e^a to use, by default gain_of(a) (exp(a) in float64 for an exact exposure).  nudge: align_restated's, and
    "gI" for the product ea I_r.
    -> align_restated.pixels' dict with rec[..., 8:11] = r_I, s_I, h_I of the joint residual, J8 [H,W,8] the photometric row, JZ8 [H,W,8]
    the depth row, terms [H,W,64]."""
    assert mutant is None or mutant in MUTANTS, mutant
    D = dtype
    nudge = dict(nudge or {})
    d_rI, d_gI = nudge.pop("rI", 0.0), nudge.pop("gI", 0.0)
    px = ar.pixels(case, D, nudge=nudge or None)
    H, W = case["H"], case["W"]
    if "exposure_exact" in case:
        a, b = (np.float64(v) for v in case["exposure_exact"])
        ea = np.exp(a) if gain is None else np.float64(gain)
    else:
        a, b = (F(v) for v in case.get("exposure", (0.0, 0.0)))
        ea = gain_of(a) if gain is None else F(gain)
    ea, b = D(ea), D(b)
    dp = D(F(case["delta_photo"]))
    with np.errstate(all="ignore"):
        ok, gate = px["valid"], px["gate"]
        Ir = ar._grey(case["ref_color"], D)
        Ic = px["rec"][..., 5]
        gI = ea * Ir
        if d_gI:
            gI = gI + D(d_gI)
        if mutant == "gain_on_current":
            rI = ea * Ic - (Ir + b)
        else:
            rI = Ic - (gI + b)
        if d_rI:
            rI = rI + D(d_rI)
        sI, hI, lI = ar._irls(rI, D(1), dp, D, None)
        col_a = -Ir if mutant == "a_column_without_gain" else gI if mutant == "a_column_sign" else -gI
        col_b = np.full((H, W), D(1) if mutant == "b_column_plus_one" else D(-1), D)
        if mutant == "a_b_swapped":
            col_a, col_b = col_b, col_a
        J8 = np.concatenate([px["JI"], col_a[..., None], col_b[..., None]], -1).astype(D)
        JZ8 = np.concatenate([px["JZ"], np.zeros((H, W, 2), D)], -1).astype(D)
        if mutant == "exposure_in_depth_term":
            JZ8[..., 6], JZ8[..., 7] = np.where(gate, col_a, D(0)), np.where(gate, col_b, D(0))
        sZ, hZ, lZ = px["rec"][..., 13], px["rec"][..., 14], px["terms"][..., 29]
        terms = np.zeros((H, W, ROW), D)
        order = [(k, l) for k in range(8) for l in range(k, 8)]
        if mutant == "h8_by_columns":
            order = [(k, l) for l in range(8) for k in range(l + 1)]
        leak = mutant == "exposure_in_depth_term"
        for n, (k, l) in enumerate(order):
            ak = hI * J8[..., k]
            if l < 6 or leak:
                terms[..., n] = ak * J8[..., l] + (hZ * JZ8[..., k]) * JZ8[..., l]
            else:
                terms[..., n] = ak * J8[..., l]
        for k in range(8):
            terms[..., NH + k] = sI * J8[..., k] + sZ * JZ8[..., k] if (k < 6 or leak) else sI * J8[..., k]
        terms[..., LOSS], terms[..., LOSS + 1], terms[..., LOSS + 2] = lI + lZ, lI, lZ
        terms[..., VALID], terms[..., GATES] = D(1), gate.astype(D)
        terms = np.where(ok[..., None], terms, D(0)).astype(D)
        rec = px["rec"].copy()
        rec[..., 8], rec[..., 9], rec[..., 10] = rI, sI, hI
        rec = np.where(ok[..., None], rec, D(0)).astype(D)
    out = dict(px, rec=rec, terms=terms, J8=np.where(ok[..., None], J8, D(0)), JZ8=np.where(ok[..., None], JZ8, D(0)))
    return out


def mirror8(case, gain=None, mutant=None):
    """The float32 mirror of k_rgbd_align8 at the gain the device reports: what pix_out / valid_out must hold, bit for bit."""
    return pixels8(case, np.float32, gain, mutant)


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------
# k_rgbd_align8_fold: the terms summed in float64, normalised by the valid count, the overlap gate -> 64 slots; the bound per slot:
# ROW_ROUNDINGS 2^-24 sum|term| / n, plus each borderline pixel's own |term| / n.  align_restated's functions at the joint row's layout.
fold8 = functools.partial(ar.fold, lay=ROW8)
row_bound8 = functools.partial(ar.row_bound, lay=ROW8)


def rounding_bound8(case, px64, border, gain=None):
    """align_restated.rounding_bound for the joint terms: every intermediate nudged by its own first-order error, one at a time, both
    ways, the per-pixel |change| summed and doubled.  The sizes are align_restated's, with the joint residual's two more roundings
    (g_I = ea I_r, g_I + b: r_I 11 -> 13, of greys <= e^a + |b| <= 2) and g_I itself (1 rounding of a grey <= 2) where it is a column."""
    zs = np.concatenate([np.asarray(case[k], np.float64).reshape(-1) for k in ("ref_depth", "cur_depth") if case.get(k) is not None])
    zmax = float(np.abs(zs[np.isfinite(zs)]).max(initial=1.0))
    side = 24 * 2 * max(case["W"], case["H"])
    size = {"u": side, "v": side, "rI": 13 * 2, "gI": 1 * 2, "rZ": 15 * zmax, "gx": 4 * 2, "gy": 4 * 2, "hx": 4 * zmax, "hy": 4 * zmax}
    base = np.asarray(px64["terms"], np.float64)
    first = np.zeros(ROW)
    for name, k in size.items():
        d = np.zeros(base.shape)
        for sg in (1.0, -1.0):
            t = pixels8(case, np.float64, gain, nudge={name: sg * k * EPS})["terms"]
            d = np.maximum(d, np.abs(t - base))
        first += d[~border].sum(0)
    t = np.abs(base).reshape(-1, ROW)
    n = max(t[:, VALID].sum(), 1.0)
    return (2.0 * first + (16 + ar.ROW_ROUNDINGS) * EPS * t.sum(0)) / n + (t[border.reshape(-1)].sum(0) / n if border.any() else 0.0)


# ---- the comparators of the GPU tests ---------------------------------------------------------------------------------------------------
# gn8_row against the float64 sum of the per-pixel terms (the mirror's): align_restated.assert_row_close at the joint row's layout
assert_row_close8 = functools.partial(ar.assert_row_close, lay=ROW8)


def assert_gain(gain, a, tag):
    """The gain the device reports: exactly 1.0f at a = 0, otherwise within 2 ulp of exp(float64(a)) -- the allowance
    tests/loss_restated.py gives expf."""
    gain, a = F(gain), F(a)
    if a == 0:
        assert gain == F(1.0), "%s: e^0 = %r, not exactly 1" % (tag, gain)
        return
    want = np.exp(np.float64(a))
    assert abs(np.float64(gain) - want) <= 2.0 * float(np.spacing(F(want))), "%s: gain %r, exp(a) = %.12g" % (tag, gain, want)


# ---- the restated loop ------------------------------------------------------------------------------------------------------------------
def relevel8(st, lambda_init):
    """gsaj_pose_gn_relevel's effect on a gn8_restated.lm8_new_state: back to the accepted pose AND exposure, a new baseline."""
    if st["has"]:
        st["exposure"] = st["acc_exposure"].copy()
    ar.relevel(st, lambda_init)
    st.update(H=np.zeros((8, 8)), g=np.zeros(8), dexposure=np.zeros(2), acc_exposure=st["exposure"].copy())
    return st


def align8_loop(case, levels, schedule=None, dtype=np.float64, lm=None, exposure_init=(0.0, 0.0), record=None):
    """The aligner's joint loop restated: from case["w2c"] and exposure_init, schedule[i] iterations at level levels - i, each
    pixels8() -> fold8() -> gn8_restated.lm8_step, relevel8 between levels.  The state's pose and exposure are handed to every
    evaluation rounded to float32, as the device holds them.  -> dict(w2c, exposure: the accepted ones, losses, st).
    record: a list that receives a copy of (w2c, exposure) after every step."""
    lm = dict(ar.LM, **(lm or {}))
    schedule = [8] + [6] * levels if schedule is None else list(schedule)
    assert len(schedule) == levels + 1
    st = gn8.lm8_new_state(np.asarray(case["w2c"], np.float64), lm["lambda_init"], exposure_init)
    losses, memo, at = [], {}, levels
    for l, n in zip(range(levels, -1, -1), schedule):
        if not n:
            continue
        if at != l:
            relevel8(st, lm["lambda_init"])
            at = l
        acc = []
        for _ in range(n):
            c = ar.level_case(case, l, st["w2c"], memo=memo)
            c["exposure"] = (F(st["exposure"][0]), F(st["exposure"][1]))
            row = fold8(pixels8(c, dtype)["terms"], c)
            gn8.lm8_step(st, gn8.sym8(row[:NH]), row[NH:NH + NX], row[LOSS], lm["nu"], lm["lambda_min"], lm["lambda_max"],
                         lm["converged_threshold"])
            acc.append(st["acc_loss"])
            if record is not None:
                record.append((st["w2c"].copy(), st["exposure"].copy()))
        losses.append((l, acc))
    return dict(w2c=st["acc_w2c"].copy(), exposure=st["acc_exposure"].copy(), losses=losses, st=st)


def behaviour_case8(m, depth, a, b):
    """align_restated.behaviour_case with the current frame's brightness changed."""
    return with_brightness(ar.behaviour_case(m, depth), a, b)


_TOL = {}


def exposure_tolerance(m, depth, a, b):
    """-> (tolerance [2] for the recovered (a, b), the float64 loop's result, the float32 loop's result).  Twice the distance between the
    restated loop in float64 and the same loop on the float32 mirror, plus EXPOSURE_FLOOR: the device differs from the float64 loop by
    float32 rounding alone, as the float32 loop does -- in another order, so the distance is doubled."""
    key = (m, depth, a, b)
    if key not in _TOL:
        case = behaviour_case8(m, depth, a, b)
        r64, r32 = align8_loop(case, 2), align8_loop(case, 2, dtype=np.float32)
        _TOL[key] = (2.0 * np.abs(r64["exposure"] - r32["exposure"]) + EXPOSURE_FLOOR, r64, r32)
    return _TOL[key]


def exposure_for(ref_exposure, rel_exposure):
    """RgbdAligner.exposure_for in float64: (a_r + a, e^a b_r + b)."""
    (ar_, br_), (a, b) = (np.asarray(v, np.float64) for v in (ref_exposure, rel_exposure))
    return np.array([ar_ + a, math.exp(a) * br_ + b])


# ---- the committed parity cases ----------------------------------------------------------------------------------------------------------
PARITY_SIZES = [(2, 2), (65, 4), (97, 61)]   # the smallest legal; two workgroups in x with a ragged lane edge; partial workgroups on both edges
LONG_FOLD = (70, 260)   # 2 x 65 = 130 rows: past one trip of the fold's four-deep load loop (16 groups x 4 = 64 rows of 64 floats)


def parity_case8(W, H, mode, a, b):
    """align_restated.parity_case with the current frame's brightness changed by (a, b) and the state's exposure AT (a, b): the
    residuals are then those of the unchanged scene, on both sides of delta."""
    return with_brightness(ar.parity_case(W, H, mode), a, b, exposure=(a, b))


def planted_case8(sign, a=0.1, b=0.03):
    """align_restated.planted_case through the joint form: the planted greys are those of the UNCHANGED scene, so the reference is taken
    to the current frame's brightness the other way round -- the reference colour r becomes (r - b) / e^a rounded to float32, and the state's
    exposure is (a, b): |r_I| still lands on either side of delta (asserted by tests/test_cpu_align_joint.py, not assumed)."""
    case, planted, sh = ar.planted_case(sign)
    rc = ((np.asarray(case["ref_color"], np.float64) - b) / np.exp(np.float64(a))).astype(F)
    return dict(case, ref_color=rc, exposure=(F(a), F(b))), planted, sh


# ---- the degenerate case ----------------------------------------------------------------------------------------------------------------
def constant_case(ref_value=0.5, cur_value=0.62, side=8):
    """An 8 x 8 constant reference and a constant current frame of another value, depth 2 everywhere, both poses the identity: every
    image gradient is zero, so the pose columns are zero and the a and b columns are collinear (-ea c and -1)."""
    cam = dict(W=side, H=side, fx=8.0, fy=8.0, cx=side / 2.0, cy=side / 2.0)
    one = np.ones((side, side), F)
    return dict(cam, ref_color=np.full((3, side, side), ref_value, F), ref_depth=2 * one, ref_w2c=np.eye(4, dtype=F),
                cur_color=np.full((3, side, side), cur_value, F), cur_depth=2 * one, w2c=np.eye(4, dtype=F), exposure=(F(0), F(0)), **ar.PARAMS)
