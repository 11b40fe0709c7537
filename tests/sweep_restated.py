"""NumPy restatement of motion stereo (include/gsaj.h "motion stereo", csrc/sweep.hip), steps a-i in the header's order of operations:
the fp32 steps as float32 operations one at a time (NumPy rounds every float32 operation once, as the kernels do without contraction;
division and floor included), everything else in int64; with a `mutant=` switch for the canaries.  TEST INFRASTRUCTURE ONLY; shared by
tests/test_cpu_motion_stereo.py and the GPU tests.

  grey_u8         float32 [3,H,W] -> the grey byte (gsaj_grey_u8)
  gradients       a: the clipped Sobel bytes Gx, Gy
  rel_pose        b: T = W2C_src inverse(W2C_ref), align_restated.rel_pose's lines in float32
  hypotheses      c: step and w_d
  warp            d: where a reference pixel lands under a hypothesis: inside, the top-left tap, the sixteenths
  pixel_costs     e: pc [H,W,D]
  cost_volume     f: C [H,W,D], the clamped box sum (two passes of one axis each: the window is a product)
  path_costs      g: stereo_restated.path_costs on C padded with D zero columns on the left -- what that function computes with its
                  first column at D -- and the padding dropped
  winner          h: argmin, uniqueness, the parabola step, the winner's own centre warp -> idx16
  depth           i: fp64, rounded to float32 once
  sweep           all of it
  case            two views of align_restated's analytic scene through grey_u8, the reference pose NOT the identity, with the ray-cast
                  depth of the reference view
  planted_sums    an S for the winner alone with every rule's edge in it

Nothing here is organised the way the kernels are: the kernels own one (pixel, hypothesis) per lane, this walks whole images per
hypothesis."""
import numpy as np

import align_restated as ar
import gn_restated as gn
import stereo_restated as sr

F = np.float32
INVALID = -16
MUTANTS = ("pixel_centres_at_integers", "t_rel_wrong_side", "step_over_D", "fa_fb_swapped", "shift_5", "outside_costs_0", "inside_W_minus_1",
           "gy_sign_flipped", "tie_highest", "subpixel_floor", "centre_outside_kept", "depth_one_over_idx")
DEFAULTS = dict(D=16, r=3, P1=100, P2=400, paths=8, uniqueness=10, outside_cost=80)
REF_TWIST = np.array([0.05, 0.02, -0.03, 0.02, 0.03, -0.01])   # the reference pose of the scenes: not the identity
MOTIONS = {"sideways": (0.15, 0.0, 0.0, 0.0, 0.0, 0.0), "mixed": (0.12, 0.05, 0.02, 0.01, -0.02, 0.01),
           "forward": (0.02, 0.01, 0.2, 0.0, 0.0, 0.0),               # the epipole lies in the image
           "rotation": (0.0, 0.0, 0.0, 0.01, -0.02, 0.015),           # every hypothesis warps alike
           "identity": (0.0,) * 6,                                    # all costs tie
           "backward": (0.0, 0.0, -1.5, 0.0, 0.0, 0.0)}               # near hypotheses fall behind the source camera


# ---- grey bytes -----------------------------------------------------------------------------------------------------------------------
def grey_u8(color):
    """float32 [3,H,W] -> uint8 [H,W]: g = ((c0 + c1) + c2) (float)(1.0 / 3.0); min(max(floorf(g 255.0f + 0.5f), 0), 255); a NaN gives 0
    (fmaxf returns its other argument)."""
    c = np.asarray(color, F)
    with np.errstate(all="ignore"):
        g = ((c[0] + c[1]) + c[2]) * F(1.0 / 3.0)
        b = np.fmin(np.fmax(np.floor(g * F(255.0) + F(0.5)), F(0.0)), F(255.0))
    return b.astype(np.uint8)


# ---- a ----------------------------------------------------------------------------------------------------------------------------------
def gradients(img, mutant=None):
    """uint8 [H,W] -> (Gx, Gy) int64 [H,W] in 0..30, coordinates clamped to the image."""
    H, W = img.shape
    I = np.pad(np.asarray(img, np.uint8).astype(np.int64), 1, mode="edge")
    gx = (I[0:H, 2:] - I[0:H, :-2]) + 2 * (I[1:H + 1, 2:] - I[1:H + 1, :-2]) + (I[2:, 2:] - I[2:, :-2])
    gy = (I[2:, 0:W] - I[:-2, 0:W]) + 2 * (I[2:, 1:W + 1] - I[:-2, 1:W + 1]) + (I[2:, 2:] - I[:-2, 2:])
    if mutant == "gy_sign_flipped":
        gy = -gy
    return np.clip(gx, -15, 15) + 15, np.clip(gy, -15, 15) + 15


# ---- b, c -------------------------------------------------------------------------------------------------------------------------------
def rel_pose(ref_w2c, src_w2c, mutant=None):
    with np.errstate(all="ignore"):
        return ar.rel_pose(src_w2c, ref_w2c, F, "t_rel_wrong_side" if mutant == "t_rel_wrong_side" else None).astype(F)


def hypotheses(w_min, w_max, D, mutant=None):
    """-> (step, w [D]) float32."""
    w_min, w_max = F(w_min), F(w_max)
    step = (w_max - w_min) / F(D if mutant == "step_over_D" else D - 1)
    return step, (w_min + np.arange(D).astype(F) * step).astype(F)


# ---- d ----------------------------------------------------------------------------------------------------------------------------------
def warp(cam, T, w, mutant=None, xs=None, ys=None):
    """Every reference pixel (or the pixels xs, ys) under inverse depth w (a float32 scalar, or an array shaped like the pixels)
    -> (inside bool, x0, y0 int64 (0 where outside), fa, fb int64)."""
    W, H = cam["W"], cam["H"]
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    if xs is None:
        ys, xs = np.mgrid[0:H, 0:W]
    w = np.asarray(w, F)
    half = F(0.0) if mutant == "pixel_centres_at_integers" else F(0.5)
    with np.errstate(all="ignore"):
        xn = ((xs.astype(F) + half) - cx) / fx
        yn = ((ys.astype(F) + half) - cy) / fy
        p = [((T[k, 0] * xn + T[k, 1] * yn) + T[k, 2]) + w * T[k, 3] for k in range(3)]
        iz = F(1.0) / p[2]
        u = ((fx * iz) * p[0] + cx) - half
        v = ((fy * iz) * p[1] + cy) - half
        x0f, y0f = np.floor(u), np.floor(v)
        xmax = F(W - 1) if mutant == "inside_W_minus_1" else F(W - 2)
        inside = (p[2] > 0) & (x0f >= 0) & (x0f <= xmax) & (y0f >= 0) & (y0f <= F(H - 2))
        fa = np.floor((u - x0f) * F(16.0))
        fb = np.floor((v - y0f) * F(16.0))
    z = lambda a: np.where(inside, a, 0).astype(np.int64)   # noqa: E731
    if mutant == "fa_fb_swapped":
        fa, fb = fb, fa
    return inside, z(x0f), z(y0f), z(fa), z(fb)


# ---- e, f ---------------------------------------------------------------------------------------------------------------------------------
def pixel_costs(ref, src, cam, T, w, outside_cost, mutant=None):
    """-> pc int64 [H,W,D]."""
    H, W = ref.shape
    Gr, Gs = gradients(ref, mutant), gradients(src, mutant)
    pc = np.empty((H, W, len(w)), np.int64)
    for d, wd in enumerate(w):
        inside, x0, y0, fa, fb = warp(cam, T, wd, mutant)
        x1 = np.minimum(x0 + 1, W - 1)   # (only the mutant inside_W_minus_1 reaches the clamp)
        y1 = np.minimum(y0 + 1, H - 1)
        tot = np.zeros((H, W), np.int64)
        for A, B in zip(Gr, Gs):
            s = (16 - fa) * (16 - fb) * B[y0, x0] + fa * (16 - fb) * B[y0, x1] + (16 - fa) * fb * B[y1, x0] + fa * fb * B[y1, x1]
            tot += np.abs(256 * A - s)
        out = 0 if mutant == "outside_costs_0" else outside_cost
        pc[:, :, d] = np.where(inside, tot >> (5 if mutant == "shift_5" else 6), out)
    return pc


def box(pc, r):
    """The sum over |dx|, |dy| <= r, coordinates clamped to the image."""
    def taps(a, axis):
        n = a.shape[axis]
        out = np.zeros_like(a)
        for o in range(-r, r + 1):
            out += np.take(a, np.clip(np.arange(n) + o, 0, n - 1), axis=axis)
        return out

    return taps(taps(pc, 1), 0)


# ---- g ----------------------------------------------------------------------------------------------------------------------------------
def path_costs(C, D, P1, P2, paths):
    H, W, _ = C.shape
    padded = np.concatenate([np.zeros((H, D, D), np.int64), np.asarray(C, np.int64)], axis=1)
    return sr.path_costs(padded, D, P1, P2, paths)[:, D:]


# ---- h, i -------------------------------------------------------------------------------------------------------------------------------
def winner(S, cam, T, w, uniqueness, mutant=None):
    """S int64 [H,W,D] -> idx16 int16 [H,W], -16 where invalid."""
    S = np.asarray(S, np.int64)
    H, W, D = S.shape
    ds = np.arange(D)
    best = S.min(axis=2)
    hit = S == best[:, :, None]
    dstar = (D - 1 - hit[:, :, ::-1].argmax(axis=2)) if mutant == "tie_highest" else hit.argmax(axis=2)
    far = np.abs(ds[None, None, :] - dstar[:, :, None]) > 1
    unique = ~((S * (100 - uniqueness) < (best * 100)[:, :, None]) & far).any(axis=2)
    sm = np.take_along_axis(S, np.clip(dstar - 1, 0, D - 1)[:, :, None], 2)[:, :, 0]
    sp = np.take_along_axis(S, np.clip(dstar + 1, 0, D - 1)[:, :, None], 2)[:, :, 0]
    den = np.maximum(sm + sp - 2 * best, 1)
    num = (sm - sp) * 16 + den
    q = num // (2 * den) if mutant == "subpixel_floor" else np.sign(num) * (np.abs(num) // (2 * den))   # C division: towards zero
    idx = 16 * dstar + np.where((dstar > 0) & (dstar < D - 1), q, 0)
    centre = warp(cam, T, np.asarray(w, F)[dstar], mutant)[0]
    ok = unique if mutant == "centre_outside_kept" else unique & centre
    return np.where(ok, idx, INVALID).astype(np.int16)


def depth(idx16, w_min, step, mutant=None):
    """fp64, rounded to float32 once: w = (double)w_min + ((double)idx16 / 16.0) (double)step; 1 / w where idx16 >= 0 and w > 0, else 0."""
    i = np.asarray(idx16, np.int16).astype(np.float64)
    with np.errstate(all="ignore"):
        w = (i / 16.0) if mutant == "depth_one_over_idx" else np.float64(F(w_min)) + (i / 16.0) * np.float64(F(step))
        z = np.where((i >= 0) & (w > 0), 1.0 / w, 0.0)
    return z.astype(F)


def sweep(ref, src, cam, ref_w2c, src_w2c, w_min, w_max, D=16, r=3, P1=100, P2=400, paths=8, uniqueness=10, outside_cost=80, mutant=None):
    """-> dict(T, step, w, grad, pc, C, S, idx16, depth); grad: int64 [2,H,W], the gradient bytes Gx | Gy << 8 of ref and src as the
    workspace holds them."""
    assert mutant is None or mutant in MUTANTS, mutant
    T = rel_pose(ref_w2c, src_w2c, mutant)
    step, w = hypotheses(w_min, w_max, D, mutant)
    pc = pixel_costs(np.asarray(ref, np.uint8), np.asarray(src, np.uint8), cam, T, w, outside_cost, mutant)
    C = box(pc, r)
    S = path_costs(C, D, P1, P2, paths)
    idx16 = winner(S, cam, T, w, uniqueness, mutant)
    grad = np.stack([gx | (gy << 8) for gx, gy in (gradients(np.asarray(im, np.uint8), mutant) for im in (ref, src))])
    return dict(T=T, step=step, w=w, grad=grad, pc=pc, C=C, S=S, idx16=idx16, depth=depth(idx16, w_min, step, mutant))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def ref_pose():
    return gn.se3_exp(REF_TWIST)


def case(W, H, motion, scale=1.0, ref_w2c=None):
    """The analytic scene seen from the reference pose (ref_w2c: another one) and from Exp(scale twist) on it -> dict(cam, ref, src uint8
    [H,W], ref_w2c, src_w2c float32 [4,4], truth float32 [H,W] the reference view's ray-cast depth)."""
    cam = ar.camera(W, H)
    twist = np.asarray(MOTIONS[motion] if isinstance(motion, str) else motion, np.float64)
    rw = ref_pose() if ref_w2c is None else np.asarray(ref_w2c, np.float64)
    sw = gn.se3_exp(scale * twist) @ rw
    rc, rd = ar.scene_frame(rw, cam)
    sc, _ = ar.scene_frame(sw, cam)
    return dict(cam=cam, ref=grey_u8(rc), src=grey_u8(sc), ref_w2c=rw.astype(F), src_w2c=sw.astype(F), truth=rd)


def run(c, w_min, w_max, mutant=None, **kw):
    return sweep(c["ref"], c["src"], c["cam"], c["ref_w2c"], c["src_w2c"], w_min, w_max, mutant=mutant, **dict(DEFAULTS, **kw))


def quality(out, truth):
    """-> (share of valid pixels, share of the valid ones within 10 % of the truth, their median relative error)."""
    z, t = np.asarray(out["depth"], np.float64), np.asarray(truth, np.float64)
    valid = np.asarray(out["idx16"]) >= 0
    rel = np.abs(z[valid] - t[valid]) / t[valid]
    return float(valid.mean()), float((rel < 0.10).mean()), float(np.median(rel))


# ---- planted sums for the winner: every rule of h that a scene need not exercise ---------------------------------------------------------
def planted_sums(D, W=24, H=6, seed=3, u=40):
    """S int64 [H,W,D], random between 50 000 and 200 000 with planted rows:
      row 0  exact ties of the minimum (at d and d + 3; at d and d + 1), so the lowest d must win
      row 1  d* = 0 and d* = D - 1 alternating, unique by a wide margin: idx16 = 0 and 16 (D - 1), no parabola step
      row 2  S(d* - 1) < S(d* + 1) by amounts that make the numerator negative and not a multiple of 2 den
      row 3  runner-ups exactly at the uniqueness bound S(d) (100 - u) == 100 S(d*) for u = 40 (S(d*) = 60 k, S(d) = 100 k): still unique
      row 4  the same, one below the bound: S(d) = 100 k - 1, a rival
    Under planted_cam the last column and the last row (row 5, nothing planted) fall to the centre rule."""
    rng = np.random.default_rng(seed)
    S = rng.integers(50_000, 200_000, (H, W, D)).astype(np.int64)
    for x in range(W):
        d = 1 + (x * 5) % (D - 6)
        S[0, x, d] = S[0, x, d + (3 if x % 2 else 1)] = 1000 + x
        S[1, x, 0 if x % 2 == 0 else D - 1] = 500
        d = 2 + (x * 3) % (D - 4)
        S[2, x, d - 1], S[2, x, d], S[2, x, d + 1] = 2010 + x, 2000, 2040 + x + 13 * (x % 5)
        S[3, x, d], S[3, x, d + 2] = 60 * (10 + x), 100 * (10 + x)
        S[4, x, d], S[4, x, d + 2] = 60 * (10 + x), 100 * (10 + x) - 1
    return S


def planted_cam(W=24, H=6):
    """A camera and poses (rotation-free, a sideways step of a fifth of a pixel at most) under which the centre warp of every pixel but
    those of the last column and the last row is inside at every hypothesis, so that the planted rows meet the winner's rules alone and
    the border meets the centre rule: -> (cam, ref_w2c, src_w2c, w_min, w_max)."""
    cam = dict(W=W, H=H, fx=20.0, fy=20.0, cx=W / 2.0, cy=H / 2.0)
    rw, sw = np.eye(4, dtype=F), np.eye(4, dtype=F)
    sw[0, 3] = 0.01
    return cam, rw, sw, 0.1, 1.0
