"""NumPy restatement of the stereo matcher of include/gsaj.h ("stereo frames", csrc/stereo.hip) in int64, with a `mutant=` switch for
the canaries, the fp32 mirror of the byte remap (gsaj_rectify_u8, through tests/ingest_restated.py) and a generator of synthetic
pairs with a known disparity.  TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_stereo.py and tests/test_gpu_stereo.py.

  prefilter, cost_volume   1a-1c: the clipped horizontal Sobel, |P_L - P_R| summed over the clamped (2r+1)^2 window
  path_costs               1e: one L_rho per direction over the valid region x >= D, a row (or a column) at a time
  winner                   1f-1i: argmin, uniqueness, sub-pixel, disp2 and the left-right check -> disp16 int16 [H,W]
  depth                    the reference's float64 lines rounded to float32 once
  match                    all of it
  rectify_u8               the byte a remap with GSAJ_INGEST_ROUND_U8 lands on, before the division by 255
  scene                    "plane", "step", "slant": left = right warped by a known disparity
  edge_scene               pairs whose winners sit at d = 0 and d = D - 1 (the GPU tests compare S itself on them)
  planted_sums             an S for the winner alone with every rule's edge in it: ties, both ends, odd negative sub-pixel
                           numerators, two left pixels for one right column at equal cost, rivals exactly at the uniqueness bound

Nothing here is organised the way the kernels are: the kernels walk lines with one disparity per lane, this walks whole rows."""
import numpy as np

import ingest_restated as ir

F = np.float32
DIRS8 = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))   # (dx, dy); the first four are paths = 4
MUTANTS = ("p1_p2_swapped", "border_terms_wrap", "s_wraps_16", "tie_highest", "subpixel_floor", "uniq_le", "uniq_adjacent",
           "disp2_tie_smallest_x", "lr_either", "path_no_reset", "box_unclamped")
INVALID = -16


def prefilter(img):
    """uint8 [H,W] -> int64 [H,W] in 0..30: clamp(gx, -15, 15) + 15, coordinates clamped to the image."""
    I = np.pad(np.asarray(img, np.uint8).astype(np.int64), 1, mode="edge")
    H, W = img.shape
    gx = (I[0:H, 2:] - I[0:H, :-2]) + 2 * (I[1:H + 1, 2:] - I[1:H + 1, :-2]) + (I[2:, 2:] - I[2:, :-2])
    return np.clip(gx, -15, 15) + 15


def cost_volume(left, right, D, r, mutant=None):
    """-> C int64 [H,W,D]: the sum of pc over the window, every column computed (only x >= D is used)."""
    H, W = left.shape
    PL, PR = prefilter(left), prefilter(right)
    xs = np.arange(W)
    pc = np.empty((H, W, D), np.int64)
    for d in range(D):
        pc[:, :, d] = np.abs(PL - PR[:, np.maximum(xs - d, 0)])

    def taps(a, axis):   # the sum over |offset| <= r along one axis: the window is a product, so two such sums are the block sum
        n = a.shape[axis]
        out = np.zeros_like(a)
        for o in range(-r, r + 1):
            at = np.arange(n) + o
            t = np.take(a, np.clip(at, 0, n - 1), axis=axis)
            if mutant == "box_unclamped":   # a tap outside the image adds nothing
                shape = [1, 1, 1]
                shape[axis] = n
                t = t * ((at >= 0) & (at < n)).reshape(shape)
            out += t
        return out

    return taps(taps(pc, 1), 0)


def _step(q, c, P1, P2, wrap):
    """q, c int64 [..., D]: C + min(L(q,d), L(q,d-1) + P1, L(q,d+1) + P1, m + P2) - m."""
    m = q.min(axis=-1, keepdims=True)
    a = np.minimum(q, m + P2)
    if wrap:   # the mutant: the d-1 of 0 is D-1, the d+1 of D-1 is 0
        a = np.minimum(a, np.roll(q, 1, axis=-1) + P1)
        a = np.minimum(a, np.roll(q, -1, axis=-1) + P1)
    else:
        a[..., 1:] = np.minimum(a[..., 1:], q[..., :-1] + P1)
        a[..., :-1] = np.minimum(a[..., :-1], q[..., 1:] + P1)
    return c + a - m


def path_costs(C, D, P1, P2, paths, mutant=None):
    """-> S int64 [H,W,D], zero for x < D (for the mutant "path_no_reset" the paths start at the image's edge instead)."""
    assert paths in (4, 8)
    if mutant == "p1_p2_swapped":
        P1, P2 = P2, P1
    H, W, _ = C.shape
    x0 = 0 if mutant == "path_no_reset" else D
    wrap = mutant == "border_terms_wrap"
    S = np.zeros_like(C)
    for dx, dy in DIRS8[:paths]:
        L = np.zeros_like(C)
        if dy == 0:   # a column at a time, all rows at once
            order = range(x0, W) if dx > 0 else range(W - 1, x0 - 1, -1)
            for x in order:
                qx = x - dx
                L[:, x] = C[:, x] if (qx < x0 or qx >= W) else _step(L[:, qx], C[:, x], P1, P2, wrap)
        else:         # a row at a time, all columns of the valid region at once
            order = range(H) if dy > 0 else range(H - 1, -1, -1)
            xs = np.arange(x0, W)
            for y in order:
                qy = y - dy
                if qy < 0 or qy >= H:
                    L[y, x0:] = C[y, x0:]
                    continue
                qx = xs - dx
                inside = (qx >= x0) & (qx < W)
                stepped = _step(L[qy, np.clip(qx, x0, W - 1)], C[y, x0:], P1, P2, wrap)
                L[y, x0:] = np.where(inside[:, None], stepped, C[y, x0:])
        S += L
    if mutant == "path_no_reset":
        S[:, :D] = 0
    if mutant == "s_wraps_16":
        S &= 0xFFFF
    return S


def _trunc_div(num, den):
    q = abs(num) // den
    return q if num >= 0 else -q


def winner(S, D, uniqueness, lr_max_diff, mutant=None):
    """S int64 [H,W,D] -> disp16 int16 [H,W], -16 where invalid (every x < D is)."""
    S = np.asarray(S, np.int64)
    H, W, _ = S.shape
    ds = np.arange(D)
    best = S.min(axis=2)
    hit = S == best[:, :, None]
    dstar = (D - 1 - hit[:, :, ::-1].argmax(axis=2)) if mutant == "tie_highest" else hit.argmax(axis=2)
    far = np.abs(ds[None, None, :] - dstar[:, :, None]) > (0 if mutant == "uniq_adjacent" else 1)
    lhs, rhs = S * (100 - uniqueness), (best * 100)[:, :, None]
    unique = ~(((lhs <= rhs) if mutant == "uniq_le" else (lhs < rhs)) & far).any(axis=2)
    out = np.full((H, W), INVALID, np.int64)
    for y in range(H):
        disp2 = {}   # right column -> (S, -x, d*) of the left pixel that owns it
        for x in range(D, W):
            if not unique[y, x]:
                continue
            d, sd = int(dstar[y, x]), int(best[y, x])
            key = (sd, x if mutant == "disp2_tie_smallest_x" else -x, d)
            if x - d not in disp2 or key[:2] < disp2[x - d][:2]:
                disp2[x - d] = key
            if 0 < d < D - 1:
                sm, sp = int(S[y, x, d - 1]), int(S[y, x, d + 1])
                den = max(sm + sp - 2 * sd, 1)
                num = (sm - sp) * 16 + den
                out[y, x] = 16 * d + (num // (2 * den) if mutant == "subpixel_floor" else _trunc_div(num, 2 * den))
            else:
                out[y, x] = 16 * d
        if lr_max_diff < 0:
            continue
        row = [int(v) for v in out[y]]
        for x in range(D, W):
            v = row[x]
            if v < 0:
                continue
            fails = 0
            for delta in (v >> 4, (v + 15) >> 4):
                x2 = x - delta
                if x2 >= 0 and x2 in disp2 and abs(disp2[x2][2] - delta) > lr_max_diff:
                    fails += 1
            if fails == 2 or (mutant == "lr_either" and fails >= 1):
                out[y, x] = INVALID
    return out.astype(np.int16)


def depth(disp16, bf):
    """The reference's lines (utils/dataset.py:388-391) in float64, rounded to float32 once."""
    d = np.asarray(disp16, np.int16).astype(np.float64) / 16.0
    d[d == 0] = 1e10
    z = np.float64(bf) / d
    z[z < 0] = 0
    return z.astype(F)


def match(left, right, D=64, r=10, P1=2, P2=5, paths=8, uniqueness=40, lr_max_diff=1, mutant=None, want_S=False):
    S = path_costs(cost_volume(left, right, D, r, mutant), D, P1, P2, paths, mutant)
    out = winner(S, D, uniqueness, lr_max_diff, mutant)
    return (out, S) if want_S else out


def rectify_u8(src, map_xy):
    """uint8 [Hs,Ws] through float32 maps [H,W] -> uint8 [H,W]: gsaj_frame_ingest's bilinear with GSAJ_INGEST_ROUND_U8, stopped before
    the division by 255 (255 plane is exact for every byte: k / 255.0f * 255.0f rounds back to k)."""
    unit = ir.ingest_color(np.asarray(src, np.uint8), ir.ROUND_U8, map_xy)[0]
    byte = np.rint(unit.astype(np.float64) * 255.0)
    assert np.array_equal((byte.astype(F) / F(255.0)).astype(F), unit)   # the lattice k / 255 holds the byte itself
    return byte.astype(np.uint8)


# ---- synthetic pairs ------------------------------------------------------------------------------------------------------------------
KINDS = ("plane", "step", "slant")


def truth(W, H, kind):
    xs, _ = np.meshgrid(np.arange(W), np.arange(H))
    if kind == "plane":
        return np.full((H, W), 7.0)
    if kind == "step":   # a foreground block in front of a plane: its left edge occludes background
        d = np.full((H, W), 5.0)
        d[H // 4:3 * H // 4, W // 2 - 10:W // 2 + 25] = 12.0
        return d
    assert kind == "slant"
    return 4.0 + 0.06 * xs


def scene(W, H, kind, seed=1, d_true=None):
    """-> (left uint8 [H,W], right uint8 [H,W], disparity float64 [H,W]): a two-scale random texture seen by the right camera, the left
    image its bilinear warp by the disparity (left(x) = right(x - d))."""
    rng = np.random.default_rng(seed)
    margin = 32 + (0 if d_true is None else int(np.ceil(np.max(d_true))))
    Wt = W + 2 * margin
    coarse = np.kron(rng.random((H // 2 + 1, Wt // 2 + 1)), np.ones((2, 2)))[:H, :Wt]
    tex = 255.0 * (0.5 * coarse + 0.5 * rng.random((H, Wt)))
    d = truth(W, H, kind) if d_true is None else np.asarray(d_true, np.float64)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    sx = xs - d + margin
    x0 = np.floor(sx).astype(np.int64)
    f = sx - x0
    left = tex[ys, x0] * (1.0 - f) + tex[ys, x0 + 1] * f
    right = tex[:, margin:margin + W]
    return np.rint(left).astype(np.uint8), np.rint(right).astype(np.uint8), d


EDGE_KINDS = ("ends", "near_top")   # D = 16: disparities that reach d = 0 and d = D - 1, where the d +- 1 terms are absent


def edge_scene(W, H, kind, seed=2):
    """Pairs whose winners lie at both ends of the disparity range ("ends": a ramp from 0 to 15.4) or just under its top
    ("near_top": 14.6 everywhere).  The GPU tests compare S itself on these."""
    xs, _ = np.meshgrid(np.arange(W), np.arange(H))
    d = 15.4 * xs / (W - 1) if kind == "ends" else np.full((H, W), 14.6)
    assert kind in EDGE_KINDS
    return scene(W, H, None, seed=seed, d_true=d)


def quality(disp16, d_true, D):
    """-> (share of the columns x >= D that are valid, share of the valid ones within 1 disparity of the truth)."""
    o = np.asarray(disp16, np.int64)[:, D:]
    valid = o >= 0
    err = np.abs(o / 16.0 - d_true[:, D:])
    return float(valid.mean()), float((err[valid] <= 1.0).mean())


# ---- planted sums for the winner: every rule of 1f-1h that a random scene need not exercise -----------------------------------------
def planted_sums(D, W=None, H=6, seed=3):
    """S int64 [H,W,D] (W default D + 24), zero for x < D, random elsewhere, with planted rows:
      row 0  exact ties of the minimum (at d and d + 3; at d and d + 1), so the lowest d must win
      row 1  d* = 0 and d* = D - 1 alternating, unique by a wide margin: d16 = 0 (the 1e10 branch) and 16 (D - 1)
      row 2  S(d* - 1) < S(d* + 1) by amounts that make the sub-pixel numerator negative and not a multiple of 2 den
      row 3  pairs of left pixels x, x + 1 with d* = k, k + 1: the same right column, the same S(d*) -- the larger x owns it
      row 4  runner-ups exactly at the uniqueness bound S(d) (100 - u) == 100 S(d*) for u = 40 (S(d*) = 60 k, S(d) = 100 k)
    The other entries lie between 50 000 and 200 000, the planted minima well below."""
    W = D + 24 if W is None else W
    rng = np.random.default_rng(seed)
    S = rng.integers(50_000, 200_000, (H, W, D)).astype(np.int64)
    S[:, :D] = 0
    for x in range(D, W):
        i = x - D
        d = 1 + (i * 5) % (D - 6)
        S[0, x, d] = S[0, x, d + (3 if i % 2 else 1)] = 1000 + i
        S[1, x, 0 if i % 2 == 0 else D - 1] = 500
        d = 2 + (i * 3) % (D - 4)
        S[2, x, d - 1], S[2, x, d], S[2, x, d + 1] = 2010 + i, 2000, 2040 + i + 13 * (i % 5)
        k = 2 + ((i // 2) * 3) % (D - 4) + (i % 2)
        S[3, x, k] = 4000
        S[4, x, d], S[4, x, d + 2] = 60 * (10 + i), 100 * (10 + i)
    return S
