"""NumPy restatement of the tracking gradient mask (csrc/frame.hip), written from the reference's Python
(utils/slam_utils.py:4-38 image_gradient / image_gradient_mask, utils/camera_utils.py:115-144 Camera.compute_grad_mask) and from
what include/gsaj.h states, independently of the kernels.  Every fp32 tensor operation of the reference is one fp32 NumPy
operation here; the one place where the reference's order of operations is not visible from its Python -- the nine-tap sum inside
conv2d -- is summed in the order include/gsaj.h states (row or column of three left to right, first minus last), which is within
a few units in the last place of any other order (tests/test_cpu_grad_mask.py bounds it against the recorded outputs).

The keyword arguments of `grad_mask` named mutant_* are WRONG on purpose: tests/test_cpu_grad_mask.py uses them to show that its
comparator rejects each of them."""
import math

import numpy as np

F = np.float32
EPS_VALID = F(0.01)
GRID = 32  # blocks per image side in block mode


def gray_image(image):
    """image.mean(dim=0): torch sums a dimension of three in order and divides by 3, in fp32."""
    im = np.asarray(image, F)
    return ((im[0] + im[1]) + im[2]) / F(3)


def intensity(image, pad_mode="reflect", norm=1.0 / 32.0):
    """-> (I [H,W] fp32, gv, gh, valid [H,W] bool, gray [H,W])."""
    g = gray_image(image)
    H, W = g.shape
    p = np.pad(g, 1, mode=pad_mode) if pad_mode != "zero" else np.pad(g, 1, mode="constant")
    t = [[p[i:i + H, j:j + W] for j in range(3)] for i in range(3)]
    n = F(norm)
    top = (F(3) * t[0][0] + F(10) * t[0][1]) + F(3) * t[0][2]
    bot = (F(3) * t[2][0] + F(10) * t[2][1]) + F(3) * t[2][2]
    left = (F(3) * t[0][0] + F(10) * t[1][0]) + F(3) * t[2][0]
    right = (F(3) * t[0][2] + F(10) * t[1][2]) + F(3) * t[2][2]
    gv = (top - bot) * n
    gh = (left - right) * n
    valid = np.ones((H, W), bool)
    for i in range(3):
        for j in range(3):
            valid &= np.abs(t[i][j]) > EPS_VALID
    gv = np.where(valid, gv, F(0)).astype(F)
    gh = np.where(valid, gh, F(0)).astype(F)
    I = np.sqrt(gv * gv + gh * gh).astype(F)
    return I, gv, gh, valid, g


def lower_median(v, upper=False):
    s = np.sort(np.asarray(v, F).reshape(-1))
    return s[s.size // 2] if upper else s[(s.size - 1) // 2]  # torch.median: order statistic (n - 1) // 2


def block_shape(H, W, ceil=False):
    return (math.ceil(H / GRID), math.ceil(W / GRID)) if ceil else (int(H / GRID), int(W / GRID))


def grad_mask(image, edge_threshold, blocks=False, mutant_pad_zero=False, mutant_strip_norm16=False, mutant_upper_median=False,
              mutant_ge=False, mutant_no_quirk_a=False, mutant_strip_zero=False, mutant_ceil_blocks=False):
    """-> dict: `value` what the reference leaves in Camera.grad_mask ([H,W]: bool in global mode, fp32 in block mode), `u8` the
    byte mask (value truncated), `I` the intensities, `t` [H,W] fp32 the threshold each pixel was compared with (NaN on the
    leftover strips of block mode, which are compared with nothing), `visited` [H,W] bool, `max_gray`."""
    I, _, _, _, g = intensity(image, "zero" if mutant_pad_zero else "reflect")
    H, W = I.shape
    thr = F(edge_threshold)  # a Python float meeting an fp32 tensor is rounded to fp32
    gt = (lambda a, b: a >= b) if mutant_ge else (lambda a, b: a > b)
    out = dict(I=I, max_gray=float(np.abs(g).max()))
    if not blocks:
        t = F(lower_median(I, mutant_upper_median) * thr)
        value = gt(I, t)
        out.update(value=value, u8=value.astype(np.uint8), t=np.full((H, W), t, F), visited=np.ones((H, W), bool))
        return out
    bh, bw = block_shape(H, W, mutant_ceil_blocks)
    if bh < 1 or bw < 1:
        raise ValueError("block mode needs H >= 32 and W >= 32")
    value = I.copy()
    if mutant_strip_norm16:
        value = intensity(image, norm=1.0 / 16.0)[0]
    if mutant_strip_zero:
        value[:] = 0
    tmap = np.full((H, W), np.nan, F)
    visited = np.zeros((H, W), bool)
    for r in range(GRID):
        for c in range(GRID):
            sl = (slice(r * bh, min((r + 1) * bh, H)), slice(c * bw, min((c + 1) * bw, W)))
            blk = I[sl]
            if blk.size == 0:
                continue
            t = F(lower_median(blk, mutant_upper_median) * thr)
            keep = gt(blk, t)
            if not mutant_no_quirk_a:
                keep = keep & (t < F(1))  # the ones are written first and then zeroed with everything <= t
            value[sl] = keep.astype(F)
            tmap[sl] = t
            visited[sl] = True
    out.update(value=value, u8=value.astype(np.uint8), t=tmap, visited=visited)  # (astype: truncation; values are in [0, 1])
    return out


# ---- the scenes of the tests and of tests/golden/make_grad_mask_goldens.py ---------------------------------------------------
def make_scene(kind, H, W, seed=0):
    """[3,H,W] fp32 in [0, 1].  "noise": a smooth sinusoid + uniform noise of +-0.15, a flat patch (0.25) and a black patch
    (validity, zero intensities, blocks whose median is 0).  "checker": a high-contrast checkerboard of 2x2 cells with a little
    noise: block medians above 0.25, so that edge_threshold 4 gives t >= 1 (quirk A zeroes the block; no intensity of an image
    in [0, 1] exceeds 0.71, so there the plain comparison gives the same).  "bright": that checkerboard times 4, an image that was
    not normalised to [0, 1]: intensities above t >= 1, which only quirk A zeroes, and leftover-strip bytes of 1.  "dyadic":
    r = g = b on a 1/256 grid."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "noise":
        img = np.stack([0.5 + 0.3 * np.sin(0.11 * x + 0.07 * y + c) * np.cos(0.05 * y - 0.02 * x * c) for c in range(3)])
        img = img + rng.uniform(-0.15, 0.15, img.shape)
        img[:, H // 8:H // 8 + H // 4, W // 2:W // 2 + W // 3] = 0.25
        img[:, H // 2:H // 2 + H // 3, W // 10:W // 10 + W // 3] = 0.0
    elif kind in ("checker", "bright"):
        cell = ((x // 2 + y // 2) % 2)[None]
        img = 0.04 + 0.92 * cell + rng.uniform(-0.02, 0.02, (3, H, W))
        if kind == "bright":
            return (4.0 * img).astype(F)
    elif kind == "dyadic":
        v = rng.integers(0, 257, (H, W)) / 256.0
        v[H // 3:H // 3 + 9, W // 4:W // 4 + 13] = 0.0
        img = np.stack([v, v, v])
    else:
        raise ValueError(kind)
    return np.clip(img, 0.0, 1.0).astype(F)


def tolerance(edge_threshold, max_gray):
    """How far |I - t| may be for a mask pixel to differ, and (with edge_threshold = 0) how far intensities may be apart: the
    roundings of the stencil (nine products and eight sums of terms up to 16 max|gray|, each within 2^-24 relative), of the
    squares, their sum and the root, and the same bound on the median times the threshold."""
    return (1.0 + float(edge_threshold)) * 16.0 * 2.0 ** -24 * float(max_gray)
