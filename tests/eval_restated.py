"""NumPy restatement of the per-frame statement of the reference's eval_rendering (utils/eval_utils.py:141-155) as include/gsaj.h
words it for gsaj_eval_frame: the elementwise steps in fp32, one rounding each; the sum and the scalar tail in fp64.

    x = clamp(image, 0, 1); m = gt > 0 per element; d = x - gt; q = d * d; n = sum m; sse = sum_m q
    mse = sse / n; psnr = 20 log10(1 / sqrt(mse)); ssim = SSIM(x, gt), unmasked; byte (h, w, c) = trunc(x[c', h, w] * 255)

`mutate=` plants one wrong reading of that statement (the canaries of tests/test_cpu_eval.py):
    mask_ge          m = gt >= 0
    mask_pixel       m per pixel: any channel of gt > 0
    no_clamp         x = image
    mean_all         mse = sse / (C H W)
    ssim_unclamped   SSIM(image, gt)
    round_bytes      bytes rounded to nearest instead of truncated
    no_reverse       the channel reversal that was asked for is not done
"""
import numpy as np

import ssim_restated as sr

MUTANTS = ("mask_ge", "mask_pixel", "no_clamp", "mean_all", "ssim_unclamped", "round_bytes", "no_reverse")
U = 2.0 ** -24


def clamp01(v):
    """torch.clamp(v, 0, 1) on fp32: a NaN stays a NaN."""
    v = np.asarray(v, np.float32)
    return np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v)).astype(np.float32)


def evaluate(image, gt, reverse=False, mutate=None, with_ssim=True):
    """image, gt [C,H,W] float32 -> dict: x (fp32), n, sse, mse, psnr, frac (fp64 or Python ints), ssim, ssim_map, ssim_partials
    (fp64, when with_ssim), u8 [H,W,C]."""
    assert mutate is None or mutate in MUTANTS, mutate
    image, gt = np.asarray(image, np.float32), np.asarray(gt, np.float32)
    C = image.shape[0]
    x = image if mutate == "no_clamp" else clamp01(image)
    if mutate == "mask_ge":
        m = gt >= 0
    elif mutate == "mask_pixel":
        m = np.broadcast_to((gt > 0).any(axis=0, keepdims=True), gt.shape)
    else:
        m = gt > 0
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - gt).astype(np.float32)
        q = (d * d).astype(np.float32)
    n = int(m.sum())
    sse = float(q[m].astype(np.float64).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mse = np.float64(sse) / np.float64(image.size if mutate == "mean_all" else n)
        psnr = 20.0 * np.log10(1.0 / np.sqrt(mse))
        s = (x * np.float32(255.0)).astype(np.float32)
    s = np.where(np.isnan(s), np.float32(0), s)
    u8 = (np.rint(s) if mutate == "round_bytes" else np.trunc(s)).astype(np.uint8).transpose(1, 2, 0)
    if reverse and mutate != "no_reverse":
        u8 = u8[:, :, ::-1]
    out = dict(x=x, n=n, sse=sse, mse=float(mse), psnr=float(psnr), frac=n / float(image.size), u8=np.ascontiguousarray(u8), C=C)
    if with_ssim:
        a = image if mutate == "ssim_unclamped" else x
        S, parts = sr.ssim_forward(a[None].astype(np.float64), gt[None].astype(np.float64))
        out.update(ssim=float(S.mean()), ssim_map=S, ssim_partials=parts)
    return out


def same_special(a, b):
    """inf and NaN must match as such: True when a and b are the same non-finite value, False when only one is non-finite or they
    are different ones, None when both are finite."""
    a, b = float(a), float(b)
    if np.isfinite(a) and np.isfinite(b):
        return None
    return bool((np.isnan(a) and np.isnan(b)) or a == b)


def psnr_bound_reference(n, psnr):
    """|restatement - the reference's own psnr|: the reference sums n fp32 squares pairwise in fp32 (relative error of the mean about
    (log2 n + 4) u, carried through 20 log10(1 / sqrt(.)) = -(10 / ln 10) ln(.)) and rounds its scalar tail in fp32 (4 u relative)."""
    return (10.0 / np.log(10.0)) * (np.log2(max(n, 1)) + 4.0) * U + 4.0 * U * max(1.0, abs(psnr))


def psnr_bound_device(psnr):
    """|device - restatement|: mse one rounding, the square root and the division one each, log10f <= 2 ulp of its result, the final
    product one rounding, carried through 20 log10."""
    return 32.0 * U + 8.0 * U * abs(psnr)
