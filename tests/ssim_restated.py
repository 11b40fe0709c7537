"""NumPy restatement of the reference SSIM (gaussian_splatting/utils/loss_utils.py:42-101) and of the colour-refinement loss
(utils/slam_backend.py:320-352) with their gradients w.r.t. the first image, for sizes no fixture can hold.

Forward: mu = blur(x), sigma^2 = blur(x*x) - mu^2, sigma12 = blur(x*y) - mu1 mu2, S = (2 mu1 mu2 + C1)(2 sigma12 + C2) /
((mu1^2 + mu2^2 + C1)(sigma1^2 + sigma2^2 + C2)), blur = 11x11 Gaussian window (sigma 1.5, the reference's float32 weights) with
zero padding 5.  Backward: the adjoint of each blur, written out (no autograd).  `dtype` selects the arithmetic (float64 = the
oracle; float32 estimates what fp32 rounding does).  `pad` ("zero" | "edge") and `shift` (window offset in pixels) exist only to
build deliberately WRONG variants for the negative canaries of tests/test_gpu_ssim.py.
"""
from math import exp

import numpy as np

C1 = 0.01 ** 2
C2 = 0.03 ** 2
R = 5
_PAD = R + 1  # room for shift = +-1


def window_1d():
    """gaussian(11, 1.5) as the reference builds it: exp() in double, stored as float32, normalised in float32."""
    g = np.array([exp(-((x - R) ** 2) / float(2 * 1.5 ** 2)) for x in range(2 * R + 1)], dtype=np.float32)
    return (g / g.sum(dtype=np.float32)).astype(np.float32)


def _pad(x, pad):
    return np.pad(x, ((0, 0), (0, 0), (_PAD, _PAD), (_PAD, _PAD)), mode="constant" if pad == "zero" else "edge")


def _unpad_adjoint(xp, pad, H, W):
    """Adjoint of _pad: crop (zero padding) or crop and fold the padding onto the edge rows / columns (edge padding)."""
    x = xp[:, :, _PAD:_PAD + H, :].copy()
    if pad == "edge":
        x[:, :, 0, :] += xp[:, :, :_PAD, :].sum(axis=2)
        x[:, :, -1, :] += xp[:, :, _PAD + H:, :].sum(axis=2)
    y = x[:, :, :, _PAD:_PAD + W].copy()
    if pad == "edge":
        y[:, :, :, 0] += x[:, :, :, :_PAD].sum(axis=3)
        y[:, :, :, -1] += x[:, :, :, _PAD + W:].sum(axis=3)
    return y


def blur(x, pad="zero", shift=0, dtype=np.float64):
    """[N,C,H,W] -> [N,C,H,W]: out[i,j] = sum_ab g[a] g[b] xpad[i + a - 5 + shift, j + b - 5 + shift] (horizontal, then vertical)."""
    g = window_1d().astype(dtype)
    N, C, H, W = x.shape
    xp = _pad(x.astype(dtype), pad)
    o = _PAD - R + shift
    h = np.zeros((N, C, H + 2 * _PAD, W), dtype)
    for b in range(2 * R + 1):
        h += g[b] * xp[:, :, :, o + b:o + b + W]
    out = np.zeros((N, C, H, W), dtype)
    for a in range(2 * R + 1):
        out += g[a] * h[:, :, o + a:o + a + H, :]
    return out


def blur_adjoint(y, pad="zero", shift=0, dtype=np.float64):
    """The adjoint of blur(): <blur(x), y> = <x, blur_adjoint(y)>."""
    g = window_1d().astype(dtype)
    N, C, H, W = y.shape
    o = _PAD - R + shift
    h = np.zeros((N, C, H + 2 * _PAD, W), dtype)
    for a in range(2 * R + 1):
        h[:, :, o + a:o + a + H, :] += g[a] * y
    xp = np.zeros((N, C, H + 2 * _PAD, W + 2 * _PAD), dtype)
    for b in range(2 * R + 1):
        xp[:, :, :, o + b:o + b + W] += g[b] * h
    return _unpad_adjoint(xp, pad, H, W)


def ssim_forward(img1, img2, pad="zero", shift=0, dtype=np.float64):
    """Returns (ssim_map, partials) with partials = (dS/dmu1, dS/dE[x^2], dS/dE[xy]) per pixel."""
    x, y = img1.astype(dtype), img2.astype(dtype)
    m1, m2 = blur(x, pad, shift, dtype), blur(y, pad, shift, dtype)
    exx, eyy, exy = blur(x * x, pad, shift, dtype), blur(y * y, pad, shift, dtype), blur(x * y, pad, shift, dtype)
    c1, c2 = dtype(C1), dtype(C2)
    A = 2 * m1 * m2 + c1
    B = 2 * (exy - m1 * m2) + c2
    Cc = m1 * m1 + m2 * m2 + c1
    D = (exx - m1 * m1) + (eyy - m2 * m2) + c2
    S = A * B / (Cc * D)
    dmu = 2 * m2 * (B - A) / (Cc * D) + 2 * m1 * S * (1 / D - 1 / Cc)
    return S, (dmu, -S / D, 2 * A / (Cc * D))


def ssim_backward(img1, img2, partials, dL_dS, pad="zero", shift=0, dtype=np.float64):
    """dL/dimg1 given the per-pixel upstream gradient dL_dS (broadcastable to [N,C,H,W])."""
    x, y = img1.astype(dtype), img2.astype(dtype)
    dmu, dxx, dxy = partials
    return (blur_adjoint(dL_dS * dmu, pad, shift, dtype) + 2 * x * blur_adjoint(dL_dS * dxx, pad, shift, dtype) +
            y * blur_adjoint(dL_dS * dxy, pad, shift, dtype))


def ssim(img1, img2, dtype=np.float64):
    """(mean SSIM, per-image means [N], ssim_map, dSSIM_mean/dimg1) for [N,C,H,W] input."""
    S, parts = ssim_forward(img1, img2, dtype=dtype)
    g = ssim_backward(img1, img2, parts, dtype(1.0 / S.size), dtype=dtype)
    return S.mean(), S.reshape(S.shape[0], -1).mean(axis=1), S, g


def refine_loss(image, gt, lambda_dssim=0.2, pad="zero", shift=0, l1_sign=True, dtype=np.float64):
    """(loss, L1, SSIM, dL/dimage) of colour refinement: (1 - lambda) mean|x - y| + lambda (1 - mean S), [3,H,W] or [N,C,H,W]."""
    x, y = image.astype(dtype), gt.astype(dtype)
    if x.ndim == 3:
        x, y = x[None], y[None]
    S, parts = ssim_forward(x, y, pad, shift, dtype)
    n = x.size
    l1 = np.abs(x - y).mean()
    s = S.mean()
    g = ssim_backward(x, y, parts, dtype(-lambda_dssim / n), pad, shift, dtype)
    if l1_sign:
        g = g + dtype((1 - lambda_dssim) / n) * np.sign(x - y)
    return (1 - lambda_dssim) * l1 + lambda_dssim * (1 - s), l1, s, g.reshape(image.shape)
