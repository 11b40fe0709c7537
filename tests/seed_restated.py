"""NumPy restatement of the keyframe seeding path (csrc/seed.hip), written from the reference's Python and from what
include/gsaj.h states, independently of the kernels: get_median_depth (utils/slam_utils.py:131-142), the monocular depth prior of
add_new_keyframe (utils/slam_frontend.py:89-103), the seeded down-sample, the back-projection of
create_pcd_from_image_and_depth (gaussian_splatting/scene/gaussian_model.py:209-279; Open3D's arithmetic in fp64) and the
parameter initialisation.  Every tensor operation of the reference that runs in fp32 is one fp32 NumPy operation here."""
import numpy as np

F = np.float32
C0 = 0.28209479177387814  # gaussian_splatting/utils/sh_utils.py


def rgb_valid(gt_image, thr):
    gt = np.asarray(gt_image, F)
    return ((gt[0] + gt[1]) + gt[2]) > F(thr)  # torch sums a dimension of three in order, in fp32


def valid_mask(depth, opacity=None, mask=None, opacity_min=0.95):
    depth = np.asarray(depth, F)
    valid = depth > 0
    if opacity is not None:
        valid = valid & (np.asarray(opacity, F).reshape(depth.shape) > F(opacity_min))
    if mask is not None:
        valid = valid & np.asarray(mask, bool).reshape(depth.shape)
    return valid


def median_depth(depth, opacity=None, mask=None):
    """-> (median fp32, std fp64 (unbiased; round to fp32 to compare), valid mask, n_valid).  torch.median is the LOWER median:
    order statistic (n - 1) // 2.  No valid pixel: (0, 0, mask, 0), the device's documented answer where the reference raises."""
    depth = np.asarray(depth, F)
    valid = valid_mask(depth, opacity, mask)
    v = np.sort(depth[valid])
    n = v.size
    if n == 0:
        return F(0), 0.0, valid, 0
    med = v[(n - 1) // 2]
    v64 = v.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = float(np.sqrt(np.sum((v64 - v64.mean()) ** 2) / (n - 1))) if n > 1 else float("nan")
    return med, std, valid, n


def keyframe_depth_prior(depth, opacity, gt_image, thr, noise=None):
    """-> (out fp32 [H,W], margin [H,W] = min(|depth - (med + std)|, |depth - (med - std)|) in fp64: how far each pixel's two
    comparisons are from flipping, med, std32)."""
    depth = np.asarray(depth, F)
    vrgb = rgb_valid(gt_image, thr).reshape(depth.shape)
    med, std, valid, n = median_depth(depth, opacity, vrgb)
    std32 = F(std)
    hi, lo = F(med + std32), F(med - std32)
    invalid = (depth > hi) | (depth < lo) | ~valid
    base = np.where(invalid, med, depth).astype(F)
    if noise is not None:
        sc = np.where(invalid, F(std32 * F(0.5)), F(std32 * F(0.2))).astype(F)
        base = (base + (np.asarray(noise, F).reshape(depth.shape) * sc).astype(F)).astype(F)
    out = np.where(vrgb, base, F(0)).astype(F)
    d64 = depth.astype(np.float64)
    margin = np.minimum(np.abs(d64 - (float(med) + std)), np.abs(d64 - (float(med) - std)))
    return out, margin, med, std32


def mix32(x):
    """The bijective 32-bit mix include/gsaj.h states, on uint64 arrays masked to 32 bits."""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def pixel_keys(n, seed):
    return mix32(np.arange(n, dtype=np.uint64) ^ mix32(np.array([seed], np.uint64))[0])


def seed_valid(depth, gt_image=None, thr=0.0, depth_trunc=100.0):
    depth = np.asarray(depth, F)
    valid = (depth > 0) & (depth < F(depth_trunc))
    if gt_image is not None:
        valid &= rgb_valid(gt_image, thr).reshape(depth.shape)
    return valid


def select(valid, factor, seed):
    """The m = int(n_valid * (1 / factor)) valid pixels with the smallest keys, as ascending flat indices; -> (indices, n_valid)."""
    flat = np.flatnonzero(np.asarray(valid).reshape(-1))
    m = int(flat.size * (1.0 / float(factor)))
    keys = pixel_keys(np.asarray(valid).size, seed)[flat]
    order = np.lexsort((flat, keys))  # by key; the index would break ties, and there are none
    return np.sort(flat[order[:m]]), flat.size


def quantised_colour(image, pix, exposure=(0.0, 0.0)):
    """-> (q uint8 [m,3], x [m,3] = the fp64 value of 255 * clamp(exp(a) * image + b, 0, 1) before the truncation)."""
    img = np.asarray(image, F).reshape(3, -1)[:, pix].T
    a, b = exposure
    x = 255.0 * np.clip(np.exp(np.float64(a)) * img.astype(np.float64) + np.float64(b), 0.0, 1.0)
    ab = (np.exp(F(a)) * img).astype(F) + F(b)
    q = (np.clip(ab, F(0), F(1)) * F(255)).astype(F).astype(np.uint8)
    return q, x


def rgb2sh(q):
    rgb = (q.astype(np.float64) / 255.0).astype(F)
    return ((rgb - F(0.5)) / F(C0)).astype(F)


def backproject(depth, pix, W, w2c, fx, fy, cx, cy):
    """World points in fp64 from the fp32 depth and the fp32 W2C: inverse(W2C) (x, y, z, 1)."""
    d = np.asarray(depth, F).reshape(-1)[pix].astype(np.float64)
    u, v = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    pc = np.stack([(u - cx) * d / fx, (v - cy) * d / fy, d, np.ones_like(d)], axis=1)
    return (pc @ np.linalg.inv(np.asarray(w2c, F).astype(np.float64).reshape(4, 4)).T)[:, :3]


def adaptive_point_size(point_size, depth):
    """min(0.05, point_size * np.median(depth image)): NumPy's median of ALL pixels in the image's fp32; the product of a Python
    float and a NumPy scalar in double; rounded when it multiplies the fp32 tensor."""
    d = np.sort(np.asarray(depth, F).reshape(-1))
    n = d.size
    med = F(F(d[(n - 1) // 2] + d[n // 2]) * F(0.5))
    return F(min(0.05, float(point_size) * float(med)))


def scales(dist2, point_size):
    with np.errstate(over="ignore"):
        return np.log(np.sqrt((np.maximum(np.asarray(dist2, F), F(1e-7)) * F(point_size)).astype(F)).astype(F)).astype(F)
