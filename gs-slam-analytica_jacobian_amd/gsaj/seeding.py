"""New Gaussians from a keyframe, on the device (C ABI gsaj_depth_stats / gsaj_keyframe_depth_prior / gsaj_seed_select /
gsaj_seed_gaussians, csrc/seed.hip).

What the reference does through the host between a tracked frame and the next mapping step: get_median_depth
(utils/slam_utils.py:131-142, once per frame), the depth a new keyframe is seeded from (utils/slam_frontend.py:57-108) and
create_pcd_from_image_and_depth (gaussian_splatting/scene/gaussian_model.py:209-279: Open3D point cloud, random down-sample,
RGB2SH, distCUDA2 scales).  Inputs are fp32 device tensors; there is no CPU path.  The only host synchronisation is the read of
the number of new Gaussians in `seed_from_keyframe`, which sizes the returned tensors.

The down-sample is a uniform m-subset of the valid pixels, reproducible from `seed` (include/gsaj.h states the key function); it
is not Open3D's subset, whose shuffle is unseeded, and the new Gaussians come in pixel order.
"""
import ctypes

import torch

from . import _lib

_WS = {}  # (device, H, W) -> workspace (carries state from the selection to the initialisation, so one per image shape)


def _image(name, t, dims, dtype=torch.float32):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise _lib.GsajError("%s must be a HIP device tensor (there is no CPU path)" % name)
    if t.dtype != dtype:
        raise _lib.GsajError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if t.dim() == dims + 1 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != dims:
        raise _lib.GsajError("%s must have %d dimensions (got %s)" % (name, dims, tuple(t.shape)))
    return t.detach().contiguous()


def _plane(name, t, H=None, W=None, dtype=torch.float32):
    t = _image(name, t, 2, dtype)
    if H is not None and tuple(t.shape) != (H, W):
        raise _lib.GsajError("%s must be [%d,%d] (got %s)" % (name, H, W, tuple(t.shape)))
    return t


def _rgb(name, t, H, W):
    t = _image(name, t, 3)
    if tuple(t.shape) != (3, H, W):
        raise _lib.GsajError("%s must be [3,%d,%d] (got %s)" % (name, H, W, tuple(t.shape)))
    return t


def _mask(name, t, H, W):
    if torch.is_tensor(t) and t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
    return _plane(name, t, H, W, torch.uint8)


def _workspace(lib, dev, H, W):
    key = (str(dev), H, W)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(lib.gsaj_seed_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
    return ws


def _ptr(t):
    return None if t is None else t.data_ptr()


def depth_stats(depth, opacity=None, mask=None, gt_image=None, rgb_boundary_threshold=0.0, opacity_min=0.95, return_valid=False):
    """stats = device tensor [4]: median, std, n_valid, 0 (no host synchronisation) and, with return_valid, the valid mask
    [H,W] bool.  valid = depth > 0 [and opacity > opacity_min] [and mask] [and gt_image.sum(0) > rgb_boundary_threshold]."""
    lib = _lib.load()
    d = _plane("depth", depth)
    H, W = d.shape
    dev = d.device
    o = None if opacity is None else _plane("opacity", opacity, H, W)
    mk = None if mask is None else _mask("mask", mask, H, W)
    gt = None if gt_image is None else _rgb("gt_image", gt_image, H, W)
    stats = torch.empty(4, dtype=torch.float32, device=dev)
    valid = torch.empty((H, W), dtype=torch.uint8, device=dev) if return_valid else None
    with torch.cuda.device(dev):
        _lib.check(lib.gsaj_depth_stats(W, H, d.data_ptr(), _ptr(o), float(opacity_min), _ptr(mk), _ptr(gt), float(rgb_boundary_threshold),
                                        stats.data_ptr(), _ptr(valid), _workspace(lib, dev, H, W).data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), "gsaj_depth_stats")
    return (stats, valid.view(torch.bool)) if return_valid else stats


def median_depth(depth, opacity=None, mask=None, return_std=False):
    """get_median_depth (utils/slam_utils.py:131-142) on the device: the lower median of the valid depths as a 0-d device tensor;
    with return_std also the unbiased standard deviation and the valid mask (shaped like `depth`).  No valid pixel: the reference
    raises, this returns 0 (and std 0)."""
    if return_std:
        stats, valid = depth_stats(depth, opacity, mask, return_valid=True)
        return stats[0], stats[1], valid.view(depth.shape)
    return depth_stats(depth, opacity, mask)[0]


def keyframe_depth_prior(depth, opacity, gt_image, rgb_boundary_threshold, noise=None, return_stats=False):
    """The depth a monocular keyframe is seeded from (utils/slam_frontend.py:89-103): rendered depth where it is within one standard
    deviation of the median and valid, the median elsewhere, plus noise * (0.2 | 0.5) std; 0 where the colour mask fails.  `noise` is
    the caller's torch.randn_like(depth) (None: no noise).  Returns [H,W] (and the stats tensor [median, std, n_valid, 0])."""
    lib = _lib.load()
    d = _plane("depth", depth)
    H, W = d.shape
    dev = d.device
    o, gt = _plane("opacity", opacity, H, W), _rgb("gt_image", gt_image, H, W)
    z = None if noise is None else _plane("noise", noise, H, W)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gsaj_keyframe_depth_prior(W, H, d.data_ptr(), o.data_ptr(), gt.data_ptr(), float(rgb_boundary_threshold), _ptr(z),
                                                 out.data_ptr(), stats.data_ptr(), _workspace(lib, dev, H, W).data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "gsaj_keyframe_depth_prior")
    return (out, stats) if return_stats else out


def seed_from_keyframe(image, depth, w2c, fx, fy, cx, cy, downsample_factor, point_size, sh_degree=0, adaptive_pointsize=False,
                       isotropic=False, exposure_ab=None, gt_image=None, rgb_boundary_threshold=0.0, depth_trunc=100.0, seed=0,
                       return_pixels=False):
    """create_pcd_from_image_and_depth (gaussian_model.py:209-279) in the reference's return layout:
    (xyz [m,3], features [m,3,(sh_degree+1)^2], scales [m,1|3], rots [m,4], opacities [m,1]).

    image [3,H,W] (the keyframe's colour; exposure_ab = device tensor {a, b} applies exp(a) * image + b first), depth [H,W], w2c = 16
    device floats, row-major W2C (a [4,4] tensor, or a DeviceTracker pose_state, whose first 16 floats are that; exposure_ab may be
    the pose tracker's `exposure` view of it).  A pixel seeds a Gaussian if 0 < depth < depth_trunc (and, with gt_image, its colour sum exceeds the
    threshold) and it is among the m = int(n_valid / downsample_factor) pixels the seed picks."""
    lib = _lib.load()
    d = _plane("depth", depth)
    H, W = d.shape
    dev = d.device
    img = _rgb("image", image, H, W)
    gt = None if gt_image is None else _rgb("gt_image", gt_image, H, W)
    for name, t, n in (("w2c", w2c, 16), ("exposure_ab", exposure_ab, 2)):
        if t is None and n == 2:
            continue
        if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise _lib.GsajError("%s must be a contiguous float32 tensor of at least %d elements on %s" % (name, n, dev))
    M = (int(sh_degree) + 1) ** 2
    ws = _workspace(lib, dev, H, W)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsaj_seed_select(W, H, d.data_ptr(), _ptr(gt), float(rgb_boundary_threshold), float(depth_trunc),
                                        float(downsample_factor), int(seed) & 0xFFFFFFFF, ws.data_ptr(), st), "gsaj_seed_select")
        nv, m = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.gsaj_seed_count(ws.data_ptr(), st, ctypes.byref(nv), ctypes.byref(m)), "gsaj_seed_count")
        m = m.value
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        xyz, f_dc, f_rest = new(m, 3), new(m, 1, 3), new(m, M - 1, 3)
        scales, rots, opac = new(m, 1 if isotropic else 3), new(m, 4), new(m, 1)
        if m > 0:
            knn_ws = torch.empty(lib.gsaj_dist2_workspace_bytes(m), dtype=torch.uint8, device=dev)
            _lib.check(lib.gsaj_seed_gaussians(m, W, H, d.data_ptr(), img.data_ptr(), _ptr(exposure_ab), w2c.data_ptr(), float(fx),
                                               float(fy), float(cx), float(cy), float(point_size), int(bool(adaptive_pointsize)), M,
                                               int(bool(isotropic)), xyz.data_ptr(), f_dc.data_ptr(), f_rest.data_ptr(),
                                               scales.data_ptr(), rots.data_ptr(), opac.data_ptr(), ws.data_ptr(), knn_ws.data_ptr(),
                                               st), "gsaj_seed_gaussians")
    features = torch.cat((f_dc, f_rest), dim=1).transpose(1, 2)
    out = (xyz, features, scales, rots, opac)
    if return_pixels:  # tests: the chosen pixel indices v * W + u, ascending (the workspace keeps them until the next selection)
        return out + (selected_pixels(dev, H, W, m),)
    return out


def selected_pixels(dev, H, W, m):
    """The pixel indices v * W + u of the last selection on this image shape ([m] int64, ascending); tests and debugging."""
    lib = _lib.load()
    out = torch.empty(m, dtype=torch.int32, device=dev)
    if m > 0:
        with torch.cuda.device(dev):
            _lib.check(lib.gsaj_debug_seed_pixels(W, H, m, _WS[(str(dev), H, W)].data_ptr(), out.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "gsaj_debug_seed_pixels")
    return out.to(torch.int64)
