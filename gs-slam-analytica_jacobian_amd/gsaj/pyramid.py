"""The image pyramid of a frame on the device (C ABI gsaj_pyramid_build, csrc/pyramid.hip): levels 1..L of the colour, the depth and
the gradient mask in one launch, for coarse-to-fine tracking (gsaj.PyramidGaussNewtonTracker).  include/gsaj.h states the arithmetic:
a level-l pixel is the box filter of a whole 2^l x 2^l block of the frame -- an odd last column or row is dropped --, its depth the
mean of the valid depths unless they straddle a depth discontinuity, its mask the OR.  There is no CPU path and no host
synchronisation.
"""
import ctypes

import torch

from . import _lib

MAX_LEVELS = 4   # GSAJ_PYRAMID_MAX_LEVELS


def _build(pyr, color, depth, mask, depth_edge_ratio):  # (the device work: host-logic tests replace it)
    with torch.cuda.device(pyr.dev):
        _lib.check(pyr.lib.gsaj_pyramid_build(pyr.W, pyr.H, pyr.levels, color.data_ptr(), None if depth is None else depth.data_ptr(),
                                              None if mask is None else mask.data_ptr(), float(depth_edge_ratio), pyr.buf.data_ptr(),
                                              torch.cuda.current_stream(pyr.dev).cuda_stream), "gsaj_pyramid_build")


class ImagePyramid:
    """Pre-allocated for one image size: the packed levels 1..levels of a [3,H,W] colour image and, with has_depth / has_mask, of its
    depth [H,W] and byte mask [H,W].  build() fills them in one launch; color(l), depth(l), mask(l) are views of the allocation,
    overwritten by the next build()."""

    def __init__(self, W, H, levels, device, has_depth=True, has_mask=False):
        self.lib = _lib.load()
        self.W, self.H, self.levels, self.dev = int(W), int(H), int(levels), torch.device(device)
        self.has_depth, self.has_mask = bool(has_depth), bool(has_mask)
        if not 1 <= self.levels <= MAX_LEVELS or (self.W >> self.levels) < 1 or (self.H >> self.levels) < 1:
            raise _lib.GsajError("ImagePyramid: levels must be 1..%d and leave at least one pixel (W=%d H=%d levels=%d)" % (
                MAX_LEVELS, self.W, self.H, self.levels))
        self.buf = torch.empty(self.lib.gsaj_pyramid_bytes(self.W, self.H, self.levels, self.has_depth, self.has_mask), dtype=torch.uint8,
                               device=self.dev)
        self._lv = {}
        for l in range(1, self.levels + 1):
            wl, hl = ctypes.c_int(), ctypes.c_int()
            off = [ctypes.c_size_t() for _ in range(3)]
            _lib.check(self.lib.gsaj_pyramid_level(self.W, self.H, self.levels, self.has_depth, self.has_mask, l, ctypes.byref(wl), ctypes.byref(hl),
                                                   *[ctypes.byref(o) for o in off]), "gsaj_pyramid_level")
            self._lv[l] = (wl.value, hl.value) + tuple(o.value for o in off)

    def _level(self, l):
        if int(l) not in self._lv:
            raise _lib.GsajError("ImagePyramid: level %r is not one of 1..%d (level 0 is the frame itself)" % (l, self.levels))
        return self._lv[int(l)]

    def size(self, l):
        """(W_l, H_l) = (W >> l, H >> l)."""
        return self._level(l)[:2]

    def build(self, color, depth=None, mask=None, depth_edge_ratio=0.1):
        """color [3,H,W], depth [H,W] (any shape of H * W elements) fp32, mask uint8 of H * W elements: contiguous device tensors,
        read in place.  Depth and mask are given exactly when the pyramid was made with has_depth / has_mask."""
        if self.dev.type != "cuda":
            raise _lib.GsajError("ImagePyramid.build needs a HIP device (there is no CPU path)")
        n = self.W * self.H
        for name, t, has, dtype, numel in (("color", color, True, torch.float32, 3 * n), ("depth", depth, self.has_depth, torch.float32, n),
                                           ("mask", mask, self.has_mask, torch.uint8, n)):
            if (t is not None) != has:
                raise _lib.GsajError("ImagePyramid.build: %s must be given exactly when the pyramid was made for it" % name)
            if t is not None and (not torch.is_tensor(t) or t.device != self.buf.device or t.dtype != dtype or t.numel() != numel
                                  or not t.is_contiguous()):
                raise _lib.GsajError("ImagePyramid.build: %s must be a contiguous %s tensor of %d elements on %s" % (name, dtype, numel, self.buf.device))
        _build(self, color, depth, mask, depth_edge_ratio)

    def color(self, l):
        wl, hl, off = self._level(l)[:3]
        return self.buf[off:off + 12 * wl * hl].view(torch.float32).view(3, hl, wl)

    def depth(self, l):
        wl, hl, _, off, _ = self._level(l)
        if not self.has_depth:
            raise _lib.GsajError("ImagePyramid: made without depth")
        return self.buf[off:off + 4 * wl * hl].view(torch.float32).view(hl, wl)

    def mask(self, l):
        wl, hl, _, _, off = self._level(l)
        if not self.has_mask:
            raise _lib.GsajError("ImagePyramid: made without a mask")
        return self.buf[off:off + wl * hl].view(1, hl, wl)

    def level_camera(self, l, fx, fy, cx, cy, znear=0.01, zfar=100.0):
        """level_camera() of this pyramid's frame."""
        return level_camera(self.W, self.H, l, fx, fy, cx, cy, znear, zfar)


def level_camera(W, H, l, fx, fy, cx, cy, znear=0.01, zfar=100.0):
    """(W_l, H_l, projection_matrix, tanfovx, tanfovy) of level l (0: the frame) from the exact intrinsics of the cropped, box-filtered
    image: fx_l = fx / 2^l, cx_l = cx / 2^l, tanfovx = W_l / (2 fx_l) (y likewise).  The rasteriser maps ndc to pixels as
    ((ndc + 1) S - 1) / 2, so a camera point lands on pixel index fx X / z + cx - 0.5: pixel i covers [i, i + 1) of the continuous
    coordinate fx X / z + cx, a level-l pixel covers 2^l of them, and the coordinate simply scales.  (With pixel centres at integer
    coordinates it would be (cx + 0.5) / 2^l - 0.5; against this rasteriser that is (2^l - 1) / 2 pixels of level 0 off.)  Where W is no
    multiple of 2^l the level shows less than the frame and tanfovx differs from level 0's: that is the crop.  projection_matrix:
    getProjectionMatrix2 transposed, as Camera.projection_matrix holds it and the trackers take it."""
    from gaussian_splatting.utils.graphics_utils import getProjectionMatrix2
    s = float(1 << int(l))
    wl, hl = int(W) >> int(l), int(H) >> int(l)
    fxl, fyl = fx / s, fy / s
    proj = getProjectionMatrix2(znear, zfar, cx / s, cy / s, fxl, fyl, wl, hl).transpose(0, 1).contiguous()
    return wl, hl, proj, wl / (2.0 * fxl), hl / (2.0 * fyl)
