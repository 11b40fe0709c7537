"""A camera frame from bytes to the tensors the trackers read, on the device (C ABI gsaj_undistort_map / gsaj_frame_ingest,
csrc/ingest.hip).

What the reference's datasets do per frame on the host (utils/dataset.py:257-278, :370-386, :499-513) -- cv2.remap of a distorted
image, image / 255.0, clamp, permute, a float32 upload, depth / depth_scale -- as one launch: the bytes travel as bytes, the colour
comes out float32 [3,H,W] in [0, 1], the depth float32 [H,W].  include/gsaj.h states the arithmetic.  The remap is an exact fp32
bilinear with a constant 0 border; bit parity with cv2.remap, which interpolates in fixed point, is not claimed.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _frames, _lib

BGR, ROUND_U8, DEPTH_MUL = 1, 2, 4   # GSAJ_INGEST_*


def _dbl(values, n, what):
    a = np.ascontiguousarray(np.asarray(values, np.float64).reshape(-1))
    if a.size != n:
        raise _lib.GsajError("%s must have %d values, got %d" % (what, n, a.size))
    return a


def _kmat(K, what):
    """(fx, fy, cx, cy) -> the 3 x 3 camera matrix, float64."""
    fx, fy, cx, cy = _dbl(K, 4, what)
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


class UndistortMap:
    """The source coordinates of every pixel of the undistorted W x H image, computed once per camera: map_x, map_y float32 [H,W]
    on the device, what cv2.initUndistortRectifyMap(K, dist, R, new_K, (W, H), CV_32FC1) is documented to compute.  K, new_K:
    (fx, fy, cx, cy); dist: (k1, k2, p1, p2, k3); R: 3 x 3, default the identity; new_K default K."""

    def __init__(self, W, H, K, dist, device, R=None, new_K=None):
        self.lib = _lib.load()
        self.W, self.H, self.dev = int(W), int(H), _frames.device(device, "UndistortMap")
        if self.W < 1 or self.H < 1:
            raise _lib.GsajError("UndistortMap needs W >= 1 and H >= 1 (got W=%d H=%d)" % (self.W, self.H))
        self.K = _dbl(K, 4, "K")
        self.dist = _dbl(dist, 5, "dist")
        Rm = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
        self.iR = np.ascontiguousarray(np.linalg.inv(_kmat(K if new_K is None else new_K, "new_K") @ Rm)).reshape(-1)
        self.map_x = torch.empty((self.H, self.W), dtype=torch.float32, device=self.dev)
        self.map_y = torch.empty((self.H, self.W), dtype=torch.float32, device=self.dev)
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_undistort_map(self.W, self.H, hp(self.K), hp(self.dist), hp(self.iR), self.map_x.data_ptr(),
                                                   self.map_y.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream), "gsaj_undistort_map")


class FrameIngest:
    """Pre-allocated for one camera.  color, depth = FrameIngest(W, H, device, ...)(image, depth) -> float32 [3,H,W] in [0, 1] and
    float32 [H,W] (None without depth), one launch on the current stream.

    channels: 1 (grey: the byte goes to all three planes), 3, or 4 (the fourth byte is ignored).  undistort: an UndistortMap of this
    W x H -- the image, src_size = (Ws, Hs) (default (W, H)), is then resampled through it; without one the image has the output's size.
    depth_scale: the divisor of the uint16 depth (depth_mul: the multiplier, a RealSense's depth unit); None: no depth.  bgr: the
    image's channels are B, G, R.  round_u8: round the remapped value to the nearest byte before the division, half up.

    image: uint8 [Hs,Ws] (channels = 1) or [Hs,Ws,channels]; depth: uint16 [H,W].  NumPy arrays go through pinned staging buffers this
    object owns, copied with non_blocking=True on the current stream; an event recorded behind the launch keeps the next call off
    the staging buffers until this one has read them, and nothing else waits.  Device tensors are read in place (rows may be
    padded: stride(0) is the row stride).  out_color / out_depth: write there -- a tracker's gt_color / gt_depth -- instead of into
    buffers this object owns, which the next call overwrites."""

    def __init__(self, W, H, device, channels=3, src_size=None, undistort=None, depth_scale=None, depth_mul=False, bgr=False, round_u8=False):
        self.lib = _lib.load()
        self.W, self.H, self.dev, self.C = int(W), int(H), _frames.device(device, "FrameIngest"), int(channels)
        if self.W < 1 or self.H < 1 or self.C not in (1, 3, 4):
            raise _lib.GsajError("FrameIngest needs W >= 1, H >= 1 and channels 1, 3 or 4 (got W=%d H=%d channels=%d)" % (self.W, self.H, self.C))
        self.Ws, self.Hs = (self.W, self.H) if src_size is None else (int(src_size[0]), int(src_size[1]))
        self.undistort = undistort
        if undistort is None:
            if (self.Ws, self.Hs) != (self.W, self.H):
                raise _lib.GsajError("FrameIngest: without an UndistortMap the source has the output's size (src_size=%r)" % (src_size,))
        elif not isinstance(undistort, UndistortMap) or (undistort.W, undistort.H) != (self.W, self.H) or undistort.dev != self.dev:
            raise _lib.GsajError("FrameIngest: undistort must be an UndistortMap of %d x %d on %s" % (self.W, self.H, self.dev))
        if self.Ws < 1 or self.Hs < 1:
            raise _lib.GsajError("FrameIngest: src_size must be positive (got %r)" % (src_size,))
        self.depth_scale = None if depth_scale is None else float(depth_scale)
        if self.depth_scale is not None and (self.depth_scale == 0.0 or not np.isfinite(self.depth_scale)):
            raise _lib.GsajError("FrameIngest: depth_scale must be finite and not zero (got %r)" % (depth_scale,))
        self.flags = (BGR if bgr else 0) | (ROUND_U8 if round_u8 else 0) | (DEPTH_MUL if depth_mul else 0)
        self.color = self.depth = None   # made by the first call that is not given out_color / out_depth
        self._stage_c = self._stage_d = self._event = None

    def __call__(self, image, depth=None, out_color=None, out_depth=None):
        if (depth is not None) != (self.depth_scale is not None):
            raise _lib.GsajError("FrameIngest: depth must be given exactly when the object was made with a depth_scale")
        if depth is None and out_depth is not None:
            raise _lib.GsajError("FrameIngest: out_depth without depth")
        oc = _frames.output(self, "color", out_color, "out_color", (3, self.H, self.W), dtype_name="float32")
        od = None if depth is None else _frames.output(self, "depth", out_depth, "out_depth", (self.H, self.W), dtype_name="float32")
        host = _frames.staging_free(self, image, depth)
        shapes = ((self.Hs, self.Ws, self.C),) + (((self.Hs, self.Ws),) if self.C == 1 else ())
        src, src_stride = _frames.source(self, image, "image", shapes, "_stage_c")
        draw, d_stride = (None, 0) if depth is None else _frames.source(self, depth, "depth", ((self.H, self.W),), "_stage_d", torch.uint16, np.uint16)
        m = self.undistort
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            _lib.check(self.lib.gsaj_frame_ingest(self.W, self.H, self.Ws, self.Hs, self.C, src_stride, src.data_ptr(),
                                                  None if m is None else m.map_x.data_ptr(), None if m is None else m.map_y.data_ptr(),
                                                  None if draw is None else draw.data_ptr(), d_stride, self.depth_scale or 1.0, self.flags,
                                                  oc.data_ptr(), None if od is None else od.data_ptr(), stream.cuda_stream), "gsaj_frame_ingest")
            _frames.staging_read(self, host, stream)
        return oc.view(3, self.H, self.W), None if od is None else od.view(self.H, self.W)
