"""A stereo pair from bytes to disparity, depth and the left colour, on the device (C ABI gsaj_rectify_u8 / gsaj_stereo_match,
csrc/stereo.hip and csrc/ingest.hip).

What the reference's StereoDataset does per frame on the host (utils/dataset.py:365-393) -- cv2.remap of both grey images,
cv2.StereoSGBM, bf / disparity -- without OpenCV: the byte remap is gsaj_frame_ingest's exact bilinear rounded to a byte, the matcher
is this library's own integer statement of semi-global matching (include/gsaj.h "stereo frames"), equal bit for bit to
tests/stereo_restated.py.  Its results DIFFER from cv2.StereoSGBM's and are not pinned against them.  There is no CPU path.
"""
import numpy as np
import torch

from . import _frames, _lib
from .ingest import UndistortMap

STAGE_COST, STAGE_PATHS, STAGE_WINNER = 1, 2, 4   # GSAJ_STEREO_STAGE_*


class StereoMatcher(_frames.Matcher):
    """Pre-allocated for one rectified camera pair: disp16 = StereoMatcher(W, H, device, ...)(left, right) -> int16 [H,W], the
    disparity in sixteenths of a pixel, -16 where invalid (every column x < num_disparities is).  depth(bf), or
    m(left, right, bf=..., out_depth=...), gives bf / disparity as float32 [H,W] with 0 at invalid pixels.

    left, right: uint8 [H,W].  NumPy arrays go through pinned staging buffers this object owns, copied with non_blocking=True on the
    current stream; an event recorded behind the launches keeps the next call off the staging buffers until this one has read them.
    Device tensors are read in place (rows may be padded).  The object owns its workspace (gsaj_stereo_workspace_bytes) and, unless
    given out_disp16 / out_depth, its outputs, which the next call overwrites."""
    SIZE_FN, OFFSETS_FN = "gsaj_stereo_workspace_bytes", "gsaj_debug_stereo_offsets"
    VIEWS = (("cost", torch.int16), ("sums", torch.int32))   # (only columns x >= D of C carry a result, and S is zero before them)

    def __init__(self, W, H, device, num_disparities=64, block_radius=10, P1=2, P2=5, paths=8, uniqueness=40, lr_max_diff=1):
        self.lib = _lib.load()
        self.W, self.H, self.dev = int(W), int(H), _frames.device(device, "StereoMatcher")
        self.D, self.r, self.P1, self.P2 = int(num_disparities), int(block_radius), int(P1), int(P2)
        self.paths, self.uniqueness, self.lr_max_diff = int(paths), int(uniqueness), int(lr_max_diff)
        if self.D not in (16, 32, 64, 128) or self.W <= self.D or self.H < 1 or self.paths not in (4, 8):
            raise _lib.GsajError("StereoMatcher needs num_disparities 16, 32, 64 or 128, W > num_disparities, H >= 1 and paths 4 or 8 "
                                 "(got W=%d H=%d num_disparities=%d paths=%d)" % (self.W, self.H, self.D, self.paths))
        if not (0 <= self.r <= 15 and 0 <= self.P1 < self.P2 <= 1024 and 0 <= self.uniqueness <= 99 and self.lr_max_diff >= -1):
            raise _lib.GsajError("StereoMatcher needs 0 <= block_radius <= 15, 0 <= P1 < P2 <= 1024, 0 <= uniqueness <= 99 and lr_max_diff >= -1 "
                                 "(got %d, %d, %d, %d, %d)" % (self.r, self.P1, self.P2, self.uniqueness, self.lr_max_diff))
        self._allocate()
        self.disp16 = self._depth = self._last = None
        self._stage_l = self._stage_r = self._event = None

    def __call__(self, left, right, bf=None, out_disp16=None, out_depth=None, stages=0):
        """stages: 0 = everything, else the STAGE_* to run on what the workspace holds (measurement and tests)."""
        if out_depth is not None and bf is None:
            raise _lib.GsajError("StereoMatcher: out_depth without bf")
        od = _frames.output(self, "disp16", out_disp16, "out_disp16", (self.H, self.W), torch.int16)
        oz = None if bf is None else _frames.output(self, "_depth", out_depth, "out_depth", (self.H, self.W))
        host = _frames.staging_free(self, left, right)
        l, ls = _frames.source(self, left, "left", ((self.H, self.W),), "_stage_l")
        r, rs = _frames.source(self, right, "right", ((self.H, self.W),), "_stage_r")
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            _frames.check(self.lib.gsaj_stereo_match(self.W, self.H, l.data_ptr(), ls, r.data_ptr(), rs, self.D, self.r, self.P1, self.P2, self.paths,
                                                     self.uniqueness, self.lr_max_diff, int(stages), self.workspace.data_ptr(), self.workspace.numel(),
                                                     od.data_ptr(), None if oz is None else oz.data_ptr(), 1.0 if bf is None else float(bf),
                                                     stream.cuda_stream), "gsaj_stereo_match")
            _frames.staging_read(self, host, stream)
        self._last = od
        return od.view(self.H, self.W) if bf is None else (od.view(self.H, self.W), oz.view(self.H, self.W))

    def depth(self, bf, out_depth=None):
        """bf / disparity of the LAST call's disparity, float32 [H,W]: the winner stage again, on the sums the workspace still holds."""
        if self._last is None:
            raise _lib.GsajError("StereoMatcher.depth: no pair has been matched yet")
        dummy = self._last.view(torch.uint8).view(self.H, 2 * self.W)[:, :self.W]   # (the images are not read by the winner stage)
        return self(dummy, dummy, bf=bf, out_disp16=self._last, out_depth=out_depth, stages=STAGE_WINNER)[1]


class StereoIngest:
    """Pre-allocated for one stereo camera.  color, depth = StereoIngest(W, H, device, bf, ...)(image_left, image_right) -> the left
    image as float32 [3,H,W] in [0, 1] (the rectified grey byte / 255.0f in all three planes) and the depth float32 [H,W] -- the
    tensors set_frame, GradMask, ImagePyramid and seeding take.

    undistort_left / undistort_right: UndistortMap objects of this W x H (made with the pair's R and new_K: the rectifying maps of
    cv2.initUndistortRectifyMap); the images, src_size = (Ws, Hs) (default (W, H)), are resampled through them to bytes.  Without
    maps the images are taken as rectified.  bf: baseline x focal length in pixels.  **matcher: StereoMatcher's parameters.
    Images: uint8 [Hs,Ws], NumPy (pinned staging, as FrameIngest) or device tensors (rows may be padded).  out_color / out_depth:
    write there instead of into buffers this object owns."""

    def __init__(self, W, H, device, bf, undistort_left=None, undistort_right=None, src_size=None, **matcher):
        self.matcher = StereoMatcher(W, H, device, **matcher)
        self.lib, self.W, self.H, self.dev = self.matcher.lib, self.matcher.W, self.matcher.H, self.matcher.dev
        self.bf = float(bf)
        if not (self.bf > 0.0 and np.isfinite(self.bf)):
            raise _lib.GsajError("StereoIngest: bf must be positive and finite (got %r)" % (bf,))
        self.Ws, self.Hs = (self.W, self.H) if src_size is None else (int(src_size[0]), int(src_size[1]))
        if (undistort_left is None) != (undistort_right is None):
            raise _lib.GsajError("StereoIngest: undistort_left and undistort_right must be given together or not at all")
        for m in (undistort_left, undistort_right):
            if m is not None and (not isinstance(m, UndistortMap) or (m.W, m.H) != (self.W, self.H) or m.dev != self.dev):
                raise _lib.GsajError("StereoIngest: the maps must be UndistortMap objects of %d x %d on %s" % (self.W, self.H, self.dev))
        if undistort_left is None and (self.Ws, self.Hs) != (self.W, self.H):
            raise _lib.GsajError("StereoIngest: without maps the source has the output's size (src_size=%r)" % (src_size,))
        if self.Ws < 1 or self.Hs < 1:
            raise _lib.GsajError("StereoIngest: src_size must be positive (got %r)" % (src_size,))
        self.maps = (undistort_left, undistort_right)
        self.rect = torch.empty((2, self.H, self.W), dtype=torch.uint8, device=self.dev)   # the rectified bytes, left then right
        self.color = self.depth = None
        self._stage_l = self._stage_r = self._event = None

    def __call__(self, image_left, image_right, out_color=None, out_depth=None):
        oc = _frames.output(self, "color", out_color, "out_color", (3, self.H, self.W))
        oz = _frames.output(self, "depth", out_depth, "out_depth", (self.H, self.W))
        host = _frames.staging_free(self, image_left, image_right)
        srcs = (_frames.source(self, image_left, "image_left", ((self.Hs, self.Ws),), "_stage_l"),
                _frames.source(self, image_right, "image_right", ((self.Hs, self.Ws),), "_stage_r"))
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            for i, ((src, stride), m) in enumerate(zip(srcs, self.maps)):
                _frames.check(self.lib.gsaj_rectify_u8(self.W, self.H, self.Ws, self.Hs, stride, src.data_ptr(),
                                                       None if m is None else m.map_x.data_ptr(), None if m is None else m.map_y.data_ptr(),
                                                       self.rect[i].data_ptr(), self.W, oc.data_ptr() if i == 0 else None, stream.cuda_stream),
                              "gsaj_rectify_u8")
            _frames.staging_read(self, host, stream)
            self.matcher(self.rect[0], self.rect[1], bf=self.bf, out_depth=oz)
        return oc.view(3, self.H, self.W), oz.view(self.H, self.W)
