"""Motion stereo: the depth of a monocular keyframe from a second frame in general relative pose, on the device (C ABI
gsaj_motion_stereo / gsaj_grey_u8, csrc/sweep.hip).

The reference has NO counterpart: it seeds a monocular keyframe's new Gaussians at the map's rendered depth or at a constant with
noise (utils/slam_frontend.py:63-104).  This is this library's own statement (include/gsaj.h "motion stereo") -- a plane sweep over
inverse-depth hypotheses, gsaj.stereo's semi-global aggregation, a winner stage without a left-right check -- equal bit for bit to
tests/sweep_restated.py and pinned against nothing else (no OpenCV parity).  There is no CPU path.
"""
import numpy as np
import torch

from . import _frames, _lib

STAGE_COST, STAGE_PATHS, STAGE_WINNER = 1, 2, 4   # GSAJ_SWEEP_STAGE_*


def grey_u8(color, out=None):
    """A tracker's frame, float32 [3,H,W] on the device, -> grey bytes uint8 [H,W]: ((c0 + c1) + c2) / 3 scaled by 255 and rounded half
    up, clamped to 0..255, 0 for a NaN.  out: a uint8 [H,W] device tensor (rows may be padded) to write instead of a new one."""
    if not torch.is_tensor(color) or color.device.type != "cuda" or color.dtype != torch.float32 or color.dim() != 3 or color.shape[0] != 3 \
            or not color.is_contiguous():
        raise _lib.GsajError("grey_u8: color must be a contiguous float32 [3,H,W] tensor on a HIP device")
    H, W = int(color.shape[1]), int(color.shape[2])
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=color.device)
    elif not torch.is_tensor(out) or out.device != color.device or out.dtype != torch.uint8 or tuple(out.shape) != (H, W) or out.stride(1) != 1 \
            or out.stride(0) < W:
        raise _lib.GsajError("grey_u8: out must be a uint8 [%d,%d] tensor on %s whose rows are contiguous" % (H, W, color.device))
    with torch.cuda.device(color.device):
        stream = torch.cuda.current_stream(color.device).cuda_stream
        _frames.check(_lib.load().gsaj_grey_u8(W, H, color.data_ptr(), out.data_ptr(), out.stride(0), stream), "gsaj_grey_u8")
    return out


class MotionStereo(_frames.Matcher):
    """Pre-allocated for one camera: idx16, depth = MotionStereo(W, H, device, fx, fy, cx, cy, ...)(ref, src, ref_w2c, src_w2c, w_min,
    w_max) -> int16 [H,W], the winning inverse-depth hypothesis in sixteenths (-16 where invalid), and float32 [H,W], the depth of the
    keyframe `ref` with 0 at invalid pixels -- the form seed_from_keyframe, median_depth and FrameEvaluator take.

    ref, src: uint8 [H,W] grey images (grey_u8 makes them from the trackers' frames).  NumPy arrays go through pinned staging buffers
    this object owns, copied with non_blocking=True on the current stream; an event recorded behind the launches keeps the next call off
    the staging buffers until this one has read them.  Device tensors are read in place (rows may be padded).
    ref_w2c, src_w2c: world-to-camera, a float32 device tensor of at least 16 elements (a pose state serves) or a 4 x 4 NumPy array,
    uploaded per call.  [w_min, w_max]: the inverse-depth range the num_hypotheses are spread over, w_min >= 0 (0: infinity).
    The object owns its workspace (gsaj_motion_stereo_bytes) and, unless given out_idx16 / out_depth, its outputs, which the next call
    overwrites."""
    SIZE_FN, OFFSETS_FN = "gsaj_motion_stereo_bytes", "gsaj_debug_motion_stereo_offsets"
    VIEWS = (("pixel", torch.uint8), ("cost", torch.int16), ("sums", torch.int32))

    def __init__(self, W, H, device, fx, fy, cx, cy, num_hypotheses=64, block_radius=3, P1=100, P2=400, paths=8, uniqueness=10, outside_cost=80):
        self.lib = _lib.load()
        self.W, self.H, self.dev = int(W), int(H), _frames.device(device, "MotionStereo")
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.D, self.r, self.P1, self.P2 = int(num_hypotheses), int(block_radius), int(P1), int(P2)
        self.paths, self.uniqueness, self.outside_cost = int(paths), int(uniqueness), int(outside_cost)
        if self.D not in (16, 32, 64, 128) or self.W < 1 or self.H < 1 or self.paths not in (4, 8):
            raise _lib.GsajError("MotionStereo needs num_hypotheses 16, 32, 64 or 128, W >= 1, H >= 1 and paths 4 or 8 "
                                 "(got W=%d H=%d num_hypotheses=%d paths=%d)" % (self.W, self.H, self.D, self.paths))
        if not (0 <= self.r <= 7 and 0 <= self.P1 < self.P2 <= 1024 and 0 <= self.uniqueness <= 99 and 0 <= self.outside_cost <= 240):
            raise _lib.GsajError("MotionStereo needs 0 <= block_radius <= 7, 0 <= P1 < P2 <= 1024, 0 <= uniqueness <= 99 and 0 <= outside_cost <= 240 "
                                 "(got %d, %d, %d, %d, %d)" % (self.r, self.P1, self.P2, self.uniqueness, self.outside_cost))
        if not (self.fx > 0.0 and self.fy > 0.0 and np.isfinite([self.fx, self.fy, self.cx, self.cy]).all()):
            raise _lib.GsajError("MotionStereo: fx and fy must be positive, all four intrinsics finite (got %r)" % ((fx, fy, cx, cy),))
        self._allocate()
        self.idx16 = self.depth = None
        self._stage_ref = self._stage_src = self._event = None
        self._pose_host = self._pose_dev = None

    def gradient_bytes(self):
        """Tests and tools: the gradient bytes Gx | Gy << 8 of ref and src, int16 [2,H,W], as the last call left them (a copy: the two
        arrays open the workspace, each padded to 256 bytes)."""
        n, half = self.W * self.H, self._offsets()[0] // 2
        return torch.stack([self.workspace[o:o + 2 * n].view(torch.int16).view(self.H, self.W) for o in (0, half)])

    def pixel_costs(self):
        """Tests and tools: pc [H,W,D] uint8 as the last call left it (a view of the workspace)."""
        return self._debug_view("pixel")

    def _pose(self, t, name, slot):
        """-> (device pointer of 16 floats, True if it went through the pinned pose staging)."""
        if isinstance(t, np.ndarray):
            if t.shape != (4, 4):
                raise _lib.GsajError("%s must be a 4 x 4 array (got %s)" % (name, t.shape))
            if self._pose_host is None:
                self._pose_host = torch.empty(32, dtype=torch.float32, pin_memory=True)
                self._pose_dev = torch.empty(32, dtype=torch.float32, device=self.dev)
            self._pose_host[16 * slot:16 * slot + 16] = torch.from_numpy(np.ascontiguousarray(t, np.float32).reshape(16))
            return self._pose_dev.data_ptr() + 64 * slot, True
        if not torch.is_tensor(t) or t.device != self.dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < 16:
            raise _lib.GsajError("%s must be a 4 x 4 NumPy array or a contiguous float32 tensor of at least 16 elements on %s" % (name, self.dev))
        return t.data_ptr(), False

    def __call__(self, ref, src, ref_w2c, src_w2c, w_min, w_max, out_idx16=None, out_depth=None, stages=0):
        """stages: 0 = everything, else the STAGE_* to run on what the workspace holds (measurement and tests)."""
        oi = _frames.output(self, "idx16", out_idx16, "out_idx16", (self.H, self.W), torch.int16)
        oz = _frames.output(self, "depth", out_depth, "out_depth", (self.H, self.W))
        host = _frames.staging_free(self, ref, src, ref_w2c, src_w2c)
        a, astride = _frames.source(self, ref, "ref", ((self.H, self.W),), "_stage_ref")
        b, bstride = _frames.source(self, src, "src", ((self.H, self.W),), "_stage_src")
        pr, up_r = self._pose(ref_w2c, "ref_w2c", 0)
        ps, up_s = self._pose(src_w2c, "src_w2c", 1)
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            if up_r or up_s:
                self._pose_dev.copy_(self._pose_host, non_blocking=True)
            _frames.check(self.lib.gsaj_motion_stereo(self.W, self.H, a.data_ptr(), astride, b.data_ptr(), bstride, self.fx, self.fy, self.cx, self.cy,
                                                      pr, ps, float(w_min), float(w_max), self.D, self.r, self.P1, self.P2, self.paths, self.uniqueness,
                                                      self.outside_cost, int(stages), self.workspace.data_ptr(), self.workspace.numel(), oi.data_ptr(),
                                                      oz.data_ptr(), stream.cuda_stream), "gsaj_motion_stereo")
            _frames.staging_read(self, host, stream)
        return oi.view(self.H, self.W), oz.view(self.H, self.W)
