"""Frame-to-frame RGB-D alignment on the device (C ABI gsaj_rgbd_align, csrc/align.hip): the start pose of a new frame from the last
tracked frame alone -- its colour, its depth and its pose -- before the map is touched.  include/gsaj.h states the arithmetic.

One iteration is two C-ABI calls that touch no host state: gsaj_rgbd_align (one pass over the pixels of a level: warp, photometric
and depth residual, their pose Jacobians, the 6x6 normal equations of the iteratively reweighted terms, normalised by the number of
valid pixels) -> gsaj_pose_gn_step on that ONE row (accept / reject, damping, the Cholesky solve, W2C <- Exp(tau) W2C).  The levels of
both frames come from gsaj.pyramid.ImagePyramid, the state goes from level to level through gsaj_pose_gn_relevel, exactly as in
gsaj.PyramidGaussNewtonTracker.  There is no CPU path and no host read before result().

JointRgbdAligner is the joint form: the affine brightness change of the new frame against the reference, I_c = e^a I_r + b, is
solved with the pose -- gsaj_rgbd_align8 -> gsaj_pose_gn8_step on the gn8 state, the same two calls per iteration.
"""
import torch

from . import _lib
from ._gn_state import GnViews, check_schedule, init_state
from ._loop import require_device, stream
from .pyramid import MAX_LEVELS, ImagePyramid, level_camera


def _residuals(al, l, depth):  # (the device work of one iteration, first half: host-logic tests replace it)
    """gsaj_rgbd_align (joint form: gsaj_rgbd_align8) at level l: the reference level against the current level at the state's pose
    -> al.row."""
    W, H, fx, fy, cx, cy = al.cams[l]
    rc, rd, cc, cd = al._level(al._ref, l) + al._level(al._cur, l)
    name = "gsaj_rgbd_align8" if al.solve_exposure else "gsaj_rgbd_align"
    # the joint form reads the state's exposure on the device; gain_out, its one more argument: the gain it used is not asked for
    gain_out = (None,) if al.solve_exposure else ()
    with torch.cuda.device(al.dev):
        _lib.check(getattr(al.lib, name)(W, H, fx, fy, cx, cy, rc.data_ptr(), rd.data_ptr(), al.ref_w2c.data_ptr(), cc.data_ptr(),
                                         cd.data_ptr() if depth else None, al.state.data_ptr(), al.w_depth, al.delta_photo, al.delta_depth,
                                         al.depth_edge_ratio, al.min_depth, al.max_depth, al.min_overlap, al.rows.data_ptr(),
                                         al.row.data_ptr(), *gain_out, None, None, None, stream(al.dev)), name)


def _step(al, l):  # (device work too)
    step = al.lib.gsaj_pose_gn8_step if al.solve_exposure else al.lib.gsaj_pose_gn_step
    with torch.cuda.device(al.dev):
        _lib.check(step(al.row.data_ptr(), 1, *al.lm_args, al.projections[l].data_ptr(), al.state.data_ptr(), None, stream(al.dev)),
                   "gsaj_pose_gn8_step" if al.solve_exposure else "gsaj_pose_gn_step")


def _relevel(al, l):  # (device work too)
    with torch.cuda.device(al.dev):
        _lib.check(al.lib.gsaj_pose_gn_relevel(al.state.data_ptr(), al.state.numel(), al.projections[l].data_ptr(), al.lm_args[0], None,
                                               stream(al.dev)), "gsaj_pose_gn_relevel")


class _Frame:
    """One frame's level 0 (buffers the aligner owns) and its pyramid."""

    def __init__(self, W, H, levels, dev):
        self.color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        self.depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        self.pyramid = ImagePyramid(W, H, levels, dev, has_depth=True) if levels else None
        self.has_depth = False
        self.filled = False


class RgbdAligner(GnViews):
    """Aligns the last tracked frame (the reference: colour, depth, pose) against a new frame (colour, optionally depth), coarse to
    fine, and leaves the new frame's pose on the device: aligner.w2c is what a map tracker's set_frame(..., w2c=) takes.  Pre-allocated
    for one image size.  w_depth weighs the depth term against the photometric one; delta_photo / delta_depth: the residual below which
    an L1 term is a quadratic; depth_edge_ratio: the relative spread of the four depth taps (and of a coarse pixel's children) beyond
    which a pixel straddles a discontinuity and carries no depth term; min_overlap: the share of valid pixels below which a level
    gives no step.  The Levenberg-Marquardt arguments are GaussNewtonTracker's.  The photometric term has no exposure model: for frames
    whose brightness changes (auto-exposure), JointRgbdAligner below.  (solve_exposure, False here, is GnViews' switch between the gn
    and the gn8 layout: the state, the rows and the calls of an iteration follow it.)"""

    def __init__(self, W, H, fx, fy, cx, cy, device, levels=2, w_depth=1.0, delta_photo=0.01, delta_depth=0.01, depth_edge_ratio=0.1,
                 min_depth=0.01, max_depth=100.0, min_overlap=0.0, znear=0.01, zfar=100.0, lambda_init=1e-3, nu=4.0, lambda_min=1e-7,
                 lambda_max=1e7, converged_threshold=1e-4):
        require_device(device, "RgbdAligner")
        self._init_host(W, H, (fx, fy, cx, cy), device, levels, (w_depth, delta_photo, delta_depth, depth_edge_ratio, min_depth, max_depth,
                                                                  min_overlap), (znear, zfar),
                        (lambda_init, nu, lambda_min, lambda_max, converged_threshold))

    def _init_host(self, W, H, intrinsics, device, levels, terms, clip, lm_args):
        """Everything that is not a kernel: the argument checks, the level cameras, the buffers."""
        self.lib = _lib.load()
        self.W, self.H, self.dev, self.levels = int(W), int(H), torch.device(device), int(levels)
        fx, fy, cx, cy = (float(v) for v in intrinsics)
        (self.w_depth, self.delta_photo, self.delta_depth, self.depth_edge_ratio, self.min_depth, self.max_depth,
         self.min_overlap) = (float(v) for v in terms)
        self.lm_args = tuple(float(v) for v in lm_args)
        if not 0 <= self.levels <= MAX_LEVELS:
            raise _lib.GsajError("RgbdAligner: levels must be 0..%d, got %d" % (MAX_LEVELS, self.levels))
        if (self.W >> self.levels) < 2 or (self.H >> self.levels) < 2 or self.lib.gsaj_rgbd_align_partial_rows(self.W, self.H) == 0:
            raise _lib.GsajError("RgbdAligner: every level must be at least 2x2 and the frame at most 16384 a side (W=%d H=%d levels=%d)" % (
                self.W, self.H, self.levels))
        if not (fx > 0 and fy > 0):
            raise _lib.GsajError("RgbdAligner: fx and fy must be positive (fx=%g fy=%g)" % (fx, fy))
        if not (self.delta_photo > 0 and self.delta_depth > 0 and self.w_depth >= 0 and self.depth_edge_ratio >= 0):
            raise _lib.GsajError("RgbdAligner: delta_photo, delta_depth > 0 and w_depth, depth_edge_ratio >= 0 (got %g, %g, %g, %g)" % (
                self.delta_photo, self.delta_depth, self.w_depth, self.depth_edge_ratio))
        if not (0 < self.min_depth < self.max_depth and 0 <= self.min_overlap <= 1):
            raise _lib.GsajError("RgbdAligner: 0 < min_depth < max_depth and min_overlap in [0, 1] (got %g, %g, %g)" % (
                self.min_depth, self.max_depth, self.min_overlap))
        li, nu, lmin, lmax, _ = self.lm_args
        if not (nu > 1 and 0 < lmin <= li <= lmax):
            raise _lib.GsajError("RgbdAligner: nu > 1 and 0 < lambda_min <= lambda_init <= lambda_max")
        self.cams, self.projections = [], []
        for l in range(self.levels + 1):   # the exact intrinsics of the cropped, box-filtered image (pyramid.level_camera)
            wl, hl, proj, _, _ = level_camera(self.W, self.H, l, fx, fy, cx, cy, *clip)
            s = float(1 << l)
            self.cams.append((wl, hl, fx / s, fy / s, cx / s, cy / s))
            self.projections.append(proj.to(torch.float32).contiguous().to(self.dev))
        self._ref = _Frame(self.W, self.H, self.levels, self.dev)
        self._cur = _Frame(self.W, self.H, self.levels, self.dev)
        self.ref_w2c = torch.zeros(16, dtype=torch.float32, device=self.dev)
        self.state = torch.zeros(self._layout.floats, dtype=torch.float32, device=self.dev)
        self.rows = torch.empty(self.lib.gsaj_rgbd_align_partial_rows(self.W, self.H), self._layout.row, dtype=torch.float32, device=self.dev)
        self.row = torch.zeros(self._layout.row, dtype=torch.float32, device=self.dev)
        self._pixels = self.W * self.H   # of the level the row was last formed at
        self.iterations = 0

    # ---- frames ----------------------------------------------------------------------------------------------------------------------
    def _level(self, frame, l):
        if l == 0:
            return frame.color, frame.depth
        return frame.pyramid.color(l), frame.pyramid.depth(l)

    def _take(self, frame, color, depth, who):
        n = self.W * self.H
        for name, t, numel in (("color", color, 3 * n), ("depth", depth, n)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.device != self.state.device:
                raise _lib.GsajError("%s: %s must be a tensor on %s (there is no CPU path)" % (who, name, self.state.device))
            if t.numel() != numel:
                raise _lib.GsajError("%s: %s must have %d elements for a %dx%d frame, got %d" % (who, name, numel, self.W, self.H, t.numel()))
        frame.color.copy_(color.reshape(3, self.H, self.W))
        if depth is None:
            frame.depth.zero_()   # (no valid depth anywhere: the levels carry none either)
        else:
            frame.depth.copy_(depth.reshape(self.H, self.W))
        frame.has_depth = depth is not None
        frame.filled = True
        if frame.pyramid is not None:
            frame.pyramid.build(frame.color, frame.depth, None, self.depth_edge_ratio)

    def _pose(self, w2c, who):
        t = torch.as_tensor(w2c, dtype=torch.float32) if not torch.is_tensor(w2c) else w2c
        if t.numel() != 16:
            raise _lib.GsajError("%s: w2c must be a 4x4 matrix" % who)
        return t.detach().to(self.dev, torch.float32).reshape(16)

    def set_reference(self, color, depth, w2c):
        """The frame to align against: colour [3,H,W], depth [H,W] (device, fp32; copied) and its world-to-camera pose, a host array or
        a device tensor such as tracker.accepted_w2c (copied device to device)."""
        if depth is None:
            raise _lib.GsajError("set_reference: the reference frame needs depth")
        pose = self._pose(w2c, "set_reference")
        self._take(self._ref, color, depth, "set_reference")
        self.ref_w2c.copy_(pose)

    def promote(self, w2c=None):
        """The current frame becomes the reference (the pyramids are swapped, nothing is copied or rebuilt); its pose becomes w2c --
        the map tracker's refined pose, device to device -- or, by default, the aligned pose."""
        if not self._cur.filled:
            raise _lib.GsajError("promote: align() a frame first")
        if not self._cur.has_depth:
            raise _lib.GsajError("promote: the frame was aligned without depth, and the reference frame needs depth")
        pose = self._pose(self.w2c if w2c is None else w2c, "promote").clone()
        self._ref, self._cur = self._cur, self._ref
        self._cur.filled = False
        self.ref_w2c.copy_(pose)

    # ---- the solve -------------------------------------------------------------------------------------------------------------------
    def default_schedule(self):
        """8 iterations at the coarsest level, 6 at every level below it."""
        return [8] + [6] * self.levels

    def _reset(self, w2c, exposure=None):
        """A new solve: pose, camera matrices of the coarsest level, no accepted step, lambda_init -- device operations only.  exposure
        (joint form): the start (a, b), a device tensor of 2; None: (0, 0)."""
        init_state(self.state, self._layout, w2c, self.projections[self.levels], None, self.lm_args[0], rigid=True)
        if exposure is not None:
            self.state[self._layout.sl["exposure"]] = exposure
            self.state[self._layout.sl["acc_exposure"]] = exposure

    def align(self, color, depth=None, w2c_init=None, schedule=None):
        """Aligns the reference against this frame (colour [3,H,W], depth [H,W] or None: the photometric term alone).  w2c_init: the
        start pose, by default the reference's -- the start the frontend takes.  schedule: the iteration counts from the coarsest level
        to level 0 (levels + 1 of them).  No host read; returns the numbers run per level."""
        return self._align(color, depth, w2c_init, schedule)

    def _align(self, color, depth, w2c_init, schedule, exposure=None):
        if not self._ref.filled:
            raise _lib.GsajError("set_reference() first")
        schedule = self.default_schedule() if schedule is None else schedule if isinstance(schedule, (list, tuple)) else [schedule]
        schedule = check_schedule(schedule, self.levels, "align")
        start = self.ref_w2c if w2c_init is None else self._pose(w2c_init, "align")
        self._take(self._cur, color, depth, "align")
        self._reset(start, exposure)
        at = self.levels
        for l, n in zip(range(self.levels, -1, -1), schedule):
            if not n:   # (a level with no iterations is passed over)
                continue
            if at != l:
                _relevel(self, l)
                at = l
            for _ in range(n):
                _residuals(self, l, depth is not None)
                _step(self, l)
            self._pixels = self.cams[l][0] * self.cams[l][1]
        self.iterations += sum(schedule)
        return schedule

    # ---- results (device) ------------------------------------------------------------------------------------------------------------
    w2c = GnViews.accepted_w2c   # the aligned pose is the accepted one: the last proposal was never judged

    @property
    def overlap(self):
        """The share of valid pixels at the last level evaluated (device scalar)."""
        return self.row[self._layout.row_valid] / float(self._pixels)

    def result(self):
        """The one host read: (w2c [4,4] ndarray, overlap, accepted loss, converged)."""
        s, o = torch.cat([self.state, self.row]).cpu().numpy(), self._layout.o
        return (s[slice(*o["acc_w2c"])].reshape(4, 4).copy(), float(s[self._layout.floats + self._layout.row_valid]) / float(self._pixels),
                float(s[o["acc_loss"][0]]), bool(s[o["conv"][0]] != 0.0))


class JointRgbdAligner(RgbdAligner):
    """RgbdAligner with the affine brightness change of the new frame solved together with the pose: the new frame is modelled as
    e^a I_ref + b, the unknowns are [rho, theta, a, b] (gsaj_rgbd_align8 -> gsaj_pose_gn8_step on the gn8 state).  (a, b) is the new
    frame's brightness RELATIVE TO THE REFERENCE FRAME -- auto-exposure between the two frames -- not an absolute camera exposure;
    exposure_for() turns it into one.  The constructor, set_reference, promote, overlap, result and lm are RgbdAligner's (lm["H"] is
    8 x 8 over [rho, theta, a, b]).  A class of its own, not a keyword of RgbdAligner: the signatures of the existing loops are kept."""
    solve_exposure = True

    def _exposure(self, exposure, who):
        """(a, b) as a device tensor of 2: a pair of numbers, a host array or a device tensor (copied device to device)."""
        t = torch.as_tensor(exposure, dtype=torch.float32) if not torch.is_tensor(exposure) else exposure
        if t.numel() != 2:
            raise _lib.GsajError("%s: an exposure is the pair (a, b), got %d values" % (who, t.numel()))
        return t.detach().to(self.dev, torch.float32).reshape(2)

    def align(self, color, depth=None, w2c_init=None, schedule=None, exposure_init=None):
        """RgbdAligner.align; exposure_init: the start (a, b) -- a pair of numbers or a device tensor -- by default (0, 0), the
        brightness of the reference."""
        return self._align(color, depth, w2c_init, schedule, None if exposure_init is None else self._exposure(exposure_init, "align"))

    @property
    def relative_exposure(self):
        """Device [2]: the accepted (a, b) -- the new frame's brightness as e^a I_ref + b."""
        return self.accepted_exposure

    def exposure_for(self, ref_exposure):
        """Device [2]: the new frame's exposure (a_r + a, e^a b_r + b) from the reference frame's (a_r, b_r) -- a pair of numbers or a
        device tensor such as tracker.accepted_exposure -- and the accepted (a, b); no host read.  With obs = e^a' render + b' for both
        frames of one scene, obs_c = e^a obs_r + b = e^(a_r + a) render + (e^a b_r + b): the start exposure of the map tracker, as
        GaussNewtonTracker.reset(w2c, exposure=) and GaussNewtonWindow.set_view(..., exposure=) take it."""
        ref = self._exposure(ref_exposure, "exposure_for")
        a, b = self.accepted_exposure[0], self.accepted_exposure[1]
        return torch.stack([ref[0] + a, torch.exp(a) * ref[1] + b])
