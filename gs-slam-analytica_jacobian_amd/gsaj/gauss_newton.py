"""Second-order tracking of one frame on the device: Gauss-Newton / Levenberg-Marquardt on the pose, next to
gsaj.tracking.DeviceTracker's first-order loop (DESIGN.md "Gauss-Newton tracking").

One iteration is three C-ABI calls that touch no host state: asynchronous forward -> gsaj_rasterize_pose_jacobian_loss (the
per-pixel pose Jacobian in forward mode and, fused, the 6x6 normal equations H = sum h J^T J, g = sum s J of the tracking loss
with the L1 terms as iteratively reweighted least squares) -> gsaj_pose_gn_step (accept / reject against the last accepted loss,
damping, a 6x6 Cholesky solve, W2C <- Exp(tau) W2C and the camera matrices of the next render).  An iteration renders at the pose
the previous one proposed; whether that pose is kept is decided by the NEXT step, from the loss rendered there.  Exposure enters as
the fixed affine e^a C + b; only tau is solved for.  No graph capture and no process group.

solve_exposure=True is the joint form: the unknowns are [rho, theta, a, b], as the frontend's tracking loop optimises them.  The same
three calls with gsaj_rasterize_pose_jacobian_loss8 (two more Jacobian columns per colour row, the forward's colour for a and 1 / e^a
for b: 8x8 normal equations in 64-float rows) and gsaj_pose_gn8_step (8x8 solve; a and b are stepped, saved on an accepted step and
restored on a rejected one together with the pose).

An asynchronous frame that does not fit its arena is aborted on the device: its kernels return at once and the step, handed the
frame's abort word, changes nothing; iterate() raises when it is done, exactly as DeviceTracker.iterate does.

PyramidGaussNewtonTracker runs the same iteration coarse to fine over the frame's image pyramid (gsaj.pyramid, csrc/pyramid.hip): one
tracker per level on one shared state, re-levelled between levels on the device (gsaj_pose_gn_relevel)."""
import torch

from . import _lib
from ._gn_state import SPANS, GnViews, check_schedule, init_state, matrices
from ._loop import FrameTarget, ViewTargets, check_slot, finish_frame, finish_window, loss_description, loss_terms, map_args, require_device, run, stream
from .losses import TRACKING
from .pyramid import MAX_LEVELS, ImagePyramid, level_camera
from .rasterizer import BatchContext, FrameContext

# field -> (a, b) of the two forms, under the names the host-logic tests know: a tracker they assemble by hand carries one as `_o`
_O, _O8 = SPANS["gn"], SPANS["gn8"]


class GaussNewtonTracker(GnViews, FrameTarget):
    def __init__(self, P, W, H, M, device, w2c, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, sh_degree=0, shs=None,
                 colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, monocular=False, alpha=0.95,
                 rgb_boundary_threshold=0.01, record_bits=32, irls_delta=0.01, lambda_init=1e-3, nu=4.0, lambda_min=1e-7,
                 lambda_max=1e7, converged_threshold=1e-4, solve_exposure=False):
        """The Gaussians (device tensors) are those of the current map: the loop reads them, it never writes them.  irls_delta: the
        residual below which an L1 term is treated as a quadratic (0: pure IRLS weights 1 / |r|).  lambda_init / nu / lambda_min /
        lambda_max: the damping and its factor; converged_threshold: |tau| below which the device reports convergence.
        solve_exposure: solve for the exposure (a, b) together with the pose (then convergence also needs |da|, |db| below the threshold)."""
        self.dev = require_device(device, "GaussNewtonTracker")
        self.lib = _lib.load()
        self.ctx = FrameContext(P, W, H, M, self.dev, has_scales=scales is not None, record_bits=record_bits)
        self.solve_exposure = bool(solve_exposure)
        self._step, self._step_name = ((self.lib.gsaj_pose_gn8_step, "gsaj_pose_gn8_step") if self.solve_exposure else
                                       (self.lib.gsaj_pose_gn_step, "gsaj_pose_gn_step"))
        self.state = torch.zeros(self._layout.floats, dtype=torch.float32, device=self.dev)
        self.projection = torch.as_tensor(projection_matrix, dtype=torch.float32).reshape(4, 4).contiguous().to(self.dev)
        self.praw = self.projection
        self.tanfov = (float(tanfovx), float(tanfovy))
        self.flags, self.alpha, self.thr, self.delta = loss_terms(monocular, alpha, rgb_boundary_threshold, irls_delta, TRACKING)
        self.lm_args = (float(lambda_init), float(nu), float(lambda_min), float(lambda_max), float(converged_threshold))
        self.bg, self.means, self.opac = bg, means3D, opacities
        self.kw = map_args(sh_degree, shs, colors_precomp, scales, rotations, cov3D_precomp)
        self._abort_ptr = self.ctx.abort_flag_ptr()
        self.gt_color = self.gt_depth = self.grad_mask = None
        self._grad_op = None
        self.iterations = 0
        self.reset(w2c)

    def reset(self, w2c, exposure=(0.0, 0.0)):
        """A new frame: pose, no accepted step, lambda back to lambda_init -- in place."""
        init_state(self.state, self._layout, w2c, self.projection, exposure, self.lm_args[0])

    _start_pose = reset   # (FrameTarget.set_frame's new start pose)

    def _iteration(self, sync):
        c, view, proj, campos = self.ctx, self.viewmatrix, self.projmatrix, self.campos   # (the views are made once per iteration)
        c.forward(self.bg, self.means, self.opac, view, proj, campos, self.tanfov[0], self.tanfov[1], sync=sync, **self.kw)
        L = loss_description(self, self.exposure_a, self.exposure_b)
        o = c.pose_jacobian_loss(L, self.bg, self.means, view, proj, self.praw, campos, self.tanfov[0], self.tanfov[1],
                                 irls_delta=self.delta, solve_exposure=self.solve_exposure, **self.kw)
        _lib.check(self._step(o["partials"].data_ptr(), o["partials"].shape[0], *self.lm_args, self.projection.data_ptr(),
                              self.state.data_ptr(), self._abort_ptr, stream(self.dev)), self._step_name)

    def iterate(self, n, check_every=0):
        """Up to n iterations; check_every > 0: stop once the device reports |tau| (and, with solve_exposure, |da|, |db|) < converged_threshold, looked at every check_every
        iterations.  Returns the number run.  Raises GsajError after the loop if an asynchronous frame was aborted on the device
        (those iterations changed nothing); the next call re-sizes the arena with one synchronous iteration."""
        if self.gt_color is None:
            raise _lib.GsajError("set_frame() first")
        with torch.cuda.device(self.dev):   # the very first iteration sizes the binning arena: synchronous forward
            done = run(n, check_every, lambda: self._iteration(self.ctx.capacity == 0), lambda: self.converged)
        self.iterations += done
        finish_frame(self.ctx)
        return done


# ---- K independent solves against ONE map, in one set of launches ------------------------------------------------------------------
def _launch(win, sync):  # (the one iteration's device work: host-logic tests replace it)
    """Batched forward at the K proposed poses -> BatchContext.pose_jacobian_loss -> gsaj_pose_gn[8]_step_batch."""
    c, n, exposure = win.ctx, win.state.shape[1], win.exposure
    views, projs, cps = win.matrices()
    c.forward(win.bg, win.means, win.opac, views, projs, cps, win.tanfov[0], win.tanfov[1], sync=sync, **win.kw)
    L = loss_description(win, exposure[:, 0], exposure[:, 1], exposure_stride=n)
    o = c.pose_jacobian_loss(L, win.bg, win.means, views, projs, win.praw, cps, win.tanfov[0], win.tanfov[1], irls_delta=win.delta,
                             solve_exposure=win.solve_exposure, **win.kw)
    skip, skip_stride = c.abort_flags()
    name = "gsaj_pose_gn8_step_batch" if win.solve_exposure else "gsaj_pose_gn_step_batch"
    _lib.check(getattr(win.lib, name)(win.K, o["partials"].data_ptr(), o["partials"].shape[1], win.active.data_ptr(), *win.lm_args,
                                      win.projection.data_ptr(), win.state.data_ptr(), skip, skip_stride,
                                      stream(win.dev)), name)


def _select(win):  # (device work too)
    """gsaj_pose_gn_select into win._best: int32 [2] = the index, the bits of its loss."""
    _lib.check(win.lib.gsaj_pose_gn_select(win.K, win.state.data_ptr(), win.state.shape[1], win.active.data_ptr(), win._best.data_ptr(),
                                           win._best.data_ptr() + 4, stream(win.dev)), "gsaj_pose_gn_select")


class GaussNewtonWindow(GnViews, ViewTargets):
    """GaussNewtonTracker for K views of ONE fixed map, solved together: every kernel of an iteration runs once with gridDim.y = K
    (batched forward, Jacobian walk, K Levenberg-Marquardt steps in one launch).  With the map fixed the K poses decouple, so the K
    solves are exact, and each view's arithmetic is the single tracker's.  Two uses:
      the keyframe window -- set_view(slot, ...): each slot has its own frame, pose and exposure;
      multi-start tracking of one frame -- set_frame(..., w2cs=K starts): one frame in all K slots; best() names the hypothesis of
      smallest accepted loss, chosen on the device.
    `active` ([K] uint8, device) is a mask: a view whose byte is 0 is rendered but its state is not touched."""

    def __init__(self, K, P, W, H, M, device, w2cs, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, sh_degree=0, shs=None,
                 colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, monocular=False, alpha=0.95,
                 rgb_boundary_threshold=0.01, record_bits=32, irls_delta=0.01, lambda_init=1e-3, nu=4.0, lambda_min=1e-7,
                 lambda_max=1e7, converged_threshold=1e-4, solve_exposure=False, streams=1):
        """The arguments of GaussNewtonTracker with K and w2cs [K,4,4]; streams: BatchContext's view groups."""
        require_device(device, "GaussNewtonWindow")
        ctx = BatchContext(K, P, W, H, M, device, has_scales=scales is not None, record_bits=record_bits, streams=streams)
        self._init_host(ctx, w2cs, projection_matrix, (tanfovx, tanfovy), bg, means3D, opacities,
                        map_args(sh_degree, shs, colors_precomp, scales, rotations, cov3D_precomp),
                        dict(monocular=monocular, alpha=alpha, rgb_boundary_threshold=rgb_boundary_threshold, irls_delta=irls_delta),
                        (lambda_init, nu, lambda_min, lambda_max, converged_threshold), solve_exposure)

    def _init_host(self, ctx, w2cs, projection_matrix, tanfov, bg, means3D, opacities, kw, loss, lm_args, solve_exposure):
        """Everything but the context: buffers and state, no kernel."""
        self.ctx, self.lib = ctx, _lib.load()
        self.K, self.W, self.H, self.dev = ctx.K, ctx.W, ctx.H, ctx.dev
        self.solve_exposure = bool(solve_exposure)
        self.state = torch.zeros((self.K, self._layout.floats), dtype=torch.float32, device=self.dev)
        self.projection = torch.as_tensor(projection_matrix, dtype=torch.float32).reshape(4, 4).contiguous().to(self.dev)
        self.praw = self.projection
        self.tanfov = (float(tanfov[0]), float(tanfov[1]))
        self.flags, self.alpha, self.thr, self.delta = loss_terms(flags=TRACKING, **loss)
        self.lm_args = tuple(float(x) for x in lm_args)
        self.bg, self.means, self.opac, self.kw = bg, means3D, opacities, kw
        self._alloc_views(loss["monocular"])
        self.grad_mask = None  # uint8 [K*H*W] once a slot was given a mask (the other slots: all ones, which is no mask)
        self.active = torch.ones(self.K, dtype=torch.uint8, device=self.dev)
        self._best = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self._filled = [False] * self.K
        self._sized = False
        self.iterations = 0
        w2cs = torch.as_tensor(w2cs, dtype=torch.float32)
        if tuple(w2cs.shape) != (self.K, 4, 4):
            raise _lib.GsajError("GaussNewtonWindow: w2cs must be [%d,4,4], got %r" % (self.K, tuple(w2cs.shape)))
        for k in range(self.K):
            self.reset(k, w2cs[k])

    def reset(self, slot, w2c, exposure=(0.0, 0.0)):
        """Slot `slot` starts over: pose (and exposure), no accepted step, lambda back to lambda_init -- as GaussNewtonTracker.reset."""
        init_state(self.state[check_slot(slot, self.K, "GaussNewtonWindow")], self._layout, w2c, self.projection, exposure, self.lm_args[0])

    def set_view(self, slot, gt_color, gt_depth=None, grad_mask=None, w2c=None, exposure=None):
        """The window use: slot `slot` gets its own frame -- ground truth (device, [3,H,W] / [H,W]; grad_mask [1,H,W] or None), copied
        into the window's [K,...] buffers -- and optionally a new start pose (with `exposure` (a, b), default (0, 0))."""
        H, W = self.H, self.W
        if grad_mask is not None and grad_mask.numel() != H * W:
            raise _lib.GsajError("set_view: grad_mask must have %d elements, got %d" % (H * W, grad_mask.numel()))
        k = self._take_view(slot, gt_color, gt_depth)
        if grad_mask is not None and self.grad_mask is None:
            self.grad_mask = torch.ones(self.K * H * W, dtype=torch.uint8, device=self.dev)
        if self.grad_mask is not None:
            m = self.grad_mask[k * H * W:(k + 1) * H * W]
            if grad_mask is None:
                m.fill_(1)
            else:
                m.copy_(grad_mask.to(self.dev, torch.uint8).reshape(-1))
        self._filled[k] = True
        if w2c is not None or exposure is not None:
            self.reset(k, self.w2c[k].clone() if w2c is None else w2c, (0.0, 0.0) if exposure is None else exposure)

    def set_frame(self, gt_color, gt_depth=None, grad_mask=None, w2cs=None, exposure=None):
        """The multi-start use: ONE frame copied into all K slots, with K start poses w2cs [K,4,4] (None: the slots keep theirs)."""
        if w2cs is not None:
            w2cs = torch.as_tensor(w2cs, dtype=torch.float32)
            if tuple(w2cs.shape) != (self.K, 4, 4):
                raise _lib.GsajError("set_frame: w2cs must be [%d,4,4], got %r" % (self.K, tuple(w2cs.shape)))
        for k in range(self.K):
            self.set_view(k, gt_color, gt_depth, grad_mask, None if w2cs is None else w2cs[k], exposure)

    def matrices(self):
        """(viewmatrices [K,4,4], projmatrices [K,4,4], campos [K,3]) of the poses the next render is at, gathered from the state."""
        return matrices(self.state)

    def _one(self):
        _launch(self, not self._sized)
        self._sized = True

    def iterate(self, n, check_every=0):
        """Up to n iterations of all K views.  The first is synchronous (it sizes the arena); after it an iteration contains no host
        read.  check_every > 0: every check_every iterations the K converged flags are read once, and the loop stops when every
        active view has converged.  Returns the number run.  Raises GsajError after the loop if a view was aborted on the device
        (its state was skipped in those iterations); the next call re-sizes the arena with one synchronous iteration."""
        if not all(self._filled):
            raise _lib.GsajError("set_view() every slot (or set_frame()) first: slots %r have no frame" %
                                 [k for k, ok in enumerate(self._filled) if not ok])
        done = run(n, check_every, self._one, lambda: ((self.converged != 0) | (self.active == 0)).all())
        self.iterations += done
        try:
            finish_window(self.ctx, "those views' states were skipped")
        except _lib.GsajError:
            self._sized = False
            raise
        return done

    def best(self):
        """(index, accepted loss) of the active view of smallest finite accepted loss (ties: the lowest index), chosen on the device
        by gsaj_pose_gn_select and read back in one copy; (-1, inf) if no active view has accepted a pose."""
        _select(self)
        h = self._best.cpu()
        return int(h[0]), float(h[1:2].view(torch.float32)[0])


# ---- coarse to fine: one solve carried down an image pyramid -----------------------------------------------------------------------------
def _level_tracker(pt, W, H, projection, tanfov, w2c):  # (device work: a context per level; host-logic tests replace it)
    return GaussNewtonTracker(pt.P, W, H, pt.M, pt.dev, w2c, projection, tanfov[0], tanfov[1], pt.bg, pt.means, pt.opac, **pt.kw)


def _relevel(pt, level, skip):  # (device work too)
    """gsaj_pose_gn_relevel of the shared state to level `level`'s projection matrix; skip: a device address or None."""
    with torch.cuda.device(pt.dev):
        _lib.check(pt.lib.gsaj_pose_gn_relevel(pt.state.data_ptr(), pt.state.numel(), pt.trackers[level].projection.data_ptr(), pt.lambda_init,
                                               skip, stream(pt.dev)), "gsaj_pose_gn_relevel")


def _level_iteration(t, sync):  # (device work too)
    """One iteration of level tracker t: forward -> pose_jacobian_loss -> step, on the shared state."""
    with torch.cuda.device(t.dev):
        t._iteration(sync)


class PyramidGaussNewtonTracker:
    """GaussNewtonTracker coarse to fine: the frame's pyramid is built on the device (gsaj.pyramid.ImagePyramid), the solve starts at
    level `levels` -- a wide basin and a cheap iteration -- and is handed from level to level down to the frame itself.  One
    GaussNewtonTracker per level, level 0 included, each with its own context at its own resolution and camera, all on ONE
    Levenberg-Marquardt state; between two levels gsaj_pose_gn_relevel takes the state to the next camera on the device.  The accepted
    loss of one level says nothing about the next one's: it starts a new baseline there.  levels=0 is GaussNewtonTracker.
    A batched form (GaussNewtonWindow) is not built."""

    def __init__(self, P, W, H, M, device, w2c, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, levels=0, fx=None, fy=None,
                 cx=None, cy=None, znear=0.01, zfar=100.0, depth_edge_ratio=0.1, **kw):
        """The arguments of GaussNewtonTracker (projection_matrix, tanfovx, tanfovy: level 0's), then levels, the intrinsics of the
        frame, from which every coarser level's camera follows (ImagePyramid.level_camera), and depth_edge_ratio: the relative depth
        spread beyond which a coarse pixel counts as a depth discontinuity and carries no depth."""
        require_device(device, "PyramidGaussNewtonTracker")
        self._init_host(P, W, H, M, device, w2c, projection_matrix, (tanfovx, tanfovy), bg, means3D, opacities, levels,
                        (fx, fy, cx, cy, znear, zfar), depth_edge_ratio, kw)

    def _init_host(self, P, W, H, M, device, w2c, projection_matrix, tanfov, bg, means3D, opacities, levels, intrinsics, depth_edge_ratio, kw):
        """Everything that is not a kernel: the level cameras, one tracker per level (through _level_tracker), the shared state."""
        self.lib = _lib.load()
        self.P, self.W, self.H, self.M, self.dev = int(P), int(W), int(H), int(M), torch.device(device)
        self.levels = int(levels)
        self.bg, self.means, self.opac, self.kw = bg, means3D, opacities, dict(kw)
        self.lambda_init = float(kw.get("lambda_init", 1e-3))
        self.depth_edge_ratio = float(depth_edge_ratio)
        if not 0 <= self.levels <= MAX_LEVELS:
            raise _lib.GsajError("PyramidGaussNewtonTracker: levels must be 0..%d, got %d" % (MAX_LEVELS, self.levels))
        if self.levels and any(v is None for v in intrinsics[:4]):
            raise _lib.GsajError("PyramidGaussNewtonTracker: levels > 0 needs the intrinsics fx, fy, cx, cy of the frame")
        cams = [(self.W, self.H, projection_matrix, float(tanfov[0]), float(tanfov[1]))]
        for l in range(1, self.levels + 1):
            cams.append(level_camera(self.W, self.H, l, *intrinsics))
            if cams[l][0] < 16 or cams[l][1] < 16:   # less than one tile carries no signal
                raise _lib.GsajError("PyramidGaussNewtonTracker: level %d of a %dx%d frame is %dx%d, smaller than one 16x16 tile" % (
                    l, self.W, self.H, cams[l][0], cams[l][1]))
        self.trackers = [_level_tracker(self, c[0], c[1], c[2], (c[3], c[4]), w2c) for c in cams]
        self.state = self.trackers[0].state
        for t in self.trackers[1:]:   # ONE Levenberg-Marquardt state
            t.state = self.state
        self.pyramid = None           # made by the first set_frame(): whether it holds a mask is known then
        self._level_mask = None       # edge_threshold: the per-level masks GradMask writes
        self._snapshot = torch.empty_like(self.state)
        self._at = 0                  # the level whose camera the state's matrices are for
        self.iterations = 0
        if self.levels:
            self.trackers[-1].reset(w2c)
            self._at = self.levels

    solve_exposure = property(lambda s: s.trackers[0].solve_exposure)
    w2c = property(lambda s: s.trackers[0].w2c)
    converged = property(lambda s: s.trackers[0].converged)
    accepted_w2c = property(lambda s: s.trackers[0].accepted_w2c)
    accepted_exposure = property(lambda s: s.trackers[0].accepted_exposure)
    loss_terms = property(lambda s: s.trackers[0].loss_terms)
    lm = property(lambda s: s.trackers[0].lm)

    def set_frame(self, gt_color, gt_depth=None, grad_mask=None, w2c=None, edge_threshold=None, grad_blocks=False):
        """GaussNewtonTracker.set_frame, then the pyramid of the frame in one launch.  A given grad_mask is OR-reduced with the
        images; with edge_threshold every level's mask is computed by gsaj.grad_mask on that level's colour: the gradient is taken
        at that scale.  w2c: the start pose; the solve starts at the coarsest level."""
        t0 = self.trackers[0]
        t0.set_frame(gt_color, gt_depth, grad_mask, None, edge_threshold, grad_blocks)
        if self.levels:
            given = grad_mask is not None
            if self.pyramid is None:
                self.pyramid = ImagePyramid(self.W, self.H, self.levels, self.dev, has_depth=t0.gt_depth is not None, has_mask=given)
                for l in range(1, self.levels + 1):   # the coarse levels read the pyramid's planes in place
                    self.trackers[l].frame_views(self.pyramid.color(l), self.pyramid.depth(l) if t0.gt_depth is not None else None,
                                                 self.pyramid.mask(l) if given else None, own_mask=edge_threshold is not None)
            self.pyramid.build(t0.gt_color, t0.gt_depth, t0.grad_mask if given else None, self.depth_edge_ratio)
            if not given and edge_threshold is not None:
                for t in self.trackers[1:]:
                    t.compute_mask(edge_threshold, grad_blocks)
        if w2c is not None:
            self.trackers[-1].reset(w2c)
            self._at = self.levels

    def relevel(self, level, skip=None):
        """The shared state to level `level`'s camera, on the device (gsaj_pose_gn_relevel)."""
        if not 0 <= int(level) <= self.levels:
            raise _lib.GsajError("PyramidGaussNewtonTracker: level %r is not one of 0..%d" % (level, self.levels))
        _relevel(self, int(level), skip)
        self._at = int(level)

    def iterate(self, schedule, check_every=0):
        """schedule: the iteration counts from the coarsest level to level 0 (levels + 1 of them; levels=0: a number will do).  Every
        level runs GaussNewtonTracker's iteration with its own context; between levels the state is re-levelled on the device, with
        the abort word of the level just finished as the skip word.  No host read but what check_every (per level: on to the next
        level once the device reports convergence) and the first, arena-sizing iteration of each level imply.  Returns the numbers
        run per level.  Raises GsajError after the loop if an asynchronous frame of any level was aborted on the device; the state is
        then what it was before the call, and the next call re-sizes that level's arena with one synchronous iteration."""
        if self.trackers[0].gt_color is None:
            raise _lib.GsajError("set_frame() first")
        if self.levels == 0:
            n = schedule[0] if isinstance(schedule, (list, tuple)) and len(schedule) == 1 else schedule
            done = self.trackers[0].iterate(n, check_every)
            self.iterations += done
            return [done]
        schedule = check_schedule(schedule, self.levels, "iterate")
        self._snapshot.copy_(self.state)
        done, prev, at = [], None, self._at
        for l, n in zip(range(self.levels, -1, -1), schedule):
            k = 0
            if n:   # (a level with no iterations is passed over: the state goes straight to the next level that has some)
                t = self.trackers[l]
                if self._at != l:
                    self.relevel(l, None if prev is None else prev._abort_ptr)
                k = run(n, check_every, lambda: _level_iteration(t, t.ctx.capacity == 0), lambda: self.converged)
                t.iterations += k
                prev = t
            done.append(k)
        self.iterations += sum(done)
        errors = []
        for l, k in zip(range(self.levels, -1, -1), done):
            if k:
                try:
                    finish_frame(self.trackers[l].ctx)
                except _lib.GsajError as e:
                    errors.append("level %d: %s" % (l, e))
        if errors:
            self.state.copy_(self._snapshot)
            self._at = at
            raise _lib.GsajError("; ".join(errors))
        return done
