"""The mapping loop of a keyframe window kept on the device: the counterpart of gsaj.tracking.DeviceTracker for BackEnd.map
(reference utils/slam_backend.py:142-318).

The reference's backend renders every keyframe of the window and up to two extra keyframes against ONE map, sums
get_loss_mapping over them, adds the isotropic regulariser, calls backward(), updates the densification statistics, steps the
keyframe optimiser (poses of the first `pose_window` window keyframes, exposures) and the Gaussians' optimiser.  Here one
iteration is a fixed sequence of C-ABI calls that read no host state:

  1. the model's activated getters (torch, no_grad)
  2. BatchContext.forward_loss      the K views + every view's mapping loss summed inside the forward compositor       (fused=True)
  3. BatchContext.backward_loss     the reverse compositor derives its pixel seeds itself: no [K,3,H,W] / [K,1,H,W] seed images
  4. IsotropicLoss(accumulate=True) weight x mean|s - mean(s)| added into g["scale"]
  5. model.densification_step       xyz_gradient_accum / denom / max_radii2D of all K views, n_obs of the window's views
  6. PoseTrackerBatch.step          dL/dtau rows, dL/d(exposure) [K,2], the active mask, the views' abort words as `skip`
  7. model.map_step                 chain rule + Adam on the six raw parameters, optionally with an opacity reset
  8. model.update_learning_rate(iteration_count)

fused=False, the default, has steps 2-3 as forward -> LossSeedsBatch -> backward (the seed images exist, the loss is a pass of its
own, the exposure columns and scalars[:, 3:5] are copied into contiguous tensors every iteration): the same per-pixel arithmetic, so
the map and the poses follow the fused loop bit for bit as long as the exposures are not learned (dL/d(exposure) is a sum of pixel
terms in another order).  Why the default is the unfused form (tools/mapper_iter_bench.py, profiles/r14_device_mapper.json, MI355X,
windows of 8): at cfg2 the fused iteration is 0.0035 ms faster (0.8257 against 0.8292 ms), at cfg5 it is 0.0176 ms slower (4.8726
against 4.8550 ms), which is more than the 0.0048 ms the unfused blocks spread over -- and a form that is measurably slower somewhere
is not the default.  fused=True is there for what it saves either way: the seed images (39 MB at cfg2, 118 MB at cfg5) and three
launches per iteration.

The first iteration after construction or refresh() runs one synchronous forward that sizes the binning arena; after that an
iteration contains no device-to-host read.  iterate() ends with ONE read: the views' abort counters.  A view whose instances did
not fit the arena was aborted on the device: it added nothing to any gradient sum, its rows of the loss scalars kept their previous
values, and its pose was skipped (no Adam moment, no pose change); the map was still stepped with the other views' gradients.
iterate() then raises GsajError and the next call re-sizes the arena with a synchronous forward.

Not captured into a graph: map_step's Adam scalars (step counts, learning rates) live on the host.  Densification and
pruning stay the caller's calls (they have a designed host read); call refresh() after them.
"""
import torch

from . import _lib
from ._loop import ViewTargets, finish_window, loss_description, loss_terms, require_device
from .losses import NO_EXPOSURE, IsotropicLoss, LossSeedsBatch
from .pose_step import PoseTracker, PoseTrackerBatch
from .rasterizer import BatchContext


class DeviceMapper(ViewTargets):
    def __init__(self, model, K, W, H, projection_matrix, tanfovx, tanfovy, bg, device=None, w2cs=None, n_window=None, uids=None,
                 pose_window=3, monocular=False, alpha=0.95, rgb_boundary_threshold=0.01, isotropic_weight=10.0, fused=False,
                 streams=1, split=False, record_bits=32, **pose_kw):
        """model: a GaussianModel with training_setup() done (the mapper reads its activated getters and steps it).
        K views = the window's n_window keyframes (slots 0 .. n_window-1, default all K) followed by the extra keyframes the
        reference draws from outside the window (slam_backend.py:200-227); uids: the keyframes' uids per slot (default: the slot
        numbers) -- the keyframe with uid 0 anchors the map and is never moved.  Poses and exposures of the first `pose_window`
        window slots are optimised (one mask for both: PoseTrackerBatch steps a view's pose and exposure together); extras never.
        pose_kw: learning rates / betas / eps of PoseTrackerBatch.  streams / split: as BatchContext."""
        self.dev = require_device(model.get_xyz.device if device is None else device, "DeviceMapper")
        self.model, self.K, self.W, self.H = model, int(K), int(W), int(H)
        self.n_window = self.K if n_window is None else int(n_window)
        if not 0 < self.n_window <= self.K or self.K - self.n_window > 2:
            raise _lib.GsajError("DeviceMapper: K = %d views must be n_window keyframes plus at most two extra ones, got n_window = %d"
                                 % (self.K, self.n_window))
        self.uids = list(range(self.K)) if uids is None else [int(u) for u in uids]
        if len(self.uids) != self.K:
            raise _lib.GsajError("DeviceMapper: uids must name all %d slots" % self.K)
        self.tanfov = (float(tanfovx), float(tanfovy))
        self.bg = bg.to(self.dev, torch.float32).contiguous()
        (self.flags, self.alpha, self.thr), self.iso_weight = loss_terms(monocular, alpha, rgb_boundary_threshold), float(isotropic_weight)
        self.fused, self.split, self._streams, self._record_bits = bool(fused), bool(split), int(streams), int(record_bits)
        f = dict(dtype=torch.float32, device=self.dev)
        self._alloc_views(monocular)
        eye = torch.eye(4)
        self._pose_args = (projection_matrix, pose_kw)
        self.poses = PoseTrackerBatch([eye] * self.K if w2cs is None else list(w2cs), projection_matrix, self.dev, **pose_kw)
        self.praw = self.poses.projection
        self.active = torch.tensor([1 if s < min(int(pose_window), self.n_window) and self.uids[s] != 0 else 0 for s in range(self.K)],
                                   dtype=torch.uint8, device=self.dev)
        self.scalars = torch.zeros((self.K, 5), **f)     # per view: loss, L_rgb, L_depth, dL/da, dL/db
        self.dexposure = torch.zeros((self.K, 2), **f)   # per view: dL/da, dL/db, contiguous for the pose step
        self.seeds = None if self.fused else LossSeedsBatch(self.K, self.W, self.H, self.dev)
        if self.seeds is not None:
            self.seeds.scalars = self.scalars
        self.iteration_count = 0   # what update_learning_rate is given (slam_backend.py:311); the caller may set it
        self.refresh()

    def refresh(self):
        """After the caller densified or pruned the model: the P-sized buffers (rasteriser context, gradient bucket, regulariser
        workspace) are allocated again for the model's new size; ground truth, poses and Adam state of the poses stay.  The next
        iteration runs the synchronous forward that sizes the arena."""
        m = self.model
        if m.optimizer is None:
            raise _lib.GsajError("DeviceMapper: the model has no optimizer (training_setup)")
        self.P, self.M = int(m.get_xyz.shape[0]), int(m.get_features.shape[1])
        if getattr(m, "max_radii2D", None) is None or m.max_radii2D.numel() != self.P:  # (a model built from tensors has none yet)
            m.max_radii2D = torch.zeros((self.P,), device=self.dev)
        self.ctx = BatchContext(self.K, self.P, self.W, self.H, self.M, self.dev, record_bits=self._record_bits, streams=self._streams)
        self.iso = IsotropicLoss(self.P, self.dev)
        self._sized = False

    def set_view(self, slot, gt_color, gt_depth=None, w2c=None, exposure=None):
        """Slot `slot` shows another keyframe: its ground truth ([3,H,W], [H,W]) is copied into the mapper's own buffers; w2c
        (and exposure = (a, b)) given: the slot's pose state starts afresh from them, Adam moments zero."""
        slot = self._take_view(slot, gt_color, gt_depth)
        if w2c is not None:
            one = PoseTracker(w2c, self._pose_args[0], self.dev, **self._pose_args[1])  # (initialises the row as the batch's were)
            if exposure is not None:
                one.reset(w2c, exposure)
            self.poses.state[slot].copy_(one.state)
        elif exposure is not None:
            self.poses.exposure[slot, 0], self.poses.exposure[slot, 1] = float(exposure[0]), float(exposure[1])

    # ---- one iteration --------------------------------------------------------------------------------------------------
    def _iteration(self, reset, initialization):
        m, c, p = self.model, self.ctx, self.poses
        tx, ty = self.tanfov
        with torch.no_grad():  # 1. the activations of gaussian_model.py:141-177
            xyz, opac = m.get_xyz.detach().contiguous(), m.get_opacity.contiguous()
            geo = dict(sh_degree=m.active_sh_degree, shs=m.get_features.contiguous(), scales=m.get_scaling.contiguous(),
                       rotations=m.get_rotation.contiguous())
        views, projs, cps = p.matrices()
        flags = self.flags | (NO_EXPOSURE if initialization else 0)
        if not self._sized:  # the synchronous forward that sizes the arena
            c.forward(self.bg, xyz, opac, views, projs, cps, tx, ty, sync=True, **geo)
            self._sized = True
            rendered = True
        else:
            rendered = False
        if self.fused:  # 2., 3.
            L = loss_description(self, None if initialization else p.exposure[:, 0], None if initialization else p.exposure[:, 1],
                                 flags=flags, masked=False, exposure_stride=p.state.stride(0), scalars=self.scalars, dexposure=self.dexposure)
            c.forward_loss(L, self.bg, xyz, opac, views, projs, cps, tx, ty, **geo)
            g = c.backward_loss(L, self.bg, xyz, views, projs, self.praw, cps, tx, ty, split=self.split, **geo)
            dexp = self.dexposure
        else:
            if not rendered:
                c.forward(self.bg, xyz, opac, views, projs, cps, tx, ty, sync=False, **geo)
            o = self.seeds(flags, self.alpha, self.thr, c.color, c.depth, c.opacity, self.gt_color, self.gt_depth, None,
                           None if initialization else p.exposure[:, 0].contiguous(), None if initialization else p.exposure[:, 1].contiguous())
            g = c.backward(self.bg, xyz, views, projs, self.praw, cps, tx, ty, o["dL_dcolor"], o["dL_ddepth"], split=self.split, **geo)
            dexp = self.scalars[:, 3:5].contiguous()
        # (multi-GPU windows, one shard of keyframes per rank: the all-reduce of the gradient bucket -- c.bucket, whose tail holds
        # the dL/dtau rows -- would sit here, between the backward and everything that consumes the summed gradients)
        self.iso(geo["scales"], self.iso_weight, grad_out=g["scale"], accumulate=True)  # 4.
        nw = self.n_window
        m.densification_step(g["mean2D"][:nw], c.radii[:nw], c.n_touched[:nw])  # 5. (n_obs counts the window's views only)
        if nw < self.K:
            m.densification_step(g["mean2D"][nw:], c.radii[nw:], None)
        skip, skip_stride = c.abort_flags()
        p.step(g["tau_all"], dexp, self.active, skip=skip, skip_stride=skip_stride)  # 6.
        m.map_step(g, reset=reset, radii=c.radii)  # 7.
        self.iteration_count += 1
        m.update_learning_rate(self.iteration_count)  # 8.

    def iterate(self, n, reset=None, initialization=False):
        """n mapping iterations.  reset: None, or the opacity reset ("all", "nonvisible", "nonvisible_keep": GaussianModel.map_step)
        fused into the LAST iteration's step, as the reference resets once per call of map() at most.  initialization: the
        exposure is left out of the loss (get_loss_mapping(initialization=True)).  Raises GsajError if a view was aborted on the
        device during the call (module docstring) or if the model's size changed without refresh()."""
        if int(self.model.get_xyz.shape[0]) != self.P:
            raise _lib.GsajError("DeviceMapper: the model has %d Gaussians, the mapper's buffers are for %d; call refresh() after "
                                 "densifying or pruning" % (int(self.model.get_xyz.shape[0]), self.P))
        with torch.cuda.device(self.dev):
            for i in range(int(n)):
                self._iteration(reset if i == int(n) - 1 else None, initialization)
            try:
                finish_window(self.ctx, "those views added nothing to the gradient sums and their poses were skipped")
            except _lib.GsajError:
                self._sized = False  # the next call re-sizes with one synchronous forward
                raise
        return int(n)

    # ---- results (device tensors; reading them is the caller's synchronisation) ------------------------------------------
    @property
    def losses(self):
        """[K,5] per view: loss, L_rgb, L_depth, dL/da, dL/db of the last iteration."""
        return self.scalars

    @property
    def window_loss(self):
        """Device scalar: the sum of the K views' mapping losses of the last iteration (without the isotropic term: self.iso.loss)."""
        return self.scalars[:, 0].sum()

    @property
    def n_touched(self):
        """[K,P] int32: per view, how many pixels each Gaussian touched in the last forward."""
        return self.ctx.n_touched

    @property
    def w2c(self):
        return self.poses.w2c

    @property
    def exposure(self):
        return self.poses.exposure
