"""What the device loops share (DESIGN.md "Device loops"): DeviceTracker, GaussNewtonTracker, GaussNewtonWindow,
PyramidGaussNewtonTracker, DeviceMapper and RgbdAligner each drive their own sequence of C-ABI calls; the frame they are aimed at, the
loss description the contexts read, the counted loop and the end of iterate() are defined here once, beside the device check, the
current HIP stream and the six optional map arguments."""
import torch

from . import _lib
from .grad_mask import GradMask
from .losses import MONOCULAR


def require_device(device, who):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GsajError("%s needs a HIP device (there is no CPU path)" % who)
    return dev


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def map_args(sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
    return dict(sh_degree=sh_degree, shs=shs, colors_precomp=colors_precomp, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)


def loss_terms(monocular, alpha, rgb_boundary_threshold, irls_delta=None, flags=0):
    """(flags, alpha, thr) as the loops store them, (flags, alpha, thr, delta) where irls_delta is taken."""
    return (flags | (MONOCULAR if monocular else 0), float(alpha), float(rgb_boundary_threshold)) + (() if irls_delta is None else (float(irls_delta),))


def loss_description(loop, exposure_a, exposure_b, flags=0, masked=True, **more):
    """The dictionary _Context._loss reads.  more: exposure_stride, scalars, dexposure; masked=False: a loop without gradient masks."""
    if masked:
        more["grad_mask"] = loop.grad_mask
    return dict(flags=loop.flags | flags, alpha=loop.alpha, rgb_boundary_threshold=loop.thr, gt_color=loop.gt_color, gt_depth=loop.gt_depth,
                exposure_a=exposure_a, exposure_b=exposure_b, **more)


class FrameTarget:
    """The frame of a single-frame loop, in the loop's own gt_color, gt_depth, grad_mask, _grad_op (None before the first frame).
    The buffers' addresses are fixed from the first frame on.  _start_pose(w2c) is the loop's: a new start pose, in place."""

    def set_frame(self, gt_color, gt_depth=None, grad_mask=None, w2c=None, edge_threshold=None, grad_blocks=False):
        """New frame: ground truth (device, [3,H,W] / [H,W]; grad_mask [1,H,W] or None) and optionally a new initial pose.
        Everything is copied into buffers the tracker owns, so a captured graph stays valid from frame to frame.
        edge_threshold (with grad_mask None): the tracker computes the frame's gradient mask itself (gsaj.grad_mask: the reference's
        Camera.compute_grad_mask; grad_blocks=True: its "replica" block form) from its own copy of gt_color into its own mask
        buffer, on the current stream.  A mask, given or computed, is there for every frame of a tracker or for none."""
        masked = grad_mask is not None or edge_threshold is not None
        if self.gt_color is None:
            self.gt_color = gt_color.to(self.dev, torch.float32).contiguous().clone()
            self.gt_depth = None if gt_depth is None else gt_depth.to(self.dev, torch.float32).contiguous().clone()
            if grad_mask is not None:
                self.grad_mask = grad_mask.to(self.dev, torch.uint8).contiguous().view(-1).clone()
            elif masked:
                self.grad_mask = torch.empty(self.gt_color[0].numel(), dtype=torch.uint8, device=self.dev)
        else:
            if (gt_depth is None) != (self.gt_depth is None) or masked != (self.grad_mask is not None):
                raise _lib.GsajError("set_frame: depth / mask must be given for every frame of a tracker or for none")
            self.gt_color.copy_(gt_color)
            if gt_depth is not None:
                self.gt_depth.copy_(gt_depth)
            if grad_mask is not None:
                self.grad_mask.copy_(grad_mask.to(self.dev, torch.uint8).view(-1))
        if grad_mask is None and masked:
            self.compute_mask(edge_threshold, grad_blocks)
        if w2c is not None:
            self._start_pose(w2c)

    def compute_mask(self, edge_threshold, grad_blocks=False):
        """The gradient mask of gt_color into the loop's own mask buffer (the GradMask is made by the first call)."""
        if self._grad_op is None:
            _, H, W = self.gt_color.shape
            self._grad_op = GradMask(W, H, self.dev)
        self._grad_op(self.gt_color, edge_threshold, blocks=grad_blocks, out=self.grad_mask)

    def frame_views(self, gt_color, gt_depth, grad_mask=None, own_mask=False):
        """Someone else's buffers as this loop's frame, read in place; own_mask (no mask given): a mask buffer for compute_mask."""
        self.gt_color, self.gt_depth = gt_color, gt_depth
        if grad_mask is not None or own_mask:
            self.grad_mask = torch.empty(gt_color[0].numel(), dtype=torch.uint8, device=self.dev) if grad_mask is None else grad_mask.view(-1)


class ViewTargets:
    """The frames of a K-view loop: gt_color [K,3,H,W] and gt_depth [K,H,W] (None: monocular) of the loop itself, beside its K, W, H."""

    def _alloc_views(self, monocular):
        self.gt_color = torch.zeros((self.K, 3, self.H, self.W), dtype=torch.float32, device=self.dev)
        self.gt_depth = None if monocular else torch.zeros((self.K, self.H, self.W), dtype=torch.float32, device=self.dev)

    def _take_view(self, slot, gt_color, gt_depth):
        """The checked copy of one view's ground truth into slot `slot`; returns the slot as an int."""
        k, H, W = check_slot(slot, self.K, "set_view"), self.H, self.W
        if tuple(gt_color.shape) != (3, H, W):
            raise _lib.GsajError("set_view: gt_color must be [3,%d,%d], got %r" % (H, W, tuple(gt_color.shape)))
        if (gt_depth is None) != (self.gt_depth is None):
            raise _lib.GsajError("set_view: a monocular window takes no depth, every other window needs it")
        if gt_depth is not None and gt_depth.numel() != H * W:
            raise _lib.GsajError("set_view: gt_depth must have %d elements, got %d" % (H * W, gt_depth.numel()))
        self.gt_color[k].copy_(gt_color)
        if gt_depth is not None:
            self.gt_depth[k].copy_(gt_depth.reshape(H, W))
        return k


def check_slot(slot, K, who):
    if not 0 <= int(slot) < K:
        raise _lib.GsajError("%s: slot %r is not one of the window's %d" % (who, slot, K))
    return int(slot)


def run(n, check_every, one_iteration, converged):
    """Up to n calls of one_iteration(), stopped once converged() -- a device scalar, read every check_every > 0 iterations -- is set."""
    done = 0
    while done < n:
        one_iteration()
        done += 1
        if check_every and done % check_every == 0 and bool(converged().item() != 0.0):
            break
    return done


def finish_frame(ctx):
    """The end of iterate() on a FrameContext.  If an asynchronous frame did not fit the arena sized earlier (the view moved onto
    more Gaussians), those iterations rendered nothing and moved nothing (the step skips an aborted frame).  The next call re-sizes
    with one synchronous iteration; the caller sees the error and decides."""
    try:
        ctx.status()
    except _lib.GsajError:
        ctx.capacity = 0
        raise


def finish_window(ctx, consequence):
    """The end of iterate() on a BatchContext: ONE read of the views' abort counters.  consequence: what the aborted views missed."""
    aborted = ctx.clear_aborts()
    if aborted:
        raise _lib.GsajError("%d asynchronous forward(s) of the window were aborted on the device (binning arena too small for a view's "
                             "instances): %s" % (aborted, consequence))
