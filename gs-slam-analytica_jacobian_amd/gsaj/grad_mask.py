"""The tracking gradient mask of a frame, on the device (C ABI gsaj_grad_intensity / gsaj_grad_mask, csrc/frame.hip).

What the reference's front end computes once per incoming frame with Camera.compute_grad_mask (utils/camera_utils.py:115-144, on
image_gradient / image_gradient_mask of utils/slam_utils.py:4-38): the pixels whose Scharr gradient intensity exceeds
edge_threshold times the median intensity -- of the whole frame, or, for dataset type "replica", of each block of a 32 x 32 grid.
include/gsaj.h states the arithmetic and the reference's quirks.  Inputs are fp32 device tensors; there is no CPU path and no
host synchronisation.
"""
import torch

from . import _lib


class GradMask:
    """Pre-allocated for one image size.  mask = GradMask(W, H, device)(image, edge_threshold, blocks=False) -> uint8 [1,H,W], the
    byte mask LossSeeds / DeviceTracker read; reference_tensor() -> what the reference would have left in Camera.grad_mask for the
    last call (bool [1,H,W], or float [1,H,W] in block mode).  The returned tensors are buffers this object owns (unless `out` is
    given) and are overwritten by the next call."""

    def __init__(self, W, H, device):
        self.lib = _lib.load()
        self.W, self.H, self.dev = int(W), int(H), torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.GsajError("GradMask needs a HIP device (there is no CPU path)")
        if self.W < 2 or self.H < 2:
            raise _lib.GsajError("GradMask needs W >= 2 and H >= 2 (got W=%d H=%d): the image is reflect-padded" % (self.W, self.H))
        self.ws = torch.empty(self.lib.gsaj_grad_mask_workspace_bytes(self.W, self.H), dtype=torch.uint8, device=self.dev)
        self.u8 = torch.empty((1, self.H, self.W), dtype=torch.uint8, device=self.dev)
        self.f32 = None  # block mode's float image, allocated by the first call that needs it
        self._last = None

    def _image(self, image):
        if not torch.is_tensor(image) or image.device.type != "cuda":
            raise _lib.GsajError("image must be a HIP device tensor (there is no CPU path)")
        if image.dtype != torch.float32 or tuple(image.shape) != (3, self.H, self.W):
            raise _lib.GsajError("image must be float32 [3,%d,%d] (got %s %s)" % (self.H, self.W, image.dtype, tuple(image.shape)))
        return image.detach().contiguous()

    def __call__(self, image, edge_threshold, blocks=False, out=None):
        img = self._image(image)
        if out is None:
            out = self.u8
        elif (not torch.is_tensor(out) or out.device != img.device or out.dtype != torch.uint8 or not out.is_contiguous()
              or out.numel() != self.H * self.W):
            raise _lib.GsajError("out must be a contiguous uint8 tensor of %d elements on %s" % (self.H * self.W, img.device))
        if blocks and self.f32 is None:
            self.f32 = torch.empty((1, self.H, self.W), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_grad_mask(self.W, self.H, img.data_ptr(), float(edge_threshold), int(bool(blocks)), out.data_ptr(),
                                               self.f32.data_ptr() if blocks else None, self.ws.data_ptr(),
                                               torch.cuda.current_stream(self.dev).cuda_stream), "gsaj_grad_mask")
        self._last = (out, bool(blocks))
        return out.view(1, self.H, self.W)

    def reference_tensor(self):
        """Camera.grad_mask of the reference for the last call: bool [1,H,W] (a view of the byte mask), float [1,H,W] in block mode."""
        if self._last is None:
            raise _lib.GsajError("reference_tensor(): call the GradMask first")
        out, blocks = self._last
        return self.f32 if blocks else out.view(1, self.H, self.W).view(torch.bool)

    def intensity(self, image):
        """sqrt(gv^2 + gh^2) of the validity-masked Scharr gradients of the gray image: float32 [1,H,W] (a new tensor)."""
        img = self._image(image)
        out = torch.empty((1, self.H, self.W), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_grad_intensity(self.W, self.H, img.data_ptr(), out.data_ptr(),
                                                    torch.cuda.current_stream(self.dev).cuda_stream), "gsaj_grad_intensity")
        return out
