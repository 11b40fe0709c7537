"""SSIM and L1 with the reference's signatures, on the device (C ABI gsaj_ssim_forward / gsaj_ssim_backward).

Mirrors reference gaussian_splatting/utils/loss_utils.py:21-101: `ssim(img1, img2, window_size=11, size_average=True)` --
11x11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2, C2 = 0.03^2 -- and `l1_loss(a, b)`.  `ssim` is an autograd
function whose forward and backward are two HIP kernels (csrc/ssim.hip); it differentiates w.r.t. img1 only.  Inputs are
[C,H,W] or [N,C,H,W] fp32 device tensors.  There is no CPU fallback: anything outside the kernels' domain raises GsajError.
"""
import torch

from . import _lib

_WS = {}  # (device, N, C, H, W) -> [zeroed workspace (holds the reduction ticket, reset by the kernels), forward count]


def _forward(lib, a, b, out, m):
    """gsaj_ssim_forward on the cached workspace of a's shape; returns (workspace entry, its forward count after this call)."""
    N, C, H, W = a.shape
    key = (str(a.device), N, C, H, W)
    ent = _WS.get(key)
    if ent is None:
        ent = [torch.zeros(lib.gsaj_ssim_workspace_bytes(N, C, W, H), dtype=torch.uint8, device=a.device), 0]
        _WS[key] = ent
    _lib.check(lib.gsaj_ssim_forward(N, C, W, H, a.data_ptr(), b.data_ptr(), out.data_ptr(), None if m is None else m.data_ptr(),
                                     ent[0].data_ptr(), torch.cuda.current_stream(a.device).cuda_stream), "gsaj_ssim_forward")
    ent[1] += 1
    return ent, ent[1]


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        out = torch.empty(img1.shape[0] + 1, dtype=torch.float32, device=img1.device)
        ctx.ent, ctx.gen = _forward(_lib.load(), img1, img2, out, None)
        ctx.save_for_backward(img1, img2)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        img1, img2 = ctx.saved_tensors
        lib = _lib.load()
        N, C, H, W = img1.shape
        g = grad_out.to(dtype=torch.float32).contiguous()
        dimg = torch.empty_like(img1)
        # the workspace holds the partial maps of the LAST forward of this shape: if another one ran since ours, redo ours (one
        # cheap kernel), so the gradient is right whatever the order of forward and backward calls
        if ctx.ent[1] != ctx.gen:
            ctx.ent, ctx.gen = _forward(lib, img1, img2, torch.empty(N + 1, dtype=torch.float32, device=img1.device), None)
        _lib.check(lib.gsaj_ssim_backward(N, C, W, H, img1.data_ptr(), img2.data_ptr(), g.data_ptr(), dimg.data_ptr(), ctx.ent[0].data_ptr(),
                                          torch.cuda.current_stream(img1.device).cuda_stream), "gsaj_ssim_backward")
        return dimg, None


def _check(img1, img2, window_size):
    for name, t in (("img1", img1), ("img2", img2)):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise _lib.GsajError("ssim: %s must be a HIP device tensor (there is no CPU path)" % name)
        if t.dtype != torch.float32:
            raise _lib.GsajError("ssim: %s must be float32 (got %s)" % (name, t.dtype))
        if t.dim() not in (3, 4):
            raise _lib.GsajError("ssim: %s must be [C,H,W] or [N,C,H,W] (got %s)" % (name, tuple(t.shape)))
    if int(window_size) != 11:
        raise _lib.GsajError("ssim: only window_size=11 is implemented (got %s)" % window_size)
    if img1.shape != img2.shape or img1.device != img2.device:
        raise _lib.GsajError("ssim: img1 and img2 must have the same shape and device (%s on %s, %s on %s)"
                             % (tuple(img1.shape), img1.device, tuple(img2.shape), img2.device))
    if img2.requires_grad:
        raise _lib.GsajError("ssim: the gradient w.r.t. img2 is not implemented; pass img2 detached")
    if min(img1.shape) < 1:
        raise _lib.GsajError("ssim: empty input %s" % (tuple(img1.shape),))


def ssim(img1, img2, window_size=11, size_average=True):
    """loss_utils.ssim: mean SSIM (size_average=True, a 0-d tensor) or, for [N,C,H,W] input, the per-image means [N]."""
    _check(img1, img2, window_size)
    four_d = img1.dim() == 4
    if not size_average and not four_d:
        # the reference reduces ssim_map.mean(1).mean(1).mean(1), which fails on a 3-D map
        raise _lib.GsajError("ssim: size_average=False needs [N,C,H,W] input")
    a = (img1 if four_d else img1.unsqueeze(0)).contiguous()
    b = (img2 if four_d else img2.unsqueeze(0)).contiguous()
    out = _SSIM.apply(a, b)
    return out[-1] if size_average else out[:-1]


def ssim_map(img1, img2):
    """The per-pixel SSIM map (what _ssim averages), same shape as img1; no autograd."""
    _check(img1, img2, 11)
    lib = _lib.load()
    a = (img1 if img1.dim() == 4 else img1.unsqueeze(0)).detach().contiguous()
    b = (img2 if img2.dim() == 4 else img2.unsqueeze(0)).detach().contiguous()
    m = torch.empty_like(a)
    _forward(lib, a, b, torch.empty(a.shape[0] + 1, dtype=torch.float32, device=a.device), m)
    return m.view(img1.shape)


def l1_loss(network_output, gt):
    """loss_utils.l1_loss."""
    return torch.abs((network_output - gt)).mean()
