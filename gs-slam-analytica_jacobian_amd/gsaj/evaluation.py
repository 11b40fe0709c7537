"""Rendering quality and trajectory error: what the reference's utils/eval_utils.py measures.

FrameEvaluator -- per frame, masked PSNR of the clamped render, SSIM and optionally the 8-bit picture (C ABI gsaj_eval_frame,
csrc/eval.hip: three launches, no host read).  Rows collect in a device table; rows() makes the one blocking copy.  There is no
CPU path: anything outside the kernels' domain raises GsajError.

umeyama / ate -- host NumPy in fp64: the estimated positions aligned to the ground truth by Umeyama's closed form (IEEE PAMI 13(4),
1991, eqs. 34-43, the reflection fix included), then the statistics of the per-pose translation error under the keys evo's
APE.get_all_statistics writes.  evo itself is not used (and its output is not what the tests pin: they pin the closed form).
"""
import numpy as np
import torch

from . import _lib
from ._lib import GsajError

REVERSE_CHANNELS = 1  # GSAJ_EVAL_REVERSE_CHANNELS
_DEVICE_TYPES = ("cuda",)  # (host-logic tests add "cpu" and replace _launch)


def _launch(C, W, H, flags, image, gt, row, count, u8, ws):
    """gsaj_eval_frame on the current stream (the one call that needs the device).  row: [4] fp32 view, count: [1] int32 view."""
    dev = image.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsaj_eval_frame(C, W, H, int(flags), image.data_ptr(), gt.data_ptr(), row.data_ptr(), count.data_ptr(),
                                               None if u8 is None else u8.data_ptr(), ws.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream), "gsaj_eval_frame")


def _workspace_bytes(C, W, H):
    return int(_lib.load().gsaj_eval_workspace_bytes(C, W, H))


class FrameEvaluator:
    """FrameEvaluator(W, H, device, C=3, capacity=256): one workspace and ONE device table [capacity, 5]: {psnr, ssim, mse, masked
    fraction} as fp32 and, in the fifth word, the masked element count's uint32 bits, so that one copy brings everything to the host;
    add() appends a row on the current stream."""

    def __init__(self, W, H, device, C=3, capacity=256):
        self.device = torch.device(device)
        if self.device.type not in _DEVICE_TYPES:
            raise GsajError("FrameEvaluator: %s is not a HIP device (there is no CPU path)" % (self.device,))
        self.W, self.H, self.C = int(W), int(H), int(C)
        if min(self.W, self.H, self.C) < 1 or int(capacity) < 1:
            raise GsajError("FrameEvaluator: W, H, C and capacity must be >= 1 (got %d, %d, %d, %d)" % (self.W, self.H, self.C, capacity))
        nbytes = _workspace_bytes(self.C, self.W, self.H)
        if nbytes <= 0:
            raise GsajError("FrameEvaluator: C * W * H = %d * %d * %d exceeds what gsaj_eval_frame takes" % (self.C, self.W, self.H))
        self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)  # zeroed once: the SSIM slice holds a ticket
        self._table = torch.zeros((int(capacity), 5), dtype=torch.float32, device=self.device)
        self.n = 0

    @property
    def capacity(self):
        return self._table.shape[0]

    def _check(self, t, name, dtype, shape):
        if not torch.is_tensor(t) or t.device.type not in _DEVICE_TYPES:
            raise GsajError("FrameEvaluator.add: %s must be a HIP device tensor (there is no CPU path)" % name)
        if t.device != self._ws.device:
            raise GsajError("FrameEvaluator.add: %s is on %s, the evaluator on %s" % (name, t.device, self._ws.device))
        if t.dtype != dtype:
            raise GsajError("FrameEvaluator.add: %s must be %s (got %s)" % (name, dtype, t.dtype))
        if tuple(t.shape) != shape:
            raise GsajError("FrameEvaluator.add: %s must have shape %s (got %s)" % (name, shape, tuple(t.shape)))
        if not t.is_contiguous():
            raise GsajError("FrameEvaluator.add: %s must be contiguous" % name)

    def _grow(self):
        cap = self.capacity
        table = torch.zeros((2 * cap, 5), dtype=torch.float32, device=self._table.device)
        table[:cap].copy_(self._table)  # a device copy on the current stream, behind the rows' launches
        self._table = table

    def add(self, image, gt, u8_out=None, reverse_channels=False):
        """One frame: image (the render, clamped by the kernel) and gt, [C,H,W] fp32 -> the index of its row.  u8_out [H,W,C] uint8
        gets the 8-bit picture, its channels reversed with reverse_channels.  Nothing is read back."""
        shape = (self.C, self.H, self.W)
        self._check(image, "image", torch.float32, shape)
        self._check(gt, "gt", torch.float32, shape)
        if u8_out is not None:
            self._check(u8_out, "u8_out", torch.uint8, (self.H, self.W, self.C))
        elif reverse_channels:
            raise GsajError("FrameEvaluator.add: reverse_channels without u8_out")
        if self.n == self.capacity:
            self._grow()
        i = self.n
        _launch(self.C, self.W, self.H, REVERSE_CHANNELS if reverse_channels else 0, image.detach(), gt.detach(), self._table[i, :4],
                self._table[i, 4:].view(torch.int32), u8_out, self._ws)
        self.n = i + 1
        return i

    def clamped(self):
        """clamp(image, 0, 1) of the last add, [C,H,W]: a view of the workspace, overwritten by the next add (for a perceptual
        metric handed in by the caller, and for the parity tests)."""
        off = (-self._ws.data_ptr()) % 256
        nbytes = 4 * self.C * self.H * self.W
        return self._ws[off:off + nbytes].view(torch.float32).view(self.C, self.H, self.W)

    def rows(self):
        """The one blocking copy: (table [n,4] float32 = psnr, ssim, mse, masked fraction; counts [n] uint32)."""
        h = self._table[:self.n].cpu().numpy()
        return np.ascontiguousarray(h[:, :4]), np.ascontiguousarray(h[:, 4]).view(np.uint32)

    def summary(self):
        """{"mean_psnr", "mean_ssim", "psnr", "ssim", "mse", "count"}: the means as float(np.mean(...)) over the per-frame fp32
        values taken to Python floats, as the reference forms them from its .item() lists (no frame: NaN, as np.mean([]))."""
        t, c = self.rows()
        psnr, ssim = [float(v) for v in t[:, 0]], [float(v) for v in t[:, 1]]
        mean = lambda v: float(np.mean(v)) if v else float("nan")  # noqa: E731
        return dict(mean_psnr=mean(psnr), mean_ssim=mean(ssim), psnr=psnr, ssim=ssim, mse=[float(v) for v in t[:, 2]],
                    count=[int(v) for v in c])


# ---- trajectory error -------------------------------------------------------------------------------------------------------------
def umeyama(x, y, with_scale):
    """Least-squares similarity (R, t, s) with y_i ~ s R x_i + t for x, y [3,n] (columns are points), Umeyama 1991; s = 1 when
    with_scale is False.  R is a proper rotation also for mirrored or degenerate point sets (S = diag(1, 1, -1) when
    det(U) det(V) < 0)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != y.shape or x.ndim != 2:
        raise GsajError("umeyama: x and y must both be [m,n] (got %s, %s)" % (x.shape, y.shape))
    m, n = x.shape
    mean_x, mean_y = x.mean(axis=1), y.mean(axis=1)
    xc, yc = x - mean_x[:, None], y - mean_y[:, None]
    sigma_x = (xc ** 2).sum() / n
    cov = yc @ xc.T / n
    u, d, vt = np.linalg.svd(cov)
    if np.count_nonzero(d > np.finfo(np.float64).eps) < m - 1:
        raise GsajError("umeyama: degenerate covariance (rank < %d)" % (m - 1))
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        s[m - 1, m - 1] = -1.0
    r = u @ s @ vt
    c = float(np.trace(np.diag(d) @ s) / sigma_x) if with_scale else 1.0
    t = mean_y - c * (r @ mean_x)
    return r, t, c


def ate(poses_gt, poses_est, correct_scale=False):
    """Absolute trajectory error of the translation parts.  poses_*: sequences of 4x4 camera-to-world matrices.  The estimated
    positions are aligned to the ground truth (rotation and translation; the scale too with correct_scale, the monocular case);
    e_i = |t_gt,i - (s R t_est,i + t)|.  Returns rmse, mean, median, std (population), min, max, sse -- the keys of evo's
    APE.get_all_statistics -- plus the alignment R, t, s and the errors."""
    gt = np.asarray([np.asarray(p, np.float64)[:3, 3] for p in poses_gt], np.float64).reshape(-1, 3).T
    est = np.asarray([np.asarray(p, np.float64)[:3, 3] for p in poses_est], np.float64).reshape(-1, 3).T
    if gt.shape != est.shape or gt.shape[1] < 1:
        raise GsajError("ate: need as many estimated poses as ground-truth poses, at least one (got %d, %d)" % (est.shape[1], gt.shape[1]))
    r, t, s = umeyama(est, gt, bool(correct_scale))
    e = np.linalg.norm(gt - (s * (r @ est) + t[:, None]), axis=0)
    sq = e ** 2
    return dict(rmse=float(np.sqrt(sq.mean())), mean=float(e.mean()), median=float(np.median(e)), std=float(e.std()), min=float(e.min()),
                max=float(e.max()), sse=float(sq.sum()), R=r, t=t, s=float(s), errors=e)
