"""Removing rows of the Gaussian map under a mask, on the device (C ABI gsaj_compact_plan / gsaj_compact_count /
gsaj_compact_rows, csrc/compact.hip).

The reference's prune_points (gaussian_splatting/scene/gaussian_model.py:559-597) indexes the six parameters, their Adam moments
and the bookkeeping vectors with one boolean mask, t[mask] each: a nonzero with a host read and a gather per tensor.  Here one
pass over the mask plans the move, one 4-byte read sizes the outputs (none when the caller knows the count) and one launch moves
the kept rows of up to 32 tensors.  The result is t[keep] bit for bit, in the stable order.  There is no CPU path.
"""
import ctypes

import torch

from . import _lib, _rows
from ._rows import MAX_ROW_BYTES, MAX_TENSORS  # noqa: F401 -- GSAJ_COMPACT_MAX_TENSORS: tensors one launch moves; the largest row


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class CompactPlan:
    """The plan of one mask: block counts and offsets of the kept rows, on the device.  mask: bool or uint8 [P] on the device, any
    non-zero byte is set; remove=True: set rows leave (the reference's to_prune), remove=False: set rows stay.  The constructor
    launches the plan on the current stream and reads nothing.  The plan keeps the mask and reads it again in apply(): do not
    write to it until the last apply() has been issued.  n_kept: the number of kept rows when the caller knows it (it is
    trusted: a wrong value sizes the outputs wrongly); otherwise the first use of .n_kept reads 4 bytes."""

    def __init__(self, mask, remove=True, n_kept=None):
        if not torch.is_tensor(mask) or mask.device.type != "cuda":
            raise _lib.GsajError("CompactPlan: the mask must be a tensor on a HIP device (there is no CPU path)")
        if mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 or mask.shape[0] == 0:
            raise _lib.GsajError("CompactPlan: the mask must be a bool or uint8 tensor of [P], P > 0 (got %s %s)" % (mask.dtype, list(mask.shape)))
        self.lib = _lib.load()
        m = mask.detach().contiguous()
        self.mask = m.view(torch.uint8) if m.dtype == torch.bool else m
        self.P, self.dev, self.remove = int(m.shape[0]), m.device, bool(remove)
        if n_kept is not None and not 0 <= int(n_kept) <= self.P:
            raise _lib.GsajError("CompactPlan: n_kept = %r is outside 0..%d" % (n_kept, self.P))
        self._n_kept = None if n_kept is None else int(n_kept)
        self.launches = 0  # rows launches issued by apply() so far
        with torch.cuda.device(self.dev):
            self.ws = torch.empty(self.lib.gsaj_compact_workspace_bytes(self.P), dtype=torch.uint8, device=self.dev)
            _lib.check(self.lib.gsaj_compact_plan(self.P, self.mask.data_ptr(), int(self.remove), self.ws.data_ptr(), _stream(self.dev)),
                       "gsaj_compact_plan")

    @property
    def n_kept(self):
        if self._n_kept is None:
            n = ctypes.c_int(0)
            with torch.cuda.device(self.dev):
                _lib.check(self.lib.gsaj_compact_count(self.ws.data_ptr(), _stream(self.dev), ctypes.byref(n)), "gsaj_compact_count")
            self._n_kept = int(n.value)
        return self._n_kept

    def keep_mask(self):
        """bool [P] on the device: True where the row stays (a new tensor)."""
        return (self.mask != 0) != self.remove

    def apply(self, *tensors):
        """The kept rows of every tensor ([P, ...], contiguous, on the mask's device, any dtype whose row is a non-zero multiple of
        4 bytes) as new tensors [P', ...], in the same order: what t[keep] gives.  One launch per 32 tensors."""
        srcs, rbs = _rows.check(self, tensors, zero_width=False)

        def rows(cnt, src, dst, rb, ks):
            _lib.check(self.lib.gsaj_compact_rows(self.P, cnt, src, dst, rb, self.ws.data_ptr(), _stream(self.dev)), "gsaj_compact_rows")

        return _rows.move(self, srcs, rbs, self.n_kept, rows)
