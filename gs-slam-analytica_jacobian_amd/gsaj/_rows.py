"""The Python side of the one row mover (csrc/row_move.h) that gsaj.pruning.CompactPlan.apply and gsaj.densify.DensifyPlan.apply
share: the per-tensor check of a table and the loop that sends it, 32 tensors per launch, to a rows entry point."""
import ctypes

import torch

from . import _lib

MAX_TENSORS = 32      # ROW_MAX_TENSORS: tensors one launch moves
MAX_ROW_BYTES = 4096


def check(plan, tensors, zero_width):
    """(detached tensors, bytes per row) of a table for plan (.dev, .P): every tensor on the plan's device, [P, ...], contiguous,
    rows a multiple of 4 bytes of at most 4096.  zero_width: rows of no bytes are let through (move() skips them)."""
    srcs = [t.detach() if torch.is_tensor(t) else t for t in tensors]
    rbs = []
    for k, t in enumerate(srcs):
        if not torch.is_tensor(t) or t.device != plan.dev:
            raise _lib.GsajError("apply: tensor %d must be a tensor on %s (there is no CPU path)" % (k, plan.dev))
        if t.dim() < 1 or t.shape[0] != plan.P:
            raise _lib.GsajError("apply: tensor %d must have %d rows (got shape %s)" % (k, plan.P, list(t.shape)))
        if not t.is_contiguous():
            raise _lib.GsajError("apply: tensor %d is not contiguous" % k)
        rb = (t.numel() // plan.P) * t.element_size()
        if (rb <= 0 and not zero_width) or rb % 4 != 0 or rb > MAX_ROW_BYTES:
            raise _lib.GsajError("apply: tensor %d has rows of %d bytes; a row must be a %smultiple of 4 bytes, at most %d"
                                 % (k, rb, "" if zero_width else "non-zero ", MAX_ROW_BYTES))
        rbs.append(rb)
    return srcs, rbs


def move(plan, srcs, rbs, n_out, rows):
    """New tensors [n_out, ...], filled by rows(cnt, src, dst, row_bytes, ks) -- one call of a rows entry point for the cnt
    tensors whose indices are ks -- once per 32 tensors with rows of some width; each call counts in plan.launches."""
    outs = [torch.empty((n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=plan.dev) for t in srcs]
    live = [k for k, rb in enumerate(rbs) if rb > 0]
    if n_out == 0 or not live:
        return outs
    with torch.cuda.device(plan.dev):
        for k0 in range(0, len(live), MAX_TENSORS):
            ks = live[k0:k0 + MAX_TENSORS]
            cnt = len(ks)
            src = (ctypes.c_void_p * cnt)(*[srcs[k].data_ptr() for k in ks])
            dst = (ctypes.c_void_p * cnt)(*[outs[k].data_ptr() for k in ks])
            rb = (ctypes.c_int * cnt)(*[rbs[k] for k in ks])
            rows(cnt, src, dst, rb, ks)
            plan.launches += 1
    return outs
