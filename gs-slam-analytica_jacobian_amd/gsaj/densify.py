"""Clone, split and prune of the Gaussian map from one plan, on the device (C ABI gsaj_densify_plan / gsaj_densify_counts /
gsaj_densify_rows / gsaj_densify_children / gsaj_densify_noise, csrc/densify_prune.hip).

The reference's densify_and_prune (gaussian_splatting/scene/gaussian_model.py:599-765) selects with boolean masks, appends with
three torch.cat of every parameter and Adam moment and prunes twice.  Here one pass classifies the P source rows, one 16-byte
read sizes the outputs (none when the caller hands the counts in), one launch writes every output row of up to 32 tensors and one
launch computes the children's positions and log-scales.  Everything but those two child tensors is a bit-for-bit function of
the inputs, in the reference's output order: kept originals, kept clones, then the kept children copy by copy.  include/gsaj.h
states the rules and the kept quirks.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib, _rows
from ._rows import MAX_ROW_BYTES, MAX_TENSORS  # noqa: F401 -- GSAJ_DENSIFY_MAX_TENSORS; the largest row
MAX_SPLIT = 4         # GSAJ_DENSIFY_MAX_SPLIT
CLONE, SPLIT, PRUNE = 1, 2, 4
ALL = CLONE | SPLIT | PRUNE


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _f32(name, t, dev, P, cols=None):
    if not torch.is_tensor(t) or t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise _lib.GsajError("DensifyPlan: %s must be a tensor on the HIP device of the others (there is no CPU path)" % name)
    if t.dtype != torch.float32 or t.shape[0] != P or (cols is not None and t.numel() != P * cols):
        raise _lib.GsajError("DensifyPlan: %s must be float32 with %d rows%s (got %s %s)"
                             % (name, P, "" if cols is None else " of %d" % cols, t.dtype, list(t.shape)))
    return t.detach().contiguous()


def thresholds(grad_threshold, min_opacity, extent, max_screen_size, percent_dense):
    """The host side of the rules: every threshold formed in double and rounded to fp32 once, as comparing a float32 tensor with a
    Python float does.  Returns (grad_threshold, t_dense, t_big, min_opacity, size_rule, size_all)."""
    size_rule = bool(max_screen_size)
    size_all = bool(size_rule and np.float32(0.0) > np.float32(max_screen_size))
    return (float(np.float32(grad_threshold)), float(np.float32(float(percent_dense) * float(extent))),
            float(np.float32(0.1 * float(extent))), float(np.float32(min_opacity)), size_rule, size_all)


class DensifyPlan:
    """The plan of one map update.  scaling [P,S] (S = 3, or 1 for an isotropic model), opacity [P] or [P,1], both raw (before
    exp / sigmoid), float32 on the device.  accum, denom: xyz_gradient_accum and denom ([P] or [P,1]), the gradient statistic is
    their quotient with NaN -> 0; denom=None: accum is taken as grads [n_grads <= P] directly and the rows behind it have
    gradient 0 (densify_and_split's padded_grad).  stages: CLONE | SPLIT | PRUNE, which rules apply.  N: children per split
    parent, 1..4.  The constructor launches the plan on the current stream and reads nothing; counts = (originals, clones,
    children per copy, P'') when the caller knows them (trusted), otherwise the first use of .counts reads 16 bytes."""

    def __init__(self, accum, denom, scaling, opacity, grad_threshold, min_opacity, extent, max_screen_size, percent_dense=0.01,
                 N=2, stages=ALL, counts=None):
        if not torch.is_tensor(scaling) or scaling.device.type != "cuda" or scaling.dim() != 2 or scaling.shape[0] == 0:
            raise _lib.GsajError("DensifyPlan: scaling must be a [P,S] tensor on a HIP device, P > 0 (there is no CPU path)")
        self.P, self.S, self.N, self.dev = int(scaling.shape[0]), int(scaling.shape[1]), int(N), scaling.device
        self.stages = int(stages)
        if self.S not in (1, 3) or not 1 <= self.N <= MAX_SPLIT or not 0 <= self.stages <= ALL:
            raise _lib.GsajError("DensifyPlan: S = %d must be 1 or 3, N = %d in 1..%d, stages = %d in 0..%d" % (self.S, self.N, MAX_SPLIT, self.stages, ALL))
        if not float(grad_threshold) > 0:
            raise _lib.GsajError("DensifyPlan: grad_threshold = %r must be greater than 0" % (grad_threshold,))
        self.lib = _lib.load()
        self.scaling = _f32("scaling", scaling, None, self.P, self.S)
        self.opacity = _f32("opacity", opacity, self.dev, self.P, 1)
        if denom is None:
            if not torch.is_tensor(accum) or accum.device != self.dev or accum.dtype != torch.float32 or accum.numel() > self.P:
                raise _lib.GsajError("DensifyPlan: grads must be float32 of at most %d elements on %s" % (self.P, self.dev))
            self.accum, self.denom, self.n_grads = accum.detach().contiguous().reshape(-1), None, int(accum.numel())
        else:
            self.accum, self.denom, self.n_grads = _f32("accum", accum, self.dev, self.P, 1), _f32("denom", denom, self.dev, self.P, 1), self.P
        thr, t_d, t_b, min_o, size_rule, size_all = thresholds(grad_threshold, min_opacity, extent, max_screen_size, percent_dense)
        if counts is not None:
            counts = tuple(int(c) for c in counts)
            if len(counts) != 4 or min(counts) < 0 or counts[3] != counts[0] + counts[1] + self.N * counts[2] or counts[0] + counts[2] > self.P:
                raise _lib.GsajError("DensifyPlan: counts = %r are not (originals, clones, children per copy, P'') of %d rows" % (counts, self.P))
        self._counts = counts
        self.launches = 0  # rows and children launches issued so far
        with torch.cuda.device(self.dev):
            self.code = torch.empty(self.P, dtype=torch.uint8, device=self.dev)
            self.ws = torch.empty(self.lib.gsaj_densify_workspace_bytes(self.P, self.N), dtype=torch.uint8, device=self.dev)
            # (an accum of zero elements has no address: any valid one serves, it is never read)
            _lib.check(self.lib.gsaj_densify_plan(self.P, self.S, self.N, self.stages, self.accum.data_ptr() or self.code.data_ptr(),
                                                  None if self.denom is None else self.denom.data_ptr(), self.n_grads,
                                                  self.scaling.data_ptr(), self.opacity.data_ptr(), thr, t_d, t_b, min_o, int(size_rule),
                                                  int(size_all), self.code.data_ptr(), self.ws.data_ptr(), _stream(self.dev)),
                       "gsaj_densify_plan")

    @property
    def counts(self):
        """(kept originals, clones, children per copy, P'')."""
        if self._counts is None:
            c = (ctypes.c_int * 4)()
            with torch.cuda.device(self.dev):
                _lib.check(self.lib.gsaj_densify_counts(self.ws.data_ptr(), _stream(self.dev), c), "gsaj_densify_counts")
            self._counts = tuple(int(v) for v in c)
        return self._counts

    @property
    def n_out(self):
        return self.counts[3]

    def apply(self, tensors, new_rows="parent"):
        """Every tensor ([P, ...], contiguous, on the plan's device, rows a multiple of 4 bytes) through the plan, as new tensors
        [P'', ...].  new_rows: "parent" (a clone or child gets its parent's row) or "zeros" (Adam moments), one word for all or one
        per tensor.  A tensor with zero-width rows is not sent to the kernel.  One launch per 32 tensors."""
        tensors = list(tensors)
        modes = [new_rows] * len(tensors) if isinstance(new_rows, str) else list(new_rows)
        if len(modes) != len(tensors) or any(m not in ("parent", "zeros") for m in modes):
            raise _lib.GsajError("apply: new_rows must be 'parent' or 'zeros', once or once per tensor")
        srcs, rbs = _rows.check(self, tensors, zero_width=True)

        def rows(cnt, src, dst, rb, ks):
            zn = (ctypes.c_int * cnt)(*[int(modes[k] == "zeros") for k in ks])
            _lib.check(self.lib.gsaj_densify_rows(self.P, self.N, cnt, src, dst, rb, zn, self.code.data_ptr(), self.ws.data_ptr(),
                                                  _stream(self.dev)), "gsaj_densify_rows")

        return _rows.move(self, srcs, rbs, self.n_out, rows)

    def children(self, xyz, scaling, rotation, dst_xyz, dst_scaling, noise=None, seed=0):
        """Overwrite the child rows of dst_xyz [P'',3] and dst_scaling [P'',S] (outputs of apply()) with the sampled positions and
        the shrunk log-scales of the children of the source rows xyz [P,3], scaling [P,S], rotation [P,4].  noise: float32
        [N,P,3] on the device, indexed by source row; None: the counter-based generator under the 64-bit seed."""
        n = self.n_out
        x, s, q = _f32("xyz", xyz, self.dev, self.P, 3), _f32("scaling", scaling, self.dev, self.P, self.S), _f32("rotation", rotation, self.dev, self.P, 4)
        for name, t, cols in (("dst_xyz", dst_xyz, 3), ("dst_scaling", dst_scaling, self.S)):
            if not torch.is_tensor(t) or t.device != self.dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n * cols:
                raise _lib.GsajError("children: %s must be a contiguous float32 tensor of [%d,%d] on %s" % (name, n, cols, self.dev))
        if noise is not None:
            if (not torch.is_tensor(noise) or noise.device != self.dev or noise.dtype != torch.float32 or not noise.is_contiguous()
                    or tuple(noise.shape) != (self.N, self.P, 3)):
                raise _lib.GsajError("children: noise must be a contiguous float32 tensor of [%d,%d,3] on %s" % (self.N, self.P, self.dev))
        if self.counts[2] == 0:
            return
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_densify_children(self.P, self.S, self.N, x.data_ptr(), s.data_ptr(), q.data_ptr(),
                                                      None if noise is None else noise.data_ptr(), int(seed) & (2 ** 64 - 1),
                                                      self.code.data_ptr(), self.ws.data_ptr(), dst_xyz.data_ptr(), dst_scaling.data_ptr(),
                                                      _stream(self.dev)), "gsaj_densify_children")
            self.launches += 1

    def source_rows(self):
        """int32 [P''] on the device: the source row of every output row (an arange sent through the rows kernel)."""
        return self.apply([torch.arange(self.P, dtype=torch.int32, device=self.dev)])[0]


def densify_noise(P, N, seed, device="cuda"):
    """float32 [N,P,3]: the standard normal draws the children kernel makes for (copy n, source row i) under the seed."""
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GsajError("densify_noise: needs a HIP device (there is no CPU path)")
    with torch.cuda.device(dev):
        out = torch.empty((max(int(N), 0), max(int(P), 0), 3), dtype=torch.float32, device=dev)
        _lib.check(lib.gsaj_densify_noise(int(P), int(N), int(seed) & (2 ** 64 - 1), out.data_ptr(), _stream(out.device)), "gsaj_densify_noise")
    return out
