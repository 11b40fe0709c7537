"""What the sensor front-end shares: FrameIngest, StereoIngest, StereoMatcher, MotionStereo and grey_u8 each make their own C-ABI calls;
the device check, the pinned staging of host inputs and its fence, the input and output checks, the GsajError form of _lib.check and
the matchers' workspace are defined here once."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._loop import require_device


def device(dev, who):
    dev = require_device(dev, who)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())   # (compares equal to tensor.device)


def check(rc, what):
    """_lib.check for the matchers: every failure is a GsajError (FrameIngest keeps _lib.check, whose -1 is a plain Exception)."""
    if rc < 0:
        raise _lib.GsajError("%s failed (%d): %s" % (what, rc, _lib.load().gsaj_last_error().decode("utf-8", "replace")))


class Staging:
    """A pinned host buffer and its device twin for one kind of input (bytes), made on first use."""

    def __init__(self, nbytes, dev):
        self.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def upload(self, array, np_dtype):
        np.copyto(self.host.numpy().view(np_dtype).reshape(array.shape), array)   # (any strides: the staging buffer is tight)
        self.dev.copy_(self.host, non_blocking=True)
        return self.dev


def source(owner, t, name, shapes, stage_attr, dtype=torch.uint8, np_dtype=np.uint8):
    """An image of one of `shapes`, [H,W] or [H,W,C]: a NumPy array (through the owner's pinned staging buffer `stage_attr`) or a tensor on
    owner.dev, read in place (rows may be padded) -> (device tensor to read, its row stride in bytes)."""
    if isinstance(t, np.ndarray):
        if t.dtype != np_dtype or tuple(t.shape) not in shapes:
            raise _lib.GsajError("%s must be %s %s (got %s %s)" % (name, np.dtype(np_dtype).name, " or ".join(map(str, shapes)), t.dtype, tuple(t.shape)))
        if getattr(owner, stage_attr) is None:
            setattr(owner, stage_attr, Staging(t.nbytes, owner.dev))
        return getattr(owner, stage_attr).upload(t, np_dtype), (t.size // t.shape[0]) * t.itemsize
    if not torch.is_tensor(t) or t.device != owner.dev:
        raise _lib.GsajError("%s must be a NumPy array or a tensor on %s" % (name, owner.dev))
    if t.dtype != dtype or tuple(t.shape) not in shapes:
        raise _lib.GsajError("%s must be %s %s (got %s %s)" % (name, dtype, " or ".join(map(str, shapes)), t.dtype, tuple(t.shape)))
    strides = t.stride()
    inner = (t.shape[2], 1) if len(strides) == 3 else (1,)
    if strides[1:] != inner or strides[0] < t.shape[1] * inner[0]:
        raise _lib.GsajError("%s: the pixels of a row must be contiguous (strides %r)" % (name, strides))
    return t, strides[0] * t.element_size()


def output(owner, attr, out, name, shape, dtype=torch.float32, dtype_name=None):
    """The tensor a call writes: `out` where given (any shape of that many elements), else owner.<attr>, made by the first call that needs
    it and overwritten by the next."""
    if out is None:
        if getattr(owner, attr) is None:
            setattr(owner, attr, torch.empty(shape, dtype=dtype, device=owner.dev))
        return getattr(owner, attr)
    numel = int(np.prod(shape))
    if not torch.is_tensor(out) or out.device != owner.dev or out.dtype != dtype or not out.is_contiguous() or out.numel() != numel:
        raise _lib.GsajError("%s must be a contiguous %s tensor of %d elements on %s" % (name, dtype_name or dtype, numel, owner.dev))
    return out


# The fence of an owner's staging buffers (owner._event): a call with a host input waits until the previous one has read them, and
# records behind its own launches; nothing else waits.
def staging_free(owner, *inputs):
    """-> whether any input is a host array; if so, after the previous call has read the staging buffers."""
    for t in inputs:
        if isinstance(t, np.ndarray):
            if owner._event is not None:
                owner._event.synchronize()
            return True
    return False


def staging_read(owner, host, stream):
    if host:
        if owner._event is None:
            owner._event = torch.cuda.Event()
        owner._event.record(stream)


class Matcher:
    """What StereoMatcher and MotionStereo share: a workspace sized by SIZE_FN(W, H, D, paths) and, for tests and tools, views of the
    [H,W,D] arrays OFFSETS_FN places in it -- VIEWS: (name, dtype) in the order of its arguments."""
    SIZE_FN = OFFSETS_FN = None
    VIEWS = ()

    def _allocate(self):
        nbytes = ctypes.c_size_t(0)
        check(getattr(self.lib, self.SIZE_FN)(self.W, self.H, self.D, self.paths, ctypes.byref(nbytes)), self.SIZE_FN)
        self.workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=self.dev)

    def _offsets(self):
        offs = [ctypes.c_size_t(0) for _ in self.VIEWS]
        check(getattr(self.lib, self.OFFSETS_FN)(self.W, self.H, self.D, self.paths, *[ctypes.byref(o) for o in offs]), self.OFFSETS_FN)
        return [o.value for o in offs]

    def _debug_view(self, which):
        (off, dtype), = [(o, d) for o, (name, d) in zip(self._offsets(), self.VIEWS) if name == which]
        n = self.W * self.H * self.D * torch.iinfo(dtype).bits // 8
        return self.workspace[off:off + n].view(dtype).view(self.H, self.W, self.D)

    def cost_volume(self):
        """Tests and tools: C [H,W,D] as the last call left it (a view of the workspace; uint16 bits in an int16 tensor)."""
        return self._debug_view("cost")

    def sums(self):
        """Tests and tools: S [H,W,D] int32 as the last call left it (a view of the workspace; StereoMatcher's columns x < D are zero)."""
        return self._debug_view("sums")
