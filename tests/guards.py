"""A guarded allocator for the memory-contract tests (tests/test_gpu_memory_contracts.py, tests/test_cpu_guards.py).

The parity tests compare values.  They cannot see WHERE a kernel writes, nor which stale bytes it reads: torch's caching allocator
rounds every block up to 512 bytes and every workspace carries alignment slack, so a store one row past the end lands in memory
nobody looks at, and fresh memory is usually zero.  `guarded` makes both visible:

    with guards.guarded(monkeypatch, fill=0xFF) as g:
        out = wrapper(...)          # every torch.empty / torch.zeros on a guarded device is now fenced and poisoned
        g.check()                   # every band of every allocation is still `fill`, byte for byte
        assert not g.payload_untouched(out)

Inside the context `torch.empty` and `torch.zeros` calls whose device passes `device_filter` (default: GPU devices) return a view
into a larger uint8 backing buffer:

    [ front band, 4096 bytes | payload, exactly numel * itemsize bytes | tail band, 4096 bytes or `tail_bytes` ]

The front band keeps the payload at the alignment the allocator gives (at least 256 bytes); the tail band starts at the byte right
after the payload, with no rounding.  The bands are filled with `fill`; a torch.empty payload is filled with `fill` too, a
torch.zeros payload with `zeros_as` (default 0).  Useful fills: 0xFF (fp32 NaN, int32 -1, a huge uint32 counter) and 0x5A (a
plausible finite float, 1.5e16, and a plausible small counter in the low byte).

The patching goes through pytest's monkeypatch and is undone when the context exits.  Host and pinned allocations, and calls with
`out=`, pass through untouched.

NOT guarded: tensors that come from any other route -- `clone`, `new_zeros`, `new_empty`, `empty_like`, `zeros_like`, `as_tensor`,
`full`, arithmetic results.  That is accepted: the wrappers of this project take their workspaces and outputs from torch.empty /
torch.zeros; a wrapper that moves to another route drops out of the guard, which `Guard.allocations` lets a test notice.
"""
import contextlib
import os
import sys

import torch

FRONT_BYTES = 4096
TAIL_BYTES = 4096
FILLS = (0xFF, 0x5A)

_HERE = os.path.abspath(__file__)


class Allocation:
    """One guarded tensor: `backing` is the whole uint8 buffer, the payload is backing[FRONT_BYTES : FRONT_BYTES + nbytes]."""

    def __init__(self, backing, nbytes, tail, shape, dtype, kind, site):
        self.backing, self.nbytes, self.tail = backing, nbytes, tail
        self.shape, self.dtype, self.kind, self.site = tuple(shape), dtype, kind, site

    @property
    def payload(self):
        return self.backing[FRONT_BYTES:FRONT_BYTES + self.nbytes]

    @property
    def front_band(self):
        return self.backing[:FRONT_BYTES]

    @property
    def tail_band(self):
        return self.backing[FRONT_BYTES + self.nbytes:]

    def describe(self):
        return "torch.%s(%s, dtype=%s) at %s" % (self.kind, list(self.shape), str(self.dtype).replace("torch.", ""), self.site)


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d in %s" % (os.path.relpath(f.f_code.co_filename, os.path.dirname(os.path.dirname(_HERE))), f.f_lineno, f.f_code.co_name)


def _damage(band, fill):
    """(first, last) damaged byte offsets of a band, or None."""
    bad = band != fill
    if not bool(bad.any()):
        return None
    idx = bad.nonzero().reshape(-1)
    return int(idx[0]), int(idx[-1]), int(idx.numel())


class Guard:
    def __init__(self, fill, zeros_as, tail_bytes, device_filter):
        assert 0 <= fill <= 255 and 0 <= zeros_as <= 255
        self.fill, self.zeros_as, self.tail_bytes, self.device_filter = fill, zeros_as, tail_bytes, device_filter
        self.allocations = []
        self._real_empty, self._real_zeros = torch.empty, torch.zeros

    # ---- allocation ------------------------------------------------------------------------------------------------------
    def _tail_for(self, shape, dtype, kind):
        t = self.tail_bytes
        if callable(t):
            t = t(tuple(shape), dtype, kind)
        return max(TAIL_BYTES, int(t or 0))

    def _make(self, kind, real, args, kwargs):
        if kwargs.get("out") is not None or kwargs.get("pin_memory") or kwargs.get("names") is not None:
            return real(*args, **kwargs)
        if kwargs.get("layout", torch.strided) is not torch.strided:
            return real(*args, **kwargs)
        size = kwargs["size"] if "size" in kwargs else args
        if len(size) == 1 and not isinstance(size[0], int) and hasattr(size[0], "__iter__"):
            size = tuple(size[0])
        try:
            shape = tuple(int(s) for s in size)
        except (TypeError, ValueError):
            return real(*args, **kwargs)
        device = kwargs.get("device")
        device = torch.device(device) if device is not None else real(0).device
        if not self.device_filter(device):
            return real(*args, **kwargs)
        dtype = kwargs.get("dtype") or torch.get_default_dtype()
        itemsize = real(0, dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        tail = self._tail_for(shape, dtype, kind)
        backing = real(FRONT_BYTES + nbytes + tail, dtype=torch.uint8, device=device)
        backing.fill_(self.fill)
        alloc = Allocation(backing, nbytes, tail, shape, dtype, kind, _call_site())
        if kind == "zeros":
            alloc.payload.fill_(self.zeros_as)
        self.allocations.append(alloc)
        t = alloc.payload.view(dtype).view(shape)
        if kwargs.get("requires_grad"):
            t.requires_grad_(True)
        return t

    def empty(self, *args, **kwargs):
        return self._make("empty", self._real_empty, args, kwargs)

    def zeros(self, *args, **kwargs):
        return self._make("zeros", self._real_zeros, args, kwargs)

    # ---- checks ----------------------------------------------------------------------------------------------------------
    def damaged(self):
        """One line per damaged band: the allocation and the first / last damaged offset, counted from the payload's start (front
        band: negative) or from its end (tail band: 0 is the byte right after the payload)."""
        out = []
        for a in self.allocations:
            d = _damage(a.front_band, self.fill)
            if d is not None:
                out.append("%s: %d byte(s) written BEFORE the payload, offsets %d .. %d from its start"
                           % (a.describe(), d[2], d[0] - FRONT_BYTES, d[1] - FRONT_BYTES))
            d = _damage(a.tail_band, self.fill)
            if d is not None:
                out.append("%s: %d byte(s) written PAST the payload (%d bytes), offsets +%d .. +%d from its end"
                           % (a.describe(), d[2], a.nbytes, d[0], d[1]))
        return out

    def check(self):
        bad = self.damaged()
        assert not bad, "guard bands damaged (fill 0x%02X):\n  " % self.fill + "\n  ".join(bad)

    def allocation_of(self, t):
        """The allocation whose payload holds tensor `t` (a guarded tensor or a view of one)."""
        ptr = t.data_ptr()
        for a in self.allocations:
            base = a.backing.data_ptr() + FRONT_BYTES
            if a.backing.device == t.device and base <= ptr and (ptr < base + a.nbytes or (ptr == base and a.nbytes == 0)):
                return a
        raise KeyError("tensor %s %s was not allocated under this guard" % (tuple(t.shape), t.dtype))

    def _bytes_of(self, t):
        self.allocation_of(t)
        assert t.is_contiguous(), "a contiguous tensor or view is needed"
        return t.detach().reshape(-1).view(torch.uint8)

    def payload_untouched(self, t):
        """True if every byte of `t` still holds `fill` (nothing wrote it; an empty tensor is trivially untouched)."""
        return bool((self._bytes_of(t) == self.fill).all())

    def unwritten(self, t):
        """Bool tensor shaped like `t`: elements whose every byte still holds `fill`."""
        b = self._bytes_of(t)
        return (b.view(-1, t.element_size()) == self.fill).all(dim=1).view(t.shape)

    def assert_fully_written(self, t, name="output"):
        """No element of `t` still holds `fill` in all of its bytes.  (A kernel that legitimately writes the fill pattern itself --
        0xFFFFFFFF = int32 -1 -- needs the other fill.)"""
        u = self.unwritten(t)
        n = int(u.sum())
        if n:
            first = u.reshape(-1).nonzero().reshape(-1)
            raise AssertionError("%s (%s): %d of %d element(s) never written (still 0x%02X), flat indices %d .. %d"
                                 % (name, self.allocation_of(t).describe(), n, u.numel(), self.fill, int(first[0]), int(first[-1])))

    def refill(self, t):
        """Poison a guarded tensor's payload again (before reusing a workspace whose contract says: no initialisation needed)."""
        self._bytes_of(t).fill_(self.fill)


def _is_gpu(device):
    return device.type == "cuda"


@contextlib.contextmanager
def guarded(monkeypatch, fill, zeros_as=0, tail_bytes=TAIL_BYTES, device_filter=_is_gpu):
    """Context manager: see the module docstring.  tail_bytes: an int, or a callable (shape, dtype, kind) -> bytes for tests that
    need one allocation's tail band larger (never below 4096).  Yields the Guard; its bands stay checkable after the context."""
    g = Guard(fill, zeros_as, tail_bytes, device_filter)
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", g.empty)
        m.setattr(torch, "zeros", g.zeros)
        yield g
