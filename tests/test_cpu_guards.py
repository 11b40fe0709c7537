"""The guarded allocator of tests/guards.py has teeth: every planted defect is reported, with the right allocation named, and a
clean run reports nothing.  Runs the allocator on CPU tensors (device_filter), plus one GPU-marked case of the same kind; no
project kernel is involved.  Also here: every size function of the library has a row in the contract table of
tests/test_gpu_memory_contracts.py."""
import re

import pytest
import torch

import guards

CPU = lambda d: d.type == "cpu"  # noqa: E731


def _report(g):
    with pytest.raises(AssertionError) as e:
        g.check()
    return str(e.value)


# payload byte sizes 28, 7 and 24: none a multiple of 256, so the tail band starts inside what an allocator would round up to
@pytest.mark.parametrize("fill", guards.FILLS)
@pytest.mark.parametrize("dtype,shape", [(torch.float32, (7,)), (torch.uint8, (7,)), (torch.float64, (3,))])
def test_one_element_past_the_end_is_reported(monkeypatch, fill, dtype, shape):
    with guards.guarded(monkeypatch, fill, device_filter=CPU) as g:
        bystander = torch.zeros(5, 3, dtype=torch.int32, device="cpu")
        victim = torch.empty(*shape, dtype=dtype, device="cpu")
        a = g.allocation_of(victim)
        assert a.nbytes == victim.numel() * victim.element_size() and a.nbytes % 256 != 0
        assert victim.data_ptr() == a.backing.data_ptr() + guards.FRONT_BYTES
        assert bool((bystander == 0).all()) and g.payload_untouched(victim)
        # "one element too many": the store a kernel with an off-by-one bound would make, through the backing buffer
        one = a.backing[guards.FRONT_BYTES + a.nbytes:guards.FRONT_BYTES + a.nbytes + victim.element_size()]
        one.view(dtype)[0] = 1
        msg = _report(g)
    lines = msg.splitlines()[1:]
    assert len(lines) == 1, msg  # the bystander is not accused
    assert "torch.empty(%s, dtype=%s)" % (list(shape), str(dtype).replace("torch.", "")) in lines[0], msg
    assert "test_cpu_guards.py" in lines[0] and "test_one_element_past_the_end_is_reported" in lines[0], msg
    assert "PAST the payload" in lines[0] and "offsets +0 .." in lines[0], msg
    last = int(re.search(r"\.\. \+(\d+) from its end", lines[0]).group(1))
    assert last < victim.element_size(), msg


@pytest.mark.parametrize("fill", guards.FILLS)
def test_one_element_before_the_start_is_reported(monkeypatch, fill):
    with guards.guarded(monkeypatch, fill, device_filter=CPU) as g:
        torch.empty(9, device="cpu")
        victim = torch.zeros((2, 3), dtype=torch.float32, device="cpu")
        a = g.allocation_of(victim)
        a.backing[guards.FRONT_BYTES - 4:guards.FRONT_BYTES].view(torch.float32)[0] = 2.5
        msg = _report(g)
    lines = msg.splitlines()[1:]
    assert len(lines) == 1 and "torch.zeros([2, 3], dtype=float32)" in lines[0] and "BEFORE the payload" in lines[0], msg
    first, last = (int(x) for x in re.search(r"offsets (-?\d+) \.\. (-?\d+) from its start", lines[0]).groups())
    assert -4 <= first <= last <= -1, msg


@pytest.mark.parametrize("fill", guards.FILLS)
def test_a_write_4000_bytes_past_the_end_is_reported(monkeypatch, fill):
    with guards.guarded(monkeypatch, fill, device_filter=CPU) as g:
        victim = torch.empty(10, dtype=torch.float32, device="cpu")
        a = g.allocation_of(victim)
        a.backing[guards.FRONT_BYTES + a.nbytes + 4000] = 0x11
        msg = _report(g)
    assert "torch.empty([10], dtype=float32)" in msg and "offsets +4000 .. +4000 from its end" in msg, msg


def test_a_larger_tail_band_catches_a_far_write(monkeypatch):
    tail = lambda shape, dtype, kind: 1 << 16 if shape == (10,) else 0  # noqa: E731
    with guards.guarded(monkeypatch, 0xFF, tail_bytes=tail, device_filter=CPU) as g:
        other = torch.empty(11, device="cpu")
        victim = torch.empty(10, dtype=torch.float32, device="cpu")
        assert g.allocation_of(other).tail == guards.TAIL_BYTES and g.allocation_of(victim).tail == 1 << 16
        g.allocation_of(victim).backing[guards.FRONT_BYTES + 40 + 60000] = 0
        msg = _report(g)
    assert "offsets +60000 .. +60000" in msg, msg


@pytest.mark.parametrize("fill", guards.FILLS)
def test_an_unwritten_output_row_is_reported(monkeypatch, fill):
    with guards.guarded(monkeypatch, fill, device_filter=CPU) as g:
        out = torch.empty(6, 5, dtype=torch.float32, device="cpu")
        assert g.payload_untouched(out)
        out[:4] = 1.0
        out[5] = 2.0  # row 4 is the one a kernel skipped
        assert not g.payload_untouched(out) and g.payload_untouched(out[4])
        assert g.unwritten(out).nonzero().tolist() == [[4, c] for c in range(5)]
        with pytest.raises(AssertionError) as e:
            g.assert_fully_written(out, "out")
        assert "5 of 30 element(s) never written" in str(e.value) and "flat indices 20 .. 24" in str(e.value), str(e.value)
        if fill == 0xFF:  # the NaN scan sees the same row
            assert torch.isnan(out).any(dim=1).tolist() == [False] * 4 + [True, False]
        out[4] = 0.0
        g.assert_fully_written(out, "out")
        g.check()


@pytest.mark.parametrize("fill", guards.FILLS)
def test_a_clean_run_reports_nothing(monkeypatch, fill):
    with guards.guarded(monkeypatch, fill, device_filter=CPU) as g:
        e = torch.empty((3, 4), dtype=torch.float16, device="cpu")
        z = torch.zeros(17, dtype=torch.int64, device="cpu")
        z2 = torch.zeros(torch.Size([2, 2]), device="cpu")
        s = torch.empty((), dtype=torch.float64, device="cpu")
        n = torch.empty(0, 3, device="cpu")
        b = torch.zeros(5, dtype=torch.bool, device="cpu")
        assert e.shape == (3, 4) and e.dtype == torch.float16 and z.dtype == torch.int64 and z2.shape == (2, 2)
        assert s.shape == () and n.shape == (0, 3) and b.dtype == torch.bool and not bool(b.any())
        assert bool((z == 0).all()) and bool((z2 == 0).all())
        assert bool((e.view(torch.uint8) == fill).all())  # torch.empty is poisoned
        for t in (e, z, z2, s, n, b):
            assert t.is_contiguous() and t.data_ptr() % 64 == 0
        e.fill_(1), z.fill_(7), z2.fill_(3), s.fill_(4), b.fill_(True)  # writes inside the payloads, up to their last byte
        assert len(g.allocations) == 6 and g.damaged() == []
        g.check()
    g.check()  # the bands stay checkable after the context


def test_zeros_as_poisons_torch_zeros_too(monkeypatch):
    with guards.guarded(monkeypatch, 0x5A, zeros_as=0x5A, device_filter=CPU) as g:
        z = torch.zeros(4, dtype=torch.int32, device="cpu")
        assert z.tolist() == [0x5A5A5A5A] * 4 and g.payload_untouched(z)


def test_allocations_outside_the_filter_pass_through(monkeypatch):
    with guards.guarded(monkeypatch, 0xFF) as g:  # default filter: GPU devices only
        t = torch.zeros(8, device="cpu")
        u = torch.empty(8)
        assert g.allocations == [] and bool((t == 0).all()) and u.shape == (8,)
        with pytest.raises(KeyError):
            g.allocation_of(t)
    with guards.guarded(monkeypatch, 0xFF, device_filter=CPU) as g:
        out = torch.empty(4)
        torch.zeros(4, out=out)  # out= is not an allocation
        assert len(g.allocations) == 1 and out.tolist() == [0.0] * 4


def test_torch_and_monkeypatch_are_restored(monkeypatch):
    real_empty, real_zeros = torch.empty, torch.zeros
    monkeypatch.setattr(guards, "TAIL_BYTES", guards.TAIL_BYTES)  # an unrelated patch of the test's own must survive the context
    with guards.guarded(monkeypatch, 0xFF, device_filter=CPU):
        assert torch.empty is not real_empty and torch.zeros is not real_zeros
    assert torch.empty is real_empty and torch.zeros is real_zeros
    with pytest.raises(RuntimeError):
        with guards.guarded(monkeypatch, 0xFF, device_filter=CPU):
            raise RuntimeError("a failing test body")
    assert torch.empty is real_empty and torch.zeros is real_zeros
    monkeypatch.setattr(torch, "empty", real_empty)  # monkeypatch itself is still usable
    assert torch.empty(3).shape == (3,)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", guards.FILLS)
def test_gpu_planted_writes_are_reported(monkeypatch, fill):
    dev = "cuda:0"
    with guards.guarded(monkeypatch, fill) as g:
        host = torch.zeros(4)  # host allocations pass through
        ws = torch.empty(301, dtype=torch.uint8, device=dev)
        out = torch.zeros(7, 3, dtype=torch.float32, device=dev)
        assert len(g.allocations) == 2 and host.device.type == "cpu"
        assert out.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
        assert g.payload_untouched(ws) and bool((out == 0).all())
        g.check()
        a = g.allocation_of(out)
        idx = torch.tensor([guards.FRONT_BYTES + a.nbytes, guards.FRONT_BYTES + a.nbytes + 3], device=dev)
        a.backing.index_put_((idx,), torch.tensor([1, 2], dtype=torch.uint8, device=dev))  # one float past the last row
        msg = _report(g)
    lines = msg.splitlines()[1:]
    assert len(lines) == 1 and "torch.zeros([7, 3], dtype=float32)" in lines[0] and "offsets +0 .. +3 from its end" in lines[0], msg


# ---- the contract table covers every workspace --------------------------------------------------------------------------------
def test_every_workspace_function_has_a_contract_row():
    """A new size function (every gsaj_*_bytes of the binding: the workspaces, the pyramid, motion stereo) cannot arrive untested: it
    needs a row in CONTRACTS, and the row names a test of the GPU file that runs the workspace under guard."""
    from gsaj import _lib

    import test_gpu_memory_contracts as mc

    sized = sorted(n for n in _lib.SIGNATURES if n.endswith("_bytes"))
    assert len(sized) >= 22, sized
    with open(_lib.HEADER) as fh:
        header = fh.read().splitlines()
    missing = [n for n in sized if n not in mc.CONTRACTS]
    assert not missing, "no row in test_gpu_memory_contracts.CONTRACTS for %s" % missing
    for name, row in mc.CONTRACTS.items():
        assert name in sized, "%s is no workspace size function of gsaj/_lib.py" % name
        assert row["init"] in ("none", "zeroed once"), (name, row["init"])
        line = header[row["line"] - 1]
        assert row["quote"] in line, "%s: include/gsaj.h:%d no longer reads %r" % (name, row["line"], row["quote"])
        for t in row["tests"]:
            assert callable(getattr(mc, t, None)), "%s: no test %s in test_gpu_memory_contracts.py" % (name, t)
        assert row["tests"], name
