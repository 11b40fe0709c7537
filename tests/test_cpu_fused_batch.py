"""CPU: the batched loss-fused entry points (gsaj_rasterize_forward_loss_batch / _backward_loss_batch) and gsaj.mapping.DeviceMapper
as far as they go without a device: declarations, the workspace size, every argument error reported before a launch, and the
mapper's own argument checks.  No kernel is launched (every pointer that would be dereferenced on the device is a made-up number
that no call gets as far as using)."""
import os
import re

import pytest
import torch

from abi import COMPUTE_LOSS, MONOCULAR, NO_EXPOSURE, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsaj_fused_loss_batch_workspace_bytes", "gsaj_rasterize_forward_loss_batch", "gsaj_rasterize_backward_loss_batch")


def _lib():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_header_signatures_and_library_agree_on_the_new_entry_points():
    mod, lib = _lib()
    with open(os.path.join(ROOT, "include", "gsaj.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"\b(gsaj_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in mod.SIGNATURES and hasattr(lib, name), name
    # one ctypes argument per declared parameter
    for name in NEW[1:]:
        decl = re.search(r"\bint %s\((.*?)\);" % name, text, re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(mod.SIGNATURES[name][1]), name
    # the batched forms take what the unfused batched forms take, plus the loss arguments
    assert len(mod.SIGNATURES[NEW[1]][1]) == len(mod.SIGNATURES["gsaj_rasterize_forward_batch"][1]) + 12
    assert len(mod.SIGNATURES[NEW[2]][1]) == len(mod.SIGNATURES["gsaj_rasterize_backward_batch"][1]) - 2 + 12
    assert lib.gsaj_version() >= 107
    from gsaj import losses
    assert (losses.COMPUTE_LOSS, losses.MONOCULAR, losses.NO_EXPOSURE) == (COMPUTE_LOSS, MONOCULAR, NO_EXPOSURE)


@pytest.mark.parametrize("W,H", [(37, 29), (160, 120), (640, 480), (1, 1)])
def test_batch_workspace_is_k_rounded_single_view_blocks(W, H):
    _, lib = _lib()
    one = (lib.gsaj_fused_loss_workspace_bytes(W, H) + 255) & ~255
    for K in (1, 3, 8):
        assert lib.gsaj_fused_loss_batch_workspace_bytes(K, W, H) == K * one


def _forward(lib, **kw):  # (the calls are built by parameter name from the argument groups of tests/abi.py)
    return call(lib, "gsaj_rasterize_forward_loss_batch", **kw)


def _backward(lib, **kw):
    return call(lib, "gsaj_rasterize_backward_loss_batch", **kw)


CASES = [("K <= 0", dict(K=0)), ("K < 0", dict(K=-2)), ("COMPUTE_LOSS", dict(loss_flags=COMPUTE_LOSS)), ("NULL gt_color", dict(gt_color=None)),
         ("NULL exposure_a without NO_EXPOSURE", dict(exposure_a=None)), ("NULL exposure_b without NO_EXPOSURE", dict(exposure_b=None)),
         ("exposure_stride 0", dict(exposure_stride=0)), ("exposure_stride < 0", dict(exposure_stride=-80)),
         ("NULL gt_depth without MONOCULAR", dict(gt_depth=None))]


@pytest.mark.parametrize("what,kw", CASES, ids=[c[0] for c in CASES])
def test_loss_argument_errors_are_returned_without_a_launch(what, kw):
    _, lib = _lib()
    for call in (_forward, _backward):
        assert call(lib, **kw) == -1, (what, call.__name__)
        msg = lib.gsaj_last_error()
        assert b"loss_batch" in msg and b"invalid" in msg, (what, msg)


@pytest.mark.parametrize("kw", [dict(out_scalars=None), dict(loss_ws=None)], ids=["NULL out_scalars", "NULL loss_ws"])
def test_forward_needs_its_outputs(kw):
    _, lib = _lib()
    assert _forward(lib, **kw) == -1
    assert b"out_scalars and loss_ws are required" in lib.gsaj_last_error()


def test_backward_needs_the_forwards_images():
    _, lib = _lib()
    assert _backward(lib, color=None) == -1
    assert b"color / depth / opacity" in lib.gsaj_last_error()


def test_device_mapper_refuses_a_cpu_device():
    from gsaj import _lib as mod
    from gsaj.mapping import DeviceMapper

    with pytest.raises(mod.GsajError, match="no CPU path"):
        DeviceMapper(None, 3, 37, 29, torch.eye(4), 0.5, 0.5, torch.zeros(3), device="cpu")


def test_the_default_form_is_the_one_the_measurement_chose():
    """profiles/r14_device_mapper.json: the fused iteration was slower than the unfused one by more than the spread of the unfused
    blocks at cfg5, so DeviceMapper defaults to fused=False (the decision rule of tools/mapper_iter_bench.py: default_fused)."""
    import inspect
    import json
    from gsaj.mapping import DeviceMapper

    with open(os.path.join(ROOT, "profiles", "r14_device_mapper.json")) as fh:
        doc = json.load(fh)
    assert doc["default_fused"] == (not any(r["fused_slower_than_the_unfused_spread"] for r in doc["results"]))
    assert inspect.signature(DeviceMapper.__init__).parameters["fused"].default is doc["default_fused"]


def test_set_view_rejects_wrong_shapes_and_slots():
    """set_view's checks come before anything touches the device: exercised on a mapper whose constructor did not run."""
    from gsaj import _lib as mod
    from gsaj.mapping import DeviceMapper

    K, W, H = 3, 37, 29
    for rgbd in (True, False):
        m = DeviceMapper.__new__(DeviceMapper)
        m.K, m.W, m.H = K, W, H
        m.gt_color = torch.zeros(K, 3, H, W)
        m.gt_depth = torch.zeros(K, H, W) if rgbd else None
        good_c, good_d = torch.ones(3, H, W), torch.ones(H, W) if rgbd else None
        for slot in (K, K + 5, -1):
            with pytest.raises(mod.GsajError, match="slot"):
                m.set_view(slot, good_c, good_d)
        for bad in (torch.ones(3, W, H), torch.ones(1, H, W), torch.ones(3, H, W + 1), torch.ones(H, W)):
            with pytest.raises(mod.GsajError, match="gt_color"):
                m.set_view(0, bad, good_d)
        with pytest.raises(mod.GsajError, match="depth"):
            m.set_view(0, good_c, None if rgbd else torch.ones(H, W))
        if rgbd:
            with pytest.raises(mod.GsajError, match="gt_depth"):
                m.set_view(0, good_c, torch.ones(H, W + 1))
        m.set_view(K - 1, good_c, good_d)  # a good view is copied into the mapper's own buffers
        assert torch.equal(m.gt_color[K - 1], good_c) and float(m.gt_color[0].abs().max()) == 0.0
        if rgbd:
            assert torch.equal(m.gt_depth[K - 1], good_d)
