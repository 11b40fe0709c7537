"""GPU: the tracking gradient mask of a frame on the device (gsaj.grad_mask / csrc/frame.hip; Camera.compute_grad_mask;
DeviceTracker.set_frame(edge_threshold=...)) against the NumPy restatement (tests/grad_mask_restated.py) and against outputs
recorded from the reference (tests/golden/grad_mask_*.npz).

Tolerances (grad_mask_restated.tolerance): intensities and the leftover strips of block mode within 16 * 2^-24 * max|gray|, the
roundings of the stencil, the squares, their sum and the root; a mask pixel may differ only where |I - t| is within
(1 + edge_threshold) times that (the same bound on the median, times the threshold), and at most max(2, 1e-4 N) pixels may.  The
kernels sum the stencil in the order the restatement does, so in practice the difference is zero; each case prints what it measured.
"""
import functools
import math
import os

import numpy as np
import pytest

import grad_mask_restated as gr

pytestmark = pytest.mark.gpu

SIZES = ((64, 96), (68, 100), (97, 131), (100, 170), (480, 640), (720, 1280))  # H, W: see the table in grad_mask_restated's tests
THRESHOLDS = (1.1, 4.0)
RECORDED = ("noise_64x96", "noise_68x100", "noise_97x131", "noise_100x170", "checker_68x100", "dyadic_68x100", "bright_68x100")


@functools.lru_cache(maxsize=None)
def _scene(kind, H, W):
    img = gr.make_scene(kind, H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _restated(kind, H, W, thr, blocks):
    return gr.grad_mask(_scene(kind, H, W), thr, blocks)


@functools.lru_cache(maxsize=None)
def _op(H, W):
    from gsaj.grad_mask import GradMask

    return GradMask(W, H, "cuda:0")


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _check(tag, got_value, got_u8, I_dev, want, thr, blocks):
    """Device outputs (NumPy) against a restated result `want`; returns the worst ratios measured."""
    H, W = want["I"].shape
    tol_i = gr.tolerance(0.0, want["max_gray"])
    tol_t = gr.tolerance(thr, want["max_gray"])
    vis = want["visited"]
    r_int = float(np.abs(I_dev.astype(np.float64) - want["I"]).max() / tol_i)
    wv = want["value"].astype(np.float32)
    gv = got_value.astype(np.float32)
    differ = (gv != wv) & vis
    margin = np.abs(want["I"].astype(np.float64) - want["t"].astype(np.float64))
    r_flip = float((margin[differ] / tol_t).max()) if differ.any() else 0.0
    r_strip = float(np.abs(gv[~vis].astype(np.float64) - wv[~vis]).max() / tol_i) if (~vis).any() else 0.0
    print("%s: intensity %.3f of its bound (%d of %d values differ), %d mask pixels differ (worst margin %.3f of its bound), strip %.3f"
          % (tag, r_int, int((I_dev != want["I"]).sum()), H * W, int(differ.sum()), r_flip, r_strip))
    assert r_int <= 1.0 and r_strip <= 1.0 and r_flip <= 1.0
    assert int(differ.sum()) <= max(2, int(1e-4 * H * W))
    assert np.array_equal(got_u8, got_value.astype(np.uint8))  # the byte is the value truncated, strips included
    assert got_value.dtype == (np.float32 if blocks else np.bool_)
    return r_int, r_flip, r_strip


@pytest.mark.parametrize("blocks", (False, True), ids=("global", "blocks"))
@pytest.mark.parametrize("H,W", SIZES)
def test_device_against_restatement(H, W, blocks):
    op = _op(H, W)
    img = _dev(_scene("noise", H, W))
    I_dev = op.intensity(img)[0].cpu().numpy()
    for thr in THRESHOLDS:
        u8 = op(img, thr, blocks=blocks)
        assert str(u8.dtype) == "torch.uint8" and tuple(u8.shape) == (1, H, W)
        ref = op.reference_tensor()
        assert tuple(ref.shape) == (1, H, W)
        _check("%dx%d %s thr %g" % (H, W, "blocks" if blocks else "global", thr), ref[0].cpu().numpy(), u8[0].cpu().numpy(), I_dev,
               _restated("noise", H, W, thr, blocks), thr, blocks)


@pytest.mark.parametrize("kind", ("checker", "bright"))
def test_quirk_a_scenes_against_restatement(kind):
    """Blocks whose threshold reaches 1: everything is zeroed there, the ones included ("bright": intensities above such a
    threshold exist, and the leftover strips hold bytes of 1)."""
    H, W = 68, 100
    op = _op(H, W)
    img = _dev(_scene(kind, H, W))
    I_dev = op.intensity(img)[0].cpu().numpy()
    for thr in THRESHOLDS:
        for blocks in (False, True):
            u8 = op(img, thr, blocks=blocks)
            _check("%s thr %g %s" % (kind, thr, blocks), op.reference_tensor()[0].cpu().numpy(), u8[0].cpu().numpy(), I_dev,
                   _restated(kind, H, W, thr, blocks), thr, blocks)
    if kind == "bright":
        want = _restated(kind, H, W, 1.1, True)
        u8 = op(img, 1.1, blocks=True)[0].cpu().numpy()
        assert not u8[want["visited"]].any() and (u8[~want["visited"]] == 1).any()


def test_dyadic_image():
    """r = g = b on a 1/256 grid: the gray image and every product and sum of the stencil are exact in fp32, in any order.  The
    RECORDED reference is still not the restatement's bits there (25 of 6800 intensities are one unit in the last place apart: what
    remains is the squares, their sum and the root, so its root is not correctly rounded everywhere), hence the recorded outputs are
    compared within the bound (test_recorded_fixtures_through_the_camera).  Device and restatement both round each of those three
    operations correctly, so THEY must agree in every bit."""
    import torch

    H, W = 68, 100
    op = _op(H, W)
    img = _dev(_scene("dyadic", H, W))
    assert torch.equal(op.intensity(img)[0].cpu(), torch.from_numpy(_restated("dyadic", H, W, 1.1, False)["I"]))
    for thr in THRESHOLDS:
        for blocks in (False, True):
            want = _restated("dyadic", H, W, thr, blocks)
            u8 = op(img, thr, blocks=blocks)
            assert torch.equal(u8[0].cpu(), torch.from_numpy(want["u8"]))
            assert torch.equal(op.reference_tensor()[0].cpu(), torch.from_numpy(want["value"]))


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_fixtures_through_the_camera(golden_dir, name):
    """Camera.compute_grad_mask on the device against what the reference's own method left in Camera.grad_mask on the CPU."""
    import torch
    from gsaj import synthetic as syn
    from utils.camera_utils import Camera

    rec = np.load(os.path.join(golden_dir, "grad_mask_%s.npz" % name))
    _, H, W = rec["image"].shape
    cam = Camera.from_synthetic(syn.fixture_camera(W=W, H=H), color=_dev(rec["image"]), device="cuda:0")
    max_gray = float(np.abs(rec["gray"]).max())
    tol_i = gr.tolerance(0.0, max_gray)
    I = rec["intensity"].astype(np.float64)
    bh, bw = gr.block_shape(H, W)
    for i, thr in enumerate(THRESHOLDS):
        for kind, key, dtype in (("tum", "global_%d" % i, torch.bool), ("replica", "block_%d" % i, torch.float32)):
            cam.compute_grad_mask({"Training": {"edge_threshold": thr}, "Dataset": {"type": kind}})
            assert cam.grad_mask.dtype == dtype and tuple(cam.grad_mask.shape) == (1, H, W) and cam.grad_mask.device.type == "cuda"
            got, want = cam.grad_mask[0].cpu().numpy().astype(np.float32), rec[key].astype(np.float32)
            inside = np.ones((H, W), bool)
            if kind == "replica":
                inside[gr.GRID * bh:, :] = False
                inside[:, gr.GRID * bw:] = False
            # the threshold each pixel met, from the recorded intensities
            t = _restated_t(I, thr, kind == "replica", bh, bw)
            differ = (got != want) & inside
            assert int(differ.sum()) <= max(2, int(1e-4 * H * W))
            if differ.any():
                assert (np.abs(I - t)[differ] <= gr.tolerance(thr, max_gray)).all()
            if (~inside).any():
                assert np.abs(got[~inside].astype(np.float64) - want[~inside]).max() <= tol_i
            print("%s %s thr %g: %d pixels differ from the recorded reference" % (name, kind, thr, int(differ.sum())))


def _restated_t(I, thr, blocks, bh, bw):
    H, W = I.shape
    I32 = I.astype(np.float32)
    if not blocks:
        return np.full((H, W), np.float32(gr.lower_median(I32) * np.float32(thr)), np.float64)
    t = np.full((H, W), np.nan)
    for r in range(gr.GRID):
        for c in range(gr.GRID):
            sl = (slice(r * bh, (r + 1) * bh), slice(c * bw, (c + 1) * bw))
            t[sl] = np.float32(gr.lower_median(I32[sl]) * np.float32(thr))
    return t


def test_edge_cases():
    import torch
    from gsaj import _lib
    from gsaj.grad_mask import GradMask

    H, W = 68, 100
    op = _op(H, W)
    for fill in (0.0, 0.5):  # all black: every intensity and the median are 0, nothing exceeds 0; constant: no gradient
        img = torch.full((3, H, W), fill, device="cuda:0")
        assert float(op.intensity(img).abs().max()) == 0.0
        for blocks in (False, True):
            assert int(op(img, 1.1, blocks=blocks).sum()) == 0
            assert float(op.reference_tensor().float().abs().max()) == 0.0
    # empty blocks (the reference raises) and a block too large for a workgroup's LDS: an error return, nothing launched
    small = GradMask(64, 31, "cuda:0")
    small.u8.fill_(7)
    with pytest.raises(Exception, match="block mode needs W >= 32 and H >= 32"):
        small(torch.rand(3, 31, 64, device="cuda:0"), 1.1, blocks=True)
    assert int((small.u8 != 7).sum()) == 0
    assert int(small(torch.rand(3, 31, 64, device="cuda:0"), 1.1).max()) == 1  # the global form has no such limit
    big = GradMask(2080, 2080, "cuda:0")  # 65 x 65 = 4225 pixels per block
    big.u8.fill_(7)
    with pytest.raises(Exception, match="exceeds the 4096 pixels"):
        big(torch.zeros(3, 2080, 2080, device="cuda:0"), 1.1, blocks=True)
    assert int((big.u8 != 7).sum()) == 0
    with pytest.raises(_lib.GsajError, match="no CPU path"):
        op(torch.zeros(3, H, W), 1.1)
    with pytest.raises(_lib.GsajError, match="no CPU path"):
        op.intensity(torch.zeros(3, H, W))
    with pytest.raises(_lib.GsajError, match=r"float32 \[3,68,100\]"):
        op(torch.zeros(3, H, W + 1, device="cuda:0"), 1.1)


def test_full_hd_blocks_fit():
    """1920 x 1080: blocks of 33 x 60 = 1980 pixels (eight passes of the 256 threads), the size the block kernel's LDS is stated
    for; 24 leftover rows, no leftover column."""
    H, W = 1080, 1920
    op = _op(H, W)
    img = _dev(_scene("noise", H, W))
    u8 = op(img, 1.1, blocks=True)
    _check("1080x1920 blocks", op.reference_tensor()[0].cpu().numpy(), u8[0].cpu().numpy(), op.intensity(img)[0].cpu().numpy(),
           _restated("noise", H, W, 1.1, True), 1.1, True)


def test_bit_reproducible_and_bytes_consistent():
    import torch

    H, W = 100, 170
    op = _op(H, W)
    img = _dev(_scene("noise", H, W))
    bits = lambda t: t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int32)  # noqa: E731
    for blocks in (False, True):
        a_u8 = op(img, 1.1, blocks=blocks).clone()
        a_ref = op.reference_tensor().clone()
        assert torch.equal(a_u8, a_ref.to(torch.uint8))  # the byte the loss kernels would make of the reference's tensor
        out = torch.empty(H * W, dtype=torch.uint8, device="cuda:0")
        b_u8 = op(img, 1.1, blocks=blocks, out=out)
        assert b_u8.data_ptr() == out.data_ptr()
        assert torch.equal(a_u8, b_u8) and torch.equal(bits(a_ref), bits(op.reference_tensor()))
    assert torch.equal(bits(op.intensity(img)), bits(op.intensity(img)))


# ---- the tracker computes its own mask --------------------------------------------------------------------------------------
def _tracking_setup(P=3000, W=160, H=120, seed=11):
    import torch
    from gsaj import synthetic as syn
    from gsaj.rasterizer import FrameContext

    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    f = 0.875 * W
    cam_gt = syn.fixture_camera(noisy=False, orthonormal=True, W=W, H=H, fx=f, fy=f, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    cam0 = syn.fixture_camera(noisy=True, orthonormal=True, W=W, H=H, fx=f, fy=f, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(P, seed, cam_gt, z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    M = sc["shs"].shape[1]
    g = dict(means3D=t(sc["means3D"]), opacities=t(sc["opacities"]), shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]),
             sh_degree=3)
    bg = torch.zeros(3, device=dev)
    gt = FrameContext(P, W, H, M, dev)
    gt.forward(bg, g["means3D"], g["opacities"], t(cam_gt["viewmatrix"]), t(cam_gt["projmatrix"]), t(cam_gt["campos"]), cam_gt["tanfovx"],
               cam_gt["tanfovy"], sh_degree=3, shs=g["shs"], scales=g["scales"], rotations=g["rotations"])
    w2c0 = np.ascontiguousarray(cam0["viewmatrix"].T)

    def tracker(**kw):
        from gsaj.tracking import DeviceTracker
        return DeviceTracker(P, W, H, M, dev, w2c0, t(cam0["projmatrix_raw"]), cam0["tanfovx"], cam0["tanfovy"], bg, alpha=0.9, **g, **kw)

    return tracker, gt.color.clone(), gt.depth[0].clone()


@pytest.mark.parametrize("use_graph", (False, True), ids=("eager", "graph"))
def test_tracker_with_its_own_mask_follows_a_tracker_handed_the_mask(use_graph):
    import torch
    from gsaj.grad_mask import GradMask

    tracker, gt_c, gt_d = _tracking_setup()
    _, H, W = gt_c.shape
    for blocks in (False, True):
        mask = GradMask(W, H, gt_c.device)(gt_c, 1.1, blocks=blocks).clone()
        assert 0 < int(mask.sum()) < H * W
        given, own = tracker(use_graph=use_graph), tracker(use_graph=use_graph)
        given.set_frame(gt_c, gt_d, grad_mask=mask)
        own.set_frame(gt_c, gt_d, edge_threshold=1.1, grad_blocks=blocks)
        assert torch.equal(own.grad_mask, mask.view(-1))
        for tr in (given, own):
            assert tr.iterate(10) == 10
        assert torch.equal(given.pose.state, own.pose.state) and torch.equal(given.w2c, own.w2c)
        assert torch.equal(given.loss_terms, own.loss_terms)
        # a second frame goes into the same buffers (a captured graph stays valid) and is masked by its own gradients
        gt2 = torch.flip(gt_c, dims=(2,)).contiguous()
        ptr = own.grad_mask.data_ptr()
        own.set_frame(gt2, gt_d, edge_threshold=1.1, grad_blocks=blocks)
        assert own.grad_mask.data_ptr() == ptr
        assert torch.equal(own.grad_mask, GradMask(W, H, gt_c.device)(gt2, 1.1, blocks=blocks).view(-1))
        assert own.iterate(2) == 2


def test_tracker_mask_for_every_frame_or_for_none():
    from gsaj import _lib

    tracker, gt_c, gt_d = _tracking_setup()
    tr = tracker()
    tr.set_frame(gt_c, gt_d, edge_threshold=1.1)
    with pytest.raises(_lib.GsajError, match="for every frame of a tracker or for none"):
        tr.set_frame(gt_c, gt_d)
    tr.set_frame(gt_c, gt_d, grad_mask=tr.grad_mask.clone().view(1, *gt_c.shape[1:]))  # a given mask after a computed one is fine
    tr2 = tracker()
    tr2.set_frame(gt_c, gt_d)
    with pytest.raises(_lib.GsajError, match="for every frame of a tracker or for none"):
        tr2.set_frame(gt_c, gt_d, edge_threshold=1.1)
    assert tr2.grad_mask is None
