"""GPU: csrc/ingest.hip against tests/ingest_restated.py.  k_frame_ingest: the raw bits of every plane on the direct path (scalar and
vector shapes, every channel count, tight and padded rows, every source-read form) and through planted and computed maps, sentinels
around every output, the vector path against the scalar path, run-to-run equality and a second stream.  k_undistort_map: the raw bits
of both maps.  gsaj.ingest: frames ingested straight into a GaussNewtonTracker's buffers against the reference's host statements."""
import numpy as np
import pytest

import ingest_restated as ir

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 8                 # sentinel floats on either side of every output (32 bytes: the output stays 16-byte aligned)
SENTINEL = F(-7777.25)
DIRECT_SHAPES = ((2, 2), (5, 3), (7, 5), (8, 4), (16, 16), (64, 3), (68, 36), (160, 120))   # W, H: W % 4 != 0 is the scalar path
ROTATION_Y_2DEG = np.array([[np.cos(np.radians(2.0)), 0.0, np.sin(np.radians(2.0))], [0.0, 1.0, 0.0],
                            [-np.sin(np.radians(2.0)), 0.0, np.cos(np.radians(2.0))]])


def _padded(torch, dev, rows, pad, junk):
    """rows [R, row_bytes] uint8 -> a device buffer whose rows are row_bytes + pad apart, the padding filled with junk."""
    R, nb = rows.shape
    host = np.full((R, nb + pad), junk, np.uint8)
    host[:, :nb] = rows
    return torch.as_tensor(host, device=dev), nb + pad


def _guarded(torch, dev, numel, misalign):
    buf = torch.full((numel + 2 * GUARD + 1,), float(SENTINEL), dtype=torch.float32, device=dev)
    off = GUARD + (1 if misalign else 0)
    view = buf[off:off + numel]
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    return buf, view, off


def _assert_guards(buf, off, numel, tag):
    host = buf.cpu().numpy()
    assert (host[:off] == SENTINEL).all() and (host[off + numel:] == SENTINEL).all(), "%s: floats outside the output were written" % tag


def _ingest(torch, src, flags=0, maps=None, W=None, H=None, pad=0, depth=None, depth_pad=0, depth_scale=1.0, misalign=False, stream=None):
    """gsaj_frame_ingest on src uint8 [Hs,Ws,C] (and depth uint16 [H,W]) -> (colour [3,H,W], depth [H,W] or None) as NumPy arrays;
    the sentinels around both outputs are checked."""
    from gsaj import _lib

    lib, dev = _lib.load(), torch.device("cuda:0")
    src = src[:, :, None] if src.ndim == 2 else src
    Hs, Ws, C = src.shape
    W, H = (Ws, Hs) if W is None else (W, H)
    d_src, stride = _padded(torch, dev, src.reshape(Hs, Ws * C), pad, 0x5A)
    d_maps = None if maps is None else [torch.as_tensor(np.ascontiguousarray(m, F), device=dev) for m in maps]
    cbuf, cview, coff = _guarded(torch, dev, 3 * W * H, misalign)
    if depth is not None:
        d_depth, dstride = _padded(torch, dev, np.ascontiguousarray(depth).view(np.uint8).reshape(H, 2 * W), depth_pad, 0xC3)
        dbuf, dview, doff = _guarded(torch, dev, W * H, misalign)

    def run():
        _lib.check(lib.gsaj_frame_ingest(W, H, Ws, Hs, C, stride, d_src.data_ptr(), None if maps is None else d_maps[0].data_ptr(),
                                         None if maps is None else d_maps[1].data_ptr(), None if depth is None else d_depth.data_ptr(),
                                         0 if depth is None else dstride, float(depth_scale), flags, cview.data_ptr(),
                                         None if depth is None else dview.data_ptr(), torch.cuda.current_stream().cuda_stream), "gsaj_frame_ingest")

    if stream is None:
        run()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            run()
        stream.synchronize()
    tag = "%dx%d from %dx%dx%d flags %d pad %d" % (W, H, Ws, Hs, C, flags, pad)
    _assert_guards(cbuf, coff, 3 * W * H, tag + " colour")
    if depth is not None:
        _assert_guards(dbuf, doff, W * H, tag + " depth")
    return cview.cpu().numpy().reshape(3, H, W), None if depth is None else dview.cpu().numpy().reshape(H, W)


def _bytes(W, H, C, seed):
    if (W, H) == (16, 16):   # every byte value, each channel starting somewhere else
        return np.stack([(np.arange(256) + 85 * c) % 256 for c in range(C)], axis=-1).astype(np.uint8).reshape(16, 16, C)
    return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("W,H", DIRECT_SHAPES, ids=["%dx%d" % s for s in DIRECT_SHAPES])
def test_direct_path_bits_against_the_mirror(W, H, C):
    import torch

    src = _bytes(W, H, C, seed=W * 100 + H + C)
    depth = np.random.default_rng(W + H).integers(0, 65536, (H, W), dtype=np.uint16)
    depth.reshape(-1)[:3] = (0, 1, 65535)
    # pads: tight rows; rows that leave neither the 4-byte source read nor the 8-byte depth read aligned; padded rows that do
    for pad, depth_pad in ((0, 0), (5, 6), (8, 8)):
        for bgr in (0, ir.BGR):
            for scale, mul in ((None, 0), (5000.0, 0), (0.001, ir.DEPTH_MUL)):
                flags = bgr | mul
                tag = "%dx%dx%d pad %d flags %d scale %r" % (W, H, C, pad, flags, scale)
                color, d = _ingest(torch, src, flags, pad=pad, depth=None if scale is None else depth, depth_pad=depth_pad, depth_scale=scale or 1.0)
                ir.assert_bits_equal(color, ir.ingest_color(src, flags), tag)
                if scale is not None:
                    ir.assert_bits_equal(d, ir.ingest_depth(depth, scale, flags), tag + " depth")
    if C == 1:   # what the canaries of tests/test_cpu_ingest.py change is in these inputs
        assert not np.array_equal(ir.ingest_color(src, ir.BGR, mutant="bgr_on_grey"), ir.ingest_color(src, ir.BGR))
    assert not np.array_equal(ir.ingest_depth(depth, 0.001, ir.DEPTH_MUL, mutant="depth_fp32"), ir.ingest_depth(depth, 0.001, ir.DEPTH_MUL))


def _camera_maps(W, H, Ws, Hs, dist, R=None):
    """The restated maps of a W x H view of a Ws x Hs camera with fr1_desk's intrinsics scaled to each size."""
    K_src, new_K = ir.scaled_K(Ws), ir.scaled_K(W)
    return ir.undistort_map(W, H, K_src, dist, ir.inverse_newK_R(K_src, R, new_K))


def test_the_vector_path_and_the_scalar_path_give_the_same_bits():
    import torch

    W, H = 68, 36
    src = _bytes(W, H, 3, seed=1)
    depth = np.random.default_rng(2).integers(0, 65536, (H, W), dtype=np.uint16)
    maps = _camera_maps(W, H, W, H, ir.FR1_DIST)
    for m, flags in ((None, 0), (None, ir.BGR), (maps, 0), (maps, ir.ROUND_U8 | ir.BGR)):
        vec = _ingest(torch, src, flags, maps=m, W=W, H=H, depth=depth, depth_scale=5000.0)
        scalar = _ingest(torch, src, flags, maps=m, W=W, H=H, depth=depth, depth_scale=5000.0, misalign=True)   # an unaligned out_color
        ir.assert_bits_equal(scalar[0], vec[0], "scalar against vector, flags %d" % flags)
        ir.assert_bits_equal(scalar[1], vec[1], "scalar against vector depth")
        ir.assert_bits_equal(vec[0], ir.ingest_color(src, flags, m), "vector against the mirror, flags %d" % flags)


@pytest.mark.parametrize("R", [None, ROTATION_Y_2DEG], ids=["R=I", "R=2deg-about-y"])
@pytest.mark.parametrize("name,dist", [("fr1_desk", ir.FR1_DIST), ("tangential", ir.SMALL_DIST)])
@pytest.mark.parametrize("W,H", [(67, 35), (160, 120)])
def test_undistort_map_bits_against_the_restatement(W, H, name, dist, R):
    import torch
    from gsaj.ingest import UndistortMap

    K = ir.scaled_K(W)
    um = UndistortMap(W, H, K, dist, "cuda:0", R=R)
    assert np.array_equal(um.iR, ir.inverse_newK_R(K, R))
    want = ir.undistort_map(W, H, K, dist, um.iR)   # (iR is an input of the kernel: the restatement gets the very one)
    ir.assert_bits_equal(um.map_x.cpu().numpy(), want[0], "%dx%d %s map_x" % (W, H, name))
    ir.assert_bits_equal(um.map_y.cpu().numpy(), want[1], "%dx%d %s map_y" % (W, H, name))
    if R is not None:
        assert np.abs(want[0] - ir.undistort_map(W, H, K, dist, ir.inverse_newK_R(K))[0]).max() > 1.0
    for mutant in ir.MAP_MUTANTS:
        assert not np.array_equal(ir.undistort_map(W, H, K, dist, um.iR, mutant=mutant)[0], want[0]), mutant
    assert torch.isfinite(um.map_x).all() and torch.isfinite(um.map_y).all()


def _plant(maps, Ws, Hs):
    """Coordinates of every kind the kernel tells apart, planted into rows 1..4 from column 0 on (W = 160: columns a thread of the
    vector path owns four at a time; W = 67: the scalar path)."""
    mx, my = maps[0].copy(), maps[1].copy()
    xs = [3.0, 0.0, -0.5, -1.0, Ws - 1.0, Ws - 0.5, float(Ws), 1e9, -1e9, np.nan, np.inf, -np.inf, -1.0 - 2.0 ** -20, -2.0 ** -30]
    ys = [2.0, 0.0, -0.5, -1.0, Hs - 1.0, Hs - 0.5, float(Hs), 1e9, -1e9, np.nan, np.inf, -np.inf, -1.0 - 2.0 ** -20, -2.0 ** -30]
    n = len(xs)
    mx[1, :n], my[1, :n] = xs, 7.25           # x of every kind, y inside
    mx[2, :n], my[2, :n] = 11.5, ys           # y of every kind, x inside
    mx[3, :n], my[3, :n] = xs, ys             # both
    mx[4, :n], my[4, :n] = xs[::-1], ys       # mixed pairs
    return mx, my


REMAP_CASES = ((67, 35, 67, 35), (67, 35, 80, 45), (160, 120, 160, 120))   # W, H, Ws, Hs


@pytest.mark.parametrize("round_u8", [0, ir.ROUND_U8], ids=["exact", "round_u8"])
@pytest.mark.parametrize("W,H,Ws,Hs", REMAP_CASES, ids=["%dx%d-from-%dx%d" % c for c in REMAP_CASES])
def test_remap_bits_against_the_mirror_and_inside_the_float64_bound(W, H, Ws, Hs, round_u8):
    import torch

    maps = _plant(_camera_maps(W, H, Ws, Hs, ir.FR1_DIST), Ws, Hs)
    for C, bgr, pad in ((3, 0, 0), (1, ir.BGR, 3), (4, ir.BGR, 0)):
        src = _bytes(Ws, Hs, C, seed=Ws + C)
        flags = round_u8 | bgr
        tag = "%dx%d from %dx%dx%d flags %d" % (W, H, Ws, Hs, C, flags)
        got, _ = _ingest(torch, src, flags, maps=maps, W=W, H=H, pad=pad)
        ir.assert_bits_equal(got, ir.ingest_color(src, flags, maps), tag)
        value, bound, inside = ir.bilinear64(src, maps, flags)
        assert (np.abs(got.astype(np.float64) - value) <= bound).all(), tag
        assert inside.any() and not inside.all()
        with np.errstate(invalid="ignore"):
            dead = ~((maps[0] >= -1) & (maps[0] <= Ws) & (maps[1] >= -1) & (maps[1] <= Hs))
        assert dead[1:5].sum() >= 20 and (got[:, dead] == 0.0).all(), "a coordinate outside [-1, Ws] x [-1, Hs] or not finite gives 0"
        if C == 3:   # what the canaries change is in these inputs
            assert not np.array_equal(ir.ingest_color(src, flags, maps, mutant="border_clamped"), ir.ingest_color(src, flags, maps))
            if round_u8:
                assert not np.array_equal(ir.ingest_color(src, flags, maps, mutant="round_half_even"), ir.ingest_color(src, flags, maps))


def test_ingest_is_the_same_bits_run_to_run_and_on_another_stream():
    import torch

    src = _bytes(80, 45, 3, seed=4)
    depth = np.random.default_rng(4).integers(0, 65536, (120, 160), dtype=np.uint16)
    maps = _camera_maps(160, 120, 80, 45, ir.SMALL_DIST)
    kw = dict(maps=maps, W=160, H=120, depth=depth, depth_scale=5000.0)
    first, again = _ingest(torch, src, **kw), _ingest(torch, src, **kw)
    other = _ingest(torch, src, stream=torch.cuda.Stream(), **kw)
    for a, b in ((first, again), (first, other)):
        ir.assert_bits_equal(a[0], b[0], "colour run to run")
        ir.assert_bits_equal(a[1], b[1], "depth run to run")


def test_frame_ingest_from_host_arrays_through_an_undistort_map_twice_in_a_row():
    """The pinned staging buffers are reused by the second call: the event keeps it off them until the first has read them."""
    import torch
    from gsaj import _lib
    from gsaj.ingest import FrameIngest, UndistortMap

    W, H, Ws, Hs = 160, 120, 80, 45
    K_src, new_K = ir.scaled_K(Ws), ir.scaled_K(W)
    um = UndistortMap(W, H, K_src, ir.FR1_DIST, "cuda:0", new_K=new_K)
    maps = (um.map_x.cpu().numpy(), um.map_y.cpu().numpy())
    ing = FrameIngest(W, H, "cuda:0", channels=3, src_size=(Ws, Hs), undistort=um, depth_scale=0.001, depth_mul=True, bgr=True)
    keep = []
    for seed in (1, 2):
        img = _bytes(Ws, Hs, 3, seed)
        depth = np.random.default_rng(seed).integers(0, 65536, (H, W), dtype=np.uint16)
        wide = np.zeros((Hs, Ws + 3, 3), np.uint8)
        wide[:, :Ws] = img
        color, d = ing(wide[:, :Ws], depth)   # (a view whose rows are not contiguous: the staging copy takes any strides)
        keep.append((color.clone(), d.clone(), img, depth))
    for color, d, img, depth in keep:
        ir.assert_bits_equal(color.cpu().numpy(), ir.ingest_color(img, ir.BGR, maps), "FrameIngest colour")
        ir.assert_bits_equal(d.cpu().numpy(), ir.ingest_depth(depth, 0.001, ir.DEPTH_MUL), "FrameIngest depth")
    dev_img = torch.as_tensor(keep[0][2], device="cuda:0")
    color, _ = ing(dev_img, torch.as_tensor(keep[0][3], device="cuda:0"))
    assert torch.equal(color, keep[0][0].to(color.device))
    for bad in (keep[0][2].astype(np.int16), keep[0][2][:, :, :2], dev_img.cpu(), dev_img.float()):
        with pytest.raises(_lib.GsajError):
            ing(bad, keep[0][3])
    with pytest.raises(_lib.GsajError):
        ing(keep[0][2])   # made with a depth_scale: the depth must come


def test_frames_ingested_into_a_trackers_buffers_are_the_host_paths_bits_and_track():
    """The bytes round(255 colour) and the uint16 depth round(5000 depth) of one frame of the 160 x 120 world of
    tests/test_gpu_track_and_map.py, ingested straight into a GaussNewtonTracker's gt_color / gt_depth, against the reference's host
    statements (utils/dataset.py:266-276) run in torch on the CPU and uploaded.  One iteration on them returns a finite loss; no
    convergence is claimed on quantised frames."""
    import torch
    from gsaj.ingest import FrameIngest
    from test_gpu_gn_tracker import _tracker
    from test_gpu_track_and_map import H, W, _true_world

    world = _true_world(n_frames=2)
    dev, cams, frames = world[0], world[2], world[7]
    w2c = np.ascontiguousarray(cams[0]["viewmatrix"].T)
    tr = _tracker(world, w2c)
    tr.set_frame(frames[0][0], frames[0][1])   # (allocates the tracker's buffers)
    image = np.ascontiguousarray(np.rint(255.0 * frames[1][0].clamp(0, 1).permute(1, 2, 0).cpu().numpy()).astype(np.uint8))
    depth = np.rint(5000.0 * frames[1][1].cpu().numpy()).clip(0, 65535).astype(np.uint16)
    assert image.shape == (H, W, 3) and depth.shape == (H, W) and depth.max() > 5000

    color, d = FrameIngest(W, H, dev, depth_scale=5000.0)(image, depth, out_color=tr.gt_color, out_depth=tr.gt_depth)
    assert color.data_ptr() == tr.gt_color.data_ptr() and d.data_ptr() == tr.gt_depth.data_ptr()
    host_color = torch.from_numpy(image / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).to(device=dev, dtype=torch.float32)
    host_depth = torch.from_numpy(depth / 5000.0).to(device=dev, dtype=torch.float32)
    assert torch.equal(tr.gt_color.view(torch.int32), host_color.contiguous().view(torch.int32))
    assert torch.equal(tr.gt_depth.view(torch.int32), host_depth.view(torch.int32))

    tr.set_frame(color, d, w2c=w2c)
    assert tr.iterate(1) == 1
    loss = float(tr.loss_terms[0])
    assert np.isfinite(loss) and loss > 0.0
