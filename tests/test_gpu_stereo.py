"""GPU: csrc/stereo.hip and the byte remap of csrc/ingest.hip against tests/stereo_restated.py.  The matcher is integer arithmetic: its
disparity, its cost volume and its path sums are compared with torch.equal / array_equal, no tolerance anywhere; the depth and the
colour are compared bit for bit.  Every number of disparities, path count, block radius (with windows taller than the image),
uniqueness and left-right setting, at sizes with one valid column, lines of length 1 and diagonals shorter than a wave's batch; the
planted sums of tests/test_cpu_stereo.py run through the winner stage alone; gsaj.stereo's two classes with host, device and padded
inputs, twice on one object and on a side stream."""
import numpy as np
import pytest

import ingest_restated as ir
import stereo_restated as sr

pytestmark = pytest.mark.gpu

BF = 47.90639384423901   # the reference's constant for EuRoC (utils/dataset.py:388)
DEV = "cuda:0"


def _sizes(D):
    return [(W, H) for (W, H) in ((D + 1, 1), (D + 17, 9), (96, 40), (150, 33)) if W > D]


CASES = [(D, W, H) for D in (16, 32, 64, 128) for (W, H) in _sizes(D)]


def _pair(W, H, D, seed=5):
    """A textured pair whose disparity ramps over most of [0, D) with a step in it."""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    d = 0.1 * D + 0.7 * D * xs / W + np.where((ys >= H // 3) & (xs >= W // 2), 0.15 * D, 0.0)
    left, right, _ = sr.scene(W, H, None, seed=seed, d_true=np.clip(d, 0.0, D - 1.5))
    return left, right


def _matcher(W, H, **kw):
    from gsaj.stereo import StereoMatcher

    return StereoMatcher(W, H, DEV, **kw)


@pytest.mark.parametrize("D,W,H", CASES, ids=["D%d-%dx%d" % c for c in CASES])
def test_disp16_equals_the_restatement(D, W, H):
    import torch

    left, right = _pair(W, H, D)
    for r in (0, 2, 10):
        C = sr.cost_volume(left, right, D, r)
        for paths in (4, 8):
            S = sr.path_costs(C, D, 2, 5, paths)
            for u in (0, 40):
                for lr in (-1, 0, 1):
                    m = _matcher(W, H, num_disparities=D, block_radius=r, paths=paths, uniqueness=u, lr_max_diff=lr)
                    got = m(left, right)
                    want = torch.from_numpy(sr.winner(S, D, u, lr))
                    tag = "D=%d %dx%d r=%d paths=%d u=%d lr=%d" % (D, W, H, r, paths, u, lr)
                    assert got.dtype == torch.int16 and torch.equal(got.cpu(), want), "%s: %d pixels differ" % (tag, int((got.cpu() != want).sum()))
                    if u == 0 and lr == -1:   # nothing can invalidate a pixel of the valid region then
                        assert (want[:, :D] == -16).all() and (want[:, D:] >= 0).all()


def test_other_penalties_equal_the_restatement():
    import torch

    W, H, D = 96, 40, 32
    left, right = _pair(W, H, D, seed=6)
    for P1, P2 in ((0, 1), (8, 32), (1023, 1024)):
        got = _matcher(W, H, num_disparities=D, block_radius=2, P1=P1, P2=P2)(left, right)
        assert torch.equal(got.cpu(), torch.from_numpy(sr.match(left, right, D, 2, P1, P2))), (P1, P2)


@pytest.mark.parametrize("kind", sr.EDGE_KINDS + ("wide",))
def test_the_cost_volume_and_the_sums_themselves(kind):
    """C and S as the call leaves them in the workspace, so that a failure above localises to costs, paths or winner.  "wide": D = 128,
    two disparities per lane, r = 10, where S passes 65 535."""
    import torch

    if kind == "wide":
        W, H, D, r = 150, 33, 128, 10
        left, right = _pair(W, H, D)
    else:
        W, H, D, r = 96, 40, 16, 2
        left, right, _ = sr.edge_scene(W, H, kind)
    m = _matcher(W, H, num_disparities=D, block_radius=r)
    got = m(left, right)
    C = sr.cost_volume(left, right, D, r)
    S = sr.path_costs(C, D, 2, 5, 8)
    got_C = m.cost_volume().cpu().numpy().view(np.uint16).astype(np.int64)
    assert np.array_equal(got_C[:, D:], C[:, D:]), "the cost volume differs at %d entries" % int((got_C[:, D:] != C[:, D:]).sum())
    got_S = m.sums().cpu().numpy().astype(np.int64)
    assert np.array_equal(got_S, S), "the sums differ at %d entries" % int((got_S != S).sum())
    assert torch.equal(got.cpu(), torch.from_numpy(sr.winner(S, D, 40, 1)))
    if kind == "wide":
        assert S.max() > 65535


@pytest.mark.parametrize("r", [0, 15])
def test_a_second_band_of_rows_equals_the_restatement(r):
    """20 x 70, D = 16: H = 70 gives k_stereo_cost two bands of rows, the second 6 rows under a window of up to 31 -- its ring is primed
    from row 64 - r > 0 and the bottom clamp falls inside it; r = 15 uses every slot of the ring."""
    import torch

    W, H, D = 20, 70, 16
    left, right = _pair(W, H, D)
    m = _matcher(W, H, num_disparities=D, block_radius=r, paths=8, uniqueness=0, lr_max_diff=-1)
    got = m(left, right)
    C = sr.cost_volume(left, right, D, r)
    S = sr.path_costs(C, D, 2, 5, 8)
    got_C = m.cost_volume().cpu().numpy().view(np.uint16).astype(np.int64)
    assert np.array_equal(got_C[:, D:], C[:, D:]), "r=%d: the cost volume differs at %d entries" % (r, int((got_C[:, D:] != C[:, D:]).sum()))
    got_S = m.sums().cpu().numpy().astype(np.int64)
    assert np.array_equal(got_S, S), "r=%d: the sums differ at %d entries" % (r, int((got_S != S).sum()))
    assert torch.equal(got.cpu(), torch.from_numpy(sr.winner(S, D, 0, -1)))
    assert len(np.unique(C[64:, D:])) > 1 and (got[:, D:] >= 0).all()


@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_planted_sums_through_the_winner_stage_alone_and_their_depth(D):
    """Ties, d* at both ends, negative sub-pixel numerators, two left pixels at equal cost for one right column, rivals exactly at the
    uniqueness bound (tests/test_cpu_stereo.py shows the planted sums contain them): S is written into the workspace and only the
    winner stage runs.  The depth: invalid -> 0, d16 = 0 -> bf 1e-10, every other value the float64 quotient rounded once."""
    import torch
    from gsaj.stereo import STAGE_WINNER

    S = sr.planted_sums(D)
    H, W, _ = S.shape
    dummy = np.zeros((H, W), np.uint8)
    for u in (0, 40):
        for lr in (-1, 0, 1):
            m = _matcher(W, H, num_disparities=D, uniqueness=u, lr_max_diff=lr)
            m.sums().copy_(torch.from_numpy(S.astype(np.int32)))
            got, z = m(dummy, dummy, bf=BF, stages=STAGE_WINNER)
            want = sr.winner(S, D, u, lr)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (D, u, lr, int((got.cpu().numpy() != want).sum()))
            ir.assert_bits_equal(z.cpu().numpy(), sr.depth(want, BF), "depth D=%d u=%d lr=%d" % (D, u, lr))
    want = sr.winner(S, D, 40, -1)
    assert (want == 0).any() and (want == -16).any() and (sr.depth(want, BF) == np.float32(BF * 1e-10)).any()


def test_depth_of_a_scene_is_the_float64_quotient_rounded_once():
    import torch

    W, H, D = 96, 40, 16
    left, right, _ = sr.scene(W, H, "step")
    m = _matcher(W, H, num_disparities=D)
    disp16, z = m(left, right, bf=BF)
    want = sr.match(left, right, D, 10)
    assert torch.equal(disp16.cpu(), torch.from_numpy(want))
    ir.assert_bits_equal(z.cpu().numpy(), sr.depth(want, BF), "depth")
    ir.assert_bits_equal(m.depth(2.0 * BF).cpu().numpy(), sr.depth(want, 2.0 * BF), "depth(bf) of the last pair")
    out = torch.full((H, W), -1.0, device=DEV)
    assert m(left, right, bf=BF, out_depth=out)[1].data_ptr() == out.data_ptr()
    ir.assert_bits_equal(out.cpu().numpy(), sr.depth(want, BF), "out_depth")


def _maps(W, H, Ws, Hs):
    from test_gpu_ingest import _camera_maps, _plant

    return _plant(_camera_maps(W, H, Ws, Hs, ir.FR1_DIST), Ws, Hs)


@pytest.mark.parametrize("W,H,Ws,Hs", [(67, 35, 80, 45), (160, 120, 160, 120)])
def test_rectify_u8_equals_the_mirror(W, H, Ws, Hs):
    """Through maps with planted coordinates of every kind (outside, on the border, not finite), padded source and output rows; the
    bytes outside the output's rows stay as they were; the colour is the byte / 255.0f in all three planes."""
    import torch
    from gsaj import _lib

    lib = _lib.load()
    maps = _maps(W, H, Ws, Hs)
    src = np.random.default_rng(Ws).integers(0, 256, (Hs, Ws), dtype=np.uint8)
    want = sr.rectify_u8(src, maps)
    d_maps = [torch.as_tensor(np.ascontiguousarray(m, np.float32), device=DEV) for m in maps]
    for spad, opad, with_color in ((0, 0, True), (3, 5, False)):
        host = np.full((Hs, Ws + spad), 0x5A, np.uint8)
        host[:, :Ws] = src
        d_src = torch.as_tensor(host, device=DEV)
        out = torch.full((H, W + opad), 0xC3, dtype=torch.uint8, device=DEV)
        color = torch.full((3, H, W), -1.0, device=DEV) if with_color else None
        _lib.check(lib.gsaj_rectify_u8(W, H, Ws, Hs, Ws + spad, d_src.data_ptr(), d_maps[0].data_ptr(), d_maps[1].data_ptr(), out.data_ptr(),
                                       W + opad, None if color is None else color.data_ptr(), torch.cuda.current_stream().cuda_stream), "gsaj_rectify_u8")
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :W], want), "%d bytes differ" % int((got[:, :W] != want).sum())
        assert (got[:, W:] == 0xC3).all()
        if with_color:
            ir.assert_bits_equal(color.cpu().numpy(), ir.ingest_color(src, ir.ROUND_U8, maps), "colour")
    assert (want == 0).any() and want.max() > 200
    same = torch.as_tensor(src, device=DEV)   # without maps the bytes are copied
    out = torch.zeros((Hs, Ws), dtype=torch.uint8, device=DEV)
    _lib.check(lib.gsaj_rectify_u8(Ws, Hs, Ws, Hs, Ws, same.data_ptr(), None, None, out.data_ptr(), Ws, None, torch.cuda.current_stream().cuda_stream), "gsaj_rectify_u8")
    assert torch.equal(out, same)


def _stereo_rig(W, H, Ws, Hs):
    """Two cameras with fr1_desk's distortion, the right one turned a little: UndistortMap objects and their maps as NumPy arrays."""
    from gsaj.ingest import UndistortMap
    from test_gpu_ingest import ROTATION_Y_2DEG

    K_src, new_K = ir.scaled_K(Ws), ir.scaled_K(W)
    ul = UndistortMap(W, H, K_src, ir.FR1_DIST, DEV, new_K=new_K)
    ur = UndistortMap(W, H, K_src, ir.SMALL_DIST, DEV, R=ROTATION_Y_2DEG, new_K=new_K)
    return ul, ur, [(u.map_x.cpu().numpy(), u.map_y.cpu().numpy()) for u in (ul, ur)]


def test_stereo_ingest_gives_the_frame_ingests_colour_and_the_restated_depth():
    import torch
    from gsaj import StereoIngest
    from gsaj.ingest import FrameIngest

    W, H, Ws, Hs, D = 96, 40, 120, 50, 16
    ul, ur, maps = _stereo_rig(W, H, Ws, Hs)
    rng = np.random.default_rng(11)
    left_src = rng.integers(0, 256, (Hs, Ws), dtype=np.uint8)
    right_src = np.roll(left_src, -6, axis=1)
    s = StereoIngest(W, H, DEV, BF, undistort_left=ul, undistort_right=ur, src_size=(Ws, Hs), num_disparities=D, block_radius=2)
    color, depth = s(left_src, right_src)
    assert color.shape == (3, H, W) and color.dtype == torch.float32 and depth.shape == (H, W) and depth.dtype == torch.float32
    through_map, _ = FrameIngest(W, H, DEV, channels=1, src_size=(Ws, Hs), undistort=ul, round_u8=True)(left_src)
    assert torch.equal(color.view(torch.int32), through_map.view(torch.int32)), "colour against FrameIngest through the same map"
    rect_l, rect_r = sr.rectify_u8(left_src, maps[0]), sr.rectify_u8(right_src, maps[1])
    assert np.array_equal(s.rect.cpu().numpy(), np.stack([rect_l, rect_r]))
    of_bytes, _ = FrameIngest(W, H, DEV, channels=1)(s.rect[0])
    assert torch.equal(color.view(torch.int32), of_bytes.view(torch.int32)), "colour against FrameIngest of the rectified bytes"
    ir.assert_bits_equal(depth.cpu().numpy(), sr.depth(sr.match(rect_l, rect_r, D, 2), BF), "depth")
    assert (depth > 0).any()
    # into a caller's buffers; device inputs; already rectified images need no maps
    oc, oz = torch.empty((3, H, W), device=DEV), torch.empty((H, W), device=DEV)
    c2, z2 = s(torch.as_tensor(left_src, device=DEV), torch.as_tensor(right_src, device=DEV), out_color=oc, out_depth=oz)
    assert c2.data_ptr() == oc.data_ptr() and z2.data_ptr() == oz.data_ptr() and torch.equal(oc, color) and torch.equal(oz, depth)
    c3, z3 = StereoIngest(W, H, DEV, BF, num_disparities=D, block_radius=2)(rect_l, rect_r)
    assert torch.equal(c3, color) and torch.equal(z3, depth)
    from gsaj import _lib

    for bad in (left_src.astype(np.int16), left_src[:, :-1], torch.as_tensor(left_src), torch.as_tensor(left_src, device=DEV).float()):
        with pytest.raises(_lib.GsajError):
            s(bad, right_src)
    with pytest.raises(_lib.GsajError):
        StereoIngest(W, H, DEV, BF, undistort_left=ul)
    with pytest.raises(_lib.GsajError):
        StereoIngest(W, H, "cpu", BF)


def test_padded_device_rows_and_host_arrays_give_the_same_result():
    import torch

    W, H, D = 150, 33, 32
    left, right = _pair(W, H, D, seed=8)
    m = _matcher(W, H, num_disparities=D, block_radius=2)
    from_host = m(left, right).clone()
    wide = np.full((2, H, W + 7), 0x5A, np.uint8)
    wide[0, :, :W], wide[1, :, :W] = left, right
    d_wide = torch.as_tensor(wide, device=DEV)
    padded = m(d_wide[0, :, :W], d_wide[1, :, :W]).clone()
    view = np.zeros((H, W + 3), np.uint8)
    view[:, :W] = left
    strided_host = m(view[:, :W], right).clone()   # (a host view whose rows are not contiguous: the staging copy takes any strides)
    want = torch.from_numpy(sr.match(left, right, D, 2))
    assert torch.equal(from_host.cpu(), want) and torch.equal(padded.cpu(), want) and torch.equal(strided_host.cpu(), want)


def test_two_calls_on_one_object_each_give_their_own_result():
    """S is summed into with atomics and disp2 is a minimum: both must start afresh.  The second pair is flat -- every sum 0 -- so
    anything left over from the first would show; then the first pair again."""
    import torch

    W, H, D = 96, 40, 16
    first = sr.scene(W, H, "step")[:2]
    flat = np.full((H, W), 90, np.uint8)
    m = _matcher(W, H, num_disparities=D, block_radius=2)
    got = [m(*pair).clone() for pair in (first, (flat, flat), first)]
    assert (m.sums().cpu().numpy() == sr.match(*first, D, 2, want_S=True)[1]).all()
    want = torch.from_numpy(sr.match(*first, D, 2))
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[2].cpu(), want)
    assert torch.equal(got[1].cpu(), torch.from_numpy(sr.match(flat, flat, D, 2))) and (got[1][:, D:] == 0).all()


def test_a_result_made_on_a_side_stream_is_correct_after_its_synchronize():
    import torch

    W, H, D = 150, 33, 64
    left, right = _pair(W, H, D, seed=9)
    d_left, d_right = torch.as_tensor(left, device=DEV), torch.as_tensor(right, device=DEV)
    m = _matcher(W, H, num_disparities=D, block_radius=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        disp16, z = m(d_left, d_right, bf=BF)
    side.synchronize()
    want = sr.match(left, right, D, 2)
    assert torch.equal(disp16.cpu(), torch.from_numpy(want))
    ir.assert_bits_equal(z.cpu().numpy(), sr.depth(want, BF), "depth on a side stream")
