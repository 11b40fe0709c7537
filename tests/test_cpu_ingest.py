"""CPU: the arithmetic of the frame ingest (csrc/ingest.hip) as tests/ingest_restated.py restates it -- the premises the kernel's
formulas rest on (byte and depth exactness), the identity calibration, a round trip through a distorted picture of an analytic
image, and the canaries: every mutant of the map must break the round trip's bound, every mutant of the kernel must change bits
on the inputs the GPU tests compare.  No GPU, no library."""
import numpy as np
import pytest

import ingest_restated as ir

F = np.float32
SIZES = ((67, 35), (160, 120))
DISTS = (("fr1_desk", ir.FR1_DIST), ("tangential", ir.SMALL_DIST))
CASES = [(W, H, name, dist) for (W, H) in SIZES for (name, dist) in DISTS]
IDS = ["%dx%d-%s" % c[:3] for c in CASES]


def test_float32_division_by_255_is_the_references_float64_divide_and_cast_for_every_byte():
    k = np.arange(256)
    want = (k / 255.0).astype(F)                       # image / 255.0, then .to(float32)
    got = (k.astype(F) / F(255.0)).astype(F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ir.ingest_color(k.astype(np.uint8).reshape(16, 16))[0].reshape(-1).view(np.uint32), want.view(np.uint32))
    recip = (k.astype(F) * F(1.0 / 255.0)).astype(F)   # what the kernel must NOT do
    assert int((recip.view(np.uint32) != want.view(np.uint32)).sum()) == 126


@pytest.mark.parametrize("scale,mul", [(5000.0, False), (6553.5, False), (1000.0, False), (0.001, True)])
def test_depth_is_numpys_float64_result_cast_once(scale, mul):
    d = np.array([[0, 1, 65535]], np.uint16)
    ref = (d * scale if mul else d / scale)            # np.array(Image.open(path)) / depth_scale: float64
    assert ref.dtype == np.float64
    got = ir.ingest_depth(d, scale, ir.DEPTH_MUL if mul else 0)
    assert got.dtype == F and np.array_equal(got.view(np.uint32), ref.astype(F).view(np.uint32))
    full = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    want = (full * scale if mul else full / scale).astype(F)
    assert np.array_equal(ir.ingest_depth(full, scale, ir.DEPTH_MUL if mul else 0).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("W,H", SIZES)
def test_identity_calibration_gives_the_pixel_grid_and_the_direct_paths_bits(W, H):
    """With intrinsics that float64 holds and inverts exactly the map is (u, v) itself.  With fr1_desk's, (u - cx) / fx * fx + cx
    leaves a float64 residue of a few 1e-15, which the cast to float32 absorbs everywhere but at u = 0 and v = 0, where the
    coordinate may come out as -3.6e-15 instead of 0: the bilinear then weighs the outside tap with 0 and the pixel itself with
    1.0f - 0.0f, so the remap through either map is the direct path bit for bit."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    src = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for K, exact in (((128.0, 64.0, 32.5, 16.25), True), (ir.scaled_K(W), False)):
        mx, my = ir.undistort_map(W, H, K, (0.0,) * 5, ir.inverse_newK_R(K))
        if exact:
            assert np.array_equal(mx, u.astype(F)) and np.array_equal(my, v.astype(F))
        assert np.abs(mx - u).max() < 1e-13 and np.abs(my - v).max() < 1e-13
        for flags in (0, ir.BGR, ir.ROUND_U8):
            ir.assert_bits_equal(ir.ingest_color(src, flags, (mx, my)), ir.ingest_color(src, flags & ir.BGR), "identity map, flags %d" % flags)


@pytest.mark.parametrize("W,H,name,dist", CASES, ids=IDS)
def test_round_trip_through_a_distorted_picture_stays_inside_the_bilinear_bound(W, H, name, dist):
    err, bound, share = ir.round_trip(W, H, dist)
    print("%dx%d %s: error %.3f grey levels, bound %.3f, %.3f of the frame compared" % (W, H, name, err, bound, share))
    assert share >= 0.85, share
    assert err < bound, (err, bound)


@pytest.mark.parametrize("mutant", ir.MAP_MUTANTS)
@pytest.mark.parametrize("W,H,name,dist", CASES, ids=IDS)
def test_every_mutant_of_the_map_breaks_the_round_trip(W, H, name, dist, mutant):
    err, bound, _ = ir.round_trip(W, H, dist, mutant=mutant)
    print("%dx%d %s %s: error %.3f grey levels, bound %.3f" % (W, H, name, mutant, err, bound))
    assert err > bound, (mutant, err, bound)


def test_the_float32_mirror_stays_inside_the_float64_bilinears_rounding_bound():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (45, 80, 3), dtype=np.uint8)
    mx = rng.uniform(-3.0, 83.0, (35, 67)).astype(F)
    my = rng.uniform(-3.0, 48.0, (35, 67)).astype(F)
    mx[0, :8] = F([-1.0, -0.5, -2.0 ** -30, 0.0, 79.0, 79.5, 80.0, np.nan])
    for flags in (0, ir.ROUND_U8, ir.BGR):
        got = ir.ingest_color(src, flags, (mx, my)).astype(np.float64)
        value, bound, inside = ir.bilinear64(src, (mx, my), flags)
        assert inside.any() and not inside.all()
        assert (np.abs(got - value) <= bound).all(), float((np.abs(got - value) - bound).max())


def test_every_mutant_of_the_kernel_changes_bits_on_the_gpu_tests_inputs():
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (45, 80, 3), dtype=np.uint8)
    K = ir.scaled_K(67)
    maps = ir.undistort_map(67, 35, K, ir.FR1_DIST, ir.inverse_newK_R(K))   # reaches outside the source at the frame's corners
    differs = lambda a, b: not np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    assert differs(ir.ingest_color(src[:35, :67], 0, maps, mutant="border_clamped"), ir.ingest_color(src[:35, :67], 0, maps))
    half = (np.zeros((4, 4), F) + F(0.5), np.arange(16, dtype=F).reshape(4, 4) % 3)   # midway between two columns: val = k + 0.5
    ramp = np.tile(np.arange(8, dtype=np.uint8), (4, 1))
    assert differs(ir.ingest_color(ramp, ir.ROUND_U8, half, mutant="round_half_even"), ir.ingest_color(ramp, ir.ROUND_U8, half))
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert differs(ir.ingest_color(grey, ir.BGR, mutant="bgr_on_grey"), ir.ingest_color(grey, ir.BGR))
    d = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    # float32 arithmetic on the depth shows where the scale is no float32: 0.001 (a RealSense's unit) and 1000 / 3 are not.  5000, 6553.5
    # and 1000 are, and a correctly rounded float32 quotient of two float32 values is then the float64 one rounded once (no double
    # rounding case among the 65536 depths): the GPU tests therefore compare a depth with x 0.001 as well
    for scale, flags in ((0.001, ir.DEPTH_MUL), (1000.0 / 3.0, 0)):
        assert differs(ir.ingest_depth(d, scale, flags, mutant="depth_fp32"), ir.ingest_depth(d, scale, flags))
    for scale in (5000.0, 6553.5, 1000.0):
        assert not differs(ir.ingest_depth(d, scale, 0, mutant="depth_fp32"), ir.ingest_depth(d, scale, 0))
