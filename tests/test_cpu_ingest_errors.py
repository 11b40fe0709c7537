"""CPU: every argument error of gsaj_undistort_map and gsaj_frame_ingest, as a table of bad calls with the return code and the whole
gsaj_last_error() text each one gets, in the pattern of tests/test_cpu_api_errors.py.  Every row is rejected before any HIP call (the
device pointers are made-up numbers), so no kernel is launched."""
import ctypes
import os

import pytest

from abi import X, call

INVALID = -1  # GSAJ_ERR_INVALID_ARGUMENT
_K = (ctypes.c_double * 4)(140.0, 140.0, 33.0, 17.0)
_DIST = (ctypes.c_double * 5)(0.1, -0.2, 0.001, 0.002, 0.05)
_IR = (ctypes.c_double * 9)(1.0 / 140.0, 0.0, -33.0 / 140.0, 0.0, 1.0 / 140.0, -17.0 / 140.0, 0.0, 0.0, 1.0)
HOST = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
# well-formed calls at 67 x 35 which no test makes: each row overrides the names that carry its defect
GOOD = {
    "gsaj_undistort_map": dict(W=67, H=35, K_src=HOST(_K), dist=HOST(_DIST), iR=HOST(_IR), map_x=X, map_y=X, stream=None),
    "gsaj_frame_ingest": dict(W=67, H=35, Ws=80, Hs=45, channels=3, src_stride=240, src=X, map_x=X, map_y=X, depth_raw=X, depth_stride=134,
                              depth_scale=5000.0, flags=0, out_color=X, out_depth=X, stream=None),
}
NO_MAP = dict(map_x=None, map_y=None, Ws=67, Hs=35, src_stride=201)
SIZES = "gsaj_frame_ingest: W, H, Ws and Hs must be positive with W * H and Ws * Hs <= INT_MAX (W=%d H=%d Ws=%d Hs=%d)"
# (entry point, the defect, what the row changes, gsaj_last_error())
ROWS = [
    ("gsaj_undistort_map", "W <= 0", dict(W=0), "gsaj_undistort_map: W and H must be positive with W * H <= INT_MAX (W=0 H=35)"),
    ("gsaj_undistort_map", "H <= 0", dict(H=-3), "gsaj_undistort_map: W and H must be positive with W * H <= INT_MAX (W=67 H=-3)"),
    ("gsaj_undistort_map", "W * H > INT_MAX", dict(W=65536, H=32768),
     "gsaj_undistort_map: W and H must be positive with W * H <= INT_MAX (W=65536 H=32768)"),
    ("gsaj_undistort_map", "NULL K_src", dict(K_src=None), "gsaj_undistort_map: K_src, dist, iR, map_x and map_y are required"),
    ("gsaj_undistort_map", "NULL dist", dict(dist=None), "gsaj_undistort_map: K_src, dist, iR, map_x and map_y are required"),
    ("gsaj_undistort_map", "NULL iR", dict(iR=None), "gsaj_undistort_map: K_src, dist, iR, map_x and map_y are required"),
    ("gsaj_undistort_map", "NULL map_y", dict(map_y=None), "gsaj_undistort_map: K_src, dist, iR, map_x and map_y are required"),
    ("gsaj_undistort_map", "two defects: the size wins over the NULL pointer", dict(W=0, iR=None),
     "gsaj_undistort_map: W and H must be positive with W * H <= INT_MAX (W=0 H=35)"),
    ("gsaj_frame_ingest", "W <= 0", dict(W=0), SIZES % (0, 35, 80, 45)),
    ("gsaj_frame_ingest", "H <= 0", dict(H=-1), SIZES % (67, -1, 80, 45)),
    ("gsaj_frame_ingest", "Ws <= 0", dict(Ws=0), SIZES % (67, 35, 0, 45)),
    ("gsaj_frame_ingest", "Hs <= 0", dict(Hs=0), SIZES % (67, 35, 80, 0)),
    ("gsaj_frame_ingest", "channels = 2", dict(channels=2), "gsaj_frame_ingest: channels must be 1, 3 or 4 (channels=2)"),
    ("gsaj_frame_ingest", "channels = 0", dict(channels=0), "gsaj_frame_ingest: channels must be 1, 3 or 4 (channels=0)"),
    ("gsaj_frame_ingest", "unknown flag bit", dict(flags=8), "gsaj_frame_ingest: unknown flag bits (flags=0x8)"),
    ("gsaj_frame_ingest", "NULL src", dict(src=None), "gsaj_frame_ingest: src and out_color are required"),
    ("gsaj_frame_ingest", "NULL out_color", dict(out_color=None), "gsaj_frame_ingest: src and out_color are required"),
    ("gsaj_frame_ingest", "src_stride < Ws * channels", dict(src_stride=239),
     "gsaj_frame_ingest: src_stride 239 is less than Ws * channels = 240"),
    ("gsaj_frame_ingest", "map_x without map_y", dict(map_y=None), "gsaj_frame_ingest: map_x and map_y must be given together or not at all"),
    ("gsaj_frame_ingest", "map_y without map_x", dict(map_x=None), "gsaj_frame_ingest: map_x and map_y must be given together or not at all"),
    ("gsaj_frame_ingest", "no map and a source of another size", dict(map_x=None, map_y=None),
     "gsaj_frame_ingest: without a map the source must have the output's size (W=67 H=35 Ws=80 Hs=45)"),
    ("gsaj_frame_ingest", "depth_raw without out_depth", dict(out_depth=None),
     "gsaj_frame_ingest: depth_raw and out_depth must be given together or not at all"),
    ("gsaj_frame_ingest", "out_depth without depth_raw", dict(depth_raw=None),
     "gsaj_frame_ingest: depth_raw and out_depth must be given together or not at all"),
    ("gsaj_frame_ingest", "depth_stride < 2 W", dict(depth_stride=132), "gsaj_frame_ingest: depth_stride 132 is less than 2 * W = 134"),
    ("gsaj_frame_ingest", "odd depth_stride", dict(depth_stride=135),
     "gsaj_frame_ingest: depth_raw and depth_stride must be 2-byte aligned (depth_stride=135)"),
    ("gsaj_frame_ingest", "depth_scale = 0", dict(depth_scale=0.0), "gsaj_frame_ingest: depth_scale must be finite and not zero (depth_scale=0)"),
    ("gsaj_frame_ingest", "depth_scale is NaN", dict(depth_scale=float("nan")),
     "gsaj_frame_ingest: depth_scale must be finite and not zero (depth_scale=nan)"),
    ("gsaj_frame_ingest", "depth_scale is infinite", dict(depth_scale=float("inf")),
     "gsaj_frame_ingest: depth_scale must be finite and not zero (depth_scale=inf)"),
    ("gsaj_frame_ingest", "out_color not 4-byte aligned", dict(out_color=X + 2),
     "gsaj_frame_ingest: out_color, out_depth, map_x and map_y must be 4-byte aligned"),
    ("gsaj_frame_ingest", "no map: the direct form's own stride check", dict(NO_MAP, src_stride=200),
     "gsaj_frame_ingest: src_stride 200 is less than Ws * channels = 201"),
    ("gsaj_frame_ingest", "two defects: the size wins over the channels", dict(W=0, channels=5), SIZES % (0, 35, 80, 45)),
    ("gsaj_frame_ingest", "two defects: the channels win over the flags", dict(channels=5, flags=64),
     "gsaj_frame_ingest: channels must be 1, 3 or 4 (channels=5)"),
    ("gsaj_frame_ingest", "a zero depth_scale without depth is not looked at: the NULL src is what is wrong",
     dict(depth_raw=None, out_depth=None, depth_scale=0.0, src=None), "gsaj_frame_ingest: src and out_color are required"),
]


def _lib():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("name,what,kw,msg", ROWS, ids=["%s: %s" % (r[0][5:], r[1]) for r in ROWS])
def test_bad_ingest_call_is_refused_with_its_code_and_message_before_any_launch(name, what, kw, msg):
    lib = _lib()
    assert call(lib, name, **dict(GOOD[name], **kw)) == INVALID, (name, what, lib.gsaj_last_error())
    assert lib.gsaj_last_error().decode() == msg, (name, what)


def test_the_table_covers_both_entry_points():
    assert {r[0] for r in ROWS} == set(GOOD)
