"""CPU: every argument error of gsaj_rgbd_align comes back as GSAJ_ERR_INVALID_ARGUMENT with its message before any launch -- the call is
made with pointers nothing may read (abi.X), so a launch would not come back at all.  No GPU."""
import os

import numpy as np
import pytest

from abi import X, call

INVALID_ARGUMENT = -1
GOOD = dict(W=80, H=60, fx=70.0, fy=70.0, cx=40.0, cy=30.0, ref_color=X, ref_depth=X, ref_w2c=X, cur_color=X, cur_depth=X, gn_state=X,
            w_depth=1.0, delta_photo=0.01, delta_depth=0.01, depth_edge_ratio=0.1, min_depth=0.01, max_depth=100.0, min_overlap=0.0, rows=X,
            gn_row=X, pix_out=X, valid_out=X, skip=None, stream=None)
MESSAGE = ("gsaj_rgbd_align: W and H must be 2..16384; ref_color, ref_depth, ref_w2c, cur_color, gn_state, rows and gn_row are required; "
           "fx, fy, delta_photo, delta_depth > 0; w_depth, depth_edge_ratio >= 0; 0 < min_depth < max_depth; min_overlap in [0, 1] "
           "(W=%d H=%d fx=%g fy=%g w_depth=%g delta_photo=%g delta_depth=%g depth_edge_ratio=%g min_depth=%g max_depth=%g min_overlap=%g)")
NAN, INF = float("nan"), float("inf")
ROWS = [
    ("W = 1", dict(W=1)), ("H = 1", dict(H=1)), ("W = 0", dict(W=0)), ("H < 0", dict(H=-3)), ("W > 16384", dict(W=16385)),
    ("H > 16384", dict(H=16385)),
    ("NULL ref_color", dict(ref_color=None)), ("NULL ref_depth", dict(ref_depth=None)), ("NULL ref_w2c", dict(ref_w2c=None)),
    ("NULL cur_color", dict(cur_color=None)), ("NULL gn_state", dict(gn_state=None)), ("NULL rows", dict(rows=None)),
    ("NULL gn_row", dict(gn_row=None)),
    ("fx = 0", dict(fx=0.0)), ("fy < 0", dict(fy=-70.0)), ("fx is NaN", dict(fx=NAN)),
    ("delta_photo = 0", dict(delta_photo=0.0)), ("delta_depth < 0", dict(delta_depth=-0.01)), ("delta_depth is NaN", dict(delta_depth=NAN)),
    ("w_depth < 0", dict(w_depth=-1.0)), ("depth_edge_ratio < 0", dict(depth_edge_ratio=-0.1)),
    ("min_depth = 0", dict(min_depth=0.0)), ("min_depth = max_depth", dict(min_depth=2.0, max_depth=2.0)),
    ("min_depth > max_depth", dict(min_depth=3.0, max_depth=2.0)), ("max_depth is NaN", dict(max_depth=NAN)),
    ("min_overlap < 0", dict(min_overlap=-0.1)), ("min_overlap > 1", dict(min_overlap=1.5)), ("min_overlap is NaN", dict(min_overlap=NAN)),
]


def _lib():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _message(kw):
    f = lambda k: float(np.float32(kw[k]))   # noqa: E731  (the call takes floats; the message prints them as doubles)
    return MESSAGE % (kw["W"], kw["H"], f("fx"), f("fy"), f("w_depth"), f("delta_photo"), f("delta_depth"), f("depth_edge_ratio"), f("min_depth"),
                      f("max_depth"), f("min_overlap"))


@pytest.mark.parametrize("what,kw", ROWS, ids=[r[0] for r in ROWS])
def test_bad_alignment_call_is_refused_with_its_code_and_message_before_any_launch(what, kw):
    lib = _lib()
    args = dict(GOOD, **kw)
    assert call(lib, "gsaj_rgbd_align", **args) == INVALID_ARGUMENT, (what, lib.gsaj_last_error())
    got = lib.gsaj_last_error().decode()
    assert got.startswith("gsaj_rgbd_align: "), "the message names the function"
    assert got == _message(args), what
