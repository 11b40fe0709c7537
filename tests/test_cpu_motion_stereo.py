"""CPU: motion stereo (include/gsaj.h "motion stereo", csrc/sweep.hip, gsaj.motion_stereo) as far as it goes without a GPU: the
restatement of tests/sweep_restated.py meets the quality conditions on the analytic scene and its number ranges at the extremes, every
mutant changes a quantity the GPU tests compare on a committed case, the planted sums contain the winner's edges, the header declares
the entry points and gsaj/_lib.py binds them, every argument error comes back before any launch, and the workspace size is the layout
written out here a second time."""
import ctypes
import os

import numpy as np
import pytest

import sweep_restated as sw
from abi import X, call, declarations

INVALID_ARGUMENT, WORKSPACE_TOO_SMALL = -1, -3
COMPARED = ("grad", "pc", "C", "S", "idx16", "depth")   # what tests/test_gpu_motion_stereo.py holds the device to
_MEMO = {}


def _lib():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _scene(motion, D=16):
    """The conditions' setting: 160 x 120, r = 3, P1 = 100, P2 = 400, 8 paths, u = 10, outside_cost 80, w in [0.2, 0.7]."""
    if (motion, D) not in _MEMO:
        c = sw.case(160, 120, motion)
        _MEMO[(motion, D)] = (c, sw.run(c, 0.2, 0.7, D=D))
    return _MEMO[(motion, D)]


# ---- the conditions on the algorithm -----------------------------------------------------------------------------------------------------
# (valid, within 10 %, median relative error) this restatement gives: the figures of the issue's prototype, digit for digit
FIGURES = {"sideways": (0.947, 0.921, 0.011), "mixed": (0.987, 0.886, 0.013), "forward": (0.826, 0.859, 0.019)}
BOUNDS = {"sideways": (0.85, 0.80), "mixed": (0.85, 0.80), "forward": (0.70, 0.75)}


@pytest.mark.parametrize("motion", sorted(FIGURES))
def test_depth_of_the_analytic_scene_meets_the_conditions(motion):
    c, out = _scene(motion)
    valid, within, median = sw.quality(out, c["truth"])
    print("%s: valid %.3f within 10 %% %.3f median %.4f" % (motion, valid, within, median))
    assert np.allclose((valid, within, median), FIGURES[motion], atol=6e-4), "the restatement no longer gives the figures DESIGN 7i records"
    assert valid >= BOUNDS[motion][0] and within >= BOUNDS[motion][1] and median <= 0.04
    z = out["depth"]
    assert z.dtype == np.float32 and ((z == 0) == (out["idx16"] < 0)).all() and (z[out["idx16"] >= 0] > 0).all()


def test_twice_the_hypotheses_do_not_push_the_depth_to_the_far_side():
    """The fixed-point bilinear against nearest-neighbour sampling: with hypotheses closer than a pixel of parallax the costs must not
    tie in runs (the lowest d would win each)."""
    c, out = _scene("sideways", D=32)
    valid, within, median = sw.quality(out, c["truth"])
    print("sideways D=32: valid %.3f within 10 %% %.3f median %.4f" % (valid, within, median))
    assert median <= 0.03


# ---- the mutants ------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return [k for k in COMPARED if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


@pytest.mark.parametrize("mutant", sw.MUTANTS)
def test_every_mutant_changes_a_compared_quantity_of_a_committed_case(mutant):
    """The cases are those of tests/test_gpu_motion_stereo.py at 96 x 40 (sideways and forward) and its planted sums."""
    changed = set()
    for motion in ("sideways", "forward"):
        c = sw.case(96, 40, motion)
        key = ("mut", motion)
        if key not in _MEMO:
            _MEMO[key] = sw.run(c, 0.2, 0.7)
        changed |= set(_differs(_MEMO[key], sw.run(c, 0.2, 0.7, mutant=mutant)))
    cam, rw, sw_, w_min, w_max = sw.planted_cam()
    T = sw.rel_pose(rw, sw_)
    step, w = sw.hypotheses(w_min, w_max, 16)
    S = sw.planted_sums(16)
    for u in (0, 40):
        good, bad = sw.winner(S, cam, T, w, u), sw.winner(S, cam, T, w, u, mutant=mutant)
        if not np.array_equal(good, bad):
            changed.add("idx16 (planted)")
        if not np.array_equal(sw.depth(good, w_min, step), sw.depth(good, w_min, step, mutant=mutant)):
            changed.add("depth (planted)")
    assert changed, "mutant %s changes nothing that is compared" % mutant
    expect = {"gy_sign_flipped": "grad", "tie_highest": "idx16 (planted)", "subpixel_floor": "idx16 (planted)",
              "centre_outside_kept": "idx16 (planted)", "depth_one_over_idx": "depth", "outside_costs_0": "pc", "shift_5": "pc"}
    if mutant in expect:
        assert expect[mutant] in changed, (mutant, sorted(changed))


def test_planted_sums_contain_the_edges_of_the_winner():
    D = 16
    cam, rw, sw_, w_min, w_max = sw.planted_cam()
    T, (step, w) = sw.rel_pose(rw, sw_), sw.hypotheses(w_min, w_max, D)
    S = sw.planted_sums(D)
    H, W, _ = S.shape
    assert (cam["W"], cam["H"]) == (W, H)
    centre = np.stack([sw.warp(cam, T, wd)[0] for wd in w], -1)
    assert centre[:H - 1, :W - 1].all() and not centre[:, W - 1].any() and not centre[H - 1].any()
    best = S.min(-1)
    assert ((S[0] == best[0][:, None]).sum(-1) == 2).all()                                       # exact ties
    assert set(S[1].argmin(-1).tolist()) == {0, D - 1}                                            # both ends
    d = S[2].argmin(-1)
    sm, sp = S[2][np.arange(W), d - 1], S[2][np.arange(W), d + 1]
    den = np.maximum(sm + sp - 2 * best[2], 1)
    num = (sm - sp) * 16 + den
    assert (num < 0).any() and (num[num < 0] % (2 * den[num < 0]) != 0).any()                     # negative, not dividing evenly
    d = S[3].argmin(-1)
    assert (S[3][np.arange(W), d + 2] * 60 == best[3] * 100).all()                                # exactly at the bound for u = 40
    assert (S[4][np.arange(W), d + 2] * 60 < best[4] * 100).all()                                 # one below it
    got = sw.winner(S, cam, T, w, 40)
    assert (got[3, :W - 1] >= 0).all() and (got[4] == -16).all() and (got[:, W - 1] == -16).all() and (got[H - 1] == -16).all()
    free = sw.winner(S, cam, T, w, 0)   # (with u = 40 the far twin of a tie is a rival)
    assert (np.abs(free[0, :W - 1] - 16 * S[0, :W - 1].argmin(-1)) <= 8).all()   # the lower d of each tie, half a step at most beside it
    assert (got[0, 1:W - 1:2] == -16).all() and (got[0, 0:W - 1:2] >= 0).all()
    assert set(got[1, :W - 1].tolist()) == {0, 16 * (D - 1)}
    z = sw.depth(got, w_min, step)
    assert z[1, 0] == np.float32(1.0 / np.float64(np.float32(w_min))) and (z[got < 0] == 0).all()
    assert sw.depth(np.array([[0, 16, -16]], np.int16), 0.0, 0.25).tolist() == [[0.0, 4.0, 0.0]]   # w = 0: a point at infinity, depth 0


# ---- number ranges at the extremes ----------------------------------------------------------------------------------------------------
def test_pc_C_and_S_stay_in_their_types_at_the_extremes():
    """r = 7, 8 paths, P2 = 1024.  A checkerboard (every gradient byte clipped to 0 or 30) against a flat image (15), and an image
    pair with nothing inside at outside_cost = 240, where C reaches 225 * 240 exactly."""
    W, H, D = 40, 36, 16
    ys, xs = np.mgrid[0:H, 0:W]
    board = np.where((xs + ys) % 2 == 0, 255, 0).astype(np.uint8)
    board2 = np.where((xs // 2 + ys // 2) % 2 == 0, 255, 0).astype(np.uint8)
    flat = np.full((H, W), 128, np.uint8)
    cam = dict(W=W, H=H, fx=35.0, fy=35.0, cx=W / 2.0, cy=H / 2.0)
    rw = sw.ref_pose().astype(np.float32)
    side = (sw.gn.se3_exp(np.array([0.1, 0, 0, 0, 0, 0.0])) @ sw.ref_pose()).astype(np.float32)
    away = (sw.gn.se3_exp(np.array([0, 0, 0, 0, 3.0, 0.0])) @ sw.ref_pose()).astype(np.float32)   # turned by 3 rad: p_z < 0 everywhere
    top = 0
    for ref, src, pose, oc in ((board2, flat, side, 240), (board2, board2[:, ::-1].copy(), side, 0), (board, flat, away, 240)):
        out = sw.sweep(ref, src, cam, rw, pose, 0.0, 1.0, D=D, r=7, P1=1023, P2=1024, paths=8, uniqueness=0, outside_cost=oc)
        assert 0 <= out["pc"].min() and out["pc"].max() <= 240
        assert out["C"].max() <= 54000 and out["S"].max() < 2 ** 25 and out["S"].min() >= 0
        top = max(top, int(out["C"].max()))
    assert top == 225 * 240 and out["pc"].min() == 240 and (out["idx16"] == -16).all()
    g = sw.gradients(board2)
    assert set(np.unique(g[0]).tolist()) <= {0, 15, 30} and g[0].min() == 0 and g[0].max() == 30


# ---- header and binding -----------------------------------------------------------------------------------------------------------------
NEW = {"gsaj_motion_stereo_bytes": 5, "gsaj_debug_motion_stereo_offsets": 7, "gsaj_motion_stereo": 27, "gsaj_grey_u8": 6}


def test_the_header_declares_the_entry_points_and_the_binding_matches():
    from gsaj import _lib as L

    lib = _lib()
    decls = declarations()
    for name, arity in NEW.items():
        assert name in decls and decls[name][0] == "int" and len(decls[name][1]) == arity, (name, decls.get(name))
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == arity and L.SIGNATURES[name][0] is ctypes.c_int, name
        assert hasattr(lib, name)
    assert lib.gsaj_version() >= 114
    names = [p for _, p in decls["gsaj_motion_stereo"][1]]
    assert names == ["W", "H", "ref", "ref_stride", "src", "src_stride", "fx", "fy", "cx", "cy", "ref_w2c", "src_w2c", "w_min", "w_max", "D", "r", "P1",
                     "P2", "paths", "uniqueness", "outside_cost", "stages", "workspace", "workspace_bytes", "idx16", "out_depth", "stream"]
    assert not any(n.endswith("_workspace_bytes") for n in NEW)   # (the guarded run: test_motion_stereo of tests/test_gpu_memory_contracts.py)
    with open(L.HEADER) as fh:
        text = fh.read()
    for macro, value in (("GSAJ_SWEEP_STAGE_COST", 1), ("GSAJ_SWEEP_STAGE_PATHS", 2), ("GSAJ_SWEEP_STAGE_WINNER", 4)):
        assert "#define %s %d\n" % (macro, value) in text
    assert text.index("motion stereo") > text.index("int gsaj_rgbd_align8(")   # the section closes the header
    import gsaj
    assert "MotionStereo" in gsaj.__all__ and "grey_u8" in gsaj.__all__


def _expected_bytes(W, H, D):
    """The layout written out independently: two gradient images of 2 bytes per pixel, pc 1, C 2 and S 4 bytes per entry, each array
    padded to 256 bytes, no base slack."""
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    n = W * H
    offs = [2 * al(2 * n)]
    offs.append(offs[-1] + al(n * D))
    offs.append(offs[-1] + al(2 * n * D))
    return offs, offs[-1] + al(4 * n * D)


@pytest.mark.parametrize("W,H,D", [(1, 1, 16), (65, 5, 32), (160, 120, 16), (640, 480, 64), (150, 33, 128)])
def test_the_workspace_size_is_the_layout_written_out(W, H, D):
    lib = _lib()
    offs, total = _expected_bytes(W, H, D)
    for paths in (4, 8):
        nbytes = ctypes.c_size_t(0)
        assert lib.gsaj_motion_stereo_bytes(W, H, D, paths, ctypes.byref(nbytes)) == 0 and nbytes.value == total
        got = [ctypes.c_size_t(0) for _ in range(3)]
        assert lib.gsaj_debug_motion_stereo_offsets(W, H, D, paths, *[ctypes.byref(o) for o in got]) == 0
        assert [o.value for o in got] == offs
    if (W, H, D) == (640, 480, 64):
        assert abs(total / (7.0 * W * H * D) - 1.0) < 0.01   # about 7 W H D: 138 MB


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
GOOD = dict(W=160, H=120, ref=X, ref_stride=160, src=X, src_stride=160, fx=140.0, fy=140.0, cx=80.0, cy=60.0, ref_w2c=X, src_w2c=X, w_min=0.2,
            w_max=0.7, D=16, r=3, P1=100, P2=400, paths=8, uniqueness=10, outside_cost=80, stages=0, workspace=X, workspace_bytes=1 << 30, idx16=X,
            out_depth=None, stream=None)
NAN, INF = float("nan"), float("inf")
BAD = [
    ("D = 24", dict(D=24), "D must be 16, 32, 64 or 128"), ("D = 0", dict(D=0), "D must be"), ("D = 256", dict(D=256), "D must be"),
    ("W = 0", dict(W=0), "needs W >= 1"), ("H < 0", dict(H=-1), "needs W >= 1"), ("W H D > INT_MAX", dict(W=8192, H=4096, D=64), "INT_MAX"),
    ("r < 0", dict(r=-1), "block radius"), ("r = 8", dict(r=8), "block radius"),
    ("P1 < 0", dict(P1=-1), "P1 < P2"), ("P1 = P2", dict(P1=400), "P1 < P2"), ("P2 > 1024", dict(P2=1025), "P1 < P2"),
    ("paths = 5", dict(paths=5), "paths must be 4 or 8"),
    ("uniqueness < 0", dict(uniqueness=-1), "uniqueness"), ("uniqueness = 100", dict(uniqueness=100), "uniqueness"),
    ("outside_cost < 0", dict(outside_cost=-1), "outside_cost"), ("outside_cost = 241", dict(outside_cost=241), "outside_cost"),
    ("fx = 0", dict(fx=0.0), "fx and fy"), ("fy < 0", dict(fy=-1.0), "fx and fy"), ("fx is NaN", dict(fx=NAN), "fx and fy"),
    ("fy is inf", dict(fy=INF), "fx and fy"),
    ("w_min < 0", dict(w_min=-0.1), "w_min < w_max"), ("w_max = w_min", dict(w_max=0.2), "w_min < w_max"),
    ("w_max < w_min", dict(w_max=0.1), "w_min < w_max"), ("w_min is NaN", dict(w_min=NAN), "w_min < w_max"),
    ("w_max is inf", dict(w_max=INF), "w_min < w_max"),
    ("unknown stage bits", dict(stages=8), "unknown stage bits"),
    ("NULL ref", dict(ref=None), "are required"), ("NULL src", dict(src=None), "are required"), ("NULL ref_w2c", dict(ref_w2c=None), "are required"),
    ("NULL src_w2c", dict(src_w2c=None), "are required"), ("NULL workspace", dict(workspace=None), "are required"),
    ("NULL idx16", dict(idx16=None), "are required"),
    ("ref_stride < W", dict(ref_stride=159), "row stride"), ("src_stride < W", dict(src_stride=0), "row stride"),
    ("workspace off 256", dict(workspace=X + 128), "aligned"), ("idx16 odd", dict(idx16=X + 1), "aligned"),
    ("out_depth off 4", dict(out_depth=X + 2), "aligned"), ("pose off 4", dict(src_w2c=X + 2), "aligned"),
]


@pytest.mark.parametrize("what,kw,phrase", BAD, ids=[b[0] for b in BAD])
def test_a_bad_call_is_refused_with_its_message_before_any_launch(what, kw, phrase):
    """The pointers are abi.X, which nothing may read: a launch would not come back at all."""
    lib = _lib()
    assert call(lib, "gsaj_motion_stereo", **dict(GOOD, **kw)) == INVALID_ARGUMENT, (what, lib.gsaj_last_error())
    got = lib.gsaj_last_error().decode()
    assert got.startswith("gsaj_motion_stereo: ") and phrase in got, (what, got)


def test_a_small_workspace_has_its_own_code():
    lib = _lib()
    _, total = _expected_bytes(160, 120, 16)
    assert call(lib, "gsaj_motion_stereo", **dict(GOOD, workspace_bytes=total - 1)) == WORKSPACE_TOO_SMALL
    assert ("%d bytes" % (total - 1)) in lib.gsaj_last_error().decode() and str(total) in lib.gsaj_last_error().decode()


def test_the_small_entry_points_refuse_bad_calls_too():
    lib = _lib()
    n = ctypes.c_size_t(0)
    assert lib.gsaj_motion_stereo_bytes(160, 120, 16, 8, None) == INVALID_ARGUMENT
    assert lib.gsaj_motion_stereo_bytes(160, 120, 48, 8, ctypes.byref(n)) == INVALID_ARGUMENT
    assert lib.gsaj_motion_stereo_bytes(160, 120, 16, 3, ctypes.byref(n)) == INVALID_ARGUMENT
    assert lib.gsaj_debug_motion_stereo_offsets(0, 120, 16, 8, None, None, None) == INVALID_ARGUMENT
    for kw in (dict(W=0), dict(H=0), dict(color=None), dict(out=None), dict(out_stride=159), dict(W=65536, H=65536, out_stride=65536)):
        args = dict(dict(W=160, H=120, color=X, out=X, out_stride=160, stream=None), **kw)
        assert call(lib, "gsaj_grey_u8", **args) == INVALID_ARGUMENT, kw
        assert lib.gsaj_last_error().decode().startswith("gsaj_grey_u8: ")


# ---- the grey byte -----------------------------------------------------------------------------------------------------------------------
def test_the_restated_grey_byte():
    c = np.zeros((3, 1, 8), np.float32)
    c[:, 0, 0] = 0.5          # 127.5 + 0.5 -> 128
    c[:, 0, 1] = -0.2         # below 0 -> 0
    c[:, 0, 2] = 1.7          # above 1 -> 255
    c[1, 0, 3] = np.nan       # a NaN -> 0
    c[:, 0, 4] = 1.0
    c[0, 0, 5] = np.inf       # +inf -> 255
    c[2, 0, 6] = -np.inf      # -inf -> 0
    c[:, 0, 7] = 0.499 / 255.0
    assert sw.grey_u8(c).tolist() == [[128, 0, 255, 0, 255, 255, 0, 0]]
