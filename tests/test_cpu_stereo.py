"""CPU: the stereo matcher as tests/stereo_restated.py restates it -- the premises the GPU comparison rests on (the cases contain every
rule's edge), the canaries (every mutant of the restatement changes what the GPU tests compare on a committed case), the quality of the
restatement on synthetic pairs with a known disparity, the header and the binding of the new entry points, and every argument error
that needs no launch.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import stereo_restated as sr
from abi import X, call, declarations, signature_mismatches

INVALID_ARGUMENT, TOO_SMALL = -1, -3
W0, H0, D0 = 96, 40, 16
SCENES = {}


def _scene(kind):
    if kind not in SCENES:
        SCENES[kind] = sr.scene(W0, H0, kind)
    return SCENES[kind]


def _matched(kind, r, memo={}):
    if (kind, r) not in memo:
        left, right, _ = _scene(kind)
        memo[kind, r] = sr.match(left, right, D0, r, want_S=True)
    return memo[kind, r]


def _edge_matched(kind, memo={}):
    if kind not in memo:
        left, right, _ = sr.edge_scene(W0, H0, kind)
        memo[kind] = sr.match(left, right, D0, 2, want_S=True)
    return memo[kind]


# ---- premises ---------------------------------------------------------------------------------------------------------------------------
def test_a_fronto_parallel_plane_gives_sixteen_times_its_disparity_on_the_interior():
    disp16, _ = _matched("plane", 10)
    inner = disp16[:, D0 + 12:W0 - 12]   # away from the columns whose window or match leaves the image
    assert (inner == 16 * 7).all(), np.unique(inner)
    small, _ = _matched("plane", 2)
    print("r = 2: %.3f of the interior is exactly 112, the rest within %d sixteenths" % ((small[:, D0 + 12:W0 - 12] == 112).mean(),
                                                                                         np.abs(small[:, D0 + 12:W0 - 12] - 112).max()))


def test_the_cases_contain_a_sum_beyond_sixteen_bits():
    _, S = _matched("plane", 10)
    assert S.max() > 65535 and S.max() < 2 ** 25, S.max()   # (2^25: the winner kernel packs S << 7 | d into 32 bits)
    assert sr.cost_volume(*_scene("plane")[:2], D0, 10).max() <= 961 * 30


def test_the_planted_sums_contain_every_edge_of_the_winner():
    for D in (16, 32, 64, 128):
        S = sr.planted_sums(D)
        H, W, _ = S.shape
        best, arg = S.min(axis=2), S.argmin(axis=2)
        ties = (S == best[:, :, None]).sum(axis=2)
        assert (ties[0, D:] == 2).all(), "row 0: the minimum is taken twice"
        assert set(arg[1, D:]) == {0, D - 1}, "row 1: d* at both ends"
        odd = 0
        for x in range(D, W):
            d = int(arg[2, x])
            den = max(int(S[2, x, d - 1] + S[2, x, d + 1] - 2 * S[2, x, d]), 1)
            num = int(S[2, x, d - 1] - S[2, x, d + 1]) * 16 + den
            odd += num < 0 and num % (2 * den) != 0
        assert odd >= 4, "row 2: negative sub-pixel numerators that do not divide evenly"
        slots = (np.arange(D, W) - arg[3, D:])
        assert (slots[0::2] == slots[1::2]).all() and (best[3, D:] == 4000).all(), "row 3: two left pixels, one right column, equal cost"
        far = np.abs(np.arange(D)[None, :] - arg[4, D:, None]) > 1
        assert ((S[4, D:] * 60 == best[4, D:, None] * 100) & far).any(axis=1).all(), "row 4: a rival exactly at the uniqueness bound"
        out = sr.winner(S, D, 40, -1)
        assert (out[1, D::2] == 0).all() and (out[1, D + 1::2] == 16 * (D - 1)).all()
        # with the left-right check the pixel at x + D - 1 (d* = D - 1) owns right column x at equal cost -- it is the larger x -- so
        # the pixel at x with d* = 0 fails both candidates; the last ones have no such rival inside the image
        checked = sr.winner(S, D, 40, 1)
        rivals = np.arange(D, W, 2) + D - 1 < W
        assert rivals.any() == (D == 16), "the planted image is D + 24 wide: only D = 16 has such rivals"
        assert (checked[1, D::2][rivals] == -16).all() and (checked[1, D::2][~rivals] == 0).all()
        z = sr.depth(out, 47.90639384423901)
        assert (z[1, D::2] == np.float32(47.90639384423901 * 1e-10)).all(), "d16 = 0 takes the 1e10 branch"
        assert (z[:, :D] == 0).all() and (out[:, :D] == -16).all(), "an invalid pixel has depth 0"
        assert (out[4, D:] >= 0).all(), "at the bound the pixel stays valid (the comparison is <)"


def test_a_flat_pair_ties_everywhere_and_the_lowest_disparity_wins():
    flat = np.full((9, D0 + 17), 77, np.uint8)
    disp16, S = sr.match(flat, flat, D0, 2, want_S=True)
    assert (S == 0).all() and (disp16[:, D0:] == 0).all() and (disp16[:, :D0] == -16).all()


# ---- canaries ---------------------------------------------------------------------------------------------------------------------------
def _differs_somewhere(mutant):
    hits = []
    for kind in sr.KINDS:
        for r in (2, 10):
            left, right, _ = _scene(kind)
            if not np.array_equal(sr.match(left, right, D0, r, mutant=mutant), _matched(kind, r)[0]):
                hits.append("%s r=%d" % (kind, r))
    for kind in sr.EDGE_KINDS:   # the cases on which the GPU tests compare S itself, not only the disparity
        left, right, _ = sr.edge_scene(W0, H0, kind)
        got, want = sr.match(left, right, D0, 2, mutant=mutant, want_S=True), _edge_matched(kind)
        if not np.array_equal(got[0], want[0]):
            hits.append("%s disp16" % kind)
        if not np.array_equal(got[1], want[1]):
            hits.append("%s S" % kind)
    S = sr.planted_sums(D0)
    for lr in (0, 1):
        if not np.array_equal(sr.winner(S, D0, 40, lr, mutant=mutant), sr.winner(S, D0, 40, lr)):
            hits.append("planted lr=%d" % lr)
    return hits


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_changes_a_committed_case(mutant):
    hits = _differs_somewhere(mutant)
    print(mutant, "differs on:", hits)
    assert hits, mutant


# ---- quality: a condition on the restatement, not a device tolerance ----------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 10])
@pytest.mark.parametrize("kind", sr.KINDS)
def test_the_restatement_recovers_a_known_disparity(kind, r):
    valid, within1 = sr.quality(_matched(kind, r)[0], _scene(kind)[2], D0)
    print("%s r=%d: %.4f valid, %.4f of the valid within 1 disparity" % (kind, r, valid, within1))
    assert valid >= 0.80 and within1 >= 0.90, (valid, within1)


def test_the_depth_is_the_references_float64_lines_rounded_once():
    d16 = np.array([[-16, 0, 1, 9, 16, 1023, 2047]], np.int16)
    bf = 47.90639384423901
    want = []
    for v in d16[0]:
        disparity = v / 16.0
        if disparity == 0:
            disparity = 1e10
        z = bf / disparity
        want.append(0.0 if z < 0 else z)
    assert np.array_equal(sr.depth(d16, bf).view(np.uint32), np.array([want]).astype(np.float32).view(np.uint32))


def test_the_byte_remap_is_the_ingests_rounded_bilinear_before_the_division():
    import ingest_restated as ir

    src = np.random.default_rng(2).integers(0, 256, (45, 80), dtype=np.uint8)
    K = ir.scaled_K(67)
    maps = ir.undistort_map(67, 35, ir.scaled_K(80), ir.FR1_DIST, ir.inverse_newK_R(ir.scaled_K(80), None, K))
    b = sr.rectify_u8(src, maps)
    assert b.dtype == np.uint8 and b.shape == (35, 67) and b.max() > 200
    ir.assert_bits_equal(ir.ingest_color(b)[0], ir.ingest_color(src, ir.ROUND_U8, maps)[0], "bytes / 255 against the rounded remap")


# ---- header and binding -----------------------------------------------------------------------------------------------------------------
NEW = ("gsaj_stereo_workspace_bytes", "gsaj_debug_stereo_offsets", "gsaj_rectify_u8", "gsaj_stereo_match")


def test_the_header_declares_the_stereo_entry_points_and_the_binding_matches_them():
    from gsaj import _lib

    decls = declarations()
    for name in NEW:
        assert name in decls and name in _lib.SIGNATURES, name
        assert len(decls[name][1]) == len(_lib.SIGNATURES[name][1]), name
    assert [m for m in signature_mismatches(_lib.SIGNATURES) if m[0] in NEW] == []
    assert decls["gsaj_stereo_match"][1][-1] == ("void *", "stream") and decls["gsaj_rectify_u8"][1][-1] == ("void *", "stream")
    import gsaj

    assert {"StereoMatcher", "StereoIngest"} <= set(gsaj.__all__)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
_BYTES = ctypes.c_size_t(0)
GOOD = {
    "gsaj_stereo_workspace_bytes": dict(W=96, H=40, D=16, paths=8, bytes=ctypes.byref(_BYTES)),
    "gsaj_rectify_u8": dict(W=67, H=35, Ws=80, Hs=45, src_stride=80, src=X, map_x=X, map_y=X, out=X, out_stride=67, out_color=X, stream=None),
    "gsaj_stereo_match": dict(W=96, H=40, left=X, left_stride=96, right=X, right_stride=96, D=16, r=10, P1=2, P2=5, paths=8, uniqueness=40,
                              lr_max_diff=1, stages=0, workspace=X, workspace_bytes=1 << 30, disp16=X, out_depth=X, bf=47.9, stream=None),
}
SIZE = "%s: needs D < W <= 4096, H >= 1 and W * H * D <= INT_MAX (W=%d H=%d D=%d)"
ROWS = [
    ("gsaj_stereo_workspace_bytes", "D = 48", dict(D=48), INVALID_ARGUMENT, "gsaj_stereo_workspace_bytes: D must be 16, 32, 64 or 128 (D=48)"),
    ("gsaj_stereo_workspace_bytes", "W = D", dict(W=16), INVALID_ARGUMENT, SIZE % ("gsaj_stereo_workspace_bytes", 16, 40, 16)),
    ("gsaj_stereo_workspace_bytes", "paths = 5", dict(paths=5), INVALID_ARGUMENT, "gsaj_stereo_workspace_bytes: paths must be 4 or 8 (paths=5)"),
    ("gsaj_stereo_workspace_bytes", "NULL bytes", dict(bytes=None), INVALID_ARGUMENT, "gsaj_stereo_workspace_bytes: bytes is required"),
    ("gsaj_stereo_match", "D = 0", dict(D=0), INVALID_ARGUMENT, "gsaj_stereo_match: D must be 16, 32, 64 or 128 (D=0)"),
    ("gsaj_stereo_match", "D = 256", dict(D=256), INVALID_ARGUMENT, "gsaj_stereo_match: D must be 16, 32, 64 or 128 (D=256)"),
    ("gsaj_stereo_match", "W = D", dict(W=16), INVALID_ARGUMENT, SIZE % ("gsaj_stereo_match", 16, 40, 16)),
    ("gsaj_stereo_match", "H = 0", dict(H=0), INVALID_ARGUMENT, SIZE % ("gsaj_stereo_match", 96, 0, 16)),
    ("gsaj_stereo_match", "W > 4096", dict(W=4097), INVALID_ARGUMENT, SIZE % ("gsaj_stereo_match", 4097, 40, 16)),
    ("gsaj_stereo_match", "W * H * D > INT_MAX", dict(W=4096, H=8192, D=64), INVALID_ARGUMENT, SIZE % ("gsaj_stereo_match", 4096, 8192, 64)),
    ("gsaj_stereo_match", "paths = 16", dict(paths=16), INVALID_ARGUMENT, "gsaj_stereo_match: paths must be 4 or 8 (paths=16)"),
    ("gsaj_stereo_match", "r = -1", dict(r=-1), INVALID_ARGUMENT, "gsaj_stereo_match: the block radius must lie in [0, 15] (r=-1)"),
    ("gsaj_stereo_match", "r = 16", dict(r=16), INVALID_ARGUMENT, "gsaj_stereo_match: the block radius must lie in [0, 15] (r=16)"),
    ("gsaj_stereo_match", "P1 < 0", dict(P1=-1), INVALID_ARGUMENT, "gsaj_stereo_match: needs 0 <= P1 < P2 <= 1024 (P1=-1 P2=5)"),
    ("gsaj_stereo_match", "P1 = P2", dict(P1=5), INVALID_ARGUMENT, "gsaj_stereo_match: needs 0 <= P1 < P2 <= 1024 (P1=5 P2=5)"),
    ("gsaj_stereo_match", "P2 > 1024", dict(P2=1025), INVALID_ARGUMENT, "gsaj_stereo_match: needs 0 <= P1 < P2 <= 1024 (P1=2 P2=1025)"),
    ("gsaj_stereo_match", "uniqueness = 100", dict(uniqueness=100), INVALID_ARGUMENT,
     "gsaj_stereo_match: uniqueness must lie in [0, 99] (uniqueness=100)"),
    ("gsaj_stereo_match", "uniqueness < 0", dict(uniqueness=-1), INVALID_ARGUMENT, "gsaj_stereo_match: uniqueness must lie in [0, 99] (uniqueness=-1)"),
    ("gsaj_stereo_match", "lr_max_diff = -2", dict(lr_max_diff=-2), INVALID_ARGUMENT, "gsaj_stereo_match: lr_max_diff must be >= -1 (lr_max_diff=-2)"),
    ("gsaj_stereo_match", "unknown stage bit", dict(stages=8), INVALID_ARGUMENT, "gsaj_stereo_match: unknown stage bits (stages=0x8)"),
    ("gsaj_stereo_match", "NULL left", dict(left=None), INVALID_ARGUMENT, "gsaj_stereo_match: left, right, workspace and disp16 are required"),
    ("gsaj_stereo_match", "NULL right", dict(right=None), INVALID_ARGUMENT, "gsaj_stereo_match: left, right, workspace and disp16 are required"),
    ("gsaj_stereo_match", "NULL workspace", dict(workspace=None), INVALID_ARGUMENT, "gsaj_stereo_match: left, right, workspace and disp16 are required"),
    ("gsaj_stereo_match", "NULL disp16", dict(disp16=None), INVALID_ARGUMENT, "gsaj_stereo_match: left, right, workspace and disp16 are required"),
    ("gsaj_stereo_match", "left_stride < W", dict(left_stride=95), INVALID_ARGUMENT,
     "gsaj_stereo_match: a row stride is less than W (left_stride=95 right_stride=96 W=96)"),
    ("gsaj_stereo_match", "right_stride < W", dict(right_stride=0), INVALID_ARGUMENT,
     "gsaj_stereo_match: a row stride is less than W (left_stride=96 right_stride=0 W=96)"),
    ("gsaj_stereo_match", "a workspace one byte short", dict(workspace_bytes=376319), TOO_SMALL,
     "gsaj_stereo_match: the workspace has 376319 bytes, gsaj_stereo_workspace_bytes says 376320"),
    ("gsaj_stereo_match", "a misaligned workspace", dict(workspace=X + 128), INVALID_ARGUMENT,
     "gsaj_stereo_match: workspace must be 256-byte, disp16 2-byte and out_depth 4-byte aligned"),
    ("gsaj_stereo_match", "an odd disp16", dict(disp16=X + 1), INVALID_ARGUMENT,
     "gsaj_stereo_match: workspace must be 256-byte, disp16 2-byte and out_depth 4-byte aligned"),
    ("gsaj_stereo_match", "bf = 0 with a depth", dict(bf=0.0), INVALID_ARGUMENT,
     "gsaj_stereo_match: with out_depth, bf must be positive and finite (bf=0)"),
    ("gsaj_stereo_match", "bf is NaN with a depth", dict(bf=float("nan")), INVALID_ARGUMENT,
     "gsaj_stereo_match: with out_depth, bf must be positive and finite (bf=nan)"),
    ("gsaj_stereo_match", "two defects: D wins over r", dict(D=7, r=99), INVALID_ARGUMENT, "gsaj_stereo_match: D must be 16, 32, 64 or 128 (D=7)"),
    ("gsaj_rectify_u8", "W <= 0", dict(W=0), INVALID_ARGUMENT,
     "gsaj_rectify_u8: W, H, Ws and Hs must be positive with W * H and Ws * Hs <= INT_MAX (W=0 H=35 Ws=80 Hs=45)"),
    ("gsaj_rectify_u8", "NULL src", dict(src=None), INVALID_ARGUMENT, "gsaj_rectify_u8: src and out are required"),
    ("gsaj_rectify_u8", "NULL out", dict(out=None), INVALID_ARGUMENT, "gsaj_rectify_u8: src and out are required"),
    ("gsaj_rectify_u8", "src_stride < Ws", dict(src_stride=79), INVALID_ARGUMENT,
     "gsaj_rectify_u8: a row stride is less than its row (src_stride=79 Ws=80 out_stride=67 W=67)"),
    ("gsaj_rectify_u8", "out_stride < W", dict(out_stride=66), INVALID_ARGUMENT,
     "gsaj_rectify_u8: a row stride is less than its row (src_stride=80 Ws=80 out_stride=66 W=67)"),
    ("gsaj_rectify_u8", "map_x without map_y", dict(map_y=None), INVALID_ARGUMENT, "gsaj_rectify_u8: map_x and map_y must be given together or not at all"),
    ("gsaj_rectify_u8", "no map and a source of another size", dict(map_x=None, map_y=None), INVALID_ARGUMENT,
     "gsaj_rectify_u8: without a map the source must have the output's size (W=67 H=35 Ws=80 Hs=45)"),
    ("gsaj_rectify_u8", "a misaligned out_color", dict(out_color=X + 2), INVALID_ARGUMENT,
     "gsaj_rectify_u8: out_color, map_x and map_y must be 4-byte aligned"),
]


def _lib():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("name,what,kw,code,msg", ROWS, ids=["%s: %s" % (r[0][5:], r[1]) for r in ROWS])
def test_bad_stereo_call_is_refused_with_its_code_and_message_before_any_launch(name, what, kw, code, msg):
    lib = _lib()
    assert call(lib, name, **dict(GOOD[name], **kw)) == code, (name, what, lib.gsaj_last_error())
    assert lib.gsaj_last_error().decode() == msg, (name, what)


def test_the_workspace_size_is_the_sum_of_its_four_aligned_blocks():
    lib = _lib()
    n = ctypes.c_size_t(0)
    assert lib.gsaj_stereo_workspace_bytes(96, 40, 16, 8, ctypes.byref(n)) == 0
    align = lambda v: (v + 255) // 256 * 256  # noqa: E731
    assert n.value == 2 * align(96 * 40) + align(96 * 40 * 16 * 2) + align(96 * 40 * 16 * 4) == 376320
    c_off, s_off = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gsaj_debug_stereo_offsets(96, 40, 16, 8, ctypes.byref(c_off), ctypes.byref(s_off)) == 0
    assert (c_off.value, s_off.value) == (2 * align(96 * 40), 2 * align(96 * 40) + align(96 * 40 * 16 * 2))
