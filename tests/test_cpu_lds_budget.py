"""CPU: the LDS of every launch that requests dynamic LDS, static + dynamic <= the limit the launcher has secured, at the far end of
every size class -- through gsaj_debug_lds_budget, i.e. the functions launch_preprocess, launch_tile_binning,
launch_gaussian_backward and the stereo launcher take their byte counts from.  Three things are held:
  1. the static bytes the library states per kernel are the ones the COMPILER reports for that kernel (tools/kernel_resources.py's
     own command and parsing, the Makefile's flags), so a helper that later gains a hidden __shared__ array shows up here;
  2. the dynamic bytes are the ones the sizes imply (4 per tile, 12 per class-local tile, 8 per key, ...), written out here
     independently, and the sum fits the limit at every edge -- with the instance scatter's counters leaving the LDS exactly where
     they no longer fit beside the 24 596 bytes k_scatter_instances declares (3411 class-local tiles; 4096, the edge this replaced,
     asked for 73 748 bytes under a 65 536-byte limit: the canary);
  3. the scenes tests/test_gpu_binning.py runs at those edges (binning_restated.BUDGET_SCENES) take the bodies their ids claim.
No device is touched."""
import ctypes
import importlib.util
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import binning_restated as br
import helpers as hp
import launch_variants as lv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 65536  # bytes of LDS a workgroup may hold unless the function's limit is raised (LDS_DEFAULT_LIMIT of gsaj_common.h)
SCAT_TILE_BYTES = 12  # count, fill cursor, staging base
STEREO_MAX_W = 4096


def _budget(P=3000, views=1, W=80, H=160, **kw):
    from gsaj import rasterizer as C

    return C.lds_budget(P, views, W, H, **kw)


def within_budget(static, dynamic, limit):
    """THE check of this file: what a workgroup holds fits what the launcher has secured."""
    return static >= 0 and dynamic >= 0 and static + dynamic <= limit


def _assert_rows_fit(b, tag):
    for name, r in b.items():
        assert within_budget(r["static"], r["dynamic"], r["limit"]), (tag, name, r)
        assert r["limit"] in (0, LIMIT) or name.startswith("tile_sort"), (tag, name, r)  # (only the sort raises its limit)


def _ltiles(W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return ((gy + 7) // 8) * gx


def _bound():
    """Class-local tiles whose counters fit beside what k_scatter_instances declares, from the library's own static figure."""
    scat = _budget()["scatter"]
    return (LIMIT - scat["static"]) // SCAT_TILE_BYTES


# ---- 1. the compiler's figure ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled():
    """(file, kernel) -> the compiler's resource figures, by tools/kernel_resources.py's own command and parsing."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    # its list of files compiled without FMA contraction is the Makefile's
    with open(os.path.join(br.CSRC, "Makefile")) as fh:
        rules = re.findall(r"^\$\(OUT\)/(\w+)\.o:[^\n]*\n(?:\t@[^\n]*\n)*\t([^\n]*)", fh.read(), flags=re.M)
    assert {n + ".hip" for n, cmd in rules if "-ffp-contract=off" in cmd} == kr.NOCONTRACT
    files = ("preprocess.hip", "gaussian_bwd.hip", "stereo.hip")
    with ThreadPoolExecutor(len(files)) as ex:
        return {(k["file"], k["kernel"]): k["res"] for ks in ex.map(lambda f: kr.one(br.CSRC, f), files) for k in ks}


# kernel as the compiler names it -> (row of the budget, the variant the row must report, arguments that select it)
KERNELS = {
    ("preprocess.hip", "k_preprocess<false, false>"): ("preprocess", 0, dict(M=1)),
    ("preprocess.hip", "k_preprocess<false, true>"): ("preprocess", 1, dict(P=65537, views=32, M=1)),
    ("preprocess.hip", "k_preprocess<true, false>"): ("preprocess", 2, dict(M=16)),
    ("preprocess.hip", "k_preprocess<true, true>"): ("preprocess", 3, dict(P=65537, views=32, M=16)),
    ("preprocess.hip", "k_frame_scan"): ("frame_scan", 0, dict()),
    ("preprocess.hip", "k_scatter_instances"): ("scatter", 0, dict()),
    ("preprocess.hip", "k_tile_sort<128>"): ("tile_sort", 128, dict(tile_list_capacity=1024)),
    ("preprocess.hip", "k_tile_sort<256>"): ("tile_sort", 256, dict(tile_list_capacity=1025)),
    ("preprocess.hip", "k_tile_sort<512>"): ("tile_sort", 512, dict(tile_list_capacity=4096)),
    ("gaussian_bwd.hip", "k_gaussian_bwd<0>"): ("gaussian_bwd", 0, dict(M=0)),
    ("gaussian_bwd.hip", "k_gaussian_bwd<3>"): ("gaussian_bwd", 3, dict(M=1)),
    ("gaussian_bwd.hip", "k_gaussian_bwd<12>"): ("gaussian_bwd", 12, dict(M=4)),
    ("gaussian_bwd.hip", "k_gaussian_bwd<27>"): ("gaussian_bwd", 27, dict(M=9)),
    ("gaussian_bwd.hip", "k_gaussian_bwd<48>"): ("gaussian_bwd", 48, dict(M=16)),
    ("stereo.hip", "k_stereo_winner<16>"): ("stereo_winner", 16, dict(stereo_D=16)),
    ("stereo.hip", "k_stereo_winner<32>"): ("stereo_winner", 32, dict(stereo_D=32)),
    ("stereo.hip", "k_stereo_winner<64>"): ("stereo_winner", 64, dict(stereo_D=64)),
    ("stereo.hip", "k_stereo_winner<128>"): ("stereo_winner", 128, dict(stereo_D=128)),
}


def test_the_static_lds_the_library_states_is_what_the_compiler_reports(compiled):
    # every instantiation of the six kernels is in the table above
    listed = {k for k in compiled if re.match(r"k_(preprocess|frame_scan|scatter_instances|tile_sort|gaussian_bwd|stereo_winner)\b", k[1])}
    assert listed == set(KERNELS), sorted(listed ^ set(KERNELS))
    for key, (row, variant, args) in KERNELS.items():
        r = _budget(**args)[row]
        assert r["variant"] == variant, (key, r)
        assert r["static"] == compiled[key]["lds_bytes"], (key, r, compiled[key])
    # (the second sort launch is the same kernel family)
    r = _budget(tile_list_capacity=4096)["tile_sort_2"]
    assert (r["variant"], r["static"]) == (256, compiled[("preprocess.hip", "k_tile_sort<256>")]["lds_bytes"])
    # and the figure the scatter's bound is derived from, as the issue of this test measured it
    assert compiled[("preprocess.hip", "k_scatter_instances")]["lds_bytes"] == 24596 and _bound() == 3411
    assert br.csrc_constants()["SCAT_LDS_TILES"] == _bound()  # (the figure the source states beside the constexpr it decides by)


# ---- 2. the budget at every edge ------------------------------------------------------------------------------------------------------
def test_the_tile_histogram_fits_up_to_8192_tiles_and_is_not_requested_beyond():
    for W, H, tiles in [(16, 16, 1), (2048, 1024, 8192), (16 * 8192, 16, 8192), (16 * 8193, 16, 8193), (3856, 544, 8194),
                        (3840, 2160, 32400), (1280, 720, 3600)]:
        b = _budget(W=W, H=H)
        _assert_rows_fit(b, (W, H))
        want = 4 * tiles if tiles <= 8192 else 0
        assert b["preprocess"]["dynamic"] == b["frame_scan"]["dynamic"] == want, (W, H, b)
        assert lv.plan(3000, 1, W, H)["hist_lds"] == (1 if want else 0)
    # the largest request there is: 32 768 bytes beside 16 and 320 declared ones
    b = _budget(W=2048, H=1024)
    assert (b["preprocess"]["static"], b["frame_scan"]["static"]) == (16, 320)


def test_the_scatter_counters_leave_the_lds_where_they_no_longer_fit_beside_the_declared_arrays():
    bound = _bound()
    assert 512 * (bound // 512) == 3072 and bound == 9 * 379 and bound + 1 == 4 * 853  # (the shapes below, and S3 / S4)
    for W, H, ltiles, lds, what in [
        (16 * bound, 16, bound, True, "the last strip"),
        (16 * (bound + 1), 16, bound + 1, False, "the first strip past the bound"),
        (16 * 512, 16 * 8 * (bound // 512), 512 * (bound // 512), True, "512 columns: the last multiple of 512 under the bound"),
        (16 * 512, 16 * 8 * (bound // 512) + 1, 512 * (bound // 512 + 1), False, "one tile row more"),
        (16 * 379, 16 * 65, bound, True, "379 x 65 tiles (scene S3): the bound exactly, nine rows in class 0"),
        (16 * 853, 16 * 25, bound + 1, False, "853 x 25 tiles (scene S4): one over"),
        (16 * 4096, 16, 4096, False, "4096 x 1: the edge before the declared arrays were counted"),
        (16 * 512, 16 * 64, 4096, False, "512 x 64: the same in the 512-column form"),
        (3840, 2160, 4080, False, "a 4K frame"),
        (1280, 720, 480, True, "1280 x 720: 80 x 45 tiles, six rows a class"),
        (16, 16, 1, True, "one tile"),
    ]:
        assert _ltiles(W, H) == ltiles, what
        b = _budget(W=W, H=H)
        _assert_rows_fit(b, what)
        assert b["scatter"]["dynamic"] == (SCAT_TILE_BYTES * ltiles if lds else 0), (what, b["scatter"])
        assert lv.plan(3000, 1, W, H)["scat_lds"] == (1 if lds else 0), what
        # the decision IS the budget: in LDS exactly when the counters fit beside the declared bytes
        assert lds == within_budget(b["scatter"]["static"], SCAT_TILE_BYTES * ltiles, LIMIT), what
    b = _budget(W=16 * bound, H=16)["scatter"]
    assert b["static"] + b["dynamic"] == 24596 + 40932 == 65528  # eight bytes to spare


def test_canary_the_checker_rejects_the_requests_the_scatter_made_before():
    """24 596 declared bytes + 12 bytes for each of 4096 (the old edge) and 4080 (3840 x 2160) class-local tiles, against the 64 KB no
    hipFuncSetAttribute had raised for this kernel: what within_budget must refuse -- and does accept at the new edge."""
    assert not within_budget(24596, 12 * 4096, LIMIT) and 24596 + 12 * 4096 == 73748
    assert not within_budget(24596, 12 * 4080, LIMIT) and 24596 + 12 * 4080 == 73556
    assert not within_budget(24596, 12 * 3412, LIMIT)
    assert within_budget(24596, 12 * 3411, LIMIT)
    assert not within_budget(0, 8 * 16384, LIMIT) and within_budget(0, 8 * 16384, 8 * 16384)  # (why the sort raises its limit)


def test_every_sort_capacity_fits_the_limit_its_launcher_secures():
    #    capacity -> keys of LDS, threads, launches
    for cap, keys, threads, two in [(128, 128, 128, False), (1024, 1024, 128, False), (1025, 2048, 256, False), (4096, 4096, 512, True),
                                    (8192, 8192, 512, True), (8193, 16384, 512, True), (16384, 16384, 512, True), (0, 16384, 512, True),
                                    (1, 128, 128, False), (100000, 16384, 512, True)]:
        b = _budget(tile_list_capacity=cap)
        _assert_rows_fit(b, cap)
        first, second = b["tile_sort"], b["tile_sort_2"]
        assert first["variant"] == threads and first["static"] == 0, (cap, first)
        if two:
            assert first["dynamic"] == 8 * keys, (cap, first)
            assert second["dynamic"] == 4 * keys and second["variant"] == (512 if keys // 2 >= 4096 else 256), (cap, second)
        else:
            assert first["dynamic"] == 8 * keys + 4 * 257, (cap, first)  # (+ the merge-path splits behind the keys)
            assert second == dict(dynamic=0, static=0, limit=0, variant=0), (cap, second)
        # the limit is raised exactly when the keys alone exceed the default, and then to exactly the request
        assert first["limit"] == (8 * keys if 8 * keys > LIMIT else LIMIT), (cap, first)


def test_the_backward_and_the_stereo_winner_fit_at_their_largest():
    for M in (0, 1, 2, 4, 9, 16):
        b = _budget(M=M)
        _assert_rows_fit(b, M)
        assert b["gaussian_bwd"]["dynamic"] == (4 * 64 * (3 * M + 1) if M else 0), (M, b["gaussian_bwd"])
        assert b["gaussian_bwd"]["variant"] == (3 * M if M in (1, 4, 9, 16) else 0)
    for D in (16, 32, 64, 128):
        for W in (D + 1, STEREO_MAX_W):
            b = _budget(stereo_W=W, stereo_D=D)
            _assert_rows_fit(b, (W, D))
            assert b["stereo_winner"] == dict(dynamic=12 * W, static=0, limit=LIMIT, variant=D)
    assert 12 * STEREO_MAX_W == 49152


def test_bad_arguments_are_refused_with_their_values():
    from gsaj import _lib

    lib = _lib.load()
    assert lib.gsaj_version() >= 113
    out = (ctypes.c_int * 28)(*([-7] * 28))
    good = dict(P=300, views=1, W=80, H=160, M=1, tile_list_capacity=0, stereo_W=640, stereo_D=64)
    for bad in [dict(P=0), dict(views=0), dict(W=0), dict(H=-1), dict(M=-1), dict(tile_list_capacity=-1), dict(stereo_W=4097),
                dict(stereo_W=64), dict(stereo_D=48), dict(budget=None)]:
        a = dict(dict(good, budget=out), **bad)
        assert lib.gsaj_debug_lds_budget(*[a[k] for k in list(good) + ["budget"]]) == -1
        assert lib.gsaj_last_error().decode() == (
            "gsaj_debug_lds_budget: invalid argument (P=%d views=%d W=%d H=%d M=%d tile_list_capacity=%d stereo_W=%d stereo_D=%d)"
            % tuple(a[k] for k in good))
    assert list(out) == [-7] * 28  # (a refused call writes nothing)
    assert lib.gsaj_debug_lds_budget(*list(good.values()), out) == 0 and -7 not in list(out)


# ---- 3. the premises of the GPU scenes ------------------------------------------------------------------------------------------------
#          id: (tile columns, tile rows, class-local tiles, histogram in LDS, scatter counters in LDS)
PREMISES = {"S3": (379, 65, 3411, 0, 1), "S4": (853, 25, 3412, 0, 0), "S5": (240, 135, 4080, 0, 0), "H1": (128, 64, 1024, 1, 1),
            "H2": (241, 34, 1205, 0, 1)}


@pytest.mark.parametrize("which", sorted(br.BUDGET_SCENES))
def test_the_gpu_scenes_sit_where_their_ids_claim(which):
    W, H, P, backward = br.BUDGET_SCENES[which]
    gx, gy, ltiles, hist, scat = PREMISES[which]
    assert ((W + 15) // 16, (H + 15) // 16, _ltiles(W, H)) == (gx, gy, ltiles)
    pl = lv.plan(P, 1, W, H)
    assert (pl["hist_lds"], pl["scat_lds"]) == (hist, scat), pl
    b = _budget(P=P, W=W, H=H, M=1)
    _assert_rows_fit(b, which)
    assert b["scatter"]["dynamic"] == (12 * ltiles if scat else 0) and b["preprocess"]["dynamic"] == (4 * gx * gy if hist else 0)
    assert not backward or max(gx, gy) <= 1023  # (the packed tile rectangle of a backward: 10 bits a side)
    bound = _bound()
    assert {"S3": ltiles == bound, "S4": ltiles == bound + 1, "S5": ltiles > bound and (W, H) == (3840, 2160),
            "H1": gx * gy == 8192 and ltiles <= bound, "H2": gx * gy in (8193, 8194) and ltiles <= bound}[which]
    # the scene fills the grid: every tile ROW holds instances, so every row class of the scatter (and, in S3, the ninth row of
    # class 0) has work, and some Gaussian spans more than one row class
    cam, sc = br.scatter_scene(which)
    (ref, st), kw = hp.oracle_forward(cam, sc, 0)
    per_row = (st["ranges"][:, 1] - st["ranges"][:, 0]).reshape(gy, gx).sum(axis=1)
    assert per_row.min() > 0 and int((ref["radii"] > 0).sum()) > 0.9 * P
    rects = br.tile_rects(st["means2D"], st["radii"], gx, gy)
    assert (rects[:, 3] - rects[:, 1]).max() > 8 or which == "S5"  # (a rectangle taller than the eight classes: two rows of one class)
    assert np.count_nonzero(rects[:, 3] - rects[:, 1] > 1) > P // 10


def test_the_benchmark_frames_keep_the_scatter_they_had():
    """Every benchmark workload is at most 1280 x 720 (ltiles 800): the counters stay in LDS, as before the bound moved."""
    for W, H in [(1280, 720), (640, 480), (320, 240)]:
        assert _ltiles(W, H) <= 800
        for P, views in [(50_000, 8), (100_000, 8), (300_000, 1), (1_000_000, 1), (1_000_000, 8)]:
            pl = lv.plan(P, views, W, H)
            assert pl["scat_lds"] == 1 and pl["hist_lds"] == 1, (W, H, P, views, pl)
