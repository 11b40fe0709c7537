"""CPU: which variant of the binning front end a launch takes, pinned through the library's own plan functions
(gsaj_debug_launch_plan -> plan_preprocess / plan_scatter of csrc/preprocess.hip, the functions launch_preprocess and
launch_tile_binning call).  bpw: 256-Gaussian blocks per k_preprocess workgroup (> 1: the MULTI instantiations); gpt: blocks per
k_scatter_instances workgroup.  Both depend on P x views only, so a retuned threshold shows up HERE, as a changed row, and not as
tests that silently moved onto another path -- and every shape tests/test_gpu_launch_variants.py runs is held to the variant its id
claims.  No device is touched."""
import ctypes

import pytest

import launch_variants as lv

# (P, views, bpw, gpt, what it is).  The expected values were worked out by hand from the two selectors as they stand:
#   bpw doubles (1 -> 2 -> 4 -> 8) while ceil(P / 256) * views / (2 bpw) >= 4096 (integer division);
#   gpt = 8 if P * views * 8 / (256 * 4 * 2) >= 1536 else 4 (integer division); at 8, with wg(g) = ceil(P / (256 g)) * 8 * views,
#   the first g of 9, 10 with wg(8) > 1536 >= wg(g) replaces it.
TABLE = [
    (50_000, 8, 1, 9, "cfg2 window (the benchmark)"),
    (100_000, 8, 1, 8, "cfg4 window"),
    (300_000, 1, 1, 4, "cfg3 frame"),
    (1_000_000, 1, 1, 8, "cfg5 frame"),
    (1_000_000, 8, 4, 8, "cfg5 window"),
    (50_000, 1, 1, 4, "cfg2 frame"),
    (100_000, 1, 1, 4, "cfg4 frame"),
    (15, 1, 1, 4, "cfg1"),
    (12_288, 32, 1, 8, "wg(8) = 1536 exactly: no 9 / 10 retry"),
    (12_289, 32, 1, 9, "one Gaussian over"),
    (13_000, 32, 1, 9, "GPU case gpt9"),
    (13_824, 32, 1, 9, "6 scatter workgroups of 9 blocks, full: the last P that 9 serves"),
    (13_825, 32, 1, 10, "one over: 9 no longer fits, 10 does"),
    (15_000, 32, 1, 10, "GPU case gpt10"),
    (15_360, 32, 1, 10, "6 workgroups of 10 blocks, full"),
    (15_361, 32, 1, 8, "one over: neither retry fits"),
    (17_000, 32, 1, 8, "GPU case gpt8"),
    (6_143, 32, 1, 4, "P * views * 8 / 2048 = 767: half the threshold, gpt stays 4"),
    (12_287, 32, 1, 4, "the last P with gpt 4 at 32 views (1535)"),
    (65_025, 128, 4, 8, "255 blocks: 32640 / 8 = 4080 < 4096 stops at 4"),
    (65_280, 32, 1, 8, "255 blocks x 32: 8160 / 2 = 4080, the last launch before the switch"),
    (65_281, 32, 2, 8, "256 blocks: the first bpw = 2"),
    (65_537, 32, 2, 8, "257 blocks, 129 workgroups (GPU cases bpw2)"),
    (65_537, 64, 4, 8, "65 workgroups (GPU case bpw4)"),
    (65_537, 128, 8, 8, "33 workgroups (GPU case bpw8)"),
    (65_537, 1, 1, 4, "one view of the GPU cases' map"),
    (13_000, 1, 1, 4, "one view of the gpt9 map"),
    (15_000, 1, 1, 4, "one view of the gpt10 map"),
    (17_000, 1, 1, 4, "one view of the gpt8 map"),
    (2_097_152, 1, 2, 8, "8192 blocks in one view: the threshold without batching"),
    (2_096_896, 1, 1, 8, "8191 blocks"),
]


def _row_id(r):
    return "P%d_x%d" % (r[0], r[1])


@pytest.mark.parametrize("P,views,bpw,gpt,what", TABLE, ids=[_row_id(r) for r in TABLE])
def test_plan_of_a_launch(P, views, bpw, gpt, what):
    pl = lv.plan(P, views)
    assert (pl["bpw"], pl["gpt"]) == (bpw, gpt), (what, pl)
    nblk = (P + 255) // 256
    # every block is some workgroup's, and the last workgroup has one at least
    assert pl["pre_workgroups"] * bpw >= nblk > (pl["pre_workgroups"] - 1) * bpw, (what, pl)
    assert pl["scat_workgroups"] % 8 == 0, (what, pl)  # (eight row classes)
    groups = pl["scat_workgroups"] // 8
    assert groups * gpt >= nblk > (groups - 1) * gpt, (what, pl)
    assert pl["hist_lds"] == 1 and pl["scat_lds"] == 1, (what, pl)  # (80 x 160: 50 tiles)


def test_the_table_holds_every_shape_the_gpu_tests_run_with_the_variant_they_claim():
    rows = {(P, views): (bpw, gpt) for P, views, bpw, gpt, _ in TABLE}
    assert len(rows) == len(TABLE)
    for name, (P, K, coeffs, bpw, gpt, _) in lv.CASES.items():
        assert rows[(P, K)] == (bpw, gpt), name
        assert rows[(P, 1)] == lv.SINGLE_VIEW, name  # (the single-view context each batched view is compared with)
        assert name.startswith("bpw%d_" % bpw) if bpw > 1 else name.startswith("gpt%d_" % gpt), name
        # the premises of the GPU cases that are arithmetic: the last workgroup's loop ends early, the last block holds ONE Gaussian
        nblk, pl = (P + 255) // 256, lv.plan(P, K)
        if bpw > 1:
            assert 0 < nblk - (pl["pre_workgroups"] - 1) * bpw < bpw, name
            assert P - (nblk - 1) * 256 == 1, name
        assert lv.pinned_ids(P)[-1] == P - 1
    # both MULTI instantiations and every bpw and gpt the selectors can return are claimed by some case
    assert {(c[3], c[2] == 16) for c in lv.CASES.values() if c[3] > 1} >= {(2, True), (2, False), (4, False), (8, True)}
    assert {c[4] for c in lv.CASES.values()} == {8, 9, 10} and {b for b, _ in rows.values()} == {1, 2, 4, 8}
    assert {g for _, g in rows.values()} == {4, 8, 9, 10}


def test_the_tile_grid_moves_the_histogram_and_the_scatter_counters_out_of_lds():
    """hist_lds: tiles <= 8192; scat_lds: ceil(tile rows / 8) x tile columns <= 3411 (the counters, 12 bytes each, beside the 24 596
    bytes k_scatter_instances declares, in 64 KB: tests/test_cpu_lds_budget.py) -- at their edges, and neither moves bpw or gpt."""
    for w, h, hist, scat, what in [
        (16 * 3411, 16, 1, 1, "3411 x 1 tiles: the last strip the scatter counts in LDS"),
        (16 * 3411 + 1, 16, 1, 0, "3412 x 1: the first strip past the budget"),
        (16 * 4096, 16, 1, 0, "4096 x 1: the edge before the budget counted the declared LDS (73 748 bytes in all)"),
        (16 * 4096 + 1, 16, 1, 0, "4097 x 1 (scene S1 of tests/binning_restated.py)"),
        (16 * 8192, 16, 1, 0, "8192 tiles: the last histogram in LDS"),
        (16 * 8192 + 1, 16, 0, 0, "8193 tiles"),
        (16 * 512, 16 * 48, 0, 1, "512 x 48 = 24576 tiles in 6 x 512 = 3072 class-local ones: the last multiple of 512 under 3411"),
        (16 * 512, 16 * 48 + 1, 0, 0, "a 49th tile row: 7 x 512 = 3584"),
        (16 * 512, 16 * 64, 0, 0, "512 x 64 in 8 x 512 = 4096: the other edge before the budget"),
        (16 * 512, 16 * 64 + 1, 0, 0, "a 65th tile row: 9 x 512"),
        (16384, 16, 1, 1, "1024 x 1: the widest image a backward takes"),
        (16, 16384, 1, 1, "1 x 1024: the tallest"),
    ]:
        pl = lv.plan(3000, 1, w, h)
        assert (pl["hist_lds"], pl["scat_lds"]) == (hist, scat), (what, pl)
        assert (pl["bpw"], pl["gpt"], pl["pre_workgroups"], pl["scat_workgroups"]) == (1, 4, 12, 24), (what, pl)


def test_the_largest_gpu_case_stays_under_the_memory_cap():
    """The machines are shared: the K = 128 case asks for K blocks of each workspace, and their total, by the library's own size
    queries, stays under 4 GB.  (Bytes per case: the module docstring of tests/test_gpu_launch_variants.py.)"""
    sizes = {name: lv.workspace_bytes(c[0], c[1]) for name, c in lv.CASES.items()}
    assert max(sizes, key=sizes.get) == "bpw8_sh16"
    assert sizes["bpw8_sh16"] < lv.MEMORY_CAP, sizes


def test_bad_arguments_are_refused_with_their_values():
    from gsaj import _lib

    lib = _lib.load()
    assert lib.gsaj_version() >= 110
    out = (ctypes.c_int * 6)(*([-7] * 6))
    for args, msg in [((0, 1, 80, 160, out), "gsaj_debug_launch_plan: invalid argument (P=0 views=1 W=80 H=160)"),
                      ((300, 0, 80, 160, out), "gsaj_debug_launch_plan: invalid argument (P=300 views=0 W=80 H=160)"),
                      ((300, 1, -1, 160, out), "gsaj_debug_launch_plan: invalid argument (P=300 views=1 W=-1 H=160)"),
                      ((300, 1, 80, 0, out), "gsaj_debug_launch_plan: invalid argument (P=300 views=1 W=80 H=0)"),
                      ((300, 1, 80, 160, None), "gsaj_debug_launch_plan: invalid argument (P=300 views=1 W=80 H=160)")]:
        assert lib.gsaj_debug_launch_plan(*args) == -1 and lib.gsaj_last_error().decode() == msg
    assert list(out) == [-7] * 6  # (a refused call writes nothing)
