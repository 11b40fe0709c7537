"""CPU: the premises of tests/test_gpu_binning.py, checked on the oracle.  The scenes with prescribed tile lists really produce
those lists, bit-exact depths and one tile per Gaussian; the one-line NumPy answer (binning_restated.expected_lists) is the
oracle's point_list and ranges; the `ties` layout really has ties in every list; the constants of the binning kernels are the
ones the layouts' boundary lengths were placed around; and the two scatter scenes reach the branches of k_scatter_instances
they are meant to reach."""
import numpy as np
import pytest

import binning_restated as br
import helpers as hp


@pytest.mark.parametrize("depths", ["log", "ties"])
@pytest.mark.parametrize("name", ["SMALL", "FULL"])
def test_layout_against_the_oracle(name, depths):
    L = br.layout(name, depths)
    (ref, st), kw = hp.oracle_forward(L["cam"], L["sc"], 0)
    assert L["P"] == sum(L["lengths"]) == {"SMALL": 24695, "FULL": 131423}[name]
    assert set(np.unique(st["radii"])) <= {4, 5}
    assert np.all(st["tiles_touched"] == 1)
    assert ref["num_rendered"] == L["R"]
    np.testing.assert_array_equal(st["ranges"][:, 1] - st["ranges"][:, 0], L["lengths"])
    np.testing.assert_array_equal(st["depths"].view(np.uint32), L["z32"].view(np.uint32))
    np.testing.assert_array_equal(st["point_list"], L["point_list"])
    np.testing.assert_array_equal(st["ranges"], L["ranges"])
    # (the tile every Gaussian was dealt to is the tile the oracle put it in)
    for t in (1, 4, 27):
        beg, end = L["ranges"][t]
        assert np.all(L["tile"][st["point_list"][beg:end]] == t)


@pytest.mark.parametrize("name", ["SMALL", "FULL"])
def test_the_ties_layout_has_ties_in_every_list(name):
    L = br.layout(name, "ties")
    bits = L["z32"].view(np.uint32)
    assert np.unique(bits).size <= 225
    for (beg, end), n in zip(L["ranges"], L["lengths"]):
        if n >= 2:
            d = bits[L["point_list"][beg:end]]
            assert np.any(d[1:] == d[:-1]), "a list of %d entries without two equal depths" % n
    # and the `log` layout is the opposite case: its depth bits spread over many exponents
    assert np.unique(br.layout(name, "log")["z32"].view(np.uint32) >> 23).size >= 13


def test_expected_lists_is_a_stable_sort_by_tile_depth_and_id():
    """The restatement on an input small enough to write the answer down."""
    tile = np.array([2, 0, 2, 2, 0, 2])
    z32 = np.array([1.5, 3.0, 1.5, 0.25, 2.0, 1.5], np.float32)
    pl, ranges = br.expected_lists(tile, z32, 4)
    np.testing.assert_array_equal(pl, [4, 1, 3, 0, 2, 5])
    np.testing.assert_array_equal(ranges, [[0, 2], [0, 0], [2, 6], [0, 0]])


def test_the_constants_are_the_ones_the_layouts_were_designed_for():
    assert br.csrc_constants() == br.DESIGN_CONSTANTS, (
        "a constant of the binning kernels changed: move the boundary lengths of binning_restated.SMALL / FULL, the capacity cases "
        "of test_gpu_binning.py and the scatter scenes S1 / S2 with it (they sit one below, on and one above these values)")
    c = br.DESIGN_CONSTANTS
    every = set(br.FULL)
    for b in (64, 128, 256, 512, c["GSAJ_SORT_128_MAX"], 2048, 4096, 8192, c["SORT_CAP"]):
        assert {b - 1, b, b + 1} <= every
    # the last merge of the longest list at T = 128 has more output blocks than one step of the merge-path split loop takes
    assert (max(br.FULL) + 127) // 128 > c["PRE_BLOCK"] and max(br.FULL) > 128 * c["PRE_BLOCK"]


def _oracle_state(which):
    cam, sc = br.scatter_scene(which)
    (ref, st), kw = hp.oracle_forward(cam, sc, 0)
    gx, gy = (cam["W"] + 15) // 16, (cam["H"] + 15) // 16
    rects = br.tile_rects(st["means2D"], st["radii"], gx, gy)
    np.testing.assert_array_equal((rects[:, 2] - rects[:, 0]) * (rects[:, 3] - rects[:, 1]), st["tiles_touched"])
    return ref, st, gx, gy, rects


def test_scene_s1_has_more_class_local_tiles_than_the_scatter_counters():
    c = br.csrc_constants()
    ref, st, gx, gy, rects = _oracle_state("S1")
    assert ((gy + c["SCAT_CLS"] - 1) // c["SCAT_CLS"]) * gx == 4097 > c["SCAT_LDS_TILES"]
    assert gx * gy <= c["LDS_TILES_MAX"]
    assert np.all(st["ranges"][:, 1] > st["ranges"][:, 0]) and st["ranges"].shape[0] == 4097
    assert ref["num_rendered"] == 586811
    assert br.class_totals(rects, st["P"], gx, gy).sum() == ref["num_rendered"]


def test_scene_s2_fills_and_overfills_the_staging_area():
    c = br.csrc_constants()
    ref, st, gx, gy, rects = _oracle_state("S2")
    P = st["P"]
    assert P * c["SCAT_CLS"] // (c["PRE_BLOCK"] * 4 * 2) < 1536  # launch_tile_binning keeps gpt = 4: 1024 Gaussians per workgroup
    tot = br.class_totals(rects, P, gx, gy, span=4 * c["PRE_BLOCK"], classes=c["SCAT_CLS"])
    assert tot.sum() == ref["num_rendered"] == 70400
    assert tot.shape == (2, 8)
    assert np.all(tot[0] == 8192) and 8192 > c["SCAT_STAGE"]   # stored directly
    assert np.all(tot[1] == 608) and 608 <= c["SCAT_STAGE"]    # staged in LDS
