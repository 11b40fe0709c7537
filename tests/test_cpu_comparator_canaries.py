"""Comparator canaries: the parity comparators of tests/helpers.py accept a correct fp32 evaluation and reject outputs with a
known bug (tests/mutants.py builds them on the CPU from the oracle).  The controls are what the MI355X returned for the same
frames (tests/golden/device_<scene>.npz, tests/golden/make_device_outputs.py).

Every frame here is a frame of test_gpu_tiled.test_forward_and_backward_parity[<scene>-False] (SH colours, background
helpers.PARITY_BG, the scene's scale modifier, seeds helpers.seeds(cam, seed=1)) or, for "random/<id>", of
test_gpu_random.test_random_scene_parity[<id>]: a mutant rejected here on a frame is rejected by that GPU test if the kernels
had the bug.  The map (margin = worst err / allowed of the rejecting layer; counts: pixels whose n_contrib differs with no
borderline contributor; "-": the frame does not exercise the bug; last column: the tests that rejected it before canary_97x61
was added to the fixed parity scenes -- every fixed and random parity scene renders with a background other than 0).

| id  | bug                                              | rejected by  | canary_97x61   | before canary_97x61                        |
|-----|--------------------------------------------------|--------------|----------------|--------------------------------------------|
| F1  | pixel centre off by half a pixel                 | image        | 2.5e3          | every parity scene                         |
| F2  | termination one entry late                       | counts+image | 284 px, 143    | random P4097_96x96, P1000_200x150, P65_16x16 |
| F3  | alpha clamp missing                              | image(+counts)| 2 px, 228     | random P4097_96x96, P1000_200x150          |
| F4  | background left out of the final colour          | image        | 1.0e3          | every parity scene                         |
| F5  | last tile column not composited                  | image        | 2.0e4          | every parity scene                         |
| F6  | longest tile list short by one entry             | image+counts | 165            | fixed scenes, most random ones             |
| F7  | n_touched without the alpha >= 1/255 test        | touched      | 95 Gaussians   | fixed scenes, most random ones             |
| F8  | fp16 record rounding missing / applied in fp32   | image, (A)   | yes            |                                            |
| F9  | one pixel off by 2 IMG_TOL / 2 borderline pixels | image        | 2.0            | (output edit)                              |
| F10 | depths stored at half precision                  | image        | 3.4            |                                            |
| A1  | off-diagonal conic gradient x2                   | (A), (C)     | 2.8e4          | every parity scene                         |
| A2  | background term of dL/dalpha dropped             | (A), (C)     | 2.0e3          | every parity scene                         |
| A3  | depth seed ignored                               | (A), (C)     | 3.5e4          | every parity scene                         |
| A4  | dL/dG zeroed where alpha is clamped              | (A), (C)     | 5.9, (C) 3.4   | random P4097_96x96 (111), P1000_200x150 (3.8) |
| A5  | reverse walk starts one entry late               | (A), (C)     | 1.1e4          | random P4097_96x96, P65_16x16              |
| A6  | one tile's share lost for one Gaussian           | (A)          | 1.2 (clean), 1.1 (flipped); one colour 1.26, (C) 8.7 |
| A7  | one sum off by k x its (A) bound                 | (A)          | k = 0.5 accepted, k >= 2 rejected, all 10 sums |
| B1  | dL/dtau halves swapped / one sign flipped        | (B), (C)     | 9.4e4 / 5.5e4  | every parity scene                         |
| B2  | SH colour clamp ignored in the chain             | (B), (C)     | 4.6e5          | fixed scenes with SH degree > 0            |
| B3  | view rotation transposed in the chain            | (B), (C)     | 1.1e7          | every parity scene                         |
| B4  | two Gaussians' chain rows exchanged              | (B), (C)     | yes            |                                            |
| B5  | scale modifier ignored in the chain              | (B), (C)     | 5.6e3          | none: no parity test had a modifier != 1   |
| B6  | chain reads the sums through fp16                | (B), (C)     | 1.4e3, (C) 5.4 |                                            |
| B7  | one chain row off by k x its (B) allowance       | (B)          | k = 0.5 accepted, k = 2 rejected |                          |
| B8  | chain reads the camera position at half precision| (B) only     | 3.0            |                                            |
| B9  | chain reads the scale modifier at half precision | (B), (C)     | 4.9, (C) 1.1   | none                                       |

B5 (and B9) were the bugs no parity test could see; canary_97x61 (modifier 0.8) closes that, and gives the fixed scenes the
saturated pixels and o G > 0.99 that F2, F3, A4 and A5 need (before, only random scenes had them).  (C) on its own (no oracle
state, GRAD_TOL) rejects A1, A6 on a clean Gaussian (its largest tile share) and B1.  Realistic bugs rejected by a margin in
[1, 10]: (A) A4, A6; (B) B8, B9; (C) A4, B6; image F10; counts F3.
"""
import numpy as np
import pytest

import helpers as hp
import mutants as mu

SCENES = ["canary_97x61", "p500_100x75_sh0", "p300_behind_64x48"]
CANARY = "canary_97x61"


def rejected(fn):
    """The AssertionError text of fn(), or None if it passed."""
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


def rejecting_layers(fr, g, **kw):
    return {L for L in "ABC" if rejected(lambda: mu.check_backward(fr, g, layers=(L,), **kw))}


def margins(fr, g, **kw):
    return mu.check_backward(fr, g, layers=(), **kw)


def counts_margin(fr, out):
    """Pixels whose n_contrib differs from the oracle's with no borderline contributor (>= 1: the counts check rejects)."""
    diff = np.asarray(out["n_contrib"]).astype(np.int64) != fr.st["n_contrib"].astype(np.int64)
    return int((diff & ~fr.gref["error_model"]["border_mask"]).sum())


# ---- controls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_control_passes_every_comparator(name):
    fr = mu.frame(name)
    fwd, g = mu.device(name)
    np.testing.assert_array_equal(fwd["radii"], fr.ref["radii"])
    assert fwd["num_rendered"] == fr.ref["num_rendered"]
    mu.check_forward(fr, fwd)
    w = mu.check_backward(fr, g)
    assert max(w["A"], w["B"], w["C"]) < 1.0
    # (C) on its own, as callers without the oracle state use it
    hp.assert_grads_close(g, {k: v for k, v in fr.gref.items() if k != "error_model"}, name + "/C-alone", layers=("C",))


def test_canary_scene_exercises_what_it_is_for():
    fr = mu.frame(CANARY)
    co, vis = fr.st["conic_opacity"], fr.visible
    assert fr.st["W"] % 16 and fr.st["H"] % 16 and np.any(fr.bg != 0) and fr.mod != 1.0 and fr.deg == 3
    assert (co[vis, 3] > 0.99).sum() >= 3          # o G > 0.99 at their centres: the alpha clamp is active
    assert (fr.st["final_T"] < 1e-4 / (1 - 0.99)).sum() > 100  # saturated pixels: walks that end on the T test
    assert fr.st["clamped"][vis].any(axis=1).sum() > 50
    assert fr.clean.sum() > 100 and (~fr.clean).sum() > 10


# ---- forward -------------------------------------------------------------------------------------------------------------------
FWD = {"F1": mu.f1_half_pixel, "F2": mu.f2_late_stop, "F3": mu.f3_no_alpha_clamp, "F4": mu.f4_no_background,
       "F5": mu.f5_ragged_column_lost, "F6": mu.f6_list_short, "F7": mu.f7_touched_no_cutoff}
# (mutant, scene) -> the comparators that must reject it; () = the scene cannot show the bug (no saturated pixel, no clamp)
FWD_MAP = {
    ("F1", CANARY): ("image", "counts", "touched"), ("F1", "p500_100x75_sh0"): ("image",), ("F1", "p300_behind_64x48"): ("image",),
    ("F2", CANARY): ("counts", "image"), ("F2", "p500_100x75_sh0"): (), ("F2", "p300_behind_64x48"): (),
    ("F3", CANARY): ("counts", "image"), ("F3", "p500_100x75_sh0"): (), ("F3", "p300_behind_64x48"): (),
    ("F4", CANARY): ("image",), ("F4", "p500_100x75_sh0"): ("image",), ("F4", "p300_behind_64x48"): ("image",),
    ("F5", CANARY): ("image", "counts"), ("F5", "p500_100x75_sh0"): ("image", "counts"), ("F5", "p300_behind_64x48"): ("image",),
    ("F6", CANARY): ("image", "counts"), ("F6", "p500_100x75_sh0"): ("image", "counts"), ("F6", "p300_behind_64x48"): ("image", "counts"),
    ("F7", CANARY): ("touched",), ("F7", "p500_100x75_sh0"): ("touched",), ("F7", "p300_behind_64x48"): ("touched",),
}


@pytest.mark.parametrize("mid,name", sorted(FWD_MAP), ids=["%s-%s" % k for k in sorted(FWD_MAP)])
def test_forward_mutant_rejected(mid, name):
    fr = mu.frame(name)
    out = FWD[mid](fr)
    want = FWD_MAP[(mid, name)]
    for which in want:
        assert rejected(lambda: mu.check_forward(fr, out, (which,))), (mid, name, which)
    if not want:  # the scene does not exercise the bug: nothing differs at all (the map above names the scene that does)
        for k in ("color", "depth", "opacity", "n_contrib", "n_touched"):
            np.testing.assert_array_equal(out[k], fr.fwd()[k])


def test_F3_subtle_counts_margin():
    fr = mu.frame(CANARY)
    assert 1 <= counts_margin(fr, mu.f3_no_alpha_clamp(fr)) <= 10


def test_F10_depth_records_at_half_precision():
    fr = mu.frame(CANARY)
    out = mu.f10_depth_half(fr)
    assert rejected(lambda: mu.check_forward(fr, out, ("image",)))
    assert not rejected(lambda: mu.check_forward(fr, out, ("counts", "touched")))
    assert 1.0 <= mu.image_margin(fr, out) <= 10.0


# (mutant, frame) -> the comparators (or layers) that reject it in the suite as it was before the canary scene: the random scenes of
# test_gpu_random.test_random_scene_parity already show saturated pixels and o G > 0.99; no parity test had a scale modifier != 1
PREVIOUS = {
    ("F2", "random/P4097_96x96"): ("image", "counts"), ("F2", "random/P1000_200x150"): ("image", "counts"),
    ("F2", "random/P65_16x16"): ("image", "counts"),
    ("F3", "random/P4097_96x96"): ("image", "counts"), ("F3", "random/P1000_200x150"): ("image",),
    ("A4", "random/P4097_96x96"): "AC", ("A4", "random/P1000_200x150"): "AC",
    ("A5", "random/P4097_96x96"): "AC", ("A5", "random/P65_16x16"): "AC",
    ("B5", "random/P4097_96x96"): "", ("B5", "random/P1000_200x150"): "",
}


@pytest.mark.parametrize("mid,name", sorted(PREVIOUS), ids=["%s-%s" % k for k in sorted(PREVIOUS)])
def test_previous_suite_map(mid, name):
    fr = mu.frame(name)
    want = PREVIOUS[(mid, name)]
    if mid in FWD:
        out = FWD[mid](fr)
        assert {w for w in ("image", "counts", "touched") if rejected(lambda: mu.check_forward(fr, out, (w,)))} == set(want)
    else:
        g = BWD[mid](fr)
        assert rejecting_layers(fr, g) == set(want), margins(fr, g)
        if not want:  # modifier 1: the mutant IS the oracle's output
            for a, b in zip(g, fr.grads()):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("bits", [16, 32])
def test_F8_record_rounding(bits):
    """bits=16: the fp16-record frame judged, the kernel forgot the rounding (it returns the fp32 frame); bits=32: the fp32 frame
    judged, the kernel rounds anyway."""
    fr = mu.frame(CANARY) if bits == 32 else mu.Frame(CANARY, record_bits=16)
    _, out, g = mu.f8_other_record_bits(fr, 48 - bits)
    assert rejected(lambda: mu.check_forward(fr, out, ("image",)))
    assert "A" in rejecting_layers(fr, g)


def test_F9_one_pixel_and_borderline_budget():
    fr = mu.frame(CANARY)
    border = fr.gref["error_model"]["border_mask"]
    ys, xs = np.nonzero(~border & (fr.st["n_contrib"] > 0))
    px = (int(ys[len(ys) // 2]), int(xs[len(xs) // 2]))
    assert not rejected(lambda: mu.check_forward(fr, mu.f9_one_pixel(fr, 0.5, px), ("image",)))
    out = mu.f9_one_pixel(fr, 2.0, px)
    assert rejected(lambda: mu.check_forward(fr, out, ("image",)))
    assert 1.0 <= mu.image_margin(fr, out) <= 10.0
    # borderline pixels may differ, but only max(1, flip_fraction H W) of them
    bys, bxs = np.nonzero(border)
    cand = [(int(y), int(x)) for y, x in zip(bys, bxs) if hp.borderline_pixel(fr.st, int(x), int(y))]
    n = int(max(1.0, hp.IMG_FLIP_FRACTION * fr.st["H"] * fr.st["W"]))
    assert len(cand) > n
    assert not rejected(lambda: mu.check_forward(fr, mu.f9_borderline_pixels(fr, cand[:n]), ("image",)))
    assert rejected(lambda: mu.check_forward(fr, mu.f9_borderline_pixels(fr, cand[:n + 1]), ("image",)))


# ---- backward: layer (A) -------------------------------------------------------------------------------------------------------
BWD = {"A1": mu.a1_conic_offdiag_x2, "A2": mu.a2_no_background_term, "A3": mu.a3_depth_seed_ignored,
       "A4": mu.a4_dG_zero_where_clamped, "A5": mu.a5_walk_one_past, "B2": mu.b2_sh_clamp_ignored,
       "B3": mu.b3_view_rotation_transposed, "B5": mu.b5_scale_modifier_ignored}
BWD_MAP = {  # (mutant, scene) -> layers that must reject it (and only those: a compositor bug leaves (B) passing, a chain bug (A))
    ("A1", CANARY): "AC", ("A1", "p500_100x75_sh0"): "AC", ("A1", "p300_behind_64x48"): "AC",
    ("A2", CANARY): "AC", ("A2", "p500_100x75_sh0"): "AC", ("A2", "p300_behind_64x48"): "AC",
    ("A3", CANARY): "AC", ("A3", "p500_100x75_sh0"): "AC", ("A3", "p300_behind_64x48"): "AC",
    ("A4", CANARY): "AC", ("A4", "p500_100x75_sh0"): "", ("A4", "p300_behind_64x48"): "",
    ("A5", CANARY): "AC", ("A5", "p500_100x75_sh0"): "", ("A5", "p300_behind_64x48"): "",
    ("B2", CANARY): "BC", ("B2", "p300_behind_64x48"): "BC",
    ("B3", CANARY): "BC", ("B3", "p500_100x75_sh0"): "BC", ("B3", "p300_behind_64x48"): "BC",
    ("B5", CANARY): "BC", ("B5", "p500_100x75_sh0"): "", ("B5", "p300_behind_64x48"): "",
}


@pytest.mark.parametrize("mid,name", sorted(BWD_MAP), ids=["%s-%s" % k for k in sorted(BWD_MAP)])
def test_backward_mutant_rejected_by_its_layer(mid, name):
    fr = mu.frame(name)
    g = BWD[mid](fr)
    assert rejecting_layers(fr, g) == set(BWD_MAP[(mid, name)]), (mid, name, margins(fr, g))
    if not BWD_MAP[(mid, name)]:  # the scene does not exercise the bug (no o G > 0.99 / modifier 1): the output is the oracle's
        for a, b in zip(g, fr.grads()):
            np.testing.assert_array_equal(a, b)


def test_A4_subtle_margins():
    fr = mu.frame(CANARY)
    w = margins(fr, mu.a4_dG_zero_where_clamped(fr))
    assert 1.0 < w["A"] < 10.0 and 1.0 < w["C"] < 10.0, w


# (Gaussian, tile) of the canary scene, fixed so that a looser bound lets the mutant through: among the Gaussians with >= 2 tiles,
# the tile whose lost share is the smallest one still over (A)'s bound (clean: no borderline pixel touches the Gaussian; flipped:
# it has a non-zero flip budget; uniform: the same rule on the canary scene painted in one colour, with that frame's own shares);
# and the Gaussians with the largest share of any tile
A6_CLEAN, A6_FLIPPED, A6_UNIFORM = (91, 13), (99, 21), (189, 15)
LARGE_CLEAN, LARGE_FLIPPED = (375, 23), (347, 21)


@pytest.mark.parametrize("kind", ["clean", "flipped"])
def test_A6_lost_atomic_subtle(kind):
    fr = mu.frame(CANARY)
    gid, tile = A6_CLEAN if kind == "clean" else A6_FLIPPED
    assert fr.clean[gid] == (kind == "clean") and (mu.lost_share_ratio(fr, gid) > 0).sum() >= 2
    g = mu.a6_lost_atomic(fr, gid, tile)
    assert rejecting_layers(fr, g) >= {"A"} and "B" not in rejecting_layers(fr, g)
    assert 1.0 < margins(fr, g)["A"] < 10.0


@pytest.mark.parametrize("kind", ["clean", "flipped"])
def test_A7_one_sum_off_by_k_bounds(kind):
    fr = mu.frame(CANARY)
    gid, _ = LARGE_CLEAN if kind == "clean" else LARGE_FLIPPED
    assert fr.clean[gid] == (kind == "clean")
    for comp in range(10):
        assert not rejected(lambda: mu.check_backward(fr, mu.a7_one_sum_off(fr, gid, comp, 0.5))), (comp,)
        for k in (2, 5, 20):
            g = mu.a7_one_sum_off(fr, gid, comp, k)
            assert rejected(lambda: hp.assert_grads_close(g, fr.gref, CANARY, layers=("A",))), (comp, k)
            assert not rejected(lambda: mu.check_backward(fr, g, layers=("B",))), (comp, k)


# ---- backward: layer (B) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_B1_tau_halves_and_sign(name):
    fr = mu.frame(name)
    _, dev = mu.device(name)
    for g in (mu.b1_tau_halves_swapped(dev), mu.b1_tau_sign(dev, 4)):
        msg = rejected(lambda: mu.check_backward(fr, g, layers=("B",)))
        assert msg and "(B)" in msg and "dL_dtau" in msg
        assert "A" not in rejecting_layers(fr, g)


def test_B4_rows_exchanged():
    fr = mu.frame(CANARY)
    _, dev = mu.device(CANARY)
    mag = np.abs(fr.gref["dL_dmean3D"]).max(axis=1)
    i, j = (int(x) for x in np.argsort(mag)[-2:])
    assert rejecting_layers(fr, mu.b4_rows_exchanged(dev, i, j)) == {"B", "C"}


def test_B6_chain_on_half_sums():
    fr = mu.frame(CANARY)
    _, dev = mu.device(CANARY)
    g = mu.b6_chain_on_half_sums(fr, dev)
    assert rejecting_layers(fr, g) == {"B", "C"}
    assert 1.0 < margins(fr, g)["C"] < 10.0


def test_B8_B9_chain_inputs_at_half_precision():
    """Realistic chain bugs that only a per-row check sees: the camera position (B8) or the scale modifier (B9) read at half
    precision.  (C) does not reject B8; it rejects B9 by a hair."""
    fr = mu.frame(CANARY)
    g = mu.b8_campos_half(fr)
    assert rejecting_layers(fr, g) == {"B"}
    assert 1.0 < margins(fr, g)["B"] < 10.0
    g = mu.b9_scale_modifier_half(fr)
    assert "B" in rejecting_layers(fr, g) and "A" not in rejecting_layers(fr, g)
    assert 1.0 < margins(fr, g)["B"] < 10.0


def test_B7_one_chain_row_off_by_k_allowances():
    fr = mu.frame(CANARY)
    _, dev = mu.device(CANARY)
    gid = int(np.argmax(np.abs(fr.gref["dL_dmean3D"]).max(axis=1)))
    for nm in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dsh"):
        assert not rejected(lambda: mu.check_backward(fr, mu.b7_one_row_off(fr, dev, nm, gid, 0.5), layers=("B",))), nm
        g = mu.b7_one_row_off(fr, dev, nm, gid, 2.0)
        msg = rejected(lambda: mu.check_backward(fr, g, layers=("B",)))
        assert msg and "(B)" in msg and nm in msg
        assert 1.0 < margins(fr, g)["B"] < 10.0


# ---- (C) on its own: no oracle state, no error model, GRAD_TOL -----------------------------------------------------------------
def test_C_alone_rejects_A1_A6_B1():
    fr = mu.frame(CANARY)
    _, dev = mu.device(CANARY)
    bare = {k: v for k, v in fr.gref.items() if k != "error_model"}
    gid, tile = LARGE_CLEAN
    for mid, g in (("A1", mu.a1_conic_offdiag_x2(fr)), ("A6", mu.a6_lost_atomic(fr, gid, tile)), ("B1", mu.b1_tau_halves_swapped(dev))):
        msg = rejected(lambda: hp.assert_grads_close(g, bare, CANARY + "/C-alone", tol=hp.GRAD_TOL))
        assert msg and "(C)" in msg, mid


# ---- the cap on cond in (C)'s clean check --------------------------------------------------------------------------------------
def test_uniform_colour_scene_A6_still_rejected():
    """A map painted in one colour (tools/fuzz_uniform.py: dL/dalpha cancels): a lost tile share of a clean Gaussian is still
    rejected by (A), and the clean check's cond stays under COND_CAP without allow_cancellation."""
    fr = mu.Frame(CANARY, shs=mu.uniform_colour)
    w = margins(fr, fr.grads())
    assert max(v for k, v in w.items() if k.endswith("/clean_cond_over_tol")) < hp.COND_CAP
    gid, tile = A6_UNIFORM
    assert fr.clean[gid]
    g = mu.a6_lost_atomic(fr, gid, tile)
    assert "A" in rejecting_layers(fr, g)
    assert 1.0 < margins(fr, g)["A"] < 10.0
