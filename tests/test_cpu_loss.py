"""The loss family's restatement (tests/loss_restated.py) without a device: pinned to the arrays recorded from the reference and to
oracle/loss_oracle.py, shown to be reachable by an honest fp32 evaluation (the fp32 mirror passes assert_loss_close on every generated
case), and shown to reject wrong kernels (the `mutant=` switch) at the output the bug lands in.

| id  | bug                                                    | case                         | rejected at                         |
|-----|--------------------------------------------------------|------------------------------|-------------------------------------|
| L1  | gt sum >= rgb_thr                                      | map, thr 0.5 (dyadic)        | dL_dcolor, planted pixel            |
| L2  | gt_depth >= 0.01 (>= 0 in the verification loss)       | map, cl-depth-mask           | dL_ddepth, planted pixel            |
| L3  | opacity >= 0.95                                        | track                        | dL_ddepth, planted pixel            |
| L4  | sgn(0) = +1                                            | map-noexp, track-mask-a0     | dL_dcolor, dL_ddepth                |
| L5  | tracking depth gate without the opacity test           | track                        | dL_ddepth                           |
| L6  | opacity weight applied in mapping                      | map                          | dL_dcolor                           |
| L7  | mask applied in mapping                                | map-mask-given               | dL_dcolor                           |
| L8  | alpha for 1 - alpha in k_d                             | map                          | dL_ddepth                           |
| L9  | b omitted                                              | track                        | dL_dcolor (signs), dL_dopacity      |
| L10 | ea missing from dL/da                                  | map                          | dL_dexposure_a                      |
| L11 | depth mean over the valid pixels instead of HW         | map                          | dL_ddepth, l1_depth                 |
| L12 | one workgroup's partial dropped                        | track-mask 37x29             | each of the five scalars            |
| L13 | a stale partial in an unused slot of the fused forward | track-mask 37x29             | each of the five scalars            |
| L14 | the dropped partial against the OLD check              | cancelling 64x48             | old: passes; new: dL_dexposure_a    |
| I1  | isotropic: sgn(0) = +1                                 | P 257, C 3                   | dL_dscales, row (1/8, 2/8, 3/8)     |
| I2  | isotropic: mean over P instead of P C                  | P 257, C 3                   | dL_dscales, loss                    |
"""
import glob
import os

import numpy as np
import pytest

import loss_restated as lr
from oracle import loss_oracle as lo

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "loss_seed*_64x48.npz")))
KINDS = {"tracking": lr.TRACKING, "mapping": 0, "mapping_init": lr.NO_EXPOSURE}


def rejected(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


def family(name):
    return name.rsplit("-", 1)[0]


# ---- pinned ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p) for p in GOLD])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_restatement_reproduces_the_reference_goldens(path, kind):
    """The tolerances of tests/test_gpu_loss.py::test_loss_seeds_match_reference_goldens."""
    g = np.load(path)
    flags = KINDS[kind] | (lr.MONOCULAR if bool(g["monocular"]) else 0)
    v = lr.restate(flags, g["alpha"], g["rgb_boundary_threshold"], g["image"], g["depth"], g["opacity"], g["gt"], g["gt_depth"],
                   g["grad_mask"], g["exposure_a"], g["exposure_b"])["value"]
    assert abs(v["loss"] - float(g[kind + "_loss"])) < 2e-7 + 1e-6 * abs(float(g[kind + "_loss"]))
    np.testing.assert_allclose(v["dL_dcolor"], g[kind + "_dL_dimage"], rtol=1e-5, atol=1e-10)
    np.testing.assert_allclose(v["dL_ddepth"], g[kind + "_dL_ddepth"], rtol=1e-5, atol=1e-10)
    if kind == "tracking":
        np.testing.assert_allclose(v["dL_dopacity"], g[kind + "_dL_dopacity"], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(v["dL_dexposure_a"], float(g[kind + "_dL_da"][0]), rtol=2e-4, atol=1e-8)
    np.testing.assert_allclose(v["dL_dexposure_b"], float(g[kind + "_dL_db"][0]), rtol=2e-4, atol=1e-8)


@pytest.mark.parametrize("flags,masked", [(lr.TRACKING, True), (0, False), (lr.MONOCULAR, False), (lr.TRACKING | lr.NO_EXPOSURE, True)])
def test_restatement_agrees_with_the_oracle_away_from_the_gates(flags, masked):
    """A random frame with nothing planted: no gt sum, gt depth or opacity within an ulp of its threshold, every residual GUARD eps from
    0 -- the one place where the oracle (float64 gt sum) and the restatement (fp32 gt sum) must say the same."""
    fr = lr.make_frame(53, 47, flags, masked, 3, plant=False)
    v = fr["want"]["value"]
    o = lo.loss_and_seeds(flags, fr["image"], fr["depth"], fr["opacity"], fr["gt"], fr["gt_depth"] if fr["gt_depth"] is not None else
                          np.zeros((47, 53), np.float32), fr["mask"], fr["a"], fr["b"], float(fr["alpha"]), float(fr["rgb_thr"]))
    for k, ko in (("dL_dcolor", "dL_dimage"), ("dL_ddepth", "dL_ddepth")):
        np.testing.assert_allclose(v[k], o[ko], rtol=1e-6, atol=0, err_msg=k)   # (the oracle hands its images out in fp32)
    # (... and forms the residual in fp32: what |r| is made of is the scale of its rounding, here and in the sums below)
    assert (np.abs(v["dL_dopacity"] - o["dL_dopacity"]) <= lr.ROUND_K * lr.EPS * fr["want"]["mass"]["dL_dopacity"]).all()
    for k, ko in (("loss", "loss"), ("l1_rgb", "l_rgb"), ("l1_depth", "l_depth"), ("dL_dexposure_a", "dL_da"), ("dL_dexposure_b", "dL_db")):
        assert abs(v[k] - o[ko]) <= 1e-6 * fr["want"]["mass"][k], k


def test_the_oracle_cannot_state_the_threshold():
    """Why the restatement decides on the fp32 sum: at the planted pixels the float64 sum of the same three values is on the other
    side of the threshold (or on it) for at least one of them."""
    fr = lr.make_case("map-37x29")
    p = fr["planted"]["rgb_thr"]
    g = fr["gt"].reshape(3, -1)[:, p]
    s32 = (g[0] + g[1]) + g[2]
    assert list(s32 > fr["rgb_thr"]) == [False, True, False]
    assert list(g.astype(np.float64).sum(axis=0) > 0.01) != [False, True, False]


# ---- reachable ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lr.cases())
def test_fp32_mirror_passes_every_case(name):
    fr = lr.make_case(name)
    mirror = lr.restate_frame(fr, dtype=np.float32)["value"]
    ratios = lr.assert_loss_close(mirror, fr["want"], name)
    print(name, {k: round(v, 4) for k, v in ratios.items()})
    lr.note("mirror_fp32_cpu", family(name), ratios)
    v = fr["want"]["value"]
    if name == "cl-no-valid-pixel-37x29":
        # max(n_valid, 1): a finite 0 where torch's mean over an empty selection (Jacobian_test.py compute_loss) gives NaN
        assert mirror["l1_depth"] == 0.0 and v["l1_depth"] == 0.0 and mirror["loss"] == mirror["l1_rgb"] and not mirror["dL_ddepth"].any()
    for strip, out in (("zero_color", "dL_dcolor"), ("zero_depth", "dL_ddepth")):
        if strip in fr["planted"]:   # open gate, residual exactly 0: the seed is exactly 0 (first planted pixel: all channels)
            p = fr["planted"][strip][0]
            assert not mirror[out].reshape(mirror[out].shape[0], -1)[:, p].any() and fr["want"]["mass"]["dL_dopacity"].reshape(-1)[p] >= 0


@pytest.mark.parametrize("P", lr.ISO_P)
@pytest.mark.parametrize("C", lr.ISO_C)
def test_fp32_mirror_passes_every_isotropic_case(P, C):
    c = lr.make_iso_case(P, C)
    for acc in (False, True):
        m = lr.iso_restate(c["scales"], lr.ISO_WEIGHT, c["grad_in"] if acc else None, dtype=np.float32)["value"]
        lr.note("mirror_fp32_cpu", "isotropic", lr.assert_iso_close(m["loss"], m["dL_dscales"], c["want_acc" if acc else "want"], "iso %d %d" % (P, C)))
        if not acc:
            assert not m["dL_dscales"][c["equal_rows"]].any()


def test_one_equal_row_in_seven_has_an_fp32_mean_off_by_an_ulp():
    a = np.exp(np.random.default_rng(0).uniform(np.log(0.01), np.log(0.2), 100000)).astype(np.float32)
    off = (((a + a) + a) / np.float32(3) != a).mean()
    assert 0.05 < off < 0.3, off


# ---- canaries ----------------------------------------------------------------------------------------------------------------------
CANARIES = [
    ("ge_rgb", "map-37x29", None, "dL_dcolor"), ("ge_rgb", "track-mask-thr0.5-37x29", None, "dL_dcolor"),
    ("ge_depth", "map-37x29", None, "dL_ddepth"), ("ge_depth", "cl-depth-mask-37x29", None, "dL_ddepth"),
    ("ge_opacity", "track-37x29", None, "dL_ddepth"),
    ("sgn0_plus", "map-noexp-37x29", None, "dL_dcolor"), ("sgn0_plus", "track-mask-a0-37x29", None, "dL_dcolor"),
    ("sgn0_plus", "track-mask-37x29", ("dL_ddepth",), "dL_ddepth"),
    ("depth_gate_without_opacity", "track-37x29", None, "dL_ddepth"),
    ("opacity_weight_in_mapping", "map-37x29", None, "dL_dcolor"),
    ("mask_in_mapping", "map-mask-given-37x29", None, "dL_dcolor"),
    ("alpha_for_one_minus_alpha", "map-37x29", None, "dL_ddepth"),
    ("b_omitted", "track-37x29", None, "dL_dcolor"), ("b_omitted", "track-37x29", ("dL_dopacity",), "dL_dopacity"),
    ("ea_missing_from_da", "map-37x29", None, "dL_dexposure_a"),
    ("depth_mean_over_valid", "map-37x29", None, "dL_ddepth"), ("depth_mean_over_valid", "map-37x29", ("l1_depth",), "l1_depth"),
] + [(m, "track-mask-37x29", (k,), k) for m in ("drop_partial", "stale_partial") for k in lr.SCALARS]


@pytest.mark.parametrize("mutant,name,outputs,where", CANARIES, ids=["%s-%s-%s" % (c[0], c[1], c[3]) for c in CANARIES])
def test_mutated_restatement_is_rejected(mutant, name, outputs, where):
    fr = lr.make_case(name)
    bad = lr.restate_frame(fr, mutant=mutant)["value"]
    msg = rejected(lambda: lr.assert_loss_close(bad, fr["want"], name, outputs))
    assert msg is not None and (": %s" % where) in msg, (mutant, name, msg)
    if mutant in ("ge_rgb", "ge_depth", "ge_opacity"):   # the ONLY pixels such a mutant moves are those exactly ON the threshold
        g = fr["gt"].reshape(3, -1)
        on = {"ge_rgb": lambda: (g[0] + g[1]) + g[2] == fr["rgb_thr"],
              "ge_depth": lambda: fr["gt_depth"].reshape(-1) == np.float32(0.0 if fr["flags"] & lr.COMPUTE_LOSS else 0.01),
              "ge_opacity": lambda: fr["opacity"].reshape(-1) == np.float32(0.95)}[mutant]()
        n = bad[where].shape[0]
        moved = (bad[where].reshape(n, -1) != fr["want"]["value"][where].reshape(n, -1)).any(axis=0)
        assert moved.any() and not (moved & ~on).any(), np.flatnonzero(moved)


def test_the_old_check_passes_a_dropped_partial_that_the_bound_rejects():
    """The checks tests/test_gpu_loss.py had: loss to 1e-6 of its value, dL/da and dL/db to rtol 1e-4 of theirs.  On the cancelling frame
    the last workgroup holds small terms (opacity 3e-5): losing its partial moves dL/da by 9e-6 of sum|term| -- four times what any
    fp32 summation of these terms can -- and by less than 1e-4 of dL/da itself.  (For dL/db, which cancels, the old tolerance is 1e-4 of
    nearly nothing: tighter than any honest evaluation's rounding, so there it is the correct evaluation the old check can fail.)"""
    fr = lr.make_case("cancelling-64x48")
    want = fr["want"]["value"]
    bad = lr.restate_frame(fr, mutant="drop_partial")["value"]
    assert abs(bad["loss"] - want["loss"]) < 1e-6 * abs(want["loss"]) + 1e-9
    for k in ("dL_dexposure_a", "dL_dexposure_b"):
        np.testing.assert_allclose(bad[k], want[k], rtol=1e-4, atol=1e-9)
    msg = rejected(lambda: lr.assert_loss_close(bad, fr["want"], "cancelling"))
    assert msg is not None and ": dL_dexposure_a" in msg, msg
    # the other half of the old check's defect: the honest fp32 mirror, inside its bound, is OUTSIDE rtol 1e-4 of the cancelling dL/db
    # as soon as the sum cancels far enough -- its error is a rounding of the terms, not of the net
    mass, net = fr["want"]["mass"]["dL_dexposure_b"], abs(want["dL_dexposure_b"])
    assert 1e-4 * net + 1e-9 < lr.SUM_K * lr.EPS * mass + lr.EPS * net


@pytest.mark.parametrize("mutant,where", [("sgn0_plus", "dL_dscales"), ("mean_over_P", "dL_dscales"), ("mean_over_P", "loss")])
def test_mutated_isotropic_restatement_is_rejected(mutant, where):
    c = lr.make_iso_case(257, 3)
    bad = lr.iso_restate(c["scales"], lr.ISO_WEIGHT, mutant=mutant)["value"]
    grad = c["want"]["value"]["dL_dscales"] if where == "loss" else bad["dL_dscales"]
    msg = rejected(lambda: lr.assert_iso_close(bad["loss"], grad, c["want"], "iso"))
    assert msg is not None and where in msg, msg
    if mutant == "sgn0_plus":
        rows = np.unique(np.argwhere(bad["dL_dscales"] != c["want"]["value"]["dL_dscales"])[:, 0])
        assert set(rows) == set(c["ramp_rows"])   # equal rows survive it (sg - ssum / C cancels); the exact-zero middle does not
