"""CPU: the frame-to-frame RGB-D alignment without a GPU -- the new C-ABI symbols and their binding; the premises the GPU tests rest on,
checked on tests/align_restated.py alone (the analytic gradient is the finite difference of the loss; the float32 mirror agrees with
the float64 restatement; every mutant is rejected by the comparators the GPU tests use; the restated pyramid loop converges, from
further away than the single level; the committed cases hold next to no borderline pixels); and the host logic of gsaj.RgbdAligner
with the device work replaced."""
import numpy as np
import pytest

import align_restated as ar
import gn_restated as gn
from abi import HEADER, declarations, signature_mismatches

F = np.float32
NEW = ("gsaj_rgbd_align_partial_rows", "gsaj_rgbd_align")


def _lib():
    import os

    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- header and binding -----------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_alignment_entry_points_and_the_binding_matches_them():
    from gsaj import _lib as binding

    decls = declarations()
    for name in NEW:
        assert name in decls and name in binding.SIGNATURES, name
    assert [m for m in signature_mismatches(binding.SIGNATURES) if m[0] in NEW] == []
    assert decls["gsaj_rgbd_align"][1][-1] == ("void *", "stream") and len(decls["gsaj_rgbd_align"][1]) == 25
    lib = _lib()
    assert lib.gsaj_version() >= 111
    for name in NEW:
        assert hasattr(lib, name), name
    import gsaj

    assert "RgbdAligner" in gsaj.__all__ and gsaj.RgbdAligner.__name__ == "RgbdAligner"


def test_the_header_says_that_the_reference_has_no_counterpart_and_keeps_earlier_sections_where_they_were():
    with open(HEADER) as fh:
        text = fh.read()
    at = text.index("frame-to-frame RGB-D alignment")
    assert "NO counterpart" in text[at:at + 1200]
    assert at > text.index("gsaj_debug_launch_plan(int P"), "the new section is appended at the end"
    assert "#define GSAJ_ALIGN_PIXEL_FLOATS 16" in text[at:]


@pytest.mark.parametrize("W,H,want", [(2, 2, 1), (64, 4, 1), (65, 4, 2), (64, 5, 2), (80, 60, 30), (97, 61, 32), (640, 480, 1200),
                                      (16384, 16384, 256 * 4096), (1, 2, 0), (2, 1, 0), (0, 0, 0), (-5, 7, 0), (16385, 2, 0), (2, 16385, 0)])
def test_the_partial_rows_are_one_per_workgroup_of_64_by_4_pixels_and_none_for_a_refused_size(W, H, want):
    assert _lib().gsaj_rgbd_align_partial_rows(W, H) == want
    if want:
        assert want == -(-W // 64) * -(-H // 4)


# ---- premises ------------------------------------------------------------------------------------------------------------------------------
def _loss_at(case, tau):
    c = dict(case, w2c_exact=gn.se3_exp(tau) @ np.asarray(case["w2c"], np.float64))
    px = ar.pixels(c)
    return ar.fold(px["terms"], c)[27], px


@pytest.mark.parametrize("mode", ar.MODES)
def test_premise_the_gradient_is_the_central_finite_difference_of_the_normalised_loss(mode):
    """Step 1e-6 in each of the six directions of the left increment, in float64, at the 33 x 17 parity case -- asserted to be a pose
    where no pixel changes its cell or a gate under the probe, so that n is constant and the loss is C^1 along it.  Central difference:
    truncation h^2 |f'''| / 6 and rounding 2^-52 |loss| / h ~ 1e-12; the loss's curvature jumps where |r| crosses delta (by at most
    kappa J^2 / delta per pixel), so a pixel within h |J| of the kink adds an error of the order h J^2 / (delta n) ~ 1e-6 x 1 / (0.01 x 500)
    x its share: the tolerance is 2e-7 + 1e-6 |g|."""
    h = 1e-6
    case = ar.parity_case(33, 17, mode)
    base_loss, base = _loss_at(case, np.zeros(6))
    row = ar.fold(base["terms"], case)
    worst = 0.0
    for k in range(6):
        tau = np.zeros(6)
        tau[k] = h
        lp, pp = _loss_at(case, tau)
        lm, pm = _loss_at(case, -tau)
        for probe in (pp, pm):
            assert np.array_equal(ar.flags_of(probe), ar.flags_of(base)), "a gate changes under the probe: choose another pose"
            cell = lambda p: np.floor(p["pre"][..., :2])[base["valid"]]   # noqa: E731
            assert np.array_equal(cell(probe), cell(base)), "a pixel changes its cell under the probe: choose another pose"
        fd = (lp - lm) / (2 * h)
        err = abs(fd - row[21 + k])
        print("direction %d: g %.9e  finite difference %.9e  |difference| %.2e" % (k, row[21 + k], fd, err))
        assert err <= 2e-7 + 1e-6 * abs(row[21 + k]), (k, fd, row[21 + k])
        worst = max(worst, err)
    assert base_loss > 0 and np.abs(row[21:27]).max() > 1e-3, "the probe sits on a slope"


@pytest.mark.parametrize("W,H", ar.parity_sizes())
@pytest.mark.parametrize("mode", ar.MODES)
def test_premise_the_mirror_agrees_with_the_float64_restatement(W, H, mode):
    """Off the borderline pixels the gates agree, and every slot of the row lies within align_restated.rounding_bound."""
    case = ar.parity_case(W, H, mode)
    p64, p32 = ar.pixels(case), ar.mirror(case)
    border = ar.borderline(case, p64)
    assert not ((ar.flags_of(p64) != ar.flags_of(p32)) & ~border).any()
    assert p32["rec"].dtype == F and p32["terms"].dtype == F, "the mirror stays in float32 from end to end"
    r64, r32 = ar.fold(p64["terms"], case), ar.fold(p32["terms"], case)
    assert abs(r64[30] - r32[30]) <= border.sum() and r64[30] >= 1
    bound = ar.rounding_bound(case, p64, border)
    err = np.abs(r64 - r32)[:30]
    assert (err <= bound[:30]).all(), (np.flatnonzero(err > bound[:30]), err, bound)
    # and the mirror is its own fixed point under the comparators
    assert ar.assert_pixels_equal(p32["rec"], ar.flags_of(p32), p32, border, "self") == 0
    ar.assert_row_close(r32.astype(F), p32["terms"], case, border, "self")


def _rejected(fake, mir, case, border):
    out = []
    try:
        ar.assert_pixels_equal(fake["rec"], ar.flags_of(fake), mir, border, "mutant")
    except AssertionError:
        out.append("pixels")
    try:
        ar.assert_row_close(ar.fold(fake["terms"], case).astype(F), mir["terms"], case, border, "mutant")
    except AssertionError:
        out.append("row")
    return out


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_every_mutant_is_rejected_by_the_comparators_of_the_gpu_tests(mutant):
    """The mutant's float32 evaluation stands in for a wrong kernel's pix_out, valid_out and gn_row on the 33 x 17 case with depth (its
    reference pose is not the identity, or the side T is multiplied on would not show).  The Jacobian is not in pix_out: the mutants of
    J alone must fall to the row comparator."""
    case = ar.parity_case(33, 17, "depth")
    if mutant == "textbook_level_intrinsics":   # a wrong camera at level 1 of the behaviour scene
        base = ar.behaviour_case(1.0)
        start = ar.motion(0.5)
        case = ar.level_case(base, 1, start)
        fake = ar.mirror(ar.level_case(base, 1, start, mutant=mutant))
    else:
        fake = ar.mirror(case, mutant)
    mir = ar.mirror(case)
    border = ar.borderline(case)
    got = _rejected(fake, mir, case, border)
    assert got, "%s passes both comparators" % mutant
    if mutant in ("cross_block_sign", "jz_without_dz"):
        assert got == ["row"], got


def test_premise_the_restated_loop_converges_and_the_pyramid_is_no_worse_than_the_single_level(record_property):
    """m = 1 and m = 2, with and without the depth term: L = 2 with the default schedule (8, 6, 6) against one level with the same 20
    iterations.  Both end at the SAME minimum of the level-0 loss when both get there, so 'below or equal' is asserted up to the length
    of the last step each loop took -- what it was still moving by when it was stopped."""
    for m in (1.0, 2.0):
        for depth in (True, False):
            case = ar.behaviour_case(m, depth)
            true = ar.motion(m)
            start = ar.pose_error(case["w2c"], true)
            pyr, one = ar.align_loop(case, 2), ar.align_loop(case, 0, [20])
            ep, e1 = ar.pose_error(pyr["w2c"], true), ar.pose_error(one["w2c"], true)
            slack = float(np.linalg.norm(pyr["st"]["tau"]) + np.linalg.norm(one["st"]["tau"]))
            line = "m=%g depth=%s: start %.4f / %.4f   single level %.5f / %.5f   pyramid %.5f / %.5f   last steps %.1e" % (
                (m, depth) + start + e1 + ep + (slack,))
            print(line)
            record_property("m%g_depth%d" % (m, depth), line)
            for k in range(2):
                assert ep[k] <= e1[k] + slack, line
                assert ep[k] < 0.1 * start[k], line
            for l, acc in pyr["losses"]:
                assert all(b <= a for a, b in zip(acc, acc[1:])), "the accepted loss rises within level %d" % l


def _committed_cases():
    for W, H in ar.parity_sizes():
        for mode in ar.MODES:
            yield "%dx%d %s" % (W, H, mode), ar.parity_case(W, H, mode)
    yield "%dx%d depth" % ar.LONG_FOLD, ar.parity_case(*ar.LONG_FOLD, "depth")
    for sign in (1, -1):
        yield "planted %+d" % sign, ar.planted_case(sign)[0]
    yield "planted near", ar.planted_near_case()[0]


def test_premise_at_most_one_percent_of_the_valid_pixels_of_a_committed_case_are_borderline():
    """Every case whose pixels are compared bit for bit.  (The behaviour runs are not: they START at the reference pose, where T is the
    identity and every u an integer, and are judged by where they end.)"""
    for name, case in _committed_cases():
        px = ar.pixels(case)
        n, nb = int(px["valid"].sum()), int(ar.borderline(case, px).sum())
        assert n >= 1, "%s has no valid pixel" % name
        assert nb <= 0.01 * n, "%s: %d of %d valid pixels are borderline" % (name, nb, n)


def test_premise_the_planted_pixels_show_what_they_were_planted_for():
    for sign in (1, -1):
        case, planted, _ = ar.planted_case(sign)
        mir = ar.mirror(case)
        fl, rec = ar.flags_of(mir), mir["rec"]
        at = lambda k: (planted[k][1], planted[k][0])   # noqa: E731
        pre = mir["pre"][at("u_exact")]
        if sign > 0:
            assert pre[0] == F(case["W"] - 1) and fl[at("u_exact")] == 0, "u = W - 1 exactly is outside"
        else:
            assert pre[0] == F(0) and fl[at("u_exact")] & 1 and rec[at("u_exact")][0] == 0, "u = 0 exactly is inside"
        for k in ("ref_depth_zero", "ref_depth_nan", "ref_depth_inf", "ref_color_nan", "ref_color_inf", "cur_color_nan", "cur_color_inf"):
            assert fl[at(k)] == 0 and not rec[at(k)].any(), k
        for k in ("cur_depth_nan", "cur_depth_inf", "edge_outside"):
            assert fl[at(k)] == 1 and not rec[at(k)][11:].any(), k
        assert fl[at("edge_inside")] == 3
        for k, s in (("r_above", 1.0), ("r_above_neg", -1.0)):
            assert rec[at(k)][9] == F(s) and rec[at(k)][13] == F(s), (k, rec[at(k)])
        for k in ("r_below", "r_below_neg"):
            assert 0.85 < abs(rec[at(k)][9]) < 0.95 and 0.85 < abs(rec[at(k)][13]) < 0.95, (k, rec[at(k)])
        assert np.isfinite(mir["terms"]).all() and np.isfinite(rec).all(), "no NaN or inf reaches a sum"
    case, planted = ar.planted_near_case()
    mir = ar.mirror(case)
    fl = ar.flags_of(mir)
    (xb, yb), (xa, ya) = planted["zc_below"], planted["zc_above"]
    assert fl[yb, xb] == 0 and mir["Zr"][yb, xb] > F(case["min_depth"]) > mir["pre"][yb, xb, 4]
    assert fl[ya, xa] & 1 and mir["pre"][ya, xa, 4] > F(case["min_depth"])


# ---- host logic of RgbdAligner ---------------------------------------------------------------------------------------------------------
def _host_aligner(monkeypatch, W=160, H=120, levels=2, **kw):
    import torch

    from gsaj import align as A
    from gsaj import pyramid as Pm

    log = []
    monkeypatch.setattr(A, "_residuals", lambda al, l, depth: log.append(("residuals", l, depth)))
    monkeypatch.setattr(A, "_step", lambda al, l: log.append(("step", l)))
    monkeypatch.setattr(A, "_relevel", lambda al, l: log.append(("relevel", l)))
    monkeypatch.setattr(Pm.ImagePyramid, "build", lambda self, c, d=None, m=None, depth_edge_ratio=0.1: log.append(("build", d is not None)))
    al = A.RgbdAligner.__new__(A.RgbdAligner)
    a = dict(w_depth=1.0, delta_photo=0.01, delta_depth=0.01, depth_edge_ratio=0.1, min_depth=0.01, max_depth=100.0, min_overlap=0.0)
    a.update({k: kw.pop(k) for k in list(kw) if k in a})
    lm = kw.pop("lm", (1e-3, 4.0, 1e-7, 1e7, 1e-4))
    assert not kw
    al._init_host(W, H, (150.0, 140.0, 80.0, 60.0), "cpu", levels, tuple(a.values()), (0.01, 100.0), lm)
    frame = lambda v: (torch.full((3, H, W), v), torch.full((H, W), 2.0))   # noqa: E731
    return al, log, frame


def test_aligner_levels_cameras_and_buffers(monkeypatch):
    al, _, _ = _host_aligner(monkeypatch, W=166, H=126)
    assert [c[:2] for c in al.cams] == [(166, 126), (83, 63), (41, 31)]
    for l, c in enumerate(al.cams):   # the exact intrinsics of the cropped, box-filtered image -- not (cx + 0.5) / 2^l - 0.5
        assert c[2:] == (150.0 / 2 ** l, 140.0 / 2 ** l, 80.0 / 2 ** l, 60.0 / 2 ** l)
        want = ar.level_intrinsics(dict(W=166, H=126, fx=150.0, fy=140.0, cx=80.0, cy=60.0), l)
        assert c == (want["W"], want["H"], want["fx"], want["fy"], want["cx"], want["cy"])
    assert al.rows.shape == (3 * 32, 32) and al.row.shape == (32,) and al.state.shape == (136,)
    assert len(al.projections) == 3 and al.projections[1].shape == (4, 4)
    assert al.default_schedule() == [8, 6, 6]
    flat, _, _ = _host_aligner(monkeypatch, levels=0)
    assert flat.default_schedule() == [8] and flat._ref.pyramid is None


def test_aligner_runs_the_schedule_coarse_to_fine_and_validates_it(monkeypatch):
    from gsaj._lib import GsajError

    al, log, frame = _host_aligner(monkeypatch)
    with pytest.raises(GsajError, match="set_reference"):
        al.align(*frame(0.4))
    al.set_reference(*frame(0.5), np.eye(4))
    del log[:]
    assert al.align(*frame(0.4), schedule=[2, 0, 1]) == [2, 0, 1]
    assert log == [("build", True), ("residuals", 2, True), ("step", 2), ("residuals", 2, True), ("step", 2), ("relevel", 0),
                   ("residuals", 0, True), ("step", 0)]
    assert float(al.state[80]) == pytest.approx(1e-3) and np.array_equal(al.state[0:16].numpy().reshape(4, 4), np.eye(4, dtype=F))
    del log[:]
    al.align(frame(0.4)[0], None, w2c_init=np.diag([1.0, 1.0, 1.0, 1.0]))
    assert [e for e in log if e[0] == "residuals"][0] == ("residuals", 2, False) and len([e for e in log if e[0] == "step"]) == 20
    assert [e for e in log if e[0] == "relevel"] == [("relevel", 1), ("relevel", 0)]
    for bad in ([1, 2], [1, 2, 3, 4], [1, -1, 1], 5):
        with pytest.raises(GsajError, match="schedule must hold 3 non-negative counts"):
            al.align(*frame(0.4), schedule=bad)


def test_aligner_promote_swaps_the_frames_and_takes_the_pose(monkeypatch):
    import torch

    from gsaj._lib import GsajError

    al, _, frame = _host_aligner(monkeypatch)
    with pytest.raises(GsajError, match="align\\(\\) a frame first"):
        al.promote()
    al.set_reference(*frame(0.5), np.eye(4))
    al.align(*frame(0.25))
    ref, cur = al._ref, al._cur
    pose = torch.eye(4)
    pose[0, 3] = 0.125
    al.state[88:104] = pose.reshape(16)
    al.promote()
    assert al._ref is cur and al._cur is ref and float(al._ref.color[0, 0, 0]) == 0.25, "swapped, not copied"
    assert torch.equal(al.ref_w2c.view(4, 4), pose), "the aligned pose by default"
    with pytest.raises(GsajError, match="align\\(\\) a frame first"):
        al.promote()
    al.align(*frame(0.75))
    other = torch.eye(4)
    other[1, 3] = -0.5
    al.promote(other)
    assert torch.equal(al.ref_w2c.view(4, 4), other) and float(al._ref.color[0, 0, 0]) == 0.75
    al.align(frame(0.1)[0], None)
    with pytest.raises(GsajError, match="needs depth"):
        al.promote()


def test_aligner_refuses_cpu_tensors_bad_sizes_and_bad_arguments(monkeypatch):
    import torch

    from gsaj import RgbdAligner
    from gsaj._lib import GsajError

    with pytest.raises(GsajError, match="there is no CPU path"):
        RgbdAligner(160, 120, 150.0, 150.0, 80.0, 60.0, "cpu")
    al, _, frame = _host_aligner(monkeypatch)
    with pytest.raises(GsajError, match="there is no CPU path"):
        al.set_reference(frame(0.5)[0].numpy(), frame(0.5)[1], np.eye(4))
    with pytest.raises(GsajError, match="there is no CPU path"):
        al.set_reference(frame(0.5)[0].to("meta"), frame(0.5)[1], np.eye(4))
    with pytest.raises(GsajError, match="must have 57600 elements"):
        al.set_reference(torch.zeros(3, 60, 80), frame(0.5)[1], np.eye(4))
    with pytest.raises(GsajError, match="the reference frame needs depth"):
        al.set_reference(frame(0.5)[0], None, np.eye(4))
    with pytest.raises(GsajError, match="4x4"):
        al.set_reference(*frame(0.5), np.eye(3))
    for kw, msg in ((dict(levels=5), "levels must be 0..4"), (dict(levels=-1), "levels must be 0..4"), (dict(W=7, H=9, levels=2), "at least 2x2"),
                    (dict(W=16385, H=4, levels=0), "at most 16384"), (dict(delta_photo=0.0), "delta_photo"), (dict(w_depth=-1.0), "w_depth"),
                    (dict(min_depth=0.0), "min_depth"), (dict(min_depth=3.0, max_depth=2.0), "min_depth"), (dict(min_overlap=1.5), "min_overlap"),
                    (dict(lm=(1e-3, 1.0, 1e-7, 1e7, 1e-4)), "nu > 1")):
        with pytest.raises(GsajError, match=msg):
            _host_aligner(monkeypatch, **kw)
    assert _host_aligner(monkeypatch, W=8, H=9, levels=2)[0].cams[2][:2] == (2, 2)
