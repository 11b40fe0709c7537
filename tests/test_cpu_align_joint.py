"""CPU: the joint frame-to-frame alignment (the affine brightness change solved with the pose) without a GPU -- the new C-ABI symbol and
its binding; the premises the GPU tests rest on, checked on tests/align_joint_restated.py alone (g8 is the finite difference of the
normalised loss over all eight unknowns; every mutant is rejected; the float32 mirror agrees with the float64 restatement; the finding
the feature answers: a brightness change takes the pose-only loop further from the truth than its start, the joint loop is back at the
unchanged scene's error; collinear exposure columns stay finite); and the host logic of gsaj.JointRgbdAligner with the device work
replaced.

The joint form is a class of its own, gsaj.JointRgbdAligner, not a solve_exposure keyword of RgbdAligner: tests/test_cpu_loops.py holds
RgbdAligner.__init__ and RgbdAligner.align to their signatures, and this suite's existing files stay as they are."""
import os

import numpy as np
import pytest

import align_joint_restated as aj
import align_restated as ar
import gn8_restated as gn8
import gn_restated as gn
from abi import HEADER, X, call, declarations, signature_mismatches

F = np.float32
INVALID_ARGUMENT = -1


def _lib():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- header and binding -------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_joint_entry_point_and_the_binding_matches_it():
    from gsaj import _gn_state as S
    from gsaj import _lib as binding

    decls = declarations()
    assert "gsaj_rgbd_align8" in decls and "gsaj_rgbd_align8" in binding.SIGNATURES
    assert [m for m in signature_mismatches(binding.SIGNATURES) if m[0] == "gsaj_rgbd_align8"] == []
    six, joint = decls["gsaj_rgbd_align"][1], decls["gsaj_rgbd_align8"][1]
    names = [n for _, n in joint]
    assert len(joint) == len(six) + 1 == 26 and joint[-1] == ("void *", "stream")
    assert names[names.index("gn8_row") + 1] == "gain_out" and "gn8_state" in names
    assert [t for t, _ in joint if _ != "gain_out"] == [t for t, _ in six], "the arguments of gsaj_rgbd_align, type for type"
    lib = _lib()
    assert hasattr(lib, "gsaj_rgbd_align8") and lib.gsaj_version() >= 112
    assert (S.ROW_VALID, S.layout("gn").row_valid, S.layout("gn8").row_valid) == (30, 30, aj.VALID)
    with open(HEADER) as fh:
        text = fh.read()
    at = text.index("gsaj_rgbd_align8 --")
    assert at > text.index("#define GSAJ_ALIGN_PIXEL_FLOATS 16"), "the joint form is stated behind the 6-form"
    for line in ("g_I = ea I_r", "r_I = I_c - (g_I + b)", "[47] n", "[49:64) zero"):
        assert line in text[at:], line


GOOD = dict(W=80, H=60, fx=70.0, fy=70.0, cx=40.0, cy=30.0, ref_color=X, ref_depth=X, ref_w2c=X, cur_color=X, cur_depth=X, gn8_state=X,
            w_depth=1.0, delta_photo=0.01, delta_depth=0.01, depth_edge_ratio=0.1, min_depth=0.01, max_depth=100.0, min_overlap=0.0, rows=X,
            gn8_row=X, gain_out=X, pix_out=X, valid_out=X, skip=None, stream=None)
MESSAGE = ("gsaj_rgbd_align8: W and H must be 2..16384; ref_color, ref_depth, ref_w2c, cur_color, gn8_state, rows and gn8_row are required; "
           "fx, fy, delta_photo, delta_depth > 0; w_depth, depth_edge_ratio >= 0; 0 < min_depth < max_depth; min_overlap in [0, 1] "
           "(W=%d H=%d fx=%g fy=%g w_depth=%g delta_photo=%g delta_depth=%g depth_edge_ratio=%g min_depth=%g max_depth=%g min_overlap=%g)")
BAD = [("W = 1", dict(W=1)), ("H > 16384", dict(H=16385)), ("NULL ref_color", dict(ref_color=None)), ("NULL ref_depth", dict(ref_depth=None)),
       ("NULL ref_w2c", dict(ref_w2c=None)), ("NULL cur_color", dict(cur_color=None)), ("NULL gn8_state", dict(gn8_state=None)),
       ("NULL rows", dict(rows=None)), ("NULL gn8_row", dict(gn8_row=None)), ("fx is NaN", dict(fx=float("nan"))), ("fy < 0", dict(fy=-70.0)),
       ("delta_photo = 0", dict(delta_photo=0.0)), ("delta_depth < 0", dict(delta_depth=-0.01)), ("w_depth < 0", dict(w_depth=-1.0)),
       ("depth_edge_ratio < 0", dict(depth_edge_ratio=-0.1)), ("min_depth = max_depth", dict(min_depth=2.0, max_depth=2.0)),
       ("min_overlap > 1", dict(min_overlap=1.5)), ("min_overlap is NaN", dict(min_overlap=float("nan")))]


@pytest.mark.parametrize("what,kw", BAD, ids=[r[0] for r in BAD])
def test_bad_joint_call_is_refused_with_its_code_and_message_before_any_launch(what, kw):
    """The pointers are ones nothing may read (abi.X): a launch would not come back."""
    lib = _lib()
    args = dict(GOOD, **kw)
    assert call(lib, "gsaj_rgbd_align8", **args) == INVALID_ARGUMENT, (what, lib.gsaj_last_error())
    f = lambda k: float(F(args[k]))   # noqa: E731
    assert lib.gsaj_last_error().decode() == MESSAGE % (args["W"], args["H"], f("fx"), f("fy"), f("w_depth"), f("delta_photo"), f("delta_depth"),
                                                        f("depth_edge_ratio"), f("min_depth"), f("max_depth"), f("min_overlap")), what


# ---- premises: the gradient ----------------------------------------------------------------------------------------------------------------
FD_TRUE, FD_AT = (0.1, 0.03), (0.08, 0.035)   # the current frame's brightness and the exposure the gradient is taken at: residuals of
#                                               0.02 I - 0.005 on top of the scene's, on both sides of delta = 0.01


def _fd_case(mode):
    return aj.with_brightness(ar.parity_case(33, 17, mode), *FD_TRUE, exposure=FD_AT)


def _exact(case, x=np.zeros(8)):
    """The case x away from its pose and exposure, both taken unrounded (and the gain exp(a) in float64)."""
    a0, b0 = (np.float64(v) for v in case["exposure"])
    return dict(case, w2c_exact=gn.se3_exp(x[:6]) @ np.asarray(case["w2c"], np.float64), exposure_exact=(a0 + x[6], b0 + x[7]))


def _loss8_at(case, x):
    c = _exact(case, x)
    px = aj.pixels8(c)
    return aj.fold8(px["terms"], c)[aj.LOSS], px


def _finite_difference(case, h=1e-6):
    """-> (the central finite difference of the normalised loss over the eight unknowns, the analytic row at the same point)."""
    _, base = _loss8_at(case, np.zeros(8))
    fd = np.zeros(8)
    for k in range(8):
        x = np.zeros(8)
        x[k] = h
        lp, pp = _loss8_at(case, x)
        lm, pm = _loss8_at(case, -x)
        for probe in (pp, pm):
            assert np.array_equal(ar.flags_of(probe), ar.flags_of(base)), "a gate changes under the probe: choose another pose"
            cell = lambda p: np.floor(p["pre"][..., :2])[base["valid"]]   # noqa: E731
            assert np.array_equal(cell(probe), cell(base)), "a pixel changes its cell under the probe: choose another pose"
        fd[k] = (lp - lm) / (2 * h)
    return fd, base


_FD = {}


def _fd(mode):
    if mode not in _FD:
        _FD[mode] = (_fd_case(mode),) + _finite_difference(_fd_case(mode))
    return _FD[mode]


def _gradient_errors(fd, terms, case):
    g = aj.fold8(terms, case)[aj.NH:aj.NH + aj.NX]
    return g, np.abs(fd - g), 2e-7 + 1e-6 * np.abs(g)


@pytest.mark.parametrize("mode", ar.MODES)
def test_premise_g8_is_the_central_finite_difference_of_the_normalised_loss_over_all_eight_unknowns(mode):
    """Step 1e-6 in each of the eight directions, in float64, at the 33 x 17 parity case with the current frame at (0.1, 0.03) and the
    state's exposure at (0.08, 0.035) -- (a, b) != 0 -- asserted to be a point where no pixel changes its cell or a gate under the probe.
    The tolerance is test_cpu_align.py's, 2e-7 + 1e-6 |g|, for its reasons: the exposure directions move every residual by at most
    h (e^a I_r or 1), no further than a pose direction moves them."""
    case, fd, base = _fd(mode)
    g, err, tol = _gradient_errors(fd, base["terms"], case)
    for k in range(8):
        print("direction %d: g %.9e  finite difference %.9e  |difference| %.2e" % (k, g[k], fd[k], err[k]))
    assert (err <= tol).all(), (np.flatnonzero(err > tol), fd, g)
    assert np.abs(g[:6]).max() > 1e-3 and abs(g[6]) > 1e-3 and abs(g[7]) > 1e-3, "the probe sits on a slope in the pose and in a and b"


# ---- premises: the mutants -----------------------------------------------------------------------------------------------------------------
def _rejected_by_parity(fake, mir, case, border):
    out = []
    try:
        ar.assert_pixels_equal(fake["rec"], ar.flags_of(fake), mir, border, "mutant")
    except AssertionError:
        out.append("pixels")
    try:
        aj.assert_row_close8(aj.fold8(fake["terms"], case).astype(F), mir["terms"], case, border, "mutant")
    except AssertionError:
        out.append("row")
    return out


@pytest.mark.parametrize("mutant", aj.MUTANTS)
def test_every_mutant_is_rejected_by_the_finite_difference_or_by_the_comparators_of_the_gpu_tests(mutant):
    """The mutant's float64 g8 against the finite difference of the TRUE loss; the mutant's float32 evaluation standing in for a wrong
    kernel's pix_out, valid_out and gn8_row, against the mirror.  What each must fall to is stated: a wrong column shows in g8 and in
    the row; a wrong residual in pix_out; a wrong packing of H8 in the row alone (g8 does not see H8)."""
    case, fd, _ = _fd("depth")
    _, err, tol = _gradient_errors(fd, aj.pixels8(_exact(case), mutant=mutant)["terms"], case)
    by_fd = bool((err > tol).any())
    mir, border = aj.mirror8(case), ar.borderline(case)
    by_parity = _rejected_by_parity(aj.mirror8(case, mutant=mutant), mir, case, border)
    print("%s: finite difference %s, comparators %s" % (mutant, "rejects" if by_fd else "passes", by_parity or "pass"))
    assert by_fd or by_parity, "%s passes the finite difference and both comparators" % mutant
    if mutant == "h8_by_columns":
        assert not by_fd and by_parity == ["row"]
    elif mutant == "gain_on_current":
        assert "pixels" in by_parity
    else:
        assert by_fd and "row" in by_parity, (by_fd, by_parity)
    assert _rejected_by_parity(mir, mir, case, border) == [], "the mirror is its own fixed point under the comparators"


# ---- premises: the mirror ------------------------------------------------------------------------------------------------------------------
def _mirror_cases():
    for W, H in aj.PARITY_SIZES + [(33, 17)]:
        for mode in ar.MODES:
            yield W, H, mode, (0.1, 0.03)
    for e in ((0.0, 0.0), (-0.15, 0.05)):
        yield 97, 61, "depth", e


@pytest.mark.parametrize("W,H,mode,exposure", list(_mirror_cases()))
def test_premise_the_mirror_agrees_with_the_float64_restatement(W, H, mode, exposure):
    """Off the borderline pixels the gates agree, and every slot of the row lies within align_joint_restated.rounding_bound8, both sides
    evaluated at the same gain (the float32 e^a: expf's own error is the device's to report, not the mirror's to absorb)."""
    case = aj.parity_case8(W, H, mode, *exposure)
    p64, p32 = aj.pixels8(case), aj.mirror8(case)
    border = ar.borderline(case, p64)
    assert not ((ar.flags_of(p64) != ar.flags_of(p32)) & ~border).any()
    assert p32["rec"].dtype == F and p32["terms"].dtype == F, "the mirror stays in float32 from end to end"
    r64, r32 = aj.fold8(p64["terms"], case), aj.fold8(p32["terms"], case)
    assert abs(r64[aj.VALID] - r32[aj.VALID]) <= border.sum() and r64[aj.VALID] >= 1
    bound = aj.rounding_bound8(case, p64, border)
    err = np.abs(r64 - r32)[:aj.VALID]
    assert (err <= bound[:aj.VALID]).all(), (np.flatnonzero(err > bound[:aj.VALID]), err, bound)
    assert not r32[aj.GATES + 1:].any() and np.abs(r32[aj.NH + 6:aj.NH + 8]).max() > 0
    assert ar.assert_pixels_equal(p32["rec"], ar.flags_of(p32), p32, border, "self") == 0
    aj.assert_row_close8(r32.astype(F), p32["terms"], case, border, "self")


def _committed_cases():
    for W, H in aj.PARITY_SIZES:
        for mode in ar.MODES:
            for e in aj.EXPOSURES:
                yield "%dx%d %s %s" % (W, H, mode, e), aj.parity_case8(W, H, mode, *e)
    yield "%dx%d depth" % aj.LONG_FOLD, aj.parity_case8(*aj.LONG_FOLD, "depth", 0.1, 0.03)
    for sign in (1, -1):
        yield "planted %+d" % sign, aj.planted_case8(sign)[0]


def test_premise_at_most_one_percent_of_the_valid_pixels_of_a_committed_joint_case_are_borderline():
    """Every case whose pixels are compared bit for bit, with the gain applied: the gates are those of the 6-form (the brightness
    reaches no gate), and so is the cap."""
    for name, case in _committed_cases():
        px = aj.pixels8(case)
        n, nb = int(px["valid"].sum()), int(ar.borderline(case, px).sum())
        assert n >= 1, "%s has no valid pixel" % name
        assert nb <= 0.01 * n, "%s: %d of %d valid pixels are borderline" % (name, nb, n)


def test_premise_the_planted_pixels_show_what_they_were_planted_for_through_the_joint_form():
    for sign in (1, -1):
        case, planted, _ = aj.planted_case8(sign)
        mir = aj.mirror8(case)
        fl, rec = ar.flags_of(mir), mir["rec"]
        at = lambda k: (planted[k][1], planted[k][0])   # noqa: E731
        assert np.array_equal(fl, ar.flags_of(ar.mirror(ar.planted_case(sign)[0]))), "the gates are the 6-form's"
        for k, s in (("r_above", 1.0), ("r_above_neg", -1.0)):
            assert rec[at(k)][9] == F(s) and rec[at(k)][13] == F(s), (k, rec[at(k)])
        for k in ("r_below", "r_below_neg"):
            assert 0.85 < abs(rec[at(k)][9]) < 0.95 and 0.85 < abs(rec[at(k)][13]) < 0.95, (k, rec[at(k)])
        assert np.isfinite(mir["terms"]).all() and np.isfinite(rec).all(), "no NaN or inf reaches a sum"


# ---- the finding: a brightness change and the two loops ---------------------------------------------------------------------------------------
BRIGHT = (0.1, 0.03)


@pytest.mark.parametrize("m", [1.0, 2.0])
@pytest.mark.parametrize("depth", [True, False], ids=["depth", "photometric"])
def test_a_brightness_change_throws_the_pose_only_loop_and_the_joint_loop_recovers(m, depth, record_property):
    """The behaviour scene at 80 x 60, L = 2, schedule 8 / 6 / 6, start at the reference pose, the current frame's colour e^a I + b with
    (a, b) = (0.1, 0.03).  The pose-only loop ends ABOVE its start error in translation; the joint loop ends below a tenth of the start
    error in both components; and where brightness did not change the joint loop costs at most a factor of two plus POSE_FLOOR."""
    true = ar.motion(m)
    plain, bright = ar.behaviour_case(m, depth), aj.behaviour_case8(m, depth, *BRIGHT)
    start = ar.pose_error(plain["w2c"], true)
    pose_only, joint = ar.align_loop(bright, 2), aj.align8_loop(bright, 2)
    e6, e8 = ar.pose_error(pose_only["w2c"], true), ar.pose_error(joint["w2c"], true)
    p6, p8 = ar.align_loop(plain, 2), aj.align8_loop(plain, 2)
    f6, f8 = ar.pose_error(p6["w2c"], true), ar.pose_error(p8["w2c"], true)
    line = ("m=%g %s: start %.4f / %.4f   (0.1, 0.03): pose only %.4f / %.4f, joint %.5f / %.5f, recovered (%.4f, %.4f)   "
            "(0, 0): pose only %.5f / %.5f, joint %.5f / %.5f, recovered (%.4f, %.4f)" % (
                (m, "depth" if depth else "photometric") + start + e6 + e8 + tuple(joint["exposure"]) + f6 + f8 + tuple(p8["exposure"])))
    print(line)
    record_property("m%g_depth%d" % (m, depth), line)
    assert e6[0] > start[0], line
    for k in range(2):
        assert e8[k] < 0.1 * start[k], line
        assert f8[k] <= 2 * f6[k] + ar.POSE_FLOOR, line
    for l, acc in joint["losses"] + p8["losses"]:
        assert all(b <= a for a, b in zip(acc, acc[1:])), "the accepted loss rises within level %d" % l


def test_the_tolerance_of_the_recovered_exposure_is_computed_from_the_two_restated_loops(record_property):
    """Twice the distance between the float64 loop and the float32 loop, plus the rounding floor: defined once, in the restatement, from
    no device result.  Printed for DESIGN; asserted only to be a tolerance -- above the floor, and far below the exposure it judges."""
    for m in (1.0, 2.0):
        for depth in (True, False):
            tol, r64, r32 = aj.exposure_tolerance(m, depth, *BRIGHT)
            line = "m=%g %s: float64 loop (%.6f, %.6f), float32 loop (%.6f, %.6f), tolerance (%.2e, %.2e)" % (
                (m, "depth" if depth else "photometric") + tuple(r64["exposure"]) + tuple(r32["exposure"]) + tuple(tol))
            print(line)
            record_property("m%g_depth%d" % (m, depth), line)
            assert (tol >= aj.EXPOSURE_FLOOR).all() and (tol < 0.1 * np.abs(r64["exposure"])).all(), line


# ---- degenerate texture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "mirror"])
def test_collinear_exposure_columns_stay_finite_and_the_pose_does_not_move(dtype):
    """An 8 x 8 constant reference (0.5) and a constant current frame (0.62): every image gradient is zero, so the six pose columns are
    zero and the a and b columns are collinear (-e^a 0.5 and -1).  The damped system is still positive definite (lambda diag(H8) on the
    exposure block, eps I on the pose block): every step stays finite, the pose does not move, e^a c + b approaches the target."""
    case = aj.constant_case()
    record = []
    out = aj.align8_loop(case, 0, [12], dtype=dtype, record=record)
    px = aj.pixels8(case, dtype)
    assert px["valid"].sum() == 49 and not px["J8"][..., :6].any() and not np.asarray(aj.fold8(px["terms"], case))[:6].any()
    model = lambda e: float(np.exp(e[0]) * 0.5 + e[1])   # noqa: E731
    target = float(np.float64(F(0.62)) * 3 * np.float64(F(1.0 / 3.0)))
    errs = [abs(model(e) - target) for _, e in record]
    for w2c, e in record:
        assert np.isfinite(w2c).all() and np.isfinite(e).all()
        assert np.array_equal(w2c, np.eye(4)), "the pose moved"
    assert np.isfinite(out["st"]["H"]).all() and np.isfinite(out["st"]["g"]).all() and out["st"]["accepted"] >= 2
    print("|e^a c + b - target| after each step:", " ".join("%.2e" % e for e in errs))
    assert abs(model(out["exposure"]) - target) < 0.01 * abs(0.5 - target), errs


# ---- host logic of JointRgbdAligner -----------------------------------------------------------------------------------------------------------
def _host_aligner(monkeypatch, joint=True, W=160, H=120, levels=2):
    import torch

    from gsaj import align as A
    from gsaj import pyramid as Pm

    log = []
    monkeypatch.setattr(A, "_residuals", lambda al, l, depth: log.append(("residuals", l, depth)))
    monkeypatch.setattr(A, "_step", lambda al, l: log.append(("step", l)))
    monkeypatch.setattr(A, "_relevel", lambda al, l: log.append(("relevel", l)))
    monkeypatch.setattr(Pm.ImagePyramid, "build", lambda self, c, d=None, m=None, depth_edge_ratio=0.1: log.append(("build", d is not None)))
    cls = A.JointRgbdAligner if joint else A.RgbdAligner
    al = cls.__new__(cls)
    al._init_host(W, H, (150.0, 140.0, 80.0, 60.0), "cpu", levels, (1.0, 0.01, 0.01, 0.1, 0.01, 100.0, 0.0), (0.01, 100.0),
                  (1e-3, 4.0, 1e-7, 1e7, 1e-4))
    frame = lambda v: (torch.full((3, H, W), v), torch.full((H, W), 2.0))   # noqa: E731
    return al, log, frame


def test_aligner_buffers_in_both_forms(monkeypatch):
    six, _, _ = _host_aligner(monkeypatch, joint=False, W=166, H=126)
    assert six.solve_exposure is False and six.rows.shape == (3 * 32, 32) and six.row.shape == (32,) and six.state.shape == (136,)
    joint, _, _ = _host_aligner(monkeypatch, W=166, H=126)
    assert joint.solve_exposure is True and joint.rows.shape == (3 * 32, 64) and joint.row.shape == (64,) and joint.state.shape == (152,)
    assert joint.cams == six.cams and joint.default_schedule() == six.default_schedule() == [8, 6, 6]
    assert joint.lm["H"].shape == (8, 8) and joint.lm["g"].shape == (8,) and six.lm["H"].shape == (6, 6)
    import inspect

    import gsaj
    assert "JointRgbdAligner" in gsaj.__all__ and issubclass(gsaj.JointRgbdAligner, gsaj.RgbdAligner)
    assert gsaj.JointRgbdAligner.__init__ is gsaj.RgbdAligner.__init__, "the constructor is RgbdAligner's"
    assert inspect.signature(gsaj.JointRgbdAligner.align).parameters["exposure_init"].default is None
    assert "exposure_init" not in inspect.signature(gsaj.RgbdAligner.align).parameters
    with pytest.raises(gsaj._lib.GsajError, match="there is no CPU path"):
        gsaj.JointRgbdAligner(160, 120, 150.0, 150.0, 80.0, 60.0, "cpu")


def test_aligner_runs_the_same_schedule_and_starts_the_exposure_where_it_is_told(monkeypatch):
    import torch

    from gsaj._lib import GsajError

    al, log, frame = _host_aligner(monkeypatch)
    al.set_reference(*frame(0.5), np.eye(4))
    del log[:]
    assert al.align(*frame(0.4), schedule=[2, 0, 1]) == [2, 0, 1]
    assert log == [("build", True), ("residuals", 2, True), ("step", 2), ("residuals", 2, True), ("step", 2), ("relevel", 0),
                   ("residuals", 0, True), ("step", 0)]
    assert float(al.state[80]) == pytest.approx(1e-3) and not al.state[33:35].any() and not al.state[148:150].any(), "(a, b) starts at (0, 0)"
    al.align(*frame(0.4), exposure_init=(0.25, -0.125))
    assert al.state[33:35].tolist() == [0.25, -0.125] and al.state[148:150].tolist() == [0.25, -0.125], "the state's and the accepted one"
    assert torch.equal(al.relative_exposure, al.state[148:150]) and al.relative_exposure.data_ptr() == al.state.data_ptr() + 4 * 148
    al.align(*frame(0.4), exposure_init=torch.tensor([0.5, 0.0625]))
    assert al.state[33:35].tolist() == [0.5, 0.0625]
    al.align(*frame(0.4))
    assert not al.state[33:35].any(), "every align() starts again at (0, 0) unless told otherwise"
    al.row[aj.VALID] = 4800.0
    al.row[30] = 1.0
    assert float(al.overlap) == pytest.approx(4800.0 / (160 * 120)), "the joint row's count slot"
    for bad in ((1.0,), (1.0, 2.0, 3.0), np.zeros((2, 2))):
        with pytest.raises(GsajError, match="an exposure is the pair"):
            al.align(*frame(0.4), exposure_init=bad)


def test_the_pose_only_aligner_has_no_exposure_arguments_and_is_what_it_was(monkeypatch):
    al, log, frame = _host_aligner(monkeypatch, joint=False)
    al.set_reference(*frame(0.5), np.eye(4))
    with pytest.raises(TypeError, match="exposure_init"):
        al.align(*frame(0.4), exposure_init=(0.0, 0.0))
    assert not hasattr(al, "relative_exposure") and not hasattr(al, "exposure_for")
    del log[:]
    al.align(*frame(0.4), schedule=[1, 0, 0])
    assert log == [("build", True), ("residuals", 2, True), ("step", 2)]
    al.row[30] = 2400.0
    assert float(al.overlap) == pytest.approx(2400.0 / (40 * 30)) and al.state.shape == (136,), "slot 30 of the 6-form's row, level 2's pixels"


@pytest.mark.parametrize("ref,rel", [((0.0, 0.0), (0.1, 0.03)), ((0.2, -0.05), (0.1, 0.03)), ((-0.3, 0.1), (-0.15, 0.05)), ((0.25, 0.5), (0.0, 0.0))])
def test_exposure_for_is_its_formula(monkeypatch, ref, rel):
    """(a_r + a, e^a b_r + b) against float64: exp within 2 ulp, one product, one sum -- 4 roundings of values below 1 + |b_r| + |b|."""
    import torch

    al, _, frame = _host_aligner(monkeypatch)
    al.state[148:150] = torch.tensor(rel)
    want = aj.exposure_for(F(ref), F(rel))
    for given in (ref, torch.tensor(ref), np.asarray(ref)):
        got = al.exposure_for(given)
        assert got.shape == (2,) and got.dtype == torch.float32 and got.device == al.state.device
        assert np.abs(got.numpy().astype(np.float64) - want).max() <= 4 * ar.EPS * (1 + abs(ref[1]) + abs(rel[1]))
    # the formula's reason: obs = e^a' render + b' holding for both frames
    render = 0.37
    obs_r = np.exp(ref[0]) * render + ref[1]
    assert np.exp(want[0]) * render + want[1] == pytest.approx(np.exp(rel[0]) * obs_r + rel[1], rel=1e-6)


def test_the_joint_loop_is_the_pose_only_loops_arithmetic_where_nothing_is_joint():
    """The restatement's own consistency: with the exposure columns cut off, pixels8 at (0, 0) IS align_restated.pixels -- the 6 x 6
    block of H8, g8[:6], the losses and the counts, bit for bit in float32."""
    case = ar.parity_case(33, 17, "depth")
    six, joint = ar.mirror(case), aj.mirror8(dict(case, exposure=(F(0), F(0))))
    idx = [n for n, (k, l) in enumerate(gn8.SYM8) if l < 6]
    assert np.array_equal(joint["terms"][..., idx], six["terms"][..., :21]) and np.array_equal(joint["terms"][..., 36:42], six["terms"][..., 21:27])
    assert np.array_equal(joint["terms"][..., 44:49], six["terms"][..., 27:32]) and np.array_equal(joint["rec"], six["rec"])
