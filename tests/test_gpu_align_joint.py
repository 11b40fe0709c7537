"""GPU: the joint frame-to-frame alignment (csrc/align.hip: k_rgbd_align8, k_rgbd_align8_fold; gsaj.JointRgbdAligner)
against tests/align_joint_restated.py.

Per-pixel parity: pix_out / valid_out against the float32 mirror EVALUATED AT THE GAIN THE DEVICE REPORTS, bit for bit at every
non-borderline pixel (expf is the one operation of the kernel NumPy cannot mirror: it is compared on its own, within 2 ulp, and exactly
1 at a = 0); the row against the float64 sum of the mirror's terms within align_joint_restated.row_bound8; the fold past one trip of its
load loop; the gates; the memory contract under tests/guards.py; the behaviour of the whole aligner on the analytic scene with a
brightness change against the restated joint loop; the hand-off of the exposure to the map tracker.  tests/test_cpu_align_joint.py
checks the premises all of this rests on."""

import numpy as np
import pytest

import align_calls
import align_joint_restated as aj
import align_restated as ar
import guards

pytestmark = pytest.mark.gpu
DEV = align_calls.DEV
F = np.float32
_MEMO = {}
_CALLS = align_calls.Calls(joint=True)   # the buffers of a gsaj_rgbd_align8 call, the call, gsaj_pose_gn8_step on its row, JointRgbdAligner
_tensors, _call, _run, _step, _aligner = _CALLS.tensors, _CALLS.call, _CALLS.run, _CALLS.step, _CALLS.aligner
_bits, _dev = align_calls.bits, align_calls.dev


def _expect(key, make, gain):
    """The mirror of a case at the device's gain, its borderline pixels: computed once per (case, gain), shared, never modified."""
    key = key + (float(gain),)
    if key not in _MEMO:
        case = make()
        _MEMO[key] = (case, aj.mirror8(case, gain), ar.borderline(case))
    return _MEMO[key]


def _compare(make, key, tag):
    """One call of the case, and every comparison of the parity test.  -> (case, mirror, borderline, outputs)."""
    out, _ = _run(make())
    gain = out["gain"][0]
    case, mir, border = _expect(key, make, gain)
    aj.assert_gain(gain, case["exposure"][0], tag)
    other = ar.assert_pixels_equal(out["pix"], out["valid"], mir, border, tag)
    worst = aj.assert_row_close8(out["row"], mir["terms"], case, border, tag)
    print("%s: gain %.9g, n %d, depth gates %d, borderline %d (other side taken: %d), row worst err / bound %.3f" % (
        tag, gain, out["row"][aj.VALID], out["row"][aj.GATES], border.sum(), other, worst))
    return case, mir, border, out


# ---- per-pixel parity and the row -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", aj.PARITY_SIZES, ids=["%dx%d" % s for s in aj.PARITY_SIZES])
@pytest.mark.parametrize("mode", ar.MODES)
@pytest.mark.parametrize("exposure", aj.EXPOSURES, ids=["a%g_b%g" % e for e in aj.EXPOSURES])
def test_pixels_equal_the_mirror_at_the_returned_gain_bit_for_bit_and_the_row_is_their_sum(W, H, mode, exposure):
    tag = "%dx%d %s (a, b) = %s" % (W, H, mode, exposure)
    case, mir, border, out = _compare(lambda: aj.parity_case8(W, H, mode, *exposure), (W, H, mode, exposure), tag)
    row = out["row"]
    assert row[aj.VALID] >= 1 and (mode != "depth" or min(W, H) < 5 or row[aj.GATES] >= 1)
    assert row[aj.NH + 6] != 0 and row[aj.NH + 7] != 0 and row[6] != 0 and row[35] > 0, "the exposure columns are in g8 and in H8"
    if mode == "w0":
        assert row[aj.LOSS + 2] == 0 and (row[aj.GATES] == mir["gate"].sum() or border.any()), "w_depth = 0: the gates are counted, the term is nothing"
    if exposure[0] == 0:
        assert out["gain"][0] == F(1.0)


def test_a_frame_of_more_rows_than_one_trip_of_the_joint_folds_load_loop():
    """70 x 260 with depth: 2 x 65 = 130 rows of 64 floats.  gn_sum_rows<64> has 16 row groups and four loads in flight: one trip takes 64
    rows, so every group takes a second and a third trip, the last a partial one.  The comparisons of the parity test."""
    W, H = aj.LONG_FOLD
    case, mir, border, out = _compare(lambda: aj.parity_case8(W, H, "depth", 0.1, 0.03), (W, H, "depth", "long"), "%dx%d depth" % (W, H))
    assert out["rows"].shape == (130, 64) and not out["rows"][:, aj.GATES + 1:].any()
    assert out["row"][aj.VALID] >= 1 and out["row"][aj.GATES] >= 1


@pytest.mark.parametrize("sign", [1, -1])
def test_planted_pixels_on_every_gate_through_the_joint_form(sign):
    """align_restated.planted_case with the reference taken to another brightness and the state's exposure undoing it
    (align_joint_restated.planted_case8; tests/test_cpu_align_joint.py asserts that the mirror still shows each planted pixel)."""
    made = _MEMO.setdefault(("plant", sign, "raw"), aj.planted_case8(sign))
    planted = made[1]
    case, mir, border, out = _compare(lambda: made[0], ("plant", sign), "planted %+d" % sign)
    assert np.isfinite(out["pix"]).all() and np.isfinite(out["row"]).all() and np.isfinite(out["rows"]).all(), "a NaN or inf reached a sum"
    x, y = planted["u_exact"]
    if sign > 0:
        assert out["valid"][y, x] == 0, "u = W - 1 exactly is outside"
    else:
        assert out["valid"][y, x] & 1 and out["pix"][y, x, 0] == 0.0, "u = 0 exactly is inside"
    for k in ("ref_depth_zero", "ref_depth_nan", "ref_depth_inf", "ref_color_nan", "ref_color_inf", "cur_color_nan", "cur_color_inf"):
        assert out["valid"][planted[k][1], planted[k][0]] == 0, k
    for k in ("cur_depth_nan", "cur_depth_inf", "edge_outside"):
        assert out["valid"][planted[k][1], planted[k][0]] == 1, k
    assert out["valid"][planted["edge_inside"][1], planted["edge_inside"][0]] == 3
    for k, s in (("r_above", 1.0), ("r_above_neg", -1.0)):
        assert out["pix"][planted[k][1], planted[k][0], 9] == F(s), k


# ---- the gates of the fold ----------------------------------------------------------------------------------------------------------------
def test_a_frame_without_a_valid_pixel_moves_neither_the_pose_nor_the_exposure():
    import torch
    good = aj.parity_case8(80, 60, "depth", 0.1, 0.03)
    good["exposure"] = (F(0.08), F(0.035))
    empty = dict(good, ref_depth=np.zeros((60, 80), F))
    proj = torch.eye(4, device=DEV)
    # a first call: accepted as the baseline (there is no other), and H8 = g8 = 0 moves nothing
    t = _tensors(empty, torch)
    t["state"][80] = ar.LM["lambda_init"]
    before = t["state"].cpu().numpy()
    _call(empty, t)
    row = t["row"].cpu().numpy()
    assert not row[:aj.LOSS].any() and np.isposinf(row[aj.LOSS:aj.VALID]).all() and not row[aj.VALID:].any(), row
    assert not t["valid"].cpu().numpy().any() and not t["pix"].cpu().numpy().any()
    _step(t, proj)
    after = t["state"].cpu().numpy()
    assert (_bits(after[0:16]) == _bits(before[0:16])).all() and (_bits(after[88:104]) == _bits(before[0:16])).all(), "the pose moved"
    assert (_bits(after[33:35]) == _bits(before[33:35])).all() and (_bits(after[148:150]) == _bits(before[33:35])).all(), "the exposure moved"
    assert not after[70:76].any() and not after[78:80].any() and after[83] == 1 and after[84] == 0
    # a later call: a real step first, then the empty frame -- rejected, the accepted pose, exposure and loss stay bit for bit
    t = _tensors(good, torch)
    t["state"][80] = ar.LM["lambda_init"]
    _call(good, t)
    _step(t, proj)
    held = t["state"].cpu().numpy()
    assert held[83] == 1 and np.isfinite(held[81]) and held[70:76].any() and held[78:80].all(), "the first step accepts and proposes, a and b too"
    assert (_bits(held[148:150]) == _bits(before[33:35])).all() and (held[33:35] != held[148:150]).all()
    t["ref_depth"].zero_()
    _call(good, t)
    assert np.isposinf(t["row"].cpu().numpy()[aj.LOSS])
    _step(t, proj)
    after = t["state"].cpu().numpy()
    assert after[84] == 1 and after[83] == 1, "rejected"
    assert (_bits(after[88:104]) == _bits(held[88:104])).all() and _bits(after[81:82]) == _bits(held[81:82]), "the accepted pose or loss changed"
    assert (_bits(after[148:150]) == _bits(held[148:150])).all(), "the accepted exposure changed"
    assert after[80] > held[80], "more damping after a rejection"


def test_min_overlap_just_above_and_just_below_the_valid_share():
    make = lambda: aj.parity_case8(80, 60, "depth", 0.1, 0.03)   # noqa: E731
    out, _ = _run(make())
    case, mir, border = _expect((80, 60, "depth", "overlap"), make, out["gain"][0])
    n, WH = float(out["row"][aj.VALID]), 80 * 60
    assert n == mir["valid"].sum() or border.any()
    below, _ = _run(dict(case, min_overlap=(n - 0.5) / WH))
    assert (_bits(below["row"]) == _bits(out["row"])).all(), "n >= ceil(min_overlap W H): the row is the ungated one"
    above, _ = _run(dict(case, min_overlap=(n + 0.5) / WH))
    assert not above["row"][:aj.LOSS].any() and np.isposinf(above["row"][aj.LOSS:aj.VALID]).all()
    assert above["row"][aj.VALID] == n and above["row"][aj.GATES] == out["row"][aj.GATES] and not above["row"][aj.GATES + 1:].any()
    exact, _ = _run(dict(case, min_overlap=1.0))
    assert np.isposinf(exact["row"][aj.LOSS]), "not every pixel is valid"


# ---- the memory contract ------------------------------------------------------------------------------------------------------------------
def test_a_nonzero_skip_word_leaves_the_rows_the_row_the_gain_and_the_state_untouched():
    import torch
    case = aj.parity_case8(33, 17, "depth", 0.1, 0.03)
    t = _tensors(case, torch)
    for k in ("rows", "row", "pix", "gain"):
        t[k].fill_(-7.0)
    t["valid"].fill_(9)
    state = t["state"].clone()
    skip = torch.tensor([3], dtype=torch.int32, device=DEV)
    _call(case, t, skip=skip)
    assert all(bool((t[k] == -7.0).all()) for k in ("rows", "row", "pix", "gain")) and bool((t["valid"] == 9).all())
    assert torch.equal(t["state"], state), "gsaj_rgbd_align8 only reads the state"
    skip.zero_()
    _call(case, t, skip=skip)
    assert not bool((t["row"] == -7.0).any()) and not bool((t["rows"] == -7.0).any()) and float(t["gain"]) > 1.0
    assert torch.equal(t["state"], state)


@pytest.mark.parametrize("W,H,mode", [(97, 61, "depth"), (2, 2, "photo"), (65, 4, "depth")])
def test_memory_contract_bands_poisoned_scratch_same_bits_on_any_stream(monkeypatch, W, H, mode):
    import torch
    case = aj.parity_case8(W, H, mode, 0.1, 0.03)
    plain, _ = _run(case)
    outputs = ("rows", "row", "gain", "pix", "valid")
    for fill in guards.FILLS:
        with guards.guarded(monkeypatch, fill) as g:
            t = _tensors(case, torch)
            assert len(g.allocations) == 11 and g.payload_untouched(t["rows"]), "rows starts poisoned"
            for run in range(2):
                for k in outputs:
                    g.refill(t[k])
                _call(case, t)
                torch.cuda.synchronize()
                g.check()
                for k in outputs:
                    g.assert_fully_written(t[k], k)
                    got = t[k].cpu().numpy()
                    assert (got.view(np.uint8) == plain[k].view(np.uint8)).all(), "%s differs from the unguarded run (fill 0x%02X, run %d)" % (k, fill, run)
            for k in ("ref_color", "ref_depth", "ref_w2c", "cur_color", "cur_depth", "state"):
                assert (t[k].cpu().numpy().view(np.uint8) == plain[k].view(np.uint8)).all(), "%s is an input and was written" % k
    # without the optional outputs, and on a second stream: the same row
    t = _tensors(case, torch)
    _call(case, t, outputs=False)
    assert (_bits(t["row"].cpu().numpy()) == _bits(plain["row"])).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    t2 = _tensors(case, torch)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _call(case, t2)
    side.synchronize()
    for k in outputs:
        assert (t2[k].cpu().numpy().view(np.uint8) == plain[k].view(np.uint8)).all(), k


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------------
BRIGHT = (0.1, 0.03)


@pytest.mark.parametrize("m", [1.0, 2.0])
@pytest.mark.parametrize("depth", [True, False], ids=["depth", "photometric"])
def test_the_joint_aligner_reaches_the_restated_joint_loops_minimum_under_a_brightness_change(m, depth):
    """L = 2, the default schedule, from the reference pose and (a, b) = (0, 0); the current frame's colour is e^0.1 I + 0.03.  Translation
    and rotation error against the true motion must each be at most 2 e_ref + align_restated.POSE_FLOOR, e_ref the restated float64 joint
    loop's error -- the rule of test_the_aligner_reaches_the_restated_loops_minimum.  The accepted loss never rises within a level, the
    pose stays rigid, and the recovered (a, b) agrees with the restated loop's within align_joint_restated.exposure_tolerance: twice the
    distance between the restated loop in float64 and on the float32 mirror, plus a rounding floor -- computed on the CPU."""
    import torch

    from gsaj import align as A
    tol, ref, _ = aj.exposure_tolerance(m, depth, *BRIGHT)
    case = aj.behaviour_case8(m, depth, *BRIGHT)
    true = ar.motion(m)
    al = _aligner()
    assert al.state.shape == (152,) and al.rows.shape[1] == 64 and al.row.shape == (64,)
    al.set_reference(_dev(case, "ref_color"), _dev(case, "ref_depth"), case["ref_w2c"])
    # the aligner's own loop, one call at a time, with the accepted loss kept after every step (device copies; read at the end)
    al._take(al._cur, _dev(case, "cur_color"), _dev(case, "cur_depth"), "align")
    al._reset(al.ref_w2c)
    kept = []
    for l, n in zip((2, 1, 0), al.default_schedule()):
        if l != 2:
            A._relevel(al, l)
        for _ in range(n):
            A._residuals(al, l, depth)
            A._step(al, l)
            kept.append((l, al.state[81].clone()))
    by_hand = al.state.cpu().numpy().copy()
    for l in (2, 1, 0):
        acc = [float(v) for (k, v) in kept if k == l]
        assert all(b <= a for a, b in zip(acc, acc[1:])), "the accepted loss rises within level %d: %s" % (l, acc)
    # align() is that loop
    assert al.align(_dev(case, "cur_color"), _dev(case, "cur_depth")) == [8, 6, 6]
    w2c, overlap, loss, _ = al.result()
    assert (_bits(al.state.cpu().numpy()) == _bits(by_hand)).all(), "align() and its own steps taken one by one differ"
    assert (_bits(w2c) == _bits(al.w2c.cpu().numpy())).all() and overlap == pytest.approx(float(al.overlap)) and 0.5 < overlap <= 1.0
    assert loss == pytest.approx(float(al.lm["accepted_loss"])) and al.loss_terms.shape == (3,)
    assert al.lm["H"].shape == (8, 8) and al.lm["g"].shape == (8,)
    R = w2c[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-4 and (w2c[3] == [0, 0, 0, 1]).all()
    e_dev, e_ref, e_start = ar.pose_error(w2c, true), ar.pose_error(ref["w2c"], true), ar.pose_error(case["w2c"], true)
    got = al.relative_exposure.cpu().numpy().astype(np.float64)
    print("m=%g %s: start %.5f / %.5f   restated %.6f / %.6f   device %.6f / %.6f   (floor %.1e)   (a, b): restated (%.6f, %.6f) device "
          "(%.6f, %.6f) |difference| (%.2e, %.2e) tolerance (%.2e, %.2e)" % (
              (m, "depth" if depth else "photometric") + e_start + e_ref + e_dev + (ar.POSE_FLOOR,) + tuple(ref["exposure"]) + tuple(got)
              + tuple(np.abs(got - ref["exposure"])) + tuple(tol)))
    for k in range(2):
        assert e_dev[k] <= 2 * e_ref[k] + ar.POSE_FLOOR, (e_dev, e_ref)
    assert (np.abs(got - ref["exposure"]) <= tol).all(), (got, ref["exposure"], tol)
    assert torch.equal(al.relative_exposure, al.accepted_exposure)


def test_promote_then_align_is_a_fresh_joint_aligner_given_that_reference():
    import torch
    cam = ar.camera()
    frames = [ar.scene_frame(ar.motion(m), cam) for m in (0.0, 1.0, 2.0)]
    gains = [(0.0, 0.0), (0.1, 0.03), (0.03, 0.05)]   # each frame at its own brightness
    dev = [(torch.from_numpy((np.exp(a) * c.astype(np.float64) + b).astype(F)).to(DEV), torch.from_numpy(d).to(DEV))
           for (c, d), (a, b) in zip(frames, gains)]
    a = _aligner()
    a.set_reference(dev[0][0], dev[0][1], np.eye(4))
    a.align(*dev[1])
    pose1 = a.w2c.clone()
    a.promote()
    a.align(*dev[2])
    b = _aligner()
    b.set_reference(dev[1][0], dev[1][1], pose1)   # a device tensor, as tracker.accepted_w2c is
    b.align(*dev[2])
    assert torch.equal(a.state, b.state) and torch.equal(a.row, b.row), "the promoted reference is not the frame itself"
    e = ar.pose_error(a.result()[0], ar.motion(2.0))
    start = ar.pose_error(ar.motion(1.0), ar.motion(2.0))
    assert e[0] < 0.1 * start[0] and e[1] < 0.1 * start[1], (e, start)
    # (a, b) is relative to the REFERENCE: frame 2 against frame 1 is e^(0.03 - 0.1) and 0.05 - e^(-0.07) 0.03, not frame 2's own
    rel = a.relative_exposure.cpu().numpy()
    want = np.array([0.03 - 0.1, 0.05 - np.exp(-0.07) * 0.03])
    assert np.abs(rel - want).max() < 0.02, (rel, want)
    # exposure_init: the solve started at the answer ends at the same minimum
    c = _aligner()
    c.set_reference(dev[1][0], dev[1][1], pose1)
    c.align(*dev[2], exposure_init=a.relative_exposure)
    assert np.abs(c.relative_exposure.cpu().numpy() - rel).max() < 1e-3


# ---- the hand-off -------------------------------------------------------------------------------------------------------------------------
def test_exposure_for_is_its_formula_on_the_device_and_the_map_tracker_takes_it():
    """(a_r + a, e^a b_r + b) against float64: exp within 2 ulp, one product, one sum -- 4 roundings of values below 1 + |b_r| + |b|.
    The result is a device tensor; GaussNewtonTracker.reset(w2c, exposure=) -- the single tracker's start of a frame, a new start pose
    and exposure in place -- takes it as it is, and so does the state every tracker and window slot is initialised through."""
    import torch

    from gsaj import _gn_state as S
    from gsaj.gauss_newton import GaussNewtonTracker
    al = _aligner()
    rel = (0.1, -0.03)
    al.state[148:150] = torch.tensor(rel, device=DEV)
    ref = torch.tensor([0.2, 0.05], device=DEV)
    got = al.exposure_for(ref)
    assert got.is_cuda and got.shape == (2,) and got.dtype == torch.float32
    want = aj.exposure_for(F([0.2, 0.05]), F(rel))
    assert np.abs(got.cpu().numpy().astype(np.float64) - want).max() <= 4 * ar.EPS * (1 + 0.05 + 0.03)
    assert torch.equal(al.exposure_for((0.2, 0.05)), got), "a pair of numbers or a device tensor"
    tr = GaussNewtonTracker.__new__(GaussNewtonTracker)   # (its reset needs the state, the projection and lambda_init: no map, no context)
    tr.solve_exposure, tr.projection, tr.lm_args = True, torch.eye(4, device=DEV), (1e-3, 4.0, 1e-7, 1e7, 1e-4)
    tr.state = torch.zeros(S.layout("gn8").floats, dtype=torch.float32, device=DEV)
    pose = torch.as_tensor(ar.motion(1.0), dtype=torch.float32, device=DEV)   # (a device tensor, as aligner.w2c is)
    tr.reset(pose, exposure=got)
    assert torch.equal(tr.exposure, got) and torch.equal(tr.accepted_exposure, got) and torch.equal(tr.w2c, pose)
