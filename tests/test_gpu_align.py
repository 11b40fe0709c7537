"""GPU: the frame-to-frame RGB-D alignment (csrc/align.hip, gsaj.RgbdAligner) against tests/align_restated.py.

Per-pixel parity: pix_out / valid_out against the float32 mirror BIT FOR BIT at every non-borderline pixel (every operation of the
kernel is mirrored: +, -, *, /, floorf, fminf / fmaxf, fabsf and comparisons are all exact or correctly rounded in NumPy's float32, so
no quantity needs an ulp bound); the row against the float64 sum of the mirror's terms within align_restated.row_bound; the gates of the
fold; the memory contract under tests/guards.py; and the behaviour of the whole aligner on the analytic scene against the restated
float64 loop.  tests/test_cpu_align.py checks the premises all of this rests on."""

import numpy as np
import pytest

import align_calls
import align_restated as ar
import guards

pytestmark = pytest.mark.gpu
DEV = align_calls.DEV
F = np.float32
_MEMO = {}
_CALLS = align_calls.Calls(joint=False)   # the buffers of a gsaj_rgbd_align call, the call, gsaj_pose_gn_step on its row, RgbdAligner
_tensors, _call, _run, _step, _aligner = _CALLS.tensors, _CALLS.call, _CALLS.run, _CALLS.step, _CALLS.aligner
_bits, _dev = align_calls.bits, align_calls.dev


def _expect(key, make):
    """The mirror of a case, its borderline pixels: computed once, shared, never modified."""
    if key not in _MEMO:
        case = make()
        mir = ar.mirror(case)
        _MEMO[key] = (case, mir, ar.borderline(case))
    return _MEMO[key]


def _compare(case, mir, border, out, tag):
    other = ar.assert_pixels_equal(out["pix"], out["valid"], mir, border, tag)
    worst = ar.assert_row_close(out["row"], mir["terms"], case, border, tag)
    print("%s: n %d, depth gates %d, borderline %d (other side taken: %d), row worst err / bound %.3f" % (
        tag, out["row"][30], out["row"][31], border.sum(), other, worst))


# ---- per-pixel parity and the row -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ar.parity_sizes(), ids=["%dx%d" % s for s in ar.parity_sizes()])
@pytest.mark.parametrize("mode", ar.MODES)
def test_pixels_equal_the_mirror_bit_for_bit_and_the_row_is_their_sum(W, H, mode):
    case, mir, border = _expect((W, H, mode), lambda: ar.parity_case(W, H, mode))
    out, _ = _run(case)
    _compare(case, mir, border, out, "%dx%d %s" % (W, H, mode))
    assert out["row"][30] >= 1 and (mode != "depth" or min(W, H) < 5 or out["row"][31] >= 1)
    if mode == "w0":
        assert out["row"][29] == 0 and (out["row"][31] == mir["gate"].sum() or border.any()), "w_depth = 0: the gates are counted, the term is nothing"


def test_a_frame_of_more_rows_than_one_trip_of_the_folds_load_loop():
    """70 x 260 with depth: 2 x 65 = 130 rows, so row group 0 and 1 of the fold (gn_sum_rows: csrc/gn_state.h) take a second trip of
    the four-deep load loop, and the last trip of every group is a partial one.  The comparisons of the parity test."""
    W, H = ar.LONG_FOLD
    case, mir, border = _expect((W, H, "depth"), lambda: ar.parity_case(W, H, "depth"))
    out, _ = _run(case)
    assert out["rows"].shape == (130, 32)
    _compare(case, mir, border, out, "%dx%d depth" % (W, H))
    assert out["row"][30] >= 1 and out["row"][31] >= 1


@pytest.mark.parametrize("sign", [1, -1])
def test_planted_pixels_on_every_gate(sign):
    """u exactly W - 1 (sign +1) and exactly 0 (sign -1), a reference depth of 0, NaN and +inf in each of the four inputs, a tap on
    either side of the edge ratio, |r| on either side of delta, both terms -- tests/test_cpu_align.py asserts that the mirror shows
    each of them; here the device must show the mirror."""
    case, planted, _ = _MEMO.setdefault(("plant", sign, "raw"), ar.planted_case(sign))
    case, mir, border = _expect(("plant", sign), lambda: case)
    out, _ = _run(case)
    _compare(case, mir, border, out, "planted %+d" % sign)
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


def test_planted_depths_on_either_side_of_min_depth_in_the_current_camera():
    made = ar.planted_near_case()
    case, mir, border = _expect(("near",), lambda: made[0])
    planted = made[1]
    out, _ = _run(case)
    _compare(case, mir, border, out, "planted near")
    (xb, yb), (xa, ya) = planted["zc_below"], planted["zc_above"]
    assert out["valid"][yb, xb] == 0 and out["valid"][ya, xa] & 1


# ---- the gates of the fold ----------------------------------------------------------------------------------------------------------------
def test_a_frame_without_a_valid_pixel_gives_no_step_and_a_loss_that_every_proposal_loses_to():
    import torch
    good = ar.parity_case(80, 60, "depth")
    empty = dict(good, ref_depth=np.zeros((60, 80), F))
    proj = torch.eye(4, device=DEV)
    # a first call: accepted as the baseline (there is no other), and H = g = 0 moves nothing
    t = _tensors(empty, torch)
    t["state"][80] = ar.LM["lambda_init"]
    before = t["state"].cpu().numpy()
    _call(empty, t)
    row = t["row"].cpu().numpy()
    assert not row[:27].any() and np.isposinf(row[27:30]).all() and row[30] == 0 and row[31] == 0, row
    assert not t["valid"].cpu().numpy().any() and not t["pix"].cpu().numpy().any()
    _step(t, proj)
    after = t["state"].cpu().numpy()
    assert (_bits(after[0:16]) == _bits(before[0:16])).all() and (_bits(after[88:104]) == _bits(before[0:16])).all(), "the pose moved"
    assert not after[70:76].any() and after[83] == 1 and after[84] == 0
    # a later call: a real step first, then the empty frame -- rejected, the accepted pose and loss stay bit for bit
    t = _tensors(good, torch)
    t["state"][80] = ar.LM["lambda_init"]
    _call(good, t)
    _step(t, proj)
    held = t["state"].cpu().numpy()
    assert held[83] == 1 and np.isfinite(held[81]) and held[70:76].any(), "the first step accepts and proposes"
    t["ref_depth"].zero_()
    _call(good, t)
    assert np.isposinf(t["row"].cpu().numpy()[27])
    _step(t, proj)
    after = t["state"].cpu().numpy()
    assert after[84] == 1 and after[83] == 1, "rejected"
    assert (_bits(after[88:104]) == _bits(held[88:104])).all() and _bits(after[81:82]) == _bits(held[81:82]), "the accepted pose or loss changed"
    assert after[80] > held[80], "more damping after a rejection"


def test_min_overlap_just_above_and_just_below_the_valid_share():
    case, mir, border = _expect((80, 60, "depth"), lambda: ar.parity_case(80, 60, "depth"))
    out, _ = _run(case)
    n, WH = float(out["row"][30]), 80 * 60
    assert n == mir["valid"].sum() or border.any()
    below, _ = _run(dict(case, min_overlap=(n - 0.5) / WH))
    assert (_bits(below["row"]) == _bits(out["row"])).all(), "n >= ceil(min_overlap W H): the row is the ungated one"
    above, _ = _run(dict(case, min_overlap=(n + 0.5) / WH))
    assert not above["row"][:27].any() and np.isposinf(above["row"][27:30]).all() and above["row"][30] == n and above["row"][31] == out["row"][31]
    exact, _ = _run(dict(case, min_overlap=1.0))
    assert np.isposinf(exact["row"][27]), "not every pixel is valid"


def test_a_nonzero_skip_word_leaves_the_row_and_the_scratch_untouched():
    import torch
    case, _, _ = _expect((33, 17, "depth"), lambda: ar.parity_case(33, 17, "depth"))
    t = _tensors(case, torch)
    for k in ("rows", "row", "pix"):
        t[k].fill_(-7.0)
    t["valid"].fill_(9)
    state = t["state"].clone()
    skip = torch.tensor([3], dtype=torch.int32, device=DEV)
    _call(case, t, skip=skip)
    assert all(bool((t[k] == -7.0).all()) for k in ("rows", "row", "pix")) and bool((t["valid"] == 9).all())
    assert torch.equal(t["state"], state), "gsaj_rgbd_align only reads the state"
    skip.zero_()
    _call(case, t, skip=skip)
    assert not bool((t["row"] == -7.0).any()) and not bool((t["rows"] == -7.0).any())


# ---- the memory contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,mode", [(97, 61, "depth"), (2, 2, "photo"), (65, 4, "depth")])
def test_memory_contract_bands_poisoned_scratch_same_bits_on_any_stream(monkeypatch, W, H, mode):
    import torch
    case, _, _ = _expect((W, H, mode), lambda: ar.parity_case(W, H, mode))
    plain, _ = _run(case)
    for fill in guards.FILLS:
        with guards.guarded(monkeypatch, fill) as g:
            t = _tensors(case, torch)
            assert len(g.allocations) == 10 and g.payload_untouched(t["rows"]), "rows starts poisoned"
            for run in range(2):
                g.refill(t["rows"])
                for k in ("row", "pix", "valid"):
                    g.refill(t[k])
                _call(case, t)
                torch.cuda.synchronize()
                g.check()
                for k in ("rows", "row", "pix", "valid"):
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
    for k in ("rows", "row", "pix", "valid"):
        assert (t2[k].cpu().numpy().view(np.uint8) == plain[k].view(np.uint8)).all(), k


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------------
def _restated(m, depth):
    key = ("loop", m, depth)
    if key not in _MEMO:
        case = ar.behaviour_case(m, depth)
        _MEMO[key] = (case, ar.align_loop(case, 2))
    return _MEMO[key]


@pytest.mark.parametrize("m", [1.0, 2.0])
@pytest.mark.parametrize("depth", [True, False], ids=["depth", "photometric"])
def test_the_aligner_reaches_the_restated_loops_minimum(m, depth):
    """L = 2, the default schedule, from the reference pose.  Translation and rotation error against the true motion must each be at most
    2 e_ref + align_restated.POSE_FLOOR, e_ref the restated float64 loop's error for the same start and schedule (the two loops differ by
    rounding only and may take one accept / reject decision differently; they must reach the same minimum).  The accepted loss never rises
    within a level and the pose stays rigid."""
    import torch

    from gsaj import align as A
    case, ref = _restated(m, depth)
    true = ar.motion(m)
    al = _aligner()
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
    assert loss == pytest.approx(float(al.lm["accepted_loss"])) and al.loss_terms.shape == (3,) and al.lm["H"].shape == (6, 6)
    R = w2c[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-4 and (w2c[3] == [0, 0, 0, 1]).all()
    e_dev, e_ref, e_start = ar.pose_error(w2c, true), ar.pose_error(ref["w2c"], true), ar.pose_error(case["w2c"], true)
    print("m=%g %s: start %.5f / %.5f   restated %.6f / %.6f   device %.6f / %.6f   (floor %.1e)" % (
        (m, "depth" if depth else "photometric") + e_start + e_ref + e_dev + (ar.POSE_FLOOR,)))
    for k in range(2):
        assert e_dev[k] <= 2 * e_ref[k] + ar.POSE_FLOOR, (e_dev, e_ref)


def test_promote_then_align_is_a_fresh_aligner_given_that_reference():
    cam = ar.camera()
    frames = [ar.scene_frame(ar.motion(m), cam) for m in (0.0, 1.0, 2.0)]
    import torch
    dev = [(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV)) for c, d in frames]
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
    start = ar.pose_error(np.eye(4), ar.motion(2.0))
    assert e[0] < 0.1 * start[0] and e[1] < 0.1 * start[1], (e, start)   # (well below the start, as tests/test_cpu_align.py asks of one alignment)
    c = _aligner()
    c.set_reference(dev[0][0], dev[0][1], np.eye(4))
    c.align(*dev[1])
    other = torch.as_tensor(ar.motion(1.0), dtype=torch.float32, device=DEV)
    c.promote(other)
    assert torch.equal(c.ref_w2c.view(4, 4), other), "promote(w2c) takes the refined pose"
    with pytest.raises(Exception, match="there is no CPU path"):
        c.align(dev[2][0].cpu(), dev[2][1].cpu())
