"""GPU: csrc/sweep.hip (gsaj.motion_stereo) against tests/sweep_restated.py.  The warp is mirrored one fp32 rounding at a time and the
rest is integer arithmetic, so the gradient bytes, pc, C, S and idx16 are compared with array_equal and the depth bit for bit: no
tolerance anywhere.  Shapes chosen for where the kernels can go wrong (1 x 1 and 2 x 2: nothing or almost nothing inside; 65 x 5: one
past a wave's columns; 20 x 70: past one band of 64 rows), every number of hypotheses, both path counts, radii with windows larger than
the image; poses that put the epipole in the image, warp every hypothesis alike, tie every cost, put near hypotheses behind the source
camera, and carry a NaN; the planted sums of tests/test_cpu_motion_stereo.py through the winner stage alone; host, device and padded
inputs, twice and three times on one object, on a side stream; gsaj_grey_u8 against its mirror; and the depth through
seed_from_keyframe."""
import numpy as np
import pytest

import ingest_restated as ir
import sweep_restated as sw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W_RANGE = (0.2, 0.7)
# id -> (W, H, D, paths, r, u, motion, w range)
CASES = {
    "1x1": (1, 1, 16, 8, 0, 0, "sideways", W_RANGE),
    "2x2": (2, 2, 16, 4, 3, 10, "mixed", W_RANGE),
    "65x5-D32": (65, 5, 32, 8, 3, 10, "sideways", W_RANGE),
    "20x70-r7": (20, 70, 16, 4, 7, 0, "mixed", W_RANGE),
    "96x40-sideways": (96, 40, 16, 8, 3, 10, "sideways", W_RANGE),
    "96x40-forward": (96, 40, 16, 8, 3, 10, "forward", W_RANGE),
    "96x40-D64-r0": (96, 40, 64, 4, 0, 10, "mixed", W_RANGE),
    "150x33-D128-r7": (150, 33, 128, 8, 7, 0, "sideways", W_RANGE),
    "150x33-D32-forward": (150, 33, 32, 4, 3, 10, "forward", W_RANGE),
    "rotation-only": (96, 40, 16, 8, 3, 10, "rotation", W_RANGE),
    "identity-u10": (96, 40, 16, 8, 3, 10, "identity", W_RANGE),
    "identity-u0": (96, 40, 32, 4, 3, 0, "identity", W_RANGE),
    "backward": (96, 40, 32, 8, 3, 0, "backward", (0.2, 1.0)),
    "w_min-0": (96, 40, 16, 8, 3, 10, "sideways", (0.0, 0.7)),
    "nan-pose": (65, 5, 64, 8, 3, 0, "nan", W_RANGE),
}
_MEMO = {}


def _case(W, H, motion):
    if motion == "nan":
        c = dict(sw.case(W, H, "sideways"))
        c["src_w2c"] = c["src_w2c"].copy()
        c["src_w2c"][1, 2] = np.nan
        return c
    if motion == "identity":   # both poses the identity: T is the identity exactly, every hypothesis warps alike
        return sw.case(W, H, motion, ref_w2c=np.eye(4))
    return sw.case(W, H, motion)


def _want(key):
    """The restatement of a case, computed once and shared."""
    if key not in _MEMO:
        W, H, D, paths, r, u, motion, (w_min, w_max) = CASES[key]
        c = _case(W, H, motion)
        _MEMO[key] = (c, sw.run(c, w_min, w_max, D=D, paths=paths, r=r, uniqueness=u))
    return _MEMO[key]


def _sweeper(c, D, **kw):
    from gsaj import MotionStereo

    cam = c["cam"]
    return MotionStereo(cam["W"], cam["H"], DEV, cam["fx"], cam["fy"], cam["cx"], cam["cy"], num_hypotheses=D, **kw)


def _sweeper_of(key):
    W, H, D, paths, r, u, motion, wr = CASES[key]
    c, want = _want(key)
    return c, want, wr, _sweeper(c, D, paths=paths, block_radius=r, uniqueness=u)


def _assert_outputs(m, got, want, tag):
    idx16, depth = got
    assert np.array_equal(m.gradient_bytes().cpu().numpy().view(np.uint16).astype(np.int64), want["grad"]), "%s: the gradient bytes differ" % tag
    for name, dev, ref in (("pc", m.pixel_costs().cpu().numpy().astype(np.int64), want["pc"]),
                           ("C", m.cost_volume().cpu().numpy().view(np.uint16).astype(np.int64), want["C"]),
                           ("S", m.sums().cpu().numpy().astype(np.int64), want["S"])):
        bad = dev != ref
        assert not bad.any(), "%s: %s differs at %d entries, first (y, x, d) = %s: got %d want %d" % (
            tag, name, int(bad.sum()), tuple(np.argwhere(bad)[0]), dev[bad][0], ref[bad][0])
    g = idx16.cpu().numpy()
    assert g.dtype == np.int16 and np.array_equal(g, want["idx16"]), "%s: idx16 differs at %d pixels" % (tag, int((g != want["idx16"]).sum()))
    ir.assert_bits_equal(depth.cpu().numpy(), want["depth"], tag + ": depth")


@pytest.mark.parametrize("key", sorted(CASES))
def test_every_stage_equals_the_restatement(key):
    c, want, (w_min, w_max), m = _sweeper_of(key)
    got = m(c["ref"], c["src"], c["ref_w2c"], c["src_w2c"], w_min, w_max)
    _assert_outputs(m, got, want, key)
    idx = want["idx16"]
    motion = CASES[key][6]
    if key in ("1x1", "nan-pose"):
        assert (idx == -16).all()                       # nothing inside
    if key == "identity-u10":   # every sum ties: each far d is a rival, except where the sums are 0 (0 < 0 is no rival: ref and src agree)
        centre = sw.warp(c["cam"], want["T"], want["w"][0])[0]
        assert (want["S"] == want["S"][:, :, :1]).all() and ((idx >= 0) == ((want["S"][:, :, 0] == 0) & centre)).all()
        assert (idx == -16).sum() > 500 and set(np.unique(idx).tolist()) == {-16, 0}
    if key in ("1x1", "nan-pose"):
        assert (want["pc"] == 80).all()
    if key == "identity-u0":
        assert (want["S"] == want["S"][:, :, :1]).all() and set(np.unique(idx).tolist()) == {-16, 0}   # all ties resolve to d = 0
    if key == "rotation-only":
        assert (want["pc"] == want["pc"][:, :, :1]).all()
    if key == "backward":
        T = want["T"]
        assert (T[2, 3] < 0) and not sw.warp(c["cam"], T, want["w"][-1])[0].any() and sw.warp(c["cam"], T, want["w"][0])[0].any()
    if key == "w_min-0":
        assert want["w"][0] == 0 and (idx >= 0).any()
    if motion in ("sideways", "forward", "mixed") and min(CASES[key][:2]) >= 33:
        assert (idx >= 0).mean() > 0.3 and (idx == -16).any()


def test_other_penalties_and_outside_costs_equal_the_restatement():
    c = _want("96x40-sideways")[0]
    for P1, P2, oc in ((0, 1, 0), (8, 32, 240), (1023, 1024, 80)):
        m = _sweeper(c, 16, P1=P1, P2=P2, outside_cost=oc)
        got = m(c["ref"], c["src"], c["ref_w2c"], c["src_w2c"], *W_RANGE)
        _assert_outputs(m, got, sw.run(c, *W_RANGE, P1=P1, P2=P2, outside_cost=oc), "P1=%d P2=%d outside=%d" % (P1, P2, oc))


@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_planted_sums_through_the_winner_stage_alone(D):
    """Ties, d* at both ends, negative numerators that do not divide evenly, rivals exactly at and one below the uniqueness bound, and
    the centre rule on the last column and row: S is written into the workspace and only the winner stage runs."""
    import torch
    from gsaj.motion_stereo import STAGE_WINNER

    cam, rw, sw_, w_min, w_max = sw.planted_cam()
    S = sw.planted_sums(D)
    H, W, _ = S.shape
    T = sw.rel_pose(rw, sw_)
    step, w = sw.hypotheses(w_min, w_max, D)
    dummy = np.zeros((H, W), np.uint8)
    for u in (0, 40):
        m = _sweeper(dict(cam=cam), D, uniqueness=u)
        m.sums().copy_(torch.from_numpy(S.astype(np.int32)))
        idx16, z = m(dummy, dummy, rw, sw_, w_min, w_max, stages=STAGE_WINNER)
        want = sw.winner(S, cam, T, w, u)
        assert np.array_equal(idx16.cpu().numpy(), want), (D, u, int((idx16.cpu().numpy() != want).sum()))
        ir.assert_bits_equal(z.cpu().numpy(), sw.depth(want, w_min, step), "depth D=%d u=%d" % (D, u))
        assert (want == -16).any() and (want == 0).any() and (want == 16 * (D - 1)).any()


def test_padded_device_rows_and_host_arrays_give_the_same_result():
    import torch

    c, want, wr, m = _sweeper_of("96x40-sideways")
    H, W = c["ref"].shape
    wide = np.full((2, H, W + 7), 0x5A, np.uint8)
    wide[0, :, :W], wide[1, :, :W] = c["ref"], c["src"]
    d_wide = torch.as_tensor(wide, device=DEV)
    state = torch.zeros(40, device=DEV)   # a pose state: only its first 16 floats are read
    state[:16] = torch.as_tensor(c["src_w2c"].reshape(16), device=DEV)
    got = m(d_wide[0, :, :W], d_wide[1, :, :W], torch.as_tensor(c["ref_w2c"], device=DEV), state, *wr)
    _assert_outputs(m, got, want, "padded device rows, device poses")
    view = np.zeros((H, W + 3), np.uint8)
    view[:, :W] = c["ref"]
    oi, oz = torch.full((H, W), 7, dtype=torch.int16, device=DEV), torch.full((H, W), -1.0, device=DEV)
    got = m(view[:, :W], torch.as_tensor(c["src"], device=DEV), c["ref_w2c"].astype(np.float64), c["src_w2c"], *wr, out_idx16=oi, out_depth=oz)
    assert got[0].data_ptr() == oi.data_ptr() and got[1].data_ptr() == oz.data_ptr()
    _assert_outputs(m, got, want, "a strided host view, a device image, host poses, caller's outputs")
    from gsaj import _lib

    for bad in (c["ref"].astype(np.int16), c["ref"][:, :-1], torch.as_tensor(c["ref"]), torch.as_tensor(c["ref"], device=DEV).float()):
        with pytest.raises(_lib.GsajError):
            m(bad, c["src"], c["ref_w2c"], c["src_w2c"], *wr)
    with pytest.raises(_lib.GsajError):
        m(c["ref"], c["src"], c["ref_w2c"][:3], c["src_w2c"], *wr)
    with pytest.raises(_lib.GsajError):
        m(c["ref"], c["src"], c["ref_w2c"], c["src_w2c"], 0.5, 0.5)
    with pytest.raises(_lib.GsajError):
        _sweeper(c, 16, block_radius=8)


def test_two_runs_are_bit_identical_and_three_calls_each_give_their_own_result():
    """S is summed into with atomics: integer adds, the same bits in any order, and every call must start from its own zeroes.  The
    second pair is flat (every inside cost 0), so anything left over from the first would show; then the first pair again."""
    c, want, wr, m = _sweeper_of("96x40-forward")
    args = (c["ref"], c["src"], c["ref_w2c"], c["src_w2c"]) + wr
    first = [t.clone() for t in m(*args)]
    first_S = m.sums().clone()
    flat = np.full(c["ref"].shape, 90, np.uint8)
    got_flat = m(flat, flat, c["ref_w2c"], c["src_w2c"], *wr)
    _assert_outputs(m, got_flat, sw.run(dict(c, ref=flat, src=flat), *wr), "the flat pair in between")
    again = m(*args)
    assert all((a.view(-1) == b.view(-1)).all() for a, b in zip(first, again)) and (first_S == m.sums()).all()
    _assert_outputs(m, again, want, "the first pair again")
    import torch

    assert torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


def test_a_result_made_on_a_side_stream_is_correct_after_its_synchronize():
    import torch

    c, want, wr, m = _sweeper_of("150x33-D32-forward")
    dev = [torch.as_tensor(c[k], device=DEV) for k in ("ref", "src", "ref_w2c", "src_w2c")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = m(*dev, *wr)
    side.synchronize()
    _assert_outputs(m, got, want, "side stream")


def test_grey_u8_equals_its_mirror():
    import torch
    from gsaj import grey_u8

    W, H = 67, 35
    rng = np.random.default_rng(4)
    color = (rng.uniform(-0.2, 1.2, (H, W)) + rng.uniform(-0.05, 0.05, (3, H, W))).astype(np.float32)   # greys below 0 and above 1 included
    color[1, 3, 5], color[0, 4, 6], color[2, 5, 7] = np.nan, np.inf, -np.inf
    color[:, 6, 8] = 0.5
    want = sw.grey_u8(color)
    assert want[3, 5] == 0 and want[4, 6] == 255 and want[5, 7] == 0 and want[6, 8] == 128 and (want == 0).sum() > 50 and (want == 255).sum() > 50
    d_color = torch.as_tensor(color, device=DEV)
    got = grey_u8(d_color)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), "%d bytes differ" % int((got.cpu().numpy() != want).sum())
    padded = torch.full((H, W + 5), 0xC3, dtype=torch.uint8, device=DEV)
    assert grey_u8(d_color, out=padded[:, :W]).data_ptr() == padded.data_ptr()
    assert np.array_equal(padded[:, :W].cpu().numpy(), want) and bool((padded[:, W:] == 0xC3).all())
    frames = sw.ar.scene_frame(sw.ref_pose(), sw.ar.camera(96, 40))[0]
    assert np.array_equal(grey_u8(torch.as_tensor(frames, device=DEV)).cpu().numpy(), sw.grey_u8(frames))   # what the scenes are made of


def test_the_sweep_depth_seeds_a_keyframe():
    """Composition: the depth of the 160 x 120 sideways case goes into seed_from_keyframe as it is.  The number of seeds is
    size_t(n_valid (1 / factor)) of the depth's valid count, and every seed's camera-space z is the depth at its source pixel: the
    seeder's xyz is within tests/test_gpu_seed.py's bound (1 fp32 ulp of the largest magnitude involved) of the fp64 back-projection
    per component, and z_c = R[2] . xyz + t_z carries that bound with the factor |R20| + |R21| + |R22|."""
    import torch
    from gsaj import seeding

    import seed_restated as sdr

    c = sw.case(160, 120, "sideways")
    cam = c["cam"]
    m = _sweeper(c, 16)
    idx16, depth = m(c["ref"], c["src"], c["ref_w2c"], c["src_w2c"], *W_RANGE)
    want = sw.run(c, *W_RANGE)
    ir.assert_bits_equal(depth.cpu().numpy(), want["depth"], "depth")
    n_valid = int((want["depth"] > 0).sum())
    assert n_valid == int((want["idx16"] >= 0).sum()) and n_valid > 0.85 * 160 * 120
    factor, seed = 8, 3
    image = torch.as_tensor(sw.ar.scene_frame(sw.ref_pose(), cam)[0], device=DEV)
    w2c = torch.as_tensor(c["ref_w2c"], device=DEV)
    out = seeding.seed_from_keyframe(image, depth, w2c, cam["fx"], cam["fy"], cam["cx"], cam["cy"], factor, 0.01, seed=seed, return_pixels=True)
    xyz, pix = out[0].cpu().numpy().astype(np.float64), out[5].cpu().numpy()
    assert pix.size == int(n_valid * (1.0 / factor)) == xyz.shape[0]
    z_src = want["depth"].reshape(-1)[pix].astype(np.float64)
    assert (z_src > 0).all()
    w32 = c["ref_w2c"].astype(np.float64)
    pw = sdr.backproject(want["depth"], pix, 160, c["ref_w2c"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    mag = np.maximum(np.abs(pw).max(axis=1), np.abs(np.linalg.inv(w32)[:3, 3]).max())
    bound = 2.0 ** -23 * mag
    assert (np.abs(xyz - pw).max(axis=1) <= bound).all()
    z_c = xyz @ w32[2, :3] + w32[2, 3]
    err = np.abs(z_c - z_src)
    print("camera-space z of %d seeds: max error %.3g, max error / bound %.3f" % (pix.size, err.max(), (err / (np.abs(w32[2, :3]).sum() * bound)).max()))
    assert (err <= np.abs(w32[2, :3]).sum() * bound + 2.0 ** -50 * mag).all()
