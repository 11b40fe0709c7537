"""CPU: the coarse-to-fine path without a GPU -- the restated pyramid and relevel (tests/pyramid_restated.py) and their canaries: every
mutant must be rejected by the comparators the GPU tests use; the new C-ABI symbols, their argument errors and the packed layout;
the level cameras against a hand computation; the host logic of ImagePyramid and PyramidGaussNewtonTracker with the device work
replaced; and the premises of the GPU behaviour tests on the restated loop."""
import ctypes
import math
import re

import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import pyramid_restated as pr
from gsaj import synthetic as syn

F = np.float32
LM = dict(nu=4.0, lambda_min=1e-7, lambda_max=1e7, converged_threshold=1e-4)


# ---- the canaries ---------------------------------------------------------------------------------------------------------------------
def test_the_restated_pyramid_gives_the_hand_computed_depth_at_every_planted_position():
    color, depth, mask = pr.planted()
    lv = pr.pyramid(color, depth, mask, 3, pr.PLANTED_RATIO)
    assert [l["color"].shape for l in lv] == [(3, 61, 81), (3, 30, 40), (3, 15, 20)], "level 2 drops level 1's odd column and row"
    for name, positions in pr.planted_positions().items():
        assert len(positions) == 3 and positions[0][0] % 2 == 0 and positions[1][0] % 2 == 1 and positions[2][0] % 16 in (0, 15)
        for (x1, y1) in positions:
            assert lv[0]["depth"][y1, x1].view(np.uint32) == F(pr.DEPTH_EXPECTED[name]).view(np.uint32), (name, x1, y1)
    pr.assert_pyramid_equal(pr.pyramid(color, depth, mask, 3, pr.PLANTED_RATIO), lv, "self")
    # colour is the stated order of additions, not another one
    c = color[:, :2, :2].astype(F)
    assert lv[0]["color"][0, 0, 0] == F(0.25) * F(F(c[0, 0, 0] + c[0, 0, 1]) + F(c[0, 1, 0] + c[0, 1, 1]))


@pytest.mark.parametrize("mutant", pr.PYRAMID_MUTANTS)
def test_every_pyramid_mutant_is_rejected_by_the_bit_comparator(mutant):
    color, depth, mask = pr.planted()
    want = pr.pyramid(color, depth, mask, 3, pr.PLANTED_RATIO)
    with pytest.raises(AssertionError, match="level"):
        pr.assert_pyramid_equal(pr.pyramid(color, depth, mask, 3, pr.PLANTED_RATIO, mutant=mutant), want, mutant)


def _stepped_state(joint, history):
    """A restated state after the given losses, as tests/test_gpu_pyramid.py steps the device's."""
    rng = np.random.default_rng(11)
    w2c0 = gn.se3_exp([0.1, -0.2, 0.05, 0.02, -0.01, 0.03])
    st = g8.lm8_new_state(w2c0, 1e-3, exposure=(0.1, -0.02)) if joint else gn.lm_new_state(w2c0, 1e-3)
    n = 8 if joint else 6
    A = rng.normal(size=(50, n))
    for loss in history:
        (g8.lm8_step if joint else gn.lm_step)(st, (A.T @ A).astype(F), (rng.normal(size=n) * 0.05).astype(F), loss, *LM.values())
    return st


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_every_relevel_mutant_is_rejected_by_the_state_comparator(joint):
    import copy

    pack, close = (g8.pack_state8, g8.assert_lm8_state_close) if joint else (gn.pack_state, gn.assert_lm_state_close)
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=160, H=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    old = np.asarray(cam["projmatrix_raw"], np.float64).reshape(4, 4)
    new = old.copy()
    new[0, 0] *= 1.0125   # (a level whose width was no multiple of 2: tanfovx differs)
    base = _stepped_state(joint, (1.0, 1.5))   # accept, then reject: a proposal is pending
    assert base["has"] and np.abs(base["w2c"] - base["acc_w2c"]).max() > 1e-4 and base["acc_loss"] == 1.0
    good, proj = pr.relevel(copy.deepcopy(base), old, new, 1e-3)
    assert proj is new and not good["has"] and good["acc_loss"] == 0.0 and np.array_equal(good["w2c"], base["acc_w2c"])
    assert (good["accepted"], good["rejected"]) == (1, 1), "the counters are kept"
    close(pack(good, proj), good, new, "self")
    pr.assert_relevelled(pack(good, proj), "self")
    for mutant in pr.RELEVEL_MUTANTS:
        bad, bproj = pr.relevel(copy.deepcopy(base), old, new, 1e-3, mutant=mutant)
        with pytest.raises(AssertionError):
            close(pack(bad, bproj), good, new, mutant)
    # a non-zero skip word changes nothing
    kept, kproj = pr.relevel(copy.deepcopy(base), old, new, 1e-3, skip=1)
    assert kproj is old and kept["has"] and np.array_equal(kept["w2c"], base["w2c"]) and kept["lam"] == base["lam"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gsaj_pyramid_bytes", "gsaj_pyramid_level", "gsaj_pyramid_build", "gsaj_pose_gn_relevel")


def test_header_declares_the_new_symbols_and_the_binding_matches_their_arity():
    from gsaj import _lib

    with open(_lib.HEADER) as fh:
        text = fh.read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\);" % name, text, re.S)
        assert m, "%s is not declared in include/gsaj.h" % name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
    assert re.search(r"#define\s+GSAJ_PYRAMID_MAX_LEVELS\s+4\b", text)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)


def _level(lib, W, H, L, has_depth, has_mask, l):
    wl, hl = ctypes.c_int(-1), ctypes.c_int(-1)
    off = [ctypes.c_size_t(0) for _ in range(3)]
    rc = lib.gsaj_pyramid_level(W, H, L, has_depth, has_mask, l, ctypes.byref(wl), ctypes.byref(hl), *[ctypes.byref(o) for o in off])
    return rc, wl.value, hl.value, [o.value for o in off]


@pytest.mark.parametrize("W,H,L", [(2, 2, 1), (7, 5, 1), (33, 17, 4), (67, 35, 4), (97, 61, 3), (160, 120, 3), (640, 480, 4)])
@pytest.mark.parametrize("has_depth,has_mask", [(1, 1), (0, 0), (1, 0), (0, 1)])
def test_level_planes_are_aligned_disjoint_and_inside_the_allocation(W, H, L, has_depth, has_mask):
    from gsaj import _lib

    lib = _lib.load()
    total = lib.gsaj_pyramid_bytes(W, H, L, has_depth, has_mask)
    none = ctypes.c_size_t(-1).value
    spans = []
    for l in range(1, L + 1):
        rc, wl, hl, (co, do, mo) = _level(lib, W, H, L, has_depth, has_mask, l)
        assert rc == 0 and (wl, hl) == (W >> l, H >> l)
        spans.append((co, 12 * wl * hl))
        assert (do == none) == (not has_depth) and (mo == none) == (not has_mask)
        if has_depth:
            spans.append((do, 4 * wl * hl))
        if has_mask:
            spans.append((mo, wl * hl))
    assert all(off % 256 == 0 for off, _ in spans)
    spans.sort()
    assert spans[0][0] == 0 and all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= total
    assert total % 256 == 0 and total == sum((n + 255) // 256 * 256 for _, n in spans), "nothing but the planes and their padding"


def test_argument_errors_are_returned_without_a_launch():
    from gsaj import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    build = lambda **kw: lib.gsaj_pyramid_build(*dict(dict(W=64, H=48, levels=2, color=p, depth=p, mask=p, ratio=0.1, pyramid=p, stream=None), **kw).values())  # noqa: E731
    for kw in (dict(levels=0), dict(levels=5), dict(levels=-1), dict(W=3, levels=2), dict(H=7, levels=3), dict(W=0), dict(color=None), dict(pyramid=None),
               dict(ratio=-0.1), dict(ratio=float("inf")), dict(ratio=float("nan"))):
        assert build(**kw) == -1 and "gsaj_pyramid_build" in lib.gsaj_last_error().decode(), kw
    assert lib.gsaj_pyramid_bytes(64, 48, 0, 1, 1) == 0 and lib.gsaj_pyramid_bytes(64, 48, 5, 1, 1) == 0 and lib.gsaj_pyramid_bytes(3, 48, 2, 1, 1) == 0
    assert lib.gsaj_pyramid_bytes(4, 4, 2, 1, 1) == 2 * 3 * 256 and lib.gsaj_pyramid_bytes(4, 4, 2, 0, 0) == 2 * 256 and lib.gsaj_pyramid_bytes(64, 48, 4, 0, 0) > 0
    for args in ((64, 48, 2, 1, 1, 0), (64, 48, 2, 1, 1, 3), (64, 48, 5, 1, 1, 1), (3, 48, 2, 1, 1, 1)):
        assert lib.gsaj_pyramid_level(*args, None, None, None, None, None) == -1 and "gsaj_pyramid_level" in lib.gsaj_last_error().decode(), args
    assert lib.gsaj_pyramid_level(64, 48, 2, 1, 1, 2, None, None, None, None, None) == 0, "every output may be NULL"
    relevel = lambda **kw: lib.gsaj_pose_gn_relevel(*dict(dict(state=p, n=136, proj=p, lam=1e-3, skip=None, stream=None), **kw).values())  # noqa: E731
    for kw in (dict(n=80), dict(n=0), dict(n=137), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(state=None), dict(proj=None)):
        assert relevel(**kw) == -1 and "gsaj_pose_gn_relevel" in lib.gsaj_last_error().decode(), kw
    assert relevel(n=152, lam=0.0) == -1


# ---- the level cameras ------------------------------------------------------------------------------------------------------------
def test_level_camera_against_a_hand_computation():
    from gsaj.pyramid import level_camera

    # 160 x 120, fx = fy = 140, principal point at the image centre (79.5, 59.5), level 2: 40 x 30
    wl, hl, proj, tx, ty = level_camera(160, 120, 2, 140.0, 140.0, 79.5, 59.5, 0.01, 100.0)
    assert (wl, hl) == (40, 30) and tx == pytest.approx(40 / 70.0) and ty == pytest.approx(30 / 70.0)
    assert tx == pytest.approx(160 / 280.0), "a multiple of 4: the field of view is the frame's"
    P = proj.numpy().T   # (the matrix comes transposed, as the trackers take it)
    # fx_2 = 35, cx_2 = 79.5 / 4 = 19.875, cy_2 = 59.5 / 4 = 14.875
    np.testing.assert_allclose([P[0, 0], P[1, 1], P[0, 2], P[1, 2]], [2 * 35.0 / 40, 2 * 35.0 / 30, (2 * 19.875 - 40) / 40, (2 * 14.875 - 30) / 30], rtol=1e-6)
    np.testing.assert_allclose([P[3, 2], P[2, 2], P[2, 3]], [1.0, 100.0 / 99.99, -1.0 / 99.99], rtol=1e-6)
    # level 0 is the frame's own camera
    w0, h0, proj0, tx0, ty0 = level_camera(160, 120, 0, 140.0, 140.0, 79.5, 59.5, 0.01, 100.0)
    cam = syn.make_camera(np.eye(4), W=160, H=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    np.testing.assert_allclose(proj0.numpy(), cam["projmatrix_raw"].reshape(4, 4), rtol=1e-6, atol=1e-7)
    assert (w0, h0, tx0, ty0) == (160, 120, cam["tanfovx"], cam["tanfovy"])
    # 97 x 61 (odd), fx = 90, fy = 80, principal point (47.2, 30.9), level 3: 12 x 7 -- 96 x 56 of the frame: a crop
    wl, hl, proj, tx, ty = level_camera(97, 61, 3, 90.0, 80.0, 47.2, 30.9, 0.01, 100.0)
    assert (wl, hl) == (12, 7)
    assert tx == pytest.approx(12 / (2 * 11.25)) and ty == pytest.approx(7 / (2 * 10.0))
    assert tx != pytest.approx(97 / 180.0) and ty != pytest.approx(61 / 160.0), "the crop narrows the field of view: not to be 'fixed'"
    P = proj.numpy().T
    cx3, cy3 = 47.2 / 8, 30.9 / 8
    np.testing.assert_allclose([P[0, 0], P[1, 1], P[0, 2], P[1, 2]], [2 * 11.25 / 12, 2 * 10.0 / 7, (2 * cx3 - 12) / 12, (2 * cy3 - 7) / 7], rtol=1e-6)
    # the same camera point lands where the box filter puts it: pixel index u of the frame is index (u + 0.5) / 8 - 0.5 of level 3
    # (ndc -> pixel index as the rasteriser maps it, csrc/gsaj_common.h ndc2pix: ((ndc + 1) S - 1) / 2)
    x, z = 0.3, 2.0
    P0 = level_camera(97, 61, 0, 90.0, 80.0, 47.2, 30.9, 0.01, 100.0)[2].numpy().T
    u0 = (((P0[0, 0] * x + P0[0, 2] * z) / z + 1.0) * 97 - 1.0) / 2
    u3 = (((P[0, 0] * x + P[0, 2] * z) / z + 1.0) * 12 - 1.0) / 2
    assert u0 == pytest.approx(90.0 * x / z + 47.2 - 0.5, abs=1e-4) and u3 == pytest.approx((u0 + 0.5) / 8 - 0.5, abs=1e-5)


# ---- host logic with the device work replaced ---------------------------------------------------------------------------------------
def test_image_pyramid_views_and_host_checks(monkeypatch):
    import torch
    import gsaj.pyramid as Pm
    from gsaj import _lib

    pyr = Pm.ImagePyramid(97, 61, 3, "cpu", has_depth=True, has_mask=True)
    assert pyr.buf.numel() == pyr.lib.gsaj_pyramid_bytes(97, 61, 3, 1, 1)
    assert [pyr.size(l) for l in (1, 2, 3)] == [(48, 30), (24, 15), (12, 7)]
    pyr.buf.zero_()
    for l in (1, 2, 3):
        w, h = pyr.size(l)
        assert tuple(pyr.color(l).shape) == (3, h, w) and tuple(pyr.depth(l).shape) == (h, w) and tuple(pyr.mask(l).shape) == (1, h, w)
        assert pyr.color(l).is_contiguous() and pyr.color(l).dtype == torch.float32 and pyr.mask(l).dtype == torch.uint8
        pyr.color(l).fill_(float(l))    # views of the one allocation, disjoint
        pyr.depth(l).fill_(10.0 + l)
        pyr.mask(l).fill_(l)
    for l in (1, 2, 3):
        assert bool((pyr.color(l) == float(l)).all()) and bool((pyr.depth(l) == 10.0 + l).all()) and bool((pyr.mask(l) == l).all())
    for l in (0, 4):
        with pytest.raises(_lib.GsajError, match="level %d is not one of 1..3" % l):
            pyr.color(l)
    with pytest.raises(_lib.GsajError, match="HIP device"):
        pyr.build(torch.zeros(3, 61, 97), torch.zeros(61, 97), torch.zeros(61, 97, dtype=torch.uint8))
    for bad in (dict(levels=0), dict(levels=5), dict(W=7, levels=3)):
        with pytest.raises(_lib.GsajError, match="levels must be 1..4"):
            Pm.ImagePyramid(**dict(dict(W=97, H=61, levels=3, device="cpu"), **bad))
    with pytest.raises(_lib.GsajError, match="made without a mask"):
        Pm.ImagePyramid(16, 16, 1, "cpu").mask(1)
    # build(): the planes it is given must be the planes it was made for (checked before the device is touched)
    calls = []
    monkeypatch.setattr(Pm, "_build", lambda *a: calls.append(a))
    pyr.dev = torch.device("cuda:0")   # (only to pass the device check: nothing is launched)
    c, d, m = torch.zeros(3, 61, 97), torch.zeros(61, 97), torch.zeros(61, 97, dtype=torch.uint8)
    pyr.build(c, d, m, depth_edge_ratio=0.2)
    assert len(calls) == 1 and calls[0][4] == 0.2
    for args, text in (((c, None, m), "depth must be given"), ((c, d, None), "mask must be given"), ((c, d.double(), m), "depth must be a contiguous"),
                       ((c[:, :, :96], d, m), "color must be a contiguous"), ((c, d, m[:60]), "mask must be a contiguous")):
        with pytest.raises(_lib.GsajError, match=text):
            pyr.build(*args)
    assert len(calls) == 1


class _FakeContext:
    def __init__(self, W, H):
        self.W, self.H, self.capacity, self.fail = W, H, 0, None

    def status(self):
        from gsaj import _lib
        if self.fail:
            msg, self.fail = self.fail, None
            raise _lib.GsajError(msg)


def _fake_level_tracker(pt, W, H, projection, tanfov, w2c):
    """What _level_tracker builds, without a device: GaussNewtonTracker's host attributes."""
    import torch
    from gsaj.gauss_newton import _O, _O8, GaussNewtonTracker

    t = GaussNewtonTracker.__new__(GaussNewtonTracker)
    t.dev, t.solve_exposure = torch.device("cpu"), bool(pt.kw.get("solve_exposure", False))
    t._o = _O8 if t.solve_exposure else _O
    t.state = torch.zeros(152 if t.solve_exposure else 136)
    t.projection = torch.as_tensor(np.asarray(projection), dtype=torch.float32).reshape(4, 4).contiguous()
    t.tanfov, t.lm_args = tanfov, (pt.lambda_init, 4.0, 1e-7, 1e7, 1e-4)
    t.ctx, t._abort_ptr = _FakeContext(W, H), 1000 + W
    t.gt_color = t.gt_depth = t.grad_mask = t._grad_op = None
    t.iterations = 0
    t.reset(w2c)
    return t


def _host_tracker(monkeypatch, W=160, H=120, levels=2, **kw):
    import torch
    import gsaj.gauss_newton as G
    import gsaj.pyramid as Pm

    log = []
    monkeypatch.setattr(G, "_level_tracker", _fake_level_tracker)
    monkeypatch.setattr(G, "_relevel", lambda pt, level, skip: log.append(("relevel", level, skip)))
    monkeypatch.setattr(G, "_level_iteration", lambda t, sync: (log.append(("iteration", t.ctx.W, sync)), setattr(t.ctx, "capacity", 1)))
    monkeypatch.setattr(Pm, "_build", lambda pyr, c, d, m, r: log.append(("build", m is not None, r)))
    monkeypatch.setattr(Pm.ImagePyramid, "build", lambda self, c, d=None, m=None, depth_edge_ratio=0.1: Pm._build(self, c, d, m, depth_edge_ratio))
    cam = syn.make_camera(np.eye(4), W=W, H=H, fx=140.0, fy=140.0, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    w2c = gn.se3_exp([0.01, 0.02, 0.03, 0.0, 0.02, 0.0])
    pt = G.PyramidGaussNewtonTracker.__new__(G.PyramidGaussNewtonTracker)
    pt._init_host(10, W, H, 16, "cpu", w2c, cam["projmatrix_raw"].reshape(4, 4), (cam["tanfovx"], cam["tanfovy"]), torch.zeros(3), torch.zeros(10, 3),
                  torch.zeros(10, 1), levels, (140.0, 140.0, W / 2 - 0.5, H / 2 - 0.5, 0.01, 100.0), 0.1, kw)
    return pt, log, w2c


@pytest.mark.parametrize("solve_exposure", [False, True])
def test_tracker_levels_share_one_state_and_start_at_the_coarsest_camera(monkeypatch, solve_exposure):
    import torch
    from gsaj.pyramid import level_camera

    # 166 x 126: no multiple of 4, so the coarse levels are crops and their projection matrices differ from the frame's
    pt, log, w2c = _host_tracker(monkeypatch, W=166, H=126, solve_exposure=solve_exposure)
    assert [(t.ctx.W, t.ctx.H) for t in pt.trackers] == [(166, 126), (83, 63), (41, 31)] and pt.levels == 2
    assert all(t.state is pt.state for t in pt.trackers) and pt.state.numel() == (152 if solve_exposure else 136)
    for l in (1, 2):
        _, _, proj, tx, ty = level_camera(166, 126, l, 140.0, 140.0, 82.5, 62.5)
        assert torch.equal(pt.trackers[l].projection, proj) and pt.trackers[l].tanfov == (tx, ty)
    # the state starts at the coarsest level: its full projection is W2C^T times THAT level's matrix
    w = pt.state[0:16].view(4, 4)
    assert torch.allclose(pt.state[51:67].view(4, 4), w.t() @ pt.trackers[2].projection) and pt._at == 2
    assert not torch.allclose(pt.state[51:67].view(4, 4), w.t() @ pt.trackers[0].projection)
    # (where the frame is a multiple of 2^l a level is the frame scaled: the same normalised camera)
    even, _, _ = _host_tracker(monkeypatch, solve_exposure=solve_exposure)
    assert torch.allclose(even.trackers[2].projection, even.trackers[0].projection) and even.trackers[2].tanfov == pytest.approx(even.trackers[0].tanfov)
    assert torch.equal(pt.accepted_w2c, pt.w2c) and tuple(pt.lm["H"].shape) == ((8, 8) if solve_exposure else (6, 6))
    assert pt.accepted_exposure.data_ptr() == pt.state.data_ptr() + 4 * (148 if solve_exposure else 33)


def test_tracker_refuses_a_level_smaller_than_a_tile_and_bad_arguments(monkeypatch):
    from gsaj import _lib
    import gsaj

    with pytest.raises(_lib.GsajError, match=r"level 3 of a 160x120 frame is 20x15, smaller than one 16x16 tile"):
        _host_tracker(monkeypatch, levels=3)
    with pytest.raises(_lib.GsajError, match=r"level 2 of a 97x61 frame is 24x15"):
        _host_tracker(monkeypatch, W=97, H=61, levels=2)
    assert _host_tracker(monkeypatch, W=97, H=61, levels=1)[0].trackers[1].ctx.W == 48
    with pytest.raises(_lib.GsajError, match="levels must be 0..4"):
        _host_tracker(monkeypatch, levels=5)
    import torch
    z = torch.zeros(3)
    with pytest.raises(_lib.GsajError, match="HIP device"):
        gsaj.PyramidGaussNewtonTracker(10, 32, 32, 16, "cpu", np.eye(4), np.eye(4), 0.5, 0.5, z, torch.zeros(10, 3), torch.zeros(10, 1), levels=1)
    pt, _, _ = _host_tracker(monkeypatch)
    with pytest.raises(_lib.GsajError, match=r"set_frame\(\) first"):
        pt.iterate((1, 1, 1))


def test_tracker_schedule_relevels_and_reports_an_aborted_level(monkeypatch):
    import torch
    from gsaj import _lib

    pt, log, w2c = _host_tracker(monkeypatch)
    c, d = torch.rand(3, 120, 160), torch.rand(120, 160)
    pt.set_frame(c, d, w2c=w2c)
    assert log == [("build", False, 0.1)] and pt.pyramid.has_depth and not pt.pyramid.has_mask
    for l in (1, 2):   # the coarse levels read the pyramid's planes in place
        assert pt.trackers[l].gt_color.data_ptr() == pt.pyramid.color(l).data_ptr() and pt.trackers[l].gt_depth.data_ptr() == pt.pyramid.depth(l).data_ptr()
        assert pt.trackers[l].grad_mask is None
    for bad in ((1, 1), (1, 1, 1, 1), (1, -1, 1)):
        with pytest.raises(_lib.GsajError, match="schedule must hold 3 non-negative counts"):
            pt.iterate(bad)
    del log[:]
    assert pt.iterate((2, 1, 2)) == [2, 1, 2] and pt.iterations == 5 and pt._at == 0
    assert log == [("iteration", 40, True), ("iteration", 40, False), ("relevel", 1, 1040), ("iteration", 80, True), ("relevel", 0, 1080),
                   ("iteration", 160, True), ("iteration", 160, False)], "the first iteration of a level sizes its arena; the skip word is the level's just finished"
    # a new frame without a new pose: back to the coarsest level on the device; a level with no iterations is passed over
    del log[:]
    pt.set_frame(c, d)
    assert pt.iterate((1, 0, 1)) == [1, 0, 1]
    assert log == [("build", False, 0.1), ("relevel", 2, None), ("iteration", 40, False), ("relevel", 0, 1040), ("iteration", 160, False)]
    # check_every: a level is left once the device reports convergence
    pt.state[77] = 1.0
    assert pt.iterate((6, 6, 6), check_every=2) == [2, 2, 2]
    pt.state[77] = 0.0
    assert pt.iterate((3, 0, 0), check_every=2) == [3, 0, 0]
    # an aborted level is reported after the loop, the state is what it was before the call, its arena is re-sized next time
    before, at = pt.state.clone(), pt._at
    pt.trackers[1].ctx.fail = "asynchronous forward aborted"
    monkeypatch.setattr("gsaj.gauss_newton._level_iteration", lambda t, sync: t.state.__setitem__(80, 5.0))
    with pytest.raises(_lib.GsajError, match="level 1: asynchronous forward aborted"):
        pt.iterate((1, 1, 1))
    assert torch.equal(pt.state, before) and pt._at == at and pt.trackers[1].ctx.capacity == 0 and pt.trackers[2].ctx.capacity == 1


def test_tracker_masks_are_for_every_frame_or_for_none(monkeypatch):
    import torch
    from gsaj import _lib

    pt, log, w2c = _host_tracker(monkeypatch)
    c, d = torch.rand(3, 120, 160), torch.rand(120, 160)
    m = (torch.rand(1, 120, 160) < 0.3).to(torch.uint8)
    pt.set_frame(c, d, grad_mask=m, w2c=w2c)
    assert log == [("build", True, 0.1)] and pt.pyramid.has_mask
    for l in (1, 2):   # a given mask is reduced with the images: the coarse levels read the pyramid's
        assert pt.trackers[l].grad_mask.data_ptr() == pt.pyramid.mask(l).data_ptr() and pt.trackers[l].grad_mask.numel() == (160 >> l) * (120 >> l)
    with pytest.raises(_lib.GsajError, match="for every frame of a tracker or for none"):
        pt.set_frame(c, d)
    with pytest.raises(_lib.GsajError, match="for every frame of a tracker or for none"):
        pt.set_frame(c, grad_mask=m)
    pt2, log2, _ = _host_tracker(monkeypatch)
    pt2.set_frame(c, d, w2c=w2c)
    with pytest.raises(_lib.GsajError, match="for every frame of a tracker or for none"):
        pt2.set_frame(c, d, grad_mask=m)
    mono, _, _ = _host_tracker(monkeypatch, monocular=True)
    mono.set_frame(c, w2c=w2c)
    assert not mono.pyramid.has_depth and all(t.gt_depth is None for t in mono.trackers)


def test_levels_0_is_the_single_tracker_on_the_host_too(monkeypatch):
    import torch

    pt, log, w2c = _host_tracker(monkeypatch, levels=0)
    assert len(pt.trackers) == 1 and pt._at == 0 and pt.pyramid is None
    calls = []
    monkeypatch.setattr(type(pt.trackers[0]), "iterate", lambda self, n, check_every=0: calls.append((n, check_every)) or n)
    pt.set_frame(torch.rand(3, 120, 160), torch.rand(120, 160), w2c=w2c)
    assert pt.iterate([4], check_every=2) == [4] and pt.iterate(3) == [3] and calls == [(4, 2), (3, 0)] and not log and pt.pyramid is None


# ---- premises of the GPU behaviour tests, on the restated loop -------------------------------------------------------------------
PYR_LEVELS = 2
PYR_BUDGET = (8, 2, 2)   # tests/test_gpu_gn_pyramid.py's BUDGET: twice the per-level counts (4, 1, 1) the nominal start needs (below)
W0, H0, FX = 160, 120, 140.0


@pytest.fixture(scope="module")
def world():
    """Frame 1 of tests/test_gpu_track_and_map.py's world from the oracle, and its restated pyramid."""
    cams = syn.keyframe_cameras(4, radius=0.25, W=W0, H=H0, fx=FX, fy=FX, cx=W0 / 2 - 0.5, cy=H0 / 2 - 0.5)
    sc = syn.make_scene(3000, 21, cams[2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    (out, _), _ = gn.oracle_forward(cams[1], sc)
    gt, gd = out["color"].astype(F), out["depth"][0].astype(F)
    true0, true1 = [np.ascontiguousarray(c["viewmatrix"].T).astype(np.float64) for c in cams[:2]]
    return dict(cams=cams, sc=sc, gt=gt, gd=gd, levels=pr.pyramid(gt, gd, None, PYR_LEVELS, 0.1), true0=true0, true1=true1,
                before=g8.pose_errors(true0, true1)[0])


def _level_intrinsics(l, pixel_centres_at_integers=False):
    s = 2.0 ** l
    cx, cy = W0 / 2 - 0.5, H0 / 2 - 0.5
    if pixel_centres_at_integers:   # (the other convention: NOT this rasteriser's)
        return dict(W=W0 >> l, H=H0 >> l, fx=FX / s, fy=FX / s, cx=(cx + 0.5) / s - 0.5, cy=(cy + 0.5) / s - 0.5)
    return dict(W=W0 >> l, H=H0 >> l, fx=FX / s, fy=FX / s, cx=cx / s, cy=cy / s)


def test_premise_the_level_cameras_render_what_the_box_filter_leaves(world):
    """What level_camera's intrinsics rest on: the map rendered through level l's camera is the box-filtered frame, up to what a box
    filter and a coarser rasterisation differ by -- and through the camera of the other pixel convention, (cx + 0.5) / 2^l - 0.5, it
    is (2^l - 1) / 2 pixels of the frame off: several times the colour error."""
    from gsaj.pyramid import level_camera

    for l in (1, 2):
        err = {}
        for other in (False, True):
            k = _level_intrinsics(l, other)
            cam = syn.make_camera(world["cams"][1]["w2c"], **k)
            (o, _), _ = gn.oracle_forward(cam, world["sc"])
            err[other] = float(np.abs(o["color"] - world["levels"][l - 1]["color"]).mean())
            if not other:
                wl, hl, proj, tx, ty = level_camera(W0, H0, l, FX, FX, W0 / 2 - 0.5, H0 / 2 - 0.5)
                np.testing.assert_allclose(proj.numpy(), cam["projmatrix_raw"].reshape(4, 4), rtol=1e-6, atol=1e-7)
                assert (wl, hl) == (cam["W"], cam["H"]) and (tx, ty) == pytest.approx((cam["tanfovx"], cam["tanfovy"]))
        print("level %d: mean |colour - box-filtered frame| %.5f through level_camera, %.5f through the other convention" % (l, err[False], err[True]))
        assert err[False] < 0.5 * err[True], (l, err)


def _restated_pyramid_loop(world, start, schedule):
    """The restated coarse-to-fine loop -> (the iteration, counted over the frame, at which the accepted pose first met the criterion of
    tests/test_gpu_gn_tracker.py or None; the iteration within each level at which it first held; the accepted losses per level; state)."""
    st = gn.lm_new_state(start, 1e-3)
    met, it, per_level, losses = None, 0, [], []
    L = len(schedule) - 1
    for l, n in zip(range(L, -1, -1), schedule):
        g, d = (world["gt"], world["gd"]) if l == 0 else (world["levels"][l - 1]["color"], world["levels"][l - 1]["depth"])
        if l != L:
            pr.relevel(st, None, None, 1e-3)
        acc, first = [], None
        for k in range(1, n + 1):
            Hm, gv, loss = g8.restated_rows(_level_intrinsics(l), world["sc"], st["w2c"], (0.0, 0.0), g, d, 0.01, False, alpha=0.9)
            gn.lm_step(st, Hm, gv, loss, *LM.values())
            it += 1
            acc.append(st["acc_loss"])
            te, re_ = g8.pose_errors(st["acc_w2c"], world["true1"])
            if te < 0.35 * world["before"] and re_ < 0.02:
                met = met or it
                first = first or k
        per_level.append(first)
        losses.append(acc)
    return met, per_level, losses, st


def _moved_start(world, m):
    """The previous true pose moved by m x the frame-to-frame translation along x."""
    start = world["true0"].copy()
    start[0, 3] += m * world["before"]
    return start


def test_premise_the_nominal_start_meets_the_criterion_within_the_budget(world):
    """The counts PYR_MEASURED of tests/test_gpu_gn_pyramid.py stand on: from the previous true pose the coarsest level meets the
    criterion after 4 iterations and the finer levels keep it from their first; within a level the accepted loss never rises."""
    met, per_level, losses, st = _restated_pyramid_loop(world, world["true0"], PYR_BUDGET)
    print("nominal start: criterion met after %s iterations, within each level after %s; accepted losses %s" % (
        met, per_level, [["%.5f" % x for x in a] for a in losses]))
    assert per_level == [4, 1, 1] and met == 4
    assert all(b <= a for acc in losses for a, b in zip(acc, acc[1:]))
    assert (st["accepted"] + st["rejected"]) == sum(PYR_BUDGET), "the counters count over the frame"
    te, re_ = g8.pose_errors(st["acc_w2c"], world["true1"])
    assert te < 0.35 * world["before"] and re_ < 0.02, (te / world["before"], re_)


# The search for the wide start of the GPU behaviour test, m = 2..6 x the frame-to-frame translation along x: the smallest m at which
# the restated single-level loop misses the criterion within 30 iterations AND the restated pyramid loop, with PYR_BUDGET, meets it.
# Recorded outcome of the whole search (iteration at which the criterion was first met; None: missed):
#     m   single level, 30 iterations   pyramid, (8, 2, 2); its final translation error over the nominal start's
#     2   7                             10    (0.26)
#     3   13                            None  (0.66)
#     4   23                            None  (1.31)
#     5   None (1.02 after 30)          None  (3.17)
#     6   not run                       None  (4.57)
# NO m separates the two in the direction the behaviour test needs: wherever the pyramid meets the criterion the single level does
# too.  On this scene an iteration moves the pose about as far at 40x30 as at 160x120 (the IRLS weights bound the step, not the
# resolution), so from a wide start the pyramid's few iterations run out before the single level's thirty: the pyramid buys time per
# iteration, not a wider basin per iteration.  The wide-start GPU test is therefore not written.  This test re-runs the decisive half
# of the table: where the single level meets the criterion (m = 2) and that the pyramid misses it for every larger m.
WIDE_SEARCH = {2: ("single", 7), 3: ("pyramid", None), 4: ("pyramid", None), 5: ("pyramid", None), 6: ("pyramid", None)}


@pytest.mark.parametrize("m", sorted(WIDE_SEARCH))
def test_premise_no_wide_start_separates_the_pyramid_from_the_single_level(world, m):
    which, want = WIDE_SEARCH[m]
    start = _moved_start(world, m)
    if which == "single":   # the single level meets the criterion: nothing to separate
        met = _restated_pyramid_loop(world, start, (want,))[0]
        assert met == want and met <= 30, (m, met)
    else:                   # the pyramid misses it: nothing to show
        met, _, _, st = _restated_pyramid_loop(world, start, PYR_BUDGET)
        te = g8.pose_errors(st["acc_w2c"], world["true1"])[0]
        print("m = %d: the restated pyramid ends at %.2f x the nominal start's translation error" % (m, te / world["before"]))
        assert met is None and te > 0.35 * world["before"], (m, met, te / world["before"])
