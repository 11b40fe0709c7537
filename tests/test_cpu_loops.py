"""CPU: what the six device loops share (gsaj/_loop.py), on objects made with __new__ and CPU tensors -- no device.  The public
signatures against a table written from the commit before the loops were folded together; ONE set_frame behind DeviceTracker and
GaussNewtonTracker; ONE checked copy behind the window's and the mapper's set_view; the loss description every loop hands its context,
key for key as that commit spelled it; the end of iterate(); and canaries for the two comparators used here."""
import contextlib
import inspect

import numpy as np
import pytest

W, H, K = 37, 29, 3
TRACKING, MONOCULAR, NO_EXPOSURE = 1, 2, 4   # gsaj.losses, as numbers

SIGNATURES = {
    "DeviceTracker": {
        "__init__": "(self, P, W, H, M, device, w2c, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, monocular=False, alpha=0.95, rgb_boundary_threshold=0.01, record_bits=32, band=None, group=None, use_graph=False, fused=True, **pose_kw)",
        "set_frame": "(self, gt_color, gt_depth=None, grad_mask=None, w2c=None, edge_threshold=None, grad_blocks=False)",
        "iterate": "(self, n, check_every=0)",
    },
    "GaussNewtonTracker": {
        "__init__": "(self, P, W, H, M, device, w2c, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, monocular=False, alpha=0.95, rgb_boundary_threshold=0.01, record_bits=32, irls_delta=0.01, lambda_init=0.001, nu=4.0, lambda_min=1e-07, lambda_max=10000000.0, converged_threshold=0.0001, solve_exposure=False)",
        "set_frame": "(self, gt_color, gt_depth=None, grad_mask=None, w2c=None, edge_threshold=None, grad_blocks=False)",
        "reset": "(self, w2c, exposure=(0.0, 0.0))",
        "iterate": "(self, n, check_every=0)",
    },
    "GaussNewtonWindow": {
        "__init__": "(self, K, P, W, H, M, device, w2cs, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, sh_degree=0, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, monocular=False, alpha=0.95, rgb_boundary_threshold=0.01, record_bits=32, irls_delta=0.01, lambda_init=0.001, nu=4.0, lambda_min=1e-07, lambda_max=10000000.0, converged_threshold=0.0001, solve_exposure=False, streams=1)",
        "set_frame": "(self, gt_color, gt_depth=None, grad_mask=None, w2cs=None, exposure=None)",
        "set_view": "(self, slot, gt_color, gt_depth=None, grad_mask=None, w2c=None, exposure=None)",
        "reset": "(self, slot, w2c, exposure=(0.0, 0.0))",
        "iterate": "(self, n, check_every=0)",
        "best": "(self)",
    },
    "PyramidGaussNewtonTracker": {
        "__init__": "(self, P, W, H, M, device, w2c, projection_matrix, tanfovx, tanfovy, bg, means3D, opacities, levels=0, fx=None, fy=None, cx=None, cy=None, znear=0.01, zfar=100.0, depth_edge_ratio=0.1, **kw)",
        "set_frame": "(self, gt_color, gt_depth=None, grad_mask=None, w2c=None, edge_threshold=None, grad_blocks=False)",
        "iterate": "(self, schedule, check_every=0)",
        "relevel": "(self, level, skip=None)",
    },
    "DeviceMapper": {
        "__init__": "(self, model, K, W, H, projection_matrix, tanfovx, tanfovy, bg, device=None, w2cs=None, n_window=None, uids=None, pose_window=3, monocular=False, alpha=0.95, rgb_boundary_threshold=0.01, isotropic_weight=10.0, fused=False, streams=1, split=False, record_bits=32, **pose_kw)",
        "set_view": "(self, slot, gt_color, gt_depth=None, w2c=None, exposure=None)",
        "iterate": "(self, n, reset=None, initialization=False)",
        "refresh": "(self)",
    },
    "RgbdAligner": {
        "__init__": "(self, W, H, fx, fy, cx, cy, device, levels=2, w_depth=1.0, delta_photo=0.01, delta_depth=0.01, depth_edge_ratio=0.1, min_depth=0.01, max_depth=100.0, min_overlap=0.0, znear=0.01, zfar=100.0, lambda_init=0.001, nu=4.0, lambda_min=1e-07, lambda_max=10000000.0, converged_threshold=0.0001)",
        "align": "(self, color, depth=None, w2c_init=None, schedule=None)",
        "set_reference": "(self, color, depth, w2c)",
        "promote": "(self, w2c=None)",
    },
}
METHODS = ("__init__", "set_frame", "set_view", "reset", "iterate", "align", "set_reference", "promote", "refresh", "best", "relevel")


def _classes():
    from gsaj.align import RgbdAligner
    from gsaj.gauss_newton import GaussNewtonTracker, GaussNewtonWindow, PyramidGaussNewtonTracker
    from gsaj.mapping import DeviceMapper
    from gsaj.tracking import DeviceTracker
    return DeviceTracker, GaussNewtonTracker, GaussNewtonWindow, PyramidGaussNewtonTracker, DeviceMapper, RgbdAligner


def test_public_signatures_are_the_ones_before_the_fold():
    got = {c.__name__: {n: str(inspect.signature(getattr(c, n))) for n in METHODS if inspect.isfunction(getattr(c, n, None))} for c in _classes()}
    assert got == SIGNATURES


# ---- hand-made loops ---------------------------------------------------------------------------------------------------------------
class _Pose:
    """What DeviceTracker asks of its PoseTracker outside a launch."""

    def __init__(self):
        import torch
        self.state, self.resets, self.steps = torch.zeros(80), [], 0
        self.viewmatrix, self.projmatrix, self.campos = self.state[35:51].view(4, 4), self.state[51:67].view(4, 4), self.state[67:70]
        self.exposure_a, self.exposure_b, self.converged = self.state[33:34], self.state[34:35], self.state[77]

    def reset(self, w2c):
        self.resets.append(w2c)

    def step(self, *a, **kw):
        self.steps += 1


class _FrameCtx:
    """A FrameContext as the loops see it: records every call, hands back what the next call reads."""

    def __init__(self, packed=None):
        import torch
        self.capacity, self.fail, self.calls, self.packed = 0, None, [], packed
        self.partials = torch.zeros(4, 32)

    def status(self):
        from gsaj import _lib
        if self.fail:
            msg, self.fail = self.fail, None
            raise _lib.GsajError(msg)

    def forward(self, *a, **kw):
        self.calls.append(("forward", kw.get("sync")))

    def forward_loss(self, L, *a, **kw):
        self.calls.append(("forward_loss", L))

    def backward_loss(self, L, *a, **kw):
        self.calls.append(("backward_loss", L))
        return dict(tau_sum=self.packed)

    def pose_jacobian_loss(self, L, *a, **kw):
        self.calls.append(("pose_jacobian_loss", L))
        return dict(partials=self.partials)

    def descriptions(self):
        return [c[1] for c in self.calls if isinstance(c[1], dict)]


def _device_tracker(fused=True):
    import torch
    from gsaj.tracking import DeviceTracker

    t = DeviceTracker.__new__(DeviceTracker)
    t.dev, t.pose, t.group, t.use_graph, t.fused = torch.device("cpu"), _Pose(), None, False, fused
    t.packed = torch.zeros(12)
    t.ctx = _FrameCtx(t.packed)
    t.flags, t.alpha, t.thr = TRACKING, 0.9, 0.02
    t.bg, t.means, t.opac, t.praw, t.tanfov, t.kw = torch.zeros(3), torch.zeros(5, 3), torch.zeros(5, 1), torch.eye(4), (0.5, 0.4), {}
    t._abort_ptr, t._abort_word, t._graphs = 0, torch.zeros(1, dtype=torch.int32), None
    t.gt_color = t.gt_depth = t.grad_mask = t._grad_op = None
    t.iterations = 0
    return t


def _gn_tracker(solve_exposure=False):
    import torch
    from gsaj.gauss_newton import GaussNewtonTracker

    t = GaussNewtonTracker.__new__(GaussNewtonTracker)
    t.dev, t.solve_exposure = torch.device("cpu"), solve_exposure
    t.state, t.projection, t.lm_args = torch.zeros(152 if solve_exposure else 136), torch.eye(4), (1e-3, 4.0, 1e-7, 1e7, 1e-4)
    t.praw, t.ctx, t._abort_ptr = t.projection, _FrameCtx(), 0
    t.flags, t.alpha, t.thr, t.delta = TRACKING | MONOCULAR, 0.9, 0.02, 0.03
    t.bg, t.means, t.opac, t.tanfov, t.kw = torch.zeros(3), torch.zeros(5, 3), torch.zeros(5, 1), (0.5, 0.4), {}
    t._step, t._step_name = (lambda *a: 0), "step"
    t.gt_color = t.gt_depth = t.grad_mask = t._grad_op = None
    t.iterations = 0
    t.reset(np.eye(4))
    return t


def _frames(n=2, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(3, H, W, generator=g), torch.rand(H, W, generator=g), (torch.rand(1, H, W, generator=g) < 0.5).to(torch.uint8)) for _ in range(n)]


def _addresses(t):
    return [None if b is None else b.data_ptr() for b in (t.gt_color, t.gt_depth, t.grad_mask)]


def addresses_kept(tracker, frames, **kw):
    """The frame-buffer rule: every buffer of the first frame is the buffer of every later frame."""
    tracker.set_frame(*frames[0], **kw)
    first = _addresses(tracker)
    for f in frames[1:]:
        tracker.set_frame(*f, **kw)
    return _addresses(tracker) == first


# ---- one set_frame -----------------------------------------------------------------------------------------------------------------
def test_both_single_frame_trackers_have_the_one_set_frame():
    import torch
    from gsaj._loop import FrameTarget
    from gsaj.gauss_newton import GaussNewtonTracker
    from gsaj.tracking import DeviceTracker

    assert DeviceTracker.set_frame is FrameTarget.set_frame and GaussNewtonTracker.set_frame is FrameTarget.set_frame
    frames = _frames()
    a, b = _device_tracker(), _gn_tracker()
    w2c = np.eye(4)
    w2c[0, 3] = 0.25
    for t in (a, b):
        assert addresses_kept(t, frames, w2c=w2c)
    for x, y in ((a.gt_color, b.gt_color), (a.gt_depth, b.gt_depth), (a.grad_mask, b.grad_mask)):
        assert torch.equal(x, y)
    assert torch.equal(a.gt_color, frames[1][0]) and torch.equal(a.gt_depth, frames[1][1]) and torch.equal(a.grad_mask, frames[1][2].view(-1))
    assert a.grad_mask.dtype == torch.uint8 and a.gt_color.data_ptr() != frames[0][0].data_ptr()   # the tracker's own buffers
    # the new start pose goes to each loop's own reset
    assert len(a.pose.resets) == 2 and a.pose.resets[0] is w2c and float(b.state[3]) == 0.25
    a.set_frame(*frames[0])
    assert len(a.pose.resets) == 2   # no pose given: the pose stays


@pytest.mark.parametrize("make", [_device_tracker, _gn_tracker])
def test_depth_and_mask_are_for_every_frame_or_for_none(make):
    from gsaj import _lib

    (c, d, m), text = _frames(1)[0], "for every frame of a tracker or for none"
    for first, later in ((dict(), dict(gt_depth=d)), (dict(gt_depth=d), dict()), (dict(gt_depth=d), dict(gt_depth=d, grad_mask=m)),
                         (dict(gt_depth=d, grad_mask=m), dict(gt_depth=d)), (dict(), dict(edge_threshold=1.1))):
        t = make()
        t.set_frame(c, **first)
        before = _addresses(t)
        with pytest.raises(_lib.GsajError, match=text):
            t.set_frame(c, **later)
        t.set_frame(c, **first)
        assert _addresses(t) == before


@pytest.mark.parametrize("make", [_device_tracker, _gn_tracker])
def test_a_computed_mask_goes_through_one_grad_mask_into_the_own_buffer(monkeypatch, make):
    import torch
    import gsaj._loop as loop

    made, calls = [], []

    class Recorder:
        def __init__(self, *a):
            made.append(a)

        def __call__(self, image, edge_threshold, blocks=False, out=None):
            calls.append((image.data_ptr(), edge_threshold, blocks, out.data_ptr()))
            out.fill_(1)

    monkeypatch.setattr(loop, "GradMask", Recorder)
    t, frames = make(), _frames(3)
    t.set_frame(frames[0][0], frames[0][1], edge_threshold=1.5)
    mask = t.grad_mask
    assert mask.dtype == torch.uint8 and mask.numel() == W * H
    t.set_frame(frames[1][0], frames[1][1], edge_threshold=2.0, grad_blocks=True)
    assert made == [(W, H, torch.device("cpu"))]
    assert calls == [(t.gt_color.data_ptr(), 1.5, False, mask.data_ptr()), (t.gt_color.data_ptr(), 2.0, True, mask.data_ptr())] and t.grad_mask is mask
    # frame_views: someone else's buffers read in place, a given mask flattened, or an own mask buffer for compute_mask
    c, d, m = frames[2]
    u = make()
    u.frame_views(c, d, m)
    assert u.gt_color is c and u.gt_depth is d and u.grad_mask.data_ptr() == m.data_ptr() and tuple(u.grad_mask.shape) == (W * H,) and u._grad_op is None
    v = make()
    v.frame_views(c, None, None, own_mask=True)
    assert v.gt_depth is None and v.grad_mask.numel() == W * H and v.grad_mask.data_ptr() != m.data_ptr()
    v.compute_mask(1.2)
    assert made[-1] == (W, H, torch.device("cpu")) and calls[-1] == (c.data_ptr(), 1.2, False, v.grad_mask.data_ptr())
    w = make()
    w.frame_views(c, d)
    assert w.grad_mask is None


def test_canary_the_address_check_rejects_a_set_frame_that_clones_again():
    class Recloning(type(_device_tracker())):
        def set_frame(self, *a, **kw):
            self.kept = (self.gt_color, self.gt_depth, self.grad_mask)   # (alive, so that the allocator cannot hand the addresses out again)
            self.gt_color = self.gt_depth = self.grad_mask = None
            super().set_frame(*a, **kw)

    t = _device_tracker()
    t.__class__ = Recloning
    assert not addresses_kept(t, _frames()) and addresses_kept(_device_tracker(), _frames())


# ---- K views -----------------------------------------------------------------------------------------------------------------------
class _BatchCtx:
    def __init__(self):
        import torch
        self.K, self.W, self.H, self.dev, self.aborts, self.calls = K, W, H, torch.device("cpu"), 0, []
        self.partials = torch.zeros(K, 4, 64)
        self.radii = self.n_touched = torch.zeros(K, 5, dtype=torch.int32)

    def clear_aborts(self):
        n, self.aborts = self.aborts, 0
        return n

    def abort_flags(self):
        return None, 0

    def forward(self, *a, **kw):
        self.calls.append(("forward", kw.get("sync")))

    def forward_loss(self, L, *a, **kw):
        self.calls.append(("forward_loss", L))

    def backward_loss(self, L, *a, **kw):
        import torch
        self.calls.append(("backward_loss", L))
        return dict(scale=torch.zeros(5, 3), mean2D=torch.zeros(K, 5, 3), tau_all=torch.zeros(K, 6))

    def pose_jacobian_loss(self, L, *a, **kw):
        self.calls.append(("pose_jacobian_loss", L))
        return dict(partials=self.partials)

    descriptions = _FrameCtx.descriptions


def _window(monocular=False, solve_exposure=True):
    import torch
    from gsaj.gauss_newton import GaussNewtonWindow

    win = GaussNewtonWindow.__new__(GaussNewtonWindow)
    win._init_host(_BatchCtx(), np.stack([np.eye(4)] * K), np.eye(4), (0.5, 0.4), torch.zeros(3), torch.zeros(5, 3), torch.zeros(5, 1), {},
                   dict(monocular=monocular, alpha=0.9, rgb_boundary_threshold=0.02, irls_delta=0.03), (1e-3, 4.0, 1e-7, 1e7, 1e-4), solve_exposure)
    return win


def _mapper_target(monocular=False):
    """The mapper as tests/test_cpu_fused_batch.py makes it: K, W, H and the two buffers, nothing else."""
    import torch
    from gsaj.mapping import DeviceMapper

    m = DeviceMapper.__new__(DeviceMapper)
    m.K, m.W, m.H = K, W, H
    m.gt_color, m.gt_depth = torch.zeros(K, 3, H, W), None if monocular else torch.zeros(K, H, W)
    return m


@pytest.mark.parametrize("make", [_window, _mapper_target])
@pytest.mark.parametrize("monocular", [False, True])
def test_set_view_makes_the_shared_checks_and_fills_one_slot(make, monocular):
    import torch
    from gsaj import _lib
    from gsaj._loop import ViewTargets

    t = make(monocular)
    assert type(t)._take_view is ViewTargets._take_view and (t.gt_depth is None) == monocular and tuple(t.gt_color.shape) == (K, 3, H, W)
    c, d = torch.ones(3, H, W), None if monocular else torch.ones(H, W)
    bad = [((K, c, d), "slot %d" % K), ((K + 5, c, d), "slot"), ((-1, c, d), "slot -1"), ((0, torch.ones(3, W, H), d), r"gt_color must be \[3,%d,%d\]" % (H, W)),
           ((0, torch.ones(1, H, W), d), "gt_color"), ((0, torch.ones(3, H, W + 1), d), "gt_color"), ((0, torch.ones(H, W), d), "gt_color"),
           ((0, c, torch.ones(H, W) if monocular else None), "monocular")]
    if not monocular:
        bad += [((0, c, torch.ones(H, W + 1)), "gt_depth must have %d" % (H * W)), ((0, c, torch.zeros(5, W)), "gt_depth")]
    for args, text in bad:
        with pytest.raises(_lib.GsajError, match=text):
            t.set_view(*args)
    assert not t.gt_color.any() and (monocular or not t.gt_depth.any())   # a refused view copied nothing
    t.set_view(K - 1, c, d)
    assert torch.equal(t.gt_color[K - 1], c) and not t.gt_color[:K - 1].any()
    if not monocular:
        assert torch.equal(t.gt_depth[K - 1], d) and not t.gt_depth[:K - 1].any()


def test_the_window_keeps_its_mask_slots_and_filled_flags():
    import torch
    from gsaj import _lib

    win, (c, d, m) = _window(), _frames(1)[0]
    with pytest.raises(_lib.GsajError, match="grad_mask must have %d" % (H * W)):
        win.set_view(0, c, d, grad_mask=torch.zeros(H * W - 1, dtype=torch.uint8))
    win.set_view(1, c, d)
    assert win.grad_mask is None and win._filled == [False, True, False]
    win.set_view(0, c, d, grad_mask=m)   # a mask on one slot: the others get all ones, which is no mask
    n = H * W
    assert tuple(win.grad_mask.shape) == (K * n,) and torch.equal(win.grad_mask[:n], m.view(-1)) and bool((win.grad_mask[n:] == 1).all())
    win.set_view(0, c, d)
    assert bool((win.grad_mask == 1).all()) and win._filled == [True, True, False]
    with pytest.raises(_lib.GsajError, match="GaussNewtonWindow: slot 3"):
        win.reset(3, np.eye(4))


# ---- the loss description ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    import torch
    if torch.is_tensor(a) and torch.is_tensor(b):
        return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype
    return type(a) is type(b) and a == b


def same_description(got, want):
    """Key for key; tensors by address, shape and stride, everything else by type and value."""
    return set(got) == set(want) and all(_same(got[k], want[k]) for k in want)


def _mapper(initialization):
    import torch
    from gsaj.mapping import DeviceMapper

    class Model:
        active_sh_degree = 3
        get_xyz, get_opacity, get_features = torch.zeros(5, 3), torch.zeros(5, 1), torch.zeros(5, 16, 3)
        get_scaling, get_rotation = torch.ones(5, 3), torch.zeros(5, 4)
        densification_step = map_step = update_learning_rate = staticmethod(lambda *a, **kw: None)

    class Poses:
        state = torch.zeros(K, 80)
        exposure = state[:, 33:35]
        matrices = staticmethod(lambda: (torch.zeros(K, 4, 4), torch.zeros(K, 4, 4), torch.zeros(K, 3)))
        step = staticmethod(lambda *a, **kw: None)

    m = _mapper_target()
    m.model, m.ctx, m.poses, m.P = Model(), _BatchCtx(), Poses(), 5
    m.tanfov, m.bg, m.praw, m.n_window = (0.5, 0.4), torch.zeros(3), torch.eye(4), K
    m.flags, m.alpha, m.thr, m.iso_weight, m.fused, m.split = MONOCULAR, 0.9, 0.02, 10.0, True, False
    m.scalars, m.dexposure, m.active, m.seeds = torch.zeros(K, 5), torch.zeros(K, 2), torch.ones(K, dtype=torch.uint8), None
    m.iso = lambda *a, **kw: None
    m._sized, m.iteration_count, m.dev = True, 0, torch.device("cpu")
    return m


def _descriptions(monkeypatch):
    """(what each loop handed its context, what the parent commit's code handed it) per loop."""
    import gsaj.gauss_newton as G

    monkeypatch.setattr(G, "stream", lambda dev: None)
    c, d, m = _frames(1)[0]
    out = {}
    t = _device_tracker()
    t.set_frame(c, d, m)
    t._render_and_grads(False)
    p = t.pose
    out["DeviceTracker"] = (t.ctx.descriptions(), 2, dict(
        flags=TRACKING, alpha=0.9, rgb_boundary_threshold=0.02, gt_color=t.gt_color, gt_depth=t.gt_depth, grad_mask=t.grad_mask, exposure_a=p.exposure_a,
        exposure_b=p.exposure_b, scalars=t.packed[6:11]))
    g = _gn_tracker()
    g.set_frame(c)
    g._iteration(False)
    out["GaussNewtonTracker"] = (g.ctx.descriptions(), 1, dict(
        flags=TRACKING | MONOCULAR, alpha=0.9, rgb_boundary_threshold=0.02, gt_color=g.gt_color, gt_depth=None, grad_mask=None, exposure_a=g.state[33:34],
        exposure_b=g.state[34:35]))
    win = _window()
    win.lib = type("Lib", (), dict(gsaj_pose_gn8_step_batch=staticmethod(lambda *a: 0)))()
    win.set_view(0, c, d, grad_mask=m)
    G._launch(win, False)
    out["GaussNewtonWindow"] = (win.ctx.descriptions(), 1, dict(
        flags=TRACKING, alpha=0.9, rgb_boundary_threshold=0.02, gt_color=win.gt_color, gt_depth=win.gt_depth, grad_mask=win.grad_mask,
        exposure_a=win.state[:, 33], exposure_b=win.state[:, 34], exposure_stride=152))
    for init in (False, True):
        mp = _mapper(init)
        mp._iteration(None, init)
        e = mp.poses.state
        out["DeviceMapper/%s" % init] = (mp.ctx.descriptions(), 2, dict(
            flags=MONOCULAR | (NO_EXPOSURE if init else 0), alpha=0.9, rgb_boundary_threshold=0.02, gt_color=mp.gt_color, gt_depth=mp.gt_depth,
            exposure_a=None if init else e[:, 33], exposure_b=None if init else e[:, 34], exposure_stride=80, scalars=mp.scalars, dexposure=mp.dexposure))
    return out


def test_every_loop_hands_its_context_the_description_it_always_did(monkeypatch):
    for name, (got, n, want) in _descriptions(monkeypatch).items():
        assert len(got) == n and all(same_description(L, want) for L in got), (name, got, want)
        assert all(L is got[0] for L in got), name   # the forward and the backward of one iteration read ONE dictionary
    assert "grad_mask" not in _descriptions(monkeypatch)["DeviceMapper/False"][0][0]


def test_canary_the_description_comparison_rejects_a_dropped_key_and_swapped_exposures(monkeypatch):
    for name, (got, _, want) in _descriptions(monkeypatch).items():
        L = got[0]
        for k in L:
            assert not same_description({j: v for j, v in L.items() if j != k}, want), (name, k)
        assert not same_description(dict(L, extra=1), want)
        if L["exposure_a"] is not None:
            assert not same_description(dict(L, exposure_a=L["exposure_b"], exposure_b=L["exposure_a"]), want), name
        assert not same_description(dict(L, gt_color=L["gt_color"].clone()), want) and not same_description(dict(L, flags=L["flags"] ^ TRACKING), want)


# ---- the end of iterate() and the counted loop ---------------------------------------------------------------------------------------
def _counted(monkeypatch, which):
    """(loop, the syncs of the iterations run, a function that sets the converged flag) with the iteration replaced by a counter."""
    import torch

    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
    syncs, c, d, _ = [], *_frames(1)[0]
    t = _device_tracker() if which == "DeviceTracker" else _gn_tracker()
    t.set_frame(c, d)
    flag = t.pose.state if which == "DeviceTracker" else t.state
    converge_at = [None]

    def one(sync):
        syncs.append(sync)
        t.ctx.capacity = 1
        if len(syncs) == converge_at[0]:
            flag[77] = 1.0

    if which == "DeviceTracker":
        t._eager = one
    else:
        t._iteration = one
    return t, syncs, converge_at


@pytest.mark.parametrize("which", ["DeviceTracker", "GaussNewtonTracker"])
def test_a_frame_loop_raises_after_the_loop_and_sizes_again_next_time(monkeypatch, which):
    from gsaj import _lib

    t, syncs, converge_at = _counted(monkeypatch, which)
    assert t.iterate(3) == 3 and syncs == [True, False, False] and t.iterations == 3
    t.ctx.fail = "an asynchronous forward was aborted on the device"
    with pytest.raises(_lib.GsajError, match="asynchronous forward was aborted"):
        t.iterate(2)
    assert syncs[3:] == [False, False] and t.ctx.capacity == 0 and t.iterations == 5   # the loop ran to its end first
    assert t.iterate(1) == 1 and syncs[5] is True
    # check_every = 2: the flag is set during iteration 3 of this call and seen at 4, the first multiple of 2 after it
    del syncs[:]
    converge_at[0] = 3
    assert t.iterate(9, check_every=2) == 4 and len(syncs) == 4 and t.iterations == 10
    assert t.iterate(5) == 5 and t.iterate(5, check_every=5) == 5 and t.iterations == 20   # no check_every: the flag is not looked at


def test_the_mapper_raises_after_the_loop_and_sizes_again_next_time(monkeypatch):
    import torch
    from gsaj import _lib

    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
    m, ran = _mapper(False), []
    m._iteration = lambda reset, initialization: ran.append((reset, initialization))
    assert m.iterate(3, reset="all") == 3 and ran == [(None, False), (None, False), ("all", False)] and m._sized
    m.ctx.aborts = 2
    with pytest.raises(_lib.GsajError, match=r"2 asynchronous forward\(s\) of the window were aborted on the device .*: those views added nothing to the "
                                             "gradient sums and their poses were skipped"):
        m.iterate(2, initialization=True)
    assert len(ran) == 5 and m._sized is False
    m._sized = True
    assert m.iterate(1) == 1 and m._sized


def test_the_window_raises_the_same_message_with_its_own_consequence(monkeypatch):
    import gsaj.gauss_newton as G
    from gsaj import _lib

    syncs = []
    monkeypatch.setattr(G, "_launch", lambda win, sync: syncs.append(sync))
    win, (c, d, _) = _window(), _frames(1)[0]
    win.set_frame(c, d)
    assert win.iterate(2) == 2 and syncs == [True, False]
    win.ctx.aborts = 2
    with pytest.raises(_lib.GsajError, match=r"2 asynchronous forward\(s\) of the window were aborted on the device .*: those views' states were skipped"):
        win.iterate(2)
    assert win._sized is False and win.iterate(1) == 1 and syncs == [True, False, False, False, True] and win.iterations == 5
    win.state[:, 77] = 1.0
    assert win.iterate(6, check_every=2) == 2


def test_the_small_helpers():
    import torch
    from gsaj import _lib
    from gsaj._loop import loss_terms, map_args, require_device

    for who in ("DeviceTracker", "PoseTracker"):
        with pytest.raises(_lib.GsajError, match=r"^%s needs a HIP device \(there is no CPU path\)$" % who):
            require_device("cpu", who)
    assert require_device("cuda:1", "x") == torch.device("cuda:1")
    assert loss_terms(True, 1, 2) == (MONOCULAR, 1.0, 2.0) and loss_terms(False, 0.5, 0.25, 0.125, TRACKING) == (TRACKING, 0.5, 0.25, 0.125)
    assert map_args(3, "s") == dict(sh_degree=3, shs="s", colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None)
