"""GPU: the batched Jacobian walk (csrc/pose_jac.hip: k_splat_jac_batch, k_render_jac_batch through
gsaj_rasterize_pose_jacobian_loss_batch / _loss8_batch and BatchContext.pose_jacobian_loss): K = 3 views of the 72x40 scene of
tests/gn_restated.py -- 5x3 tiles, 60 workgroups padded to 64 rows per view -- each with its own camera, ground truth, mask and
exposure (tests/gn_window_restated.py), so that a kernel which reads another view's block cannot pass.

Every view is judged (a) against the float64 restatement applied to the DEVICE's own Jacobian and images of that view, within the
bounds derived in gn_restated / gn8_restated from the count of fp32 roundings, (b) bit for bit against the single-view entry point
run on view v's workspace blocks of the same batched forward, (c) by the transpose identity against BatchContext.backward."""
import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import gn_window_restated as gw
import helpers as hp
import loss_restated as lr

pytestmark = pytest.mark.gpu

K, W, H = gw.K, gn.JAC_W, gn.JAC_H
ROWS = 64                      # gsaj_pose_jac_partial_rows(72, 40): 15 tiles x 4 quadrants in the grid of 32-workgroup groups
PADDING = (39, 47, 55, 63)     # the workgroups whose rank (blockIdx >> 5) * 8 + (blockIdx & 7) is beyond the 15 tiles
SENTINEL = -7.0


class Window:
    """One batched forward of the K views on the device; the device's own images and each view's ground truth."""

    def __init__(self, record_bits, precomp, K_=K, streams=1):
        import torch
        from gsaj import synthetic as syn
        from gsaj.rasterizer import BatchContext

        self.dev = torch.device("cuda:0")
        self.t = t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.dev)  # noqa: E731
        cams, sc, _ = gw.window_cameras()
        self.K, self.cams = K_, cams[:K_]
        P = sc["means3D"].shape[0]
        self.ctx = BatchContext(K_, P, W, H, 16, self.dev, has_scales=not precomp, record_bits=record_bits, streams=streams)
        self.bg, self.means, self.opac = t(gn.JAC_BG), t(sc["means3D"]), t(sc["opacities"])
        self.kw = dict(sh_degree=gn.JAC_DEG, shs=t(sc["shs"]))
        if precomp:   # no view then depends on view 0's geometry block for cov3D
            self.kw["cov3D_precomp"] = t(syn.covariance6(sc["scales"], sc["rotations"]))
        else:
            self.kw.update(scales=t(sc["scales"]), rotations=t(sc["rotations"]))
        self.views = tuple(t(np.stack([c[k] for c in self.cams])) for k in ("viewmatrix", "projmatrix", "campos"))
        self.praw = t(cams[0]["projmatrix_raw"])
        self.tan = (cams[0]["tanfovx"], cams[0]["tanfovy"])
        self.forward()
        self.img = [dict(image=self.ctx.color[v].cpu().numpy(), depth=self.ctx.depth[v].cpu().numpy(), opacity=self.ctx.opacity[v].cpu().numpy())
                    for v in range(K_)]
        self.truths = [gw.ground_truth(self.img[v]["image"], self.img[v]["depth"], v) for v in range(K_)]
        self.E = t(np.asarray(gw.EXPOSURES[:K_], np.float32))      # [K,2]: the pair read in place with exposure_stride = 2
        self.gt_c = t(np.stack([tr[0] for tr in self.truths]))
        self.gt_d = t(np.stack([tr[1] for tr in self.truths]))
        self.mask = torch.as_tensor(np.stack([tr[2] for tr in self.truths]).reshape(-1), device=self.dev)

    def forward(self):
        st = self.ctx.forward(self.bg, self.means, self.opac, *self.views, *self.tan, sync=True, **self.kw)
        assert not any(ab for _, _, ab in st)

    def loss(self, mono, masked, flags_extra=0):
        return dict(flags=lr.TRACKING | (lr.MONOCULAR if mono else 0) | flags_extra, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=self.gt_c,
                    gt_depth=None if mono else self.gt_d, grad_mask=self.mask if masked else None, exposure_a=self.E[:, 0], exposure_b=self.E[:, 1],
                    exposure_stride=2)

    def jac_loss(self, L, ctx=None, **kw):
        return (ctx or self.ctx).pose_jacobian_loss(L, self.bg, self.means, self.views[0], self.views[1], self.praw, self.views[2], *self.tan,
                                                    **kw, **self.kw)

    def single_view(self, v, L, delta, joint, want_jacobian=True):
        """The single-view entry point on view v's workspace blocks of the batched forward -> (rows [64, 32 | 64], jac [H,W,4,6])."""
        import torch
        from gsaj import _lib
        from gsaj.rasterizer import _scene, _view

        c = self.ctx
        if not hasattr(self, "jac_ws1"):
            self.jac_ws1 = torch.empty(c.lib.gsaj_pose_jac_workspace_bytes(c.P, W, H), device=self.dev, dtype=torch.uint8)
        rows = torch.full((ROWS, 64 if joint else 32), SENTINEL, device=self.dev)
        jac = torch.empty((H, W, 4, 6), device=self.dev) if want_jacobian else None
        Lv = dict(L, gt_color=L["gt_color"][v], gt_depth=None if L["gt_depth"] is None else L["gt_depth"][v],
                  grad_mask=None if L["grad_mask"] is None else L["grad_mask"][v * H * W:(v + 1) * H * W],
                  exposure_a=self.E[v, 0:1], exposure_b=self.E[v, 1:2])
        la = c._loss(Lv)
        name = "gsaj_rasterize_pose_jacobian_loss8" if joint else "gsaj_rasterize_pose_jacobian_loss"
        kw = self.kw
        _lib.check(getattr(c.lib, name)(
            *c._head(kw["sh_degree"], self.bg, c.capacity),
            *_scene(self.means, kw["shs"], None, kw.get("scales"), 1.0, kw.get("rotations"), kw.get("cov3D_precomp")),
            *_view(*self.views, *self.tan, projmatrix_raw=self.praw, v0=v), *c._bwd_state(v), self.jac_ws1.data_ptr(), *la[:3], *c._images(v),
            *la[3:], float(delta), rows.data_ptr(), None if jac is None else jac.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream), name)
        return rows, jac


_WINDOWS = {}


def _window(record_bits, precomp):
    key = (record_bits, precomp)
    if key not in _WINDOWS:
        _WINDOWS[key] = Window(record_bits, precomp)
    return _WINDOWS[key]


def _filled(w, joint, K_=K):
    import torch
    return torch.full((K_, ROWS, 64 if joint else 32), SENTINEL, device=w.dev)


@pytest.mark.parametrize("record_bits", [32, 16], ids=["fp32-records", "fp16-records"])
@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
@pytest.mark.parametrize("mono", [False, True], ids=["rgbd", "mono"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masked"])
def test_every_view_against_the_restatement_on_its_own_jacobian_and_images(record_bits, joint, mono, masked):
    w = _window(record_bits, False)
    L = w.loss(mono, masked)
    for delta in (0.0, 0.03):
        o = w.jac_loss(L, irls_delta=delta, solve_exposure=joint, want_jacobian=True, partials=_filled(w, joint))
        rows, J = o["partials"].cpu().numpy(), o["jacobian"].cpu().numpy()
        assert rows.shape == (K, ROWS, 64 if joint else 32) and J.shape == (K, H, W, 4, 6) and np.isfinite(rows).all()
        for v in range(K):
            tag = "view %d %s mono=%s masked=%s delta=%g records=%d" % (v, "joint" if joint else "6-form", mono, masked, delta, record_bits)
            assert not rows[v, PADDING, :].any(), "%s: the padding rows of every view are written as zero" % tag
            if joint:
                assert not rows[v, :, 49:].any(), "%s: slots [49:64) are zero" % tag
            tot = rows[v].astype(np.float64).sum(axis=0)
            want, q = gw.view_equations(J[v], w.img[v], w.truths[v], gw.EXPOSURES[v], delta, joint, mono, masked)
            if joint:
                r = gn.assert_normal_equations_close(g8.sym8(tot[:36]), tot[36:44], want, tag)
                ls = tot[44:47]
            else:
                r = gn.assert_normal_equations_close(gn.sym6(tot[:21]), tot[21:27], want, tag)
                ls = tot[27:30]
            ratios = lr.assert_loss_close(dict(loss=ls[0], l1_rgb=ls[1], l1_depth=ls[2]), q["loss"], tag, outputs=("loss", "l1_rgb", "l1_depth"))
            print("%s: H, g worst err / bound %.3f, loss terms %s" % (tag, r, ratios))


@pytest.mark.parametrize("record_bits", [32, 16], ids=["fp32-records", "fp16-records"])
@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
@pytest.mark.parametrize("precomp", [True, False], ids=["cov3D_precomp", "scales-rotations"])
def test_every_view_is_the_single_view_entry_point_bit_for_bit(record_bits, joint, precomp):
    """cov3D_precomp: every view's blocks are a complete single-view workspace, so every view must equal.  Scales / rotations: only
    view 0's geometry block holds cov3D (the batched kernel reads it there for every view), so the single-view call is valid on view 0
    only; the other views are held by the restatement above."""
    import torch

    w = _window(record_bits, precomp)
    for mono, masked, delta in ((False, True, 0.03), (True, False, 0.0)):
        L = w.loss(mono, masked)
        o = w.jac_loss(L, irls_delta=delta, solve_exposure=joint, want_jacobian=True, partials=_filled(w, joint))
        for v in (range(K) if precomp else (0,)):
            rows1, jac1 = w.single_view(v, L, delta, joint)
            assert torch.equal(o["jacobian"][v], jac1), "view %d: jac_out differs from the single-view entry point" % v
            assert torch.equal(o["partials"][v], rows1), "view %d: the partial rows differ from the single-view entry point" % v
        # without jac_out the rows are the same bits
        again = w.jac_loss(L, irls_delta=delta, solve_exposure=joint, partials=_filled(w, joint))
        assert again["jacobian"] is None and torch.equal(again["partials"], o["partials"])


@pytest.mark.parametrize("record_bits", [32, 16], ids=["fp32-records", "fp16-records"])
def test_transpose_identity_per_view_against_the_batched_backward(record_bits):
    """sum s J contracted on the host from jac_out[v] against tau_all[v] of BatchContext.backward under the same seed images: the
    existing limit, 5e-5 of the row's maximum."""
    w = _window(record_bits, False)
    rng = np.random.default_rng(5)
    s_c = rng.normal(size=(K, 3, H, W)).astype(np.float32) / (3 * H * W)
    s_d = rng.normal(size=(K, 1, H, W)).astype(np.float32) / (H * W)
    J = w.jac_loss(w.loss(False, False), irls_delta=0.03, want_jacobian=True)["jacobian"].cpu().numpy()
    g = w.ctx.backward(w.bg, w.means, w.views[0], w.views[1], w.praw, w.views[2], *w.tan, w.t(s_c), w.t(s_d), **w.kw)
    tau = g["tau_all"].cpu().numpy().astype(np.float64)
    for v in range(K):
        e = hp.rel_err(gn.contract(J[v], s_c[v], s_d[v]), tau[v])
        print("view %d: transpose identity rel err %.3e" % (v, e))
        assert np.abs(tau[v]).max() > 0 and e < hp.GRAD_TOL, (v, e)
        for u in range(K):   # ... and it is view v's Jacobian, not another view's
            assert u == v or hp.rel_err(gn.contract(J[u], s_c[v], s_d[v]), tau[v]) > 100 * hp.GRAD_TOL


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_run_to_run_view_groups_and_the_degenerate_window(joint):
    import torch

    w = _window(32, False)
    L = w.loss(False, True)
    a = w.jac_loss(L, irls_delta=0.03, solve_exposure=joint, want_jacobian=True, partials=_filled(w, joint))
    w.forward()
    b = w.jac_loss(L, irls_delta=0.03, solve_exposure=joint, want_jacobian=True, partials=_filled(w, joint))
    assert torch.equal(a["partials"], b["partials"]) and torch.equal(a["jacobian"], b["jacobian"]), "two runs: identical bits"
    # streams = 2: views (0, 1) and (2) as two calls on two streams -- view 2's group reads cov3D from ITS first block
    g = Window(32, False, streams=2)
    assert len(g.ctx.groups) == 2
    c = g.jac_loss(L, irls_delta=0.03, solve_exposure=joint, want_jacobian=True, partials=_filled(g, joint))
    torch.cuda.synchronize()
    assert torch.equal(a["partials"], c["partials"]) and torch.equal(a["jacobian"], c["jacobian"]), "the view groups change no bit"
    # K = 1: the batched entry point on a window of one view is view 0 of the window of three
    one = Window(32, False, K_=1)
    L1 = dict(L, gt_color=L["gt_color"][:1].contiguous(), gt_depth=L["gt_depth"][:1].contiguous(), grad_mask=L["grad_mask"][:H * W].contiguous(),
              exposure_a=w.E[:1, 0], exposure_b=w.E[:1, 1])
    d = one.jac_loss(L1, irls_delta=0.03, solve_exposure=joint, want_jacobian=True, partials=_filled(one, joint, 1))
    assert torch.equal(d["partials"][0], a["partials"][0]) and torch.equal(d["jacobian"][0], a["jacobian"][0])


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_one_aborted_view_keeps_its_rows_and_state_and_the_others_are_unaffected(joint):
    """The construction of tests/test_gpu_fused_batch.py: the arena holds one instance less than the largest view needs.  That
    view's rows keep the sentinel they were filled with and its state is not stepped; every other view equals an undisturbed run."""
    import torch
    from gsaj import _lib
    from gsaj.rasterizer import BatchContext

    w = _window(32, False)
    Rs = [s[0] for s in w.ctx.status()]
    big = int(np.argmax(Rs))
    assert sorted(Rs)[-1] > sorted(Rs)[-2], Rs
    L = w.loss(False, True)
    full = w.jac_loss(L, irls_delta=0.03, solve_exposure=joint, want_jacobian=True, partials=_filled(w, joint))
    b2 = BatchContext(K, w.ctx.P, W, H, 16, w.dev)
    b2._size(Rs[big] - 1)
    b2.tile_list_capacity = w.ctx.tile_list_capacity
    b2.auto_grow = False
    b2.forward(w.bg, w.means, w.opac, *w.views, *w.tan, sync=False, **w.kw)
    o = w.jac_loss(L, ctx=b2, irls_delta=0.03, solve_exposure=joint, partials=_filled(w, joint))
    st = b2.status()
    assert [s[2] for s in st] == [v == big for v in range(K)], (Rs, st)
    for v in range(K):
        if v == big:
            assert bool((o["partials"][v] == SENTINEL).all()), "the aborted view's rows are unchanged"
        else:
            assert torch.equal(o["partials"][v], full["partials"][v]), v
    # the batched step, handed the views' abort words: the aborted view's state is untouched bit for bit, the others are stepped as
    # in the undisturbed run
    n = 152 if joint else 136
    lib = w.ctx.lib
    step = lib.gsaj_pose_gn8_step_batch if joint else lib.gsaj_pose_gn_step_batch
    proj = w.praw.reshape(4, 4).contiguous()
    states = []
    for ctx, rows in ((w.ctx, full["partials"]), (b2, o["partials"])):
        s = torch.zeros((K, n), device=w.dev)
        for v in range(K):
            s[v, 0:16] = w.t(np.ascontiguousarray(w.cams[v]["viewmatrix"].T).reshape(16))
            s[v, 33:35] = w.E[v]
        start = s.clone()
        skip, stride = ctx.abort_flags()
        _lib.check(step(K, rows.data_ptr(), ROWS, None, 1e-3, 4.0, 1e-7, 1e7, 1e-4, proj.data_ptr(), s.data_ptr(), skip, stride,
                        torch.cuda.current_stream().cuda_stream), "step")
        states.append((start, s))
    (_, s_full), (start2, s2) = states
    for v in range(K):
        if v == big:
            assert torch.equal(s2[v], start2[v]) and not torch.equal(s_full[v], start2[v])
        else:
            assert torch.equal(s2[v], s_full[v]) and float(s2[v, 83]) == 1.0
    assert b2.clear_aborts() == 1


def test_argument_errors_raise():
    import torch
    from gsaj import _lib

    w = _window(32, False)
    L = w.loss(False, False)
    with pytest.raises(Exception, match="joint form"):
        w.jac_loss(dict(L, flags=L["flags"] | lr.NO_EXPOSURE), irls_delta=0.03, solve_exposure=True)
    with pytest.raises(Exception, match="joint form"):
        w.jac_loss(dict(L, flags=L["flags"] | lr.NO_EXPOSURE, exposure_a=None, exposure_b=None), irls_delta=0.03, solve_exposure=True)
    with pytest.raises(Exception, match="irls_delta"):
        w.jac_loss(L, irls_delta=-1.0)
    with pytest.raises(Exception, match="loss_batch"):
        w.jac_loss(dict(L, gt_depth=None), irls_delta=0.03)
    with pytest.raises(_lib.GsajError, match="64"):
        w.jac_loss(L, irls_delta=0.03, solve_exposure=True, partials=torch.zeros((K, ROWS, 32), device=w.dev))
    with pytest.raises(_lib.GsajError, match="must be device tensors"):
        w.ctx.pose_jacobian_loss(L, w.bg, w.means.cpu(), w.views[0], w.views[1], w.praw, w.views[2], *w.tan, **w.kw)
    with pytest.raises(_lib.GsajError, match="contiguous device tensor"):
        w.jac_loss(dict(L, gt_color=L["gt_color"].cpu()), irls_delta=0.03)
    # a tile band on any view
    band = Window(32, False)
    band.ctx.set_tile_band(0, 2, views=[1])
    with pytest.raises(_lib.GsajError, match="tile band"):
        band.jac_loss(L, irls_delta=0.03)
    band.ctx.set_tile_band(0, 3, views=[1])
    band.forward()
    assert tuple(band.jac_loss(L, irls_delta=0.03)["partials"].shape) == (K, ROWS, 32)
    # the 6-form accepts GSAJ_LOSS_NO_EXPOSURE
    assert w.jac_loss(dict(L, flags=L["flags"] | lr.NO_EXPOSURE, exposure_a=None, exposure_b=None), irls_delta=0.03)["partials"].shape == (K, ROWS, 32)
