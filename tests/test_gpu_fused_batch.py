"""GPU: the mapping loss fused into the BATCHED compositors (gsaj_rasterize_forward_loss_batch / _backward_loss_batch through
BatchContext.forward_loss / backward_loss): K views of one map, every view with its own ground truth, mask and exposure pair, so
that a pointer the kernels forget to move on by the view changes a result.  Against the unfused batched path
(forward -> LossSeedsBatch -> backward) every image and gradient is the same bits; the five scalars of every view hold the bound
of the single-view fused test against the float64 restatement (tests/loss_restated.py) and equal the single-view fused call's."""
import math

import numpy as np
import pytest

import helpers as hp
import loss_restated as lr
from gsaj import synthetic as syn
from test_gpu_device_tracker import FUSED_MODES

pytestmark = pytest.mark.gpu

K = 3
EA, EB = (0.07, -0.05, 0.11), (0.02, 0.03, -0.01)   # one exposure pair per view
ALPHA, THR = 0.9, 0.01


def _window(W, H, bg_rgb, P=300, n_ctx=2, streams=1):
    """The scene of test_gpu_device_tracker._fused_pair seen from K keyframe cameras; n_ctx BatchContexts with a sized arena."""
    import torch
    from gsaj.rasterizer import BatchContext

    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)  # noqa: E731
    f = 0.875 * W
    cams = syn.keyframe_cameras(K, radius=0.25, W=W, H=H, fx=f, fy=f, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(P, 11, cams[K // 2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    M = sc["shs"].shape[1]
    bg = t(np.array(bg_rgb, np.float32))
    views, projs, cps = (t(np.stack([c[k] for c in cams])) for k in ("viewmatrix", "projmatrix", "campos"))
    kw = dict(sh_degree=3, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    means, opac = t(sc["means3D"]), t(sc["opacities"])
    tx, ty = cams[0]["tanfovx"], cams[0]["tanfovy"]
    fwd = (bg, means, opac, views, projs, cps, tx, ty)
    bwd = (bg, means, views, projs, t(cams[0]["projmatrix_raw"]), cps, tx, ty)
    ctxs = [BatchContext(K, P, W, H, M, dev, per_gaussian_tau=True, streams=streams) for _ in range(n_ctx)]
    for c in ctxs:
        c.forward(*fwd, sync=True, **kw)
    return dev, t, ctxs, fwd, bwd, kw, (P, M)


def _truth(ctx, t, flags, masked, W, H):
    """Per-view ground truth on what the device rendered (loss_restated.gt_for_render, another seed per view), a mask per view, the
    float64 restatement per view, and the tensors the device calls take."""
    import torch

    color, depth, opacity = (x.cpu().numpy() for x in (ctx.color, ctx.depth, ctx.opacity))
    near = np.abs(opacity.astype(np.float64) - float(np.float32(0.95))) <= lr.OPACITY_ULPS * 2.0 ** -24
    assert not near.any(), "a rendered opacity within 4 ulp of 0.95"
    mono, noexp = bool(flags & 2), bool(flags & 4)
    masks = np.stack([np.random.default_rng(5 + k).choice(np.array([0, 1, 255], np.uint8), size=H * W, p=[0.3, 0.5, 0.2]) for k in range(K)])
    gts, wants, planted = [], [], set()
    for k in range(K):
        gtd = lr.gt_for_render(color[k], depth[k], flags, EA[k], EB[k], THR, seed=flags + 16 * masked + 100 * k)
        planted |= set(gtd["planted"])
        want = lr.restate(flags, ALPHA, THR, color[k], depth[k], opacity[k], gtd["gt"], gtd["gt_depth"], masks[k] if masked else None, EA[k], EB[k])
        lr.check_guards(gtd, "view %d flags %d" % (k, flags), want, gtd["zero_c"], gtd["zero_d"])
        gts.append(gtd)
        wants.append(want)
    gt_c = t(np.stack([g["gt"] for g in gts]))
    gt_d = None if mono else t(np.stack([g["gt_depth"] for g in gts]))
    mask = torch.as_tensor(masks.reshape(-1), device=ctx.dev) if masked else None
    ea, eb = (None, None) if noexp else (t(np.array(EA, np.float32)), t(np.array(EB, np.float32)))
    return dict(gt_c=gt_c, gt_d=gt_d, mask=mask, ea=ea, eb=eb, wants=wants, planted=planted)


def _unfused(a, ls, tr, flags, fwd, bwd, kw, split=False):
    import torch

    a.forward(*fwd, sync=False, **kw)
    L = ls(flags, ALPHA, THR, a.color, a.depth, a.opacity, tr["gt_c"], tr["gt_d"], tr["mask"], tr["ea"], tr["eb"])
    ga = a.backward(*bwd, L["dL_dcolor"], L["dL_ddepth"], split=split, **kw)
    return {n: x.clone() for n, x in ga.items() if torch.is_tensor(x)}, ls.scalars.clone()


def _fused(b, tr, flags, fwd, bwd, kw, split=False, ea=None, eb=None, stride=1, sentinel=0.0):
    import torch

    scalars, dexp = torch.full((K, 5), sentinel, device=b.dev), torch.full((K, 2), sentinel, device=b.dev)
    FL = dict(flags=flags, alpha=ALPHA, rgb_boundary_threshold=THR, gt_color=tr["gt_c"], gt_depth=tr["gt_d"], grad_mask=tr["mask"],
              exposure_a=tr["ea"] if ea is None else ea, exposure_b=tr["eb"] if eb is None else eb, exposure_stride=stride,
              scalars=scalars, dexposure=dexp)
    b.forward_loss(FL, *fwd, **kw)
    gb = b.backward_loss(FL, *bwd, split=split, **kw)
    return {n: x.clone() for n, x in gb.items() if torch.is_tensor(x)}, scalars, dexp


def _same_images(a, b, tag):
    import torch

    for n in ("color", "depth", "opacity", "n_touched", "radii"):
        assert torch.equal(getattr(a, n), getattr(b, n)), "%s: %s differs" % (tag, n)


def _same_grads(ga, gb, tag):
    import torch

    assert set(ga) == set(gb) and {"mean2D", "tau_all", "tau", "mean3D", "opacity", "sh", "scale", "rot"} <= set(ga), sorted(ga)
    for n, x in ga.items():
        assert torch.equal(gb[n], x), "%s: dL/d%s of the fused path differs from the unfused path" % (tag, n)


def _scalars_close(scalars, wants, tag):
    got = scalars.cpu().numpy()
    worst = {}
    for k in range(K):
        r = lr.assert_loss_close(dict(zip(lr.SCALARS, got[k])), wants[k], "%s view %d" % (tag, k), lr.SCALARS)
        worst = {n: max(worst.get(n, 0.0), v) for n, v in r.items()}
    return worst


@pytest.mark.parametrize("W,H,bg_rgb", [(37, 29, (0, 0, 0)), (37, 29, (0.1, 0.2, 0.3)), (160, 120, (0, 0, 0)), (160, 120, (0.1, 0.2, 0.3))])
def test_batched_fused_equals_unfused_bit_for_bit_in_every_mode(W, H, bg_rgb):
    """Every flag combination the compositors accept, on 37x29 (6 tiles: workgroups with rank >= tiles exist in every view and own
    partial slots; ragged right and bottom edges) and 160x120, zero and non-zero background.  Images, n_touched and every tensor of g
    (bucket fields, mean2D, tau_all, per-Gaussian tau) are the unfused path's bits; each view's five scalars are within
    SUM_K eps sum|term| + eps |value| of the float64 restatement on that view's rendered images (loss_restated.assert_loss_close: the
    single-view fused test's bound); dexposure is columns 3:5 of the scalars."""
    import torch
    from gsaj.losses import LossSeedsBatch

    dev, t, (a, b), fwd, bwd, kw, _ = _window(W, H, bg_rgb)
    ls = LossSeedsBatch(K, W, H, dev)
    reached = set()
    for flags, masked in FUSED_MODES:
        tag = "%dx%d bg %s flags %d%s" % (W, H, bg_rgb, flags, " masked" if masked else "")
        a.forward(*fwd, sync=False, **kw)
        tr = _truth(a, t, flags, masked, W, H)
        reached |= tr["planted"]
        ga, sa = _unfused(a, ls, tr, flags, fwd, bwd, kw)
        assert all(float(ga["tau_all"][k].abs().max()) > 0.0 for k in range(K)), tag
        _scalars_close(sa, tr["wants"], tag + " (gsaj_loss_seeds_batch)")
        gb, sb, dexp = _fused(b, tr, flags, fwd, bwd, kw)
        _same_images(a, b, tag)
        _same_grads(ga, gb, tag)
        worst = _scalars_close(sb, tr["wants"], tag + " (fused)")
        print(tag, {n: round(v, 4) for n, v in worst.items()})
        assert torch.equal(dexp, sb[:, 3:5]), tag
    assert {"rgb_thr", "gt_depth", "zero_depth", "zero_color"} <= reached, reached
    assert not any(ab for _, _, ab in b.status())


@pytest.mark.parametrize("W,H", [(37, 29), (160, 120)])
@pytest.mark.parametrize("flags,masked", [(0, False), (1, True), (2, False)])
def test_batch_row_equals_the_single_view_fused_call(W, H, flags, masked):
    """Row k of the batch is view k through gsaj_rasterize_forward_loss on its own: same partial grid, same summation order, so the
    five scalars are the same bits.  The exposures once as contiguous [K] tensors and once as columns 33 / 34 of a [K,80] tensor
    read in place (exposure_stride = 80, PoseTrackerBatch.state): identical results."""
    import torch
    from gsaj.rasterizer import FrameContext

    dev, t, (a, b), fwd, bwd, kw, (P, M) = _window(W, H, (0.1, 0.2, 0.3))
    a.forward(*fwd, sync=False, **kw)
    tr = _truth(a, t, flags, masked, W, H)
    g1, s1, d1 = _fused(b, tr, flags, fwd, bwd, kw)
    state = torch.full((K, 80), 123.0, device=dev)
    state[:, 33], state[:, 34] = tr["ea"], tr["eb"]
    g2, s2, d2 = _fused(b, tr, flags, fwd, bwd, kw, ea=state[:, 33], eb=state[:, 34], stride=80)
    assert torch.equal(s1, s2) and torch.equal(d1, d2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    bg, means, opac, views, projs, cps, tx, ty = fwd
    for k in range(K):
        fc = FrameContext(P, W, H, M, dev)
        fc.forward(bg, means, opac, views[k], projs[k], cps[k], tx, ty, sync=True, **kw)
        one = torch.zeros(5, device=dev)
        FL = dict(flags=flags, alpha=ALPHA, rgb_boundary_threshold=THR, gt_color=tr["gt_c"][k], gt_depth=None if tr["gt_d"] is None else tr["gt_d"][k],
                  grad_mask=None if tr["mask"] is None else tr["mask"].view(K, -1)[k], exposure_a=tr["ea"][k:k + 1], exposure_b=tr["eb"][k:k + 1],
                  scalars=one)
        fc.forward_loss(FL, bg, means, opac, views[k], projs[k], cps[k], tx, ty, **kw)
        assert torch.equal(fc.color, b.color[k])
        assert torch.equal(one, s1[k]), (k, one.tolist(), s1[k].tolist())


def test_batched_fused_forward_is_not_reached_by_stale_partials():
    """test_fused_forward_is_not_reached_by_stale_partials per view: 37x29 launches 32 workgroups per view for 8 tile ranks of which 6
    are tiles; after a window with large loss terms the WHOLE workspace is overwritten with 1e6, then a window with small losses on
    the same context must meet the bound in every view -- a view's idle workgroups zero their own view's slots."""
    import torch

    W, H = 37, 29
    dev, t, (a, b), fwd, bwd, kw, _ = _window(W, H, (0, 0, 0))
    a.forward(*fwd, sync=False, **kw)
    color, depth, opacity = (x.cpu().numpy() for x in (a.color, a.depth, a.opacity))
    rng = np.random.default_rng(9)
    fm = np.stack([float(np.exp(np.float64(np.float32(EA[k])))) * color[k].astype(np.float64) + float(np.float32(EB[k])) for k in range(K)])
    frames = [((fm + 100.0).astype(np.float32), (depth[:, 0] + np.float32(50.0)).astype(np.float32)),
              ((fm + rng.choice([-1.0, 1.0], fm.shape) * 1e-3).astype(np.float32),
               (depth[:, 0] + rng.choice([-1.0, 1.0], depth[:, 0].shape) * 1e-3).astype(np.float32))]
    values = []
    for i, (gt, gtd) in enumerate(frames):
        wants = [lr.restate(0, ALPHA, THR, color[k], depth[k], opacity[k], gt[k], gtd[k], None, EA[k], EB[k]) for k in range(K)]
        for k in range(K):
            lr.check_guards(dict(gt_depth=gtd[k]), "frame %d view %d" % (i, k), wants[k], np.zeros((3, H * W), bool), np.zeros(H * W, bool))
        tr = dict(gt_c=t(gt), gt_d=t(gtd), mask=None, ea=t(np.array(EA, np.float32)), eb=t(np.array(EB, np.float32)))
        _, scalars, _ = _fused(b, tr, 0, fwd, bwd, kw)
        _scalars_close(scalars, wants, "frame %d" % i)
        values.append([w["value"]["loss"] for w in wants])
        n = b.loss_ws.numel() // 4 * 4
        b.loss_ws[:n].view(torch.float32).fill_(1e6)   # what another window, or another owner of the memory, could have left
    assert all(values[0][k] > 1e4 * values[1][k] > 0 for k in range(K))


def _abort_scene():
    """The smallest scene of tests/helpers whose K = 4 keyframe views differ by more than 8 instances between the largest and the
    smallest view: (cams, sc, deg, per-view instance counts)."""
    import torch
    from gsaj.rasterizer import BatchContext

    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)  # noqa: E731
    for name in sorted(hp.SCENES, key=lambda n: hp.SCENES[n]["P"] * hp.SCENES[n]["W"] * hp.SCENES[n]["H"]):
        cam0, sc, deg = hp.make(name)
        cams = syn.keyframe_cameras(4, W=cam0["W"], H=cam0["H"], fx=cam0["fx"], fy=cam0["fy"], cx=cam0["cx"], cy=cam0["cy"])
        P, M = sc["means3D"].shape[0], sc["shs"].shape[1]
        bc = BatchContext(4, P, cam0["W"], cam0["H"], M, dev)
        views, projs, cps = (t(np.stack([c[k] for c in cams])) for k in ("viewmatrix", "projmatrix", "campos"))
        kw = dict(sh_degree=deg, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
        fwd = (t(np.array([0.1, 0.2, 0.3])), t(sc["means3D"]), t(sc["opacities"]), views, projs, cps, cam0["tanfovx"], cam0["tanfovy"])
        bwd = (fwd[0], fwd[1], views, projs, t(cams[0]["projmatrix_raw"]), cps, cam0["tanfovx"], cam0["tanfovy"])
        Rs = [s[0] for s in bc.forward(*fwd, sync=True, **kw)]
        if max(Rs) > min(Rs) + 8:
            return name, bc, fwd, bwd, kw, Rs, (P, M, cam0["W"], cam0["H"])
    raise AssertionError("no scene of tests/helpers has views that differ by more than 8 instances")


def test_one_aborted_view_keeps_its_rows_and_the_others_are_unaffected():
    """The construction of test_gpu_batch.py::test_batch_aborted_view_contributes_nothing_and_is_reported through the fused calls: the
    arena holds one instance less than the largest view needs.  That view's rows of scalars / dexposure keep the sentinel they were
    filled with, its dL/dtau row is zero and status() reports it; every other view's rows are those of a window in which everything
    fits, bit for bit."""
    import torch
    from gsaj.rasterizer import BatchContext

    name, full, fwd, bwd, kw, Rs, (P, M, W, H) = _abort_scene()
    Kv, dev = 4, full.dev
    big = int(np.argmax(Rs))
    gen = torch.Generator(device=dev).manual_seed(3)
    tr = dict(gt_c=(full.color + 0.05 * torch.randn(full.color.shape, generator=gen, device=dev)).contiguous(),
              gt_d=(full.depth[:, 0] + 0.05 * torch.randn(full.depth[:, 0].shape, generator=gen, device=dev)).contiguous(), mask=None,
              ea=torch.tensor([0.07, -0.05, 0.11, 0.0], device=dev), eb=torch.tensor([0.02, 0.03, -0.01, 0.01], device=dev))

    def run(ctx, sentinel):
        scalars, dexp = torch.full((Kv, 5), sentinel, device=dev), torch.full((Kv, 2), sentinel, device=dev)
        FL = dict(flags=0, alpha=ALPHA, rgb_boundary_threshold=THR, gt_color=tr["gt_c"], gt_depth=tr["gt_d"], grad_mask=None, exposure_a=tr["ea"],
                  exposure_b=tr["eb"], scalars=scalars, dexposure=dexp)
        ctx.forward_loss(FL, *fwd, **kw)
        g = ctx.backward_loss(FL, *bwd, **kw)
        return scalars, dexp, g["tau_all"].clone()

    s_full, d_full, tau_full = run(full, 0.0)
    assert not any(ab for _, _, ab in full.status())
    b2 = BatchContext(Kv, P, W, H, M, dev)
    b2._size(Rs[big] - 1)  # every view but the largest fits
    b2.tile_list_capacity = full.tile_list_capacity
    s2, d2, tau2 = run(b2, -7.0)
    st2 = b2.status()
    fits = [r <= Rs[big] - 1 for r in Rs]
    assert not all(fits) and fits.count(True) >= 1 and [s[2] for s in st2] == [not f for f in fits] and st2[big][0] == Rs[big], (name, Rs, st2)
    for k in range(Kv):
        if fits[k]:
            assert torch.equal(s2[k], s_full[k]) and torch.equal(d2[k], d_full[k]) and torch.equal(tau2[k], tau_full[k]), (name, k)
            assert torch.equal(b2.color[k], full.color[k])
        else:
            assert bool((s2[k] == -7.0).all()) and bool((d2[k] == -7.0).all()), (name, k, s2[k].tolist())
            assert float(tau2[k].abs().max()) == 0.0
    assert b2.clear_aborts() == fits.count(False)


@pytest.mark.parametrize("streams,split", [(2, False), (1, True)])
@pytest.mark.parametrize("flags,masked", [(0, False), (1, True), (2 | 4, False)])
def test_view_groups_and_split_backward_fused_equal_unfused(streams, split, flags, masked):
    """streams=2 (two view groups, every loss pointer moved on to the group's first view) and split=True (the two halves of the
    backward as two calls; the chain half ignores the loss arguments): the fused results are the unfused results of the same
    configuration, bit for bit."""
    import torch
    from gsaj.losses import LossSeedsBatch

    W, H = 37, 29
    dev, t, (a, b), fwd, bwd, kw, _ = _window(W, H, (0.1, 0.2, 0.3), streams=streams)
    assert len(a.groups) == streams
    a.forward(*fwd, sync=False, **kw)
    tr = _truth(a, t, flags, masked, W, H)
    ga, sa = _unfused(a, LossSeedsBatch(K, W, H, dev), tr, flags, fwd, bwd, kw, split=split)
    gb, sb, dexp = _fused(b, tr, flags, fwd, bwd, kw, split=split)
    tag = "streams %d split %s flags %d" % (streams, split, flags)
    _same_images(a, b, tag)
    _same_grads(ga, gb, tag)
    _scalars_close(sb, tr["wants"], tag)
    assert torch.equal(dexp, sb[:, 3:5])


def test_two_fused_runs_are_bit_identical():
    import torch

    W, H = 160, 120
    dev, t, (a, b), fwd, bwd, kw, _ = _window(W, H, (0.1, 0.2, 0.3))
    a.forward(*fwd, sync=False, **kw)
    tr = _truth(a, t, 0, False, W, H)
    g1, s1, d1 = _fused(a, tr, 0, fwd, bwd, kw)
    g2, s2, d2 = _fused(b, tr, 0, fwd, bwd, kw)
    g3, s3, d3 = _fused(b, tr, 0, fwd, bwd, kw)
    for g, s, d in ((g2, s2, d2), (g3, s3, d3)):
        assert torch.equal(s, s1) and torch.equal(d, d1)
        for n in g1:
            assert torch.equal(g[n], g1[n]), n
    _same_images(a, b, "two runs")
