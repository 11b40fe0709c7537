"""GPU: gsaj.mapping.DeviceMapper -- the mapping loop of a keyframe window (reference utils/slam_backend.py:142-318) kept on the
device.  The world is tests/test_gpu_track_and_map.py's: a true map of 3000 Gaussians seen from 4 keyframes, ground truth rendered
from it, and a disturbed copy of the map to refine.  Two window keyframes (the second one has uid 0) and two extra keyframes:
only slot 0's pose is optimised."""
import types

import numpy as np
import pytest

from test_gpu_track_and_map import H, W, _true_world

pytestmark = pytest.mark.gpu

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1e-3, position_lr_final=1e-3, position_lr_delay_mult=1.0,
                             position_lr_max_steps=30000, feature_lr=5e-3, opacity_lr=2e-2, scaling_lr=2e-3, rotation_lr=1e-3)
N_WINDOW, UIDS, POSE_WINDOW = 2, (4, 0, 7, 9), 3
ALPHA, THR, ISO = 0.95, 0.01, 10.0
_WORLD = []


def _world():
    if not _WORLD:  # rendered once, shared, never written
        _WORLD.append(_true_world())
    return _WORLD[0]


def _model():
    """The true map disturbed (the existing window test's disturbance and learning rates), as a GaussianModel with training_setup."""
    import torch
    from gaussian_splatting.scene.gaussian_model import GaussianModel

    dev, t, cams, sc, g, bg, M, frames = _world()
    P = g["means3D"].shape[0]
    rng = np.random.default_rng(5)
    shs = g["shs"] + t(rng.normal(scale=0.05, size=tuple(g["shs"].shape)))
    m = GaussianModel(3)
    m._set_params(g["means3D"] + t(rng.normal(scale=0.01, size=(P, 3))), shs[:, :1], shs[:, 1:],
                  torch.logit(g["opacities"].clamp(0.02, 0.98)) + t(rng.normal(scale=0.3, size=(P, 1))),
                  torch.log(g["scales"]) + t(rng.normal(scale=0.05, size=(P, 3))), g["rotations"] + t(rng.normal(scale=0.01, size=(P, 4))), dev)
    m.active_sh_degree = 3
    m.init_lr(1.0)
    m.training_setup(ARGS)
    for group in m.optimizer.param_groups:  # (training_setup gives f_rest feature_lr / 20; the existing test steps all of SH alike)
        if group["name"] == "f_rest":
            group["lr"] = ARGS.feature_lr
    return m


def _pose_kw(lr_exp):
    return dict(lr_rot=0.001, lr_trans=0.001, lr_exposure_a=lr_exp, lr_exposure_b=lr_exp)


def _mapper(model, fused, lr_exp=0.0, **kw):
    from gsaj.mapping import DeviceMapper

    dev, t, cams, sc, g, bg, M, frames = _world()
    w2cs = [np.ascontiguousarray(c["viewmatrix"].T).astype(np.float32) for c in cams]
    mp = DeviceMapper(model, len(cams), W, H, t(cams[0]["projmatrix_raw"]), cams[0]["tanfovx"], cams[0]["tanfovy"], bg, w2cs=w2cs,
                      n_window=N_WINDOW, uids=UIDS, pose_window=POSE_WINDOW, alpha=ALPHA, rgb_boundary_threshold=THR, isotropic_weight=ISO,
                      fused=fused, **_pose_kw(lr_exp), **kw)
    for k, (c, d) in enumerate(frames):
        mp.set_view(k, c, d)
    return mp


def _state(model, poses):
    """Everything an iteration changes: raw parameters, Adam moments, densification statistics, the K poses."""
    out = {n: p.detach().clone() for n, p in zip(NAMES, model.parameters())}
    for n, p in zip(NAMES, model.parameters()):
        st = model.optimizer.state[p]
        out["m_" + n], out["v_" + n], out["step_" + n] = st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone()
    for n in ("xyz_gradient_accum", "denom", "max_radii2D", "n_obs"):
        out[n] = getattr(model, n).clone()
    out["w2c"], out["exposure"] = poses.w2c.clone(), poses.exposure.clone()
    return out


def _by_hand(model, n, lr_exp=0.0):
    """The unfused iteration written out call by call (module docstring of gsaj.mapping, steps 1-8)."""
    import torch
    from gsaj.losses import IsotropicLoss, LossSeedsBatch
    from gsaj.pose_step import PoseTrackerBatch
    from gsaj.rasterizer import BatchContext

    dev, t, cams, sc, g, bg, M, frames = _world()
    K, P = len(cams), model.get_xyz.shape[0]
    praw = t(cams[0]["projmatrix_raw"])
    tx, ty = cams[0]["tanfovx"], cams[0]["tanfovy"]
    poses = PoseTrackerBatch([np.ascontiguousarray(c["viewmatrix"].T).astype(np.float32) for c in cams], praw, dev, **_pose_kw(lr_exp))
    active = torch.tensor([1 if s < min(POSE_WINDOW, N_WINDOW) and UIDS[s] != 0 else 0 for s in range(K)], dtype=torch.uint8, device=dev)
    bc, ls, iso = BatchContext(K, P, W, H, M, dev), LossSeedsBatch(K, W, H, dev), IsotropicLoss(P, dev)
    gt_color, gt_depth = torch.stack([f[0] for f in frames]).contiguous(), torch.stack([f[1] for f in frames]).contiguous()
    for it in range(n):
        with torch.no_grad():
            xyz, opac = model.get_xyz.detach().contiguous(), model.get_opacity.contiguous()
            geo = dict(sh_degree=3, shs=model.get_features.contiguous(), scales=model.get_scaling.contiguous(), rotations=model.get_rotation.contiguous())
        views, projs, cps = poses.matrices()
        bc.forward(bg, xyz, opac, views, projs, cps, tx, ty, sync=(it == 0), **geo)
        o = ls(0, ALPHA, THR, bc.color, bc.depth, bc.opacity, gt_color, gt_depth, None, poses.exposure[:, 0].contiguous(), poses.exposure[:, 1].contiguous())
        gr = bc.backward(bg, xyz, views, projs, praw, cps, tx, ty, o["dL_dcolor"], o["dL_ddepth"], **geo)
        iso(geo["scales"], ISO, grad_out=gr["scale"], accumulate=True)
        model.densification_step(gr["mean2D"][:N_WINDOW], bc.radii[:N_WINDOW], bc.n_touched[:N_WINDOW])
        model.densification_step(gr["mean2D"][N_WINDOW:], bc.radii[N_WINDOW:], None)
        skip, stride = bc.abort_flags()
        poses.step(gr["tau_all"], ls.scalars[:, 3:5].contiguous(), active, skip=skip, skip_stride=stride)
        model.map_step(gr, reset=None, radii=bc.radii)
        model.update_learning_rate(it + 1)
    assert bc.clear_aborts() == 0
    return poses


def test_fused_and_unfused_mappers_and_the_loop_by_hand_agree():
    """10 iterations.  Exposure learning rates 0: the fused mapper, the unfused mapper and the unfused sequence written out by hand
    leave the same bits in the six raw parameters, every Adam moment, xyz_gradient_accum / denom / max_radii2D / n_obs and the K
    poses -- the per-pixel loss arithmetic is one definition, and the mapper adds nothing of its own to the sequence.  Exposure
    learning rates 0.01: dL/d(exposure) is a sum of pixel terms in another order in the fused form, so poses and parameters agree to
    the 1e-6 of test_fused_tracker_follows_the_unfused_tracker_bit_for_bit; the hand-written loop still equals fused=False bit for bit."""
    import torch

    res = {}
    for lr_exp in (0.0, 0.01):
        for kind in ("fused", "unfused", "hand"):
            m = _model()
            if kind == "hand":
                poses = _by_hand(m, 10, lr_exp)
            else:
                mp = _mapper(m, kind == "fused", lr_exp)
                assert mp.iterate(10) == 10
                poses = mp.poses
                assert float(mp.window_loss) > 0.0 and tuple(mp.losses.shape) == (4, 5) and tuple(mp.n_touched.shape) == (4, m.get_xyz.shape[0])
            res[kind, lr_exp] = _state(m, poses)
    for lr_exp in (0.0, 0.01):
        for n, x in res["unfused", lr_exp].items():
            assert torch.equal(res["hand", lr_exp][n], x), "lr_exposure %g: %s of the loop by hand differs from DeviceMapper(fused=False)" % (lr_exp, n)
    for n, x in res["unfused", 0.0].items():
        assert torch.equal(res["fused", 0.0][n], x), "%s of the fused mapper differs from the unfused mapper" % n
    assert 0 < float(res["unfused", 0.0]["n_obs"].max()) <= N_WINDOW and float(res["unfused", 0.0]["denom"].max()) > N_WINDOW * 10
    for n in NAMES + ("w2c", "exposure"):
        d = float((res["fused", 0.01][n] - res["unfused", 0.01][n]).abs().max())
        print("lr_exposure 0.01: max |fused - unfused| of %s = %.3g" % (n, d))
        assert d < 1e-6, (n, d)
    assert float(res["fused", 0.01]["exposure"][0].abs().max()) > 0.0  # (the active view's exposure was learned)


def test_window_loss_falls_and_only_the_active_pose_moves():
    """40 iterations on the disturbed map: the window loss falls below 0.6 of its start (the figure of
    test_mapping_window_lowers_its_loss_with_adam_on_the_bucket_gradients for this scene); the keyframe with uid 0 (slot 1) and the
    two extra views (slots 2, 3) keep their poses and exposures bit for bit, the active pose (slot 0) moves."""
    import torch

    m = _model()
    mp = _mapper(m, True, 0.01)
    before, exp0 = mp.w2c.clone(), mp.exposure.clone()
    mp.iterate(1)
    first = float(mp.window_loss)
    mp.iterate(39)
    last = float(mp.window_loss)
    print("window loss %.6f -> %.6f" % (first, last))
    assert last < 0.6 * first, (first, last)
    assert mp.active.tolist() == [1, 0, 0, 0]
    for k in (1, 2, 3):
        assert torch.equal(mp.w2c[k], before[k]) and torch.equal(mp.exposure[k], exp0[k]), k
    assert not torch.equal(mp.w2c[0], before[0])
    w = mp.w2c[0].cpu().numpy()
    assert np.allclose(w[:3, :3] @ w[:3, :3].T, np.eye(3), atol=1e-4)
    assert mp.iteration_count == 40


def test_opacity_reset_through_the_mapper_keeps_map_steps_contract():
    """An iteration with reset="nonvisible": the opacity group is not stepped -- its step count stays, its moments are zeros -- while
    the other groups step as usual (GaussianModel.map_step's contract seen through the mapper)."""
    m = _model()
    mp = _mapper(m, True)
    mp.iterate(3)
    prm = dict(zip(NAMES, m.parameters()))
    steps = {n: float(m.optimizer.state[prm[n]]["step"]) for n in NAMES}
    assert set(steps.values()) == {3.0}
    mp.iterate(1, reset="nonvisible")
    prm = dict(zip(NAMES, m.parameters()))  # (the reset installs a new opacity leaf)
    st = m.optimizer.state[prm["opacity"]]
    assert float(st["step"]) == 3.0
    assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0
    for n in NAMES:
        if n != "opacity":
            assert float(m.optimizer.state[prm[n]]["step"]) == 4.0, n
    mp.iterate(1)
    assert float(m.optimizer.state[dict(zip(NAMES, m.parameters()))["opacity"]]["step"]) == 4.0


@pytest.mark.parametrize("fused", [True, False])
def test_iterations_after_the_first_read_nothing_back(fused):
    """After the iteration that sizes the arena, iterations run under torch's sync debug mode "error": no torch operation of the loop
    synchronises with the host.  The rasteriser launches of one iteration (gsaj_profile_begin / _end) are the same in both forms --
    the fused form drops the loss launch and adds the finalize, neither of which is a rasteriser stage."""
    import torch
    from gsaj.rasterizer import profile_stages

    m = _model()
    mp = _mapper(m, fused)
    mp.iterate(1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert mp.iterate(4) == 4
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with profile_stages() as ps:
        mp.iterate(1)
        torch.cuda.synchronize()
    n = {k: v for k, v in ps.launches.items() if v}
    print("fused=%s: rasteriser launches of one iteration: %d %r" % (fused, sum(n.values()), n))
    assert n.get("render_fwd") == 1 and n.get("render_bwd") == 1, n


def test_a_resized_model_needs_refresh():
    from gsaj import _lib

    m = _model()
    mp = _mapper(m, True)
    mp.iterate(5)
    P0 = m.get_xyz.shape[0]
    m.densify_and_prune(1e-7, 0.005, 6.0, 20, seed=1)
    assert m.get_xyz.shape[0] != P0, "the densification was meant to change the number of Gaussians"
    with pytest.raises(_lib.GsajError, match="refresh"):
        mp.iterate(1)
    mp.refresh()
    assert mp.iterate(3) == 3 and mp.P == m.get_xyz.shape[0]
    assert tuple(mp.n_touched.shape) == (4, m.get_xyz.shape[0])
