"""CPU: the NumPy restatement of the keyframe seeding path (tests/seed_restated.py) against outputs recorded from the reference
(tests/golden/median_depth_*.npz, seed_scalars.npz; make_seed_goldens.py), its own invariants (selection, uniformity,
back-projection round trip), and GaussianModel.extend_from_pcd on CPU tensors.  No kernel is launched."""
import glob
import os

import numpy as np
import pytest
import torch

import seed_restated as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("median_depth_"):-4] for p in glob.glob(os.path.join(GOLDEN, "median_depth_*.npz")))
ULP32 = 2.0 ** -23


def load_case(name):
    z = np.load(os.path.join(GOLDEN, "median_depth_%s.npz" % name))
    return z, (z["opacity"] if bool(z["use_opacity"]) else None), (z["mask"] if bool(z["use_mask"]) else None)


def test_fixtures_cover_odd_and_even_counts_with_and_without_opacity_and_mask():
    assert len(CASES) >= 7
    seen = set()
    for name in CASES:
        z, o, m = load_case(name)
        seen.add((o is not None, m is not None, int(z["n_valid"]) % 2))
    assert {(False, False, 0), (False, False, 1), (True, False, 0), (True, False, 1), (True, True, 0), (True, True, 1)} <= seen


@pytest.mark.parametrize("name", CASES)
def test_restated_median_depth_reproduces_the_reference(name):
    z, o, m = load_case(name)
    med, std, valid, n = sr.median_depth(z["depth"], o, m)
    assert n == int(z["n_valid"]) and np.array_equal(valid, z["valid"])
    assert med.dtype == np.float32 and med.tobytes() == z["median"].tobytes()  # bit-exact: an order statistic
    # both sides sum in fp64 (n ~ 10^2..10^3 terms: ~n 2^-53 relative) and round once to fp32: at most one fp32 ulp apart
    assert abs(float(np.float32(std)) - float(z["std"])) <= ULP32 * float(z["std"])


@pytest.mark.parametrize("name", CASES)
def test_overlay_get_median_depth_on_cpu_tensors(name):
    from utils.slam_utils import get_median_depth

    z, o, m = load_case(name)
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    med, std, valid = get_median_depth(t(z["depth"]), t(o), t(m), return_std=True)
    assert med.numpy().tobytes() == z["median"].tobytes() and std.numpy().tobytes() == z["std"].tobytes()
    assert np.array_equal(valid.numpy(), z["valid"])
    assert get_median_depth(t(z["depth"]), t(o), t(m)).numpy().tobytes() == z["median"].tobytes()


def test_restated_rgb2sh_and_inverse_sigmoid_against_the_reference():
    z = np.load(os.path.join(GOLDEN, "seed_scalars.npz"))
    q = np.arange(256, dtype=np.uint8)
    assert np.array_equal((q.astype(np.float64) / 255.0).astype(np.float32), z["rgb"])
    # (rgb - 0.5) / C0: a correctly rounded quotient here; a tensor library may multiply by the rounded reciprocal instead
    # (half an ulp for the reciprocal + half for the product + half for the quotient it is compared with): 2 ulp
    got, want = sr.rgb2sh(q), z["rgb2sh"]
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2 * ULP32 * np.abs(want))
    assert z["inverse_sigmoid"][0] == 0.0  # inverse_sigmoid(0.5): the initial opacity parameter is exactly 0


def _valid_image(H, W, frac, rng):
    return rng.uniform(size=(H, W)) < frac


def test_selection_is_an_exact_sorted_unique_subset_of_the_valid_pixels():
    rng = np.random.default_rng(1)
    valid = _valid_image(48, 64, 0.8, rng)
    nv = int(valid.sum())
    sets = {}
    for factor in (1, 2, 4, 32, 64, 2.5):
        for seed in (0, 1, 7):
            idx, n = sr.select(valid, factor, seed)
            assert n == nv and idx.size == int(nv * (1.0 / factor))
            assert np.all(np.diff(idx) > 0) and valid.reshape(-1)[idx].all()
            sets[(factor, seed)] = idx
    assert np.array_equal(sets[(1, 0)], np.flatnonzero(valid.reshape(-1)))  # factor 1 keeps everything
    assert not np.array_equal(sets[(4, 0)], sets[(4, 1)]) and not np.array_equal(sets[(4, 1)], sets[(4, 7)])
    few = np.zeros((48, 64), bool)
    few.reshape(-1)[[5, 77, 900]] = True
    idx, n = sr.select(few, 4, 0)  # n_valid < factor: nothing
    assert n == 3 and idx.size == 0
    idx, n = sr.select(np.zeros((4, 4), bool), 1, 0)
    assert n == 0 and idx.size == 0


def test_pixel_keys_are_a_bijection():
    for seed in (0, 1, 12345, 2 ** 32 - 1):
        k = sr.pixel_keys(1280 * 720, seed)
        assert np.unique(k).size == k.size and int(k.max()) < 2 ** 32
    assert not np.array_equal(sr.pixel_keys(1000, 0), sr.pixel_keys(1000, 1))


def test_selection_is_spatially_uniform():
    """Per-block counts on an 8 x 8 grid at 640 x 480, 80 % valid: given a block's number of valid pixels the count of a uniform
    m-subset is hypergeometric; the largest standardised deviation over blocks, seeds 0-4 and factors 4-128 stays below 5 (a
    degenerate key mix -- stripes, clusters -- gives tens).  Measured with this restatement: 3.26."""
    H, W = 480, 640
    valid = _valid_image(H, W, 0.8, np.random.default_rng(0))
    N = int(valid.sum())
    blocks = (np.arange(H)[:, None] // 60) * 8 + (np.arange(W)[None, :] // 80)
    K = np.bincount(blocks[valid], minlength=64).astype(np.float64)
    worst = 0.0
    for factor in (4, 32, 64, 128):
        for seed in range(5):
            idx, _ = sr.select(valid, factor, seed)
            m = idx.size
            got = np.bincount(blocks.reshape(-1)[idx], minlength=64)
            mean = m * K / N
            var = m * (K / N) * (1 - K / N) * (N - m) / (N - 1)
            worst = max(worst, float(np.abs((got - mean) / np.sqrt(var)).max()))
    print("largest standardised deviation of a block count: %.2f" % worst)
    assert worst <= 5.0


@pytest.mark.parametrize("orthonormal", [True, False])
def test_backprojection_round_trip(orthonormal):
    """Projecting the fp32-rounded restated world points through W2C and the intrinsics in fp64 returns (u, v, d) up to what the
    rounding of the stored point allows: a coordinate error of 2^-24 |p_c| moves the camera-space point by at most
    e_r = sum_c |W2C_rc| 2^-24 |p_c|, the depth by e_z and the pixel by fx / z (e_x + |x / z| e_z)."""
    from gsaj import synthetic as syn

    W, H = 160, 120
    cam = syn.fixture_camera(noisy=True, orthonormal=orthonormal, W=W, H=H, fx=140.0, fy=139.0, cx=79.5, cy=59.5)
    rng = np.random.default_rng(3)
    depth = rng.uniform(0.5, 6.0, (H, W)).astype(np.float32)
    pix = np.sort(rng.choice(W * H, 4000, replace=False))
    w2c32 = cam["w2c"].astype(np.float32)
    pw = sr.backproject(depth, pix, W, w2c32, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    stored = pw.astype(np.float32).astype(np.float64)
    A = w2c32.astype(np.float64)
    pc = stored @ A[:3, :3].T + A[:3, 3]
    e = (2.0 ** -24 * np.abs(stored)) @ np.abs(A[:3, :3]).T
    u, v, d = pix % W, pix // W, depth.reshape(-1)[pix].astype(np.float64)
    slack = 1.0 + 1e-6
    assert np.all(np.abs(pc[:, 2] - d) <= e[:, 2] * slack + 1e-12)
    eu = cam["fx"] / pc[:, 2] * (e[:, 0] + np.abs(pc[:, 0] / pc[:, 2]) * e[:, 2])
    ev = cam["fy"] / pc[:, 2] * (e[:, 1] + np.abs(pc[:, 1] / pc[:, 2]) * e[:, 2])
    assert np.all(np.abs(cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"] - u) <= eu * slack + 1e-9)
    assert np.all(np.abs(cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"] - v) <= ev * slack + 1e-9)
    assert float(np.abs(pc[:, 2] - d).max()) > 0  # (the rounding is there: the check is not vacuous)


def _cpu_model(n, M, with_optimizer):
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj import synthetic as syn

    cam = syn.fixture_camera()
    sc = syn.make_scene(n, 0, cam, sh_coeffs=M)
    deg = int(round(M ** 0.5)) - 1
    m = GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"], sh_degree=deg, device="cpu")
    m._init_aux()
    m.unique_kfIDs[:] = 3
    if with_optimizer:
        groups = [{"params": [p], "lr": 1e-3, "name": nm} for p, nm in zip(
            m.parameters(), ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))]
        m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for p in m.parameters():
            p.grad = torch.full_like(p, 0.5)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    return m


@pytest.mark.parametrize("with_optimizer", [False, True])
def test_extend_from_pcd_on_cpu_tensors(with_optimizer):
    n, k, M = 11, 5, 4
    model = _cpu_model(n, M, with_optimizer)
    before = [p.detach().clone() for p in model.parameters()]
    if with_optimizer:
        mom = [model.optimizer.state[p]["exp_avg"].clone() for p in model.parameters()]
        assert all(float(x.abs().sum()) > 0 for x in mom if x.numel())
    g = torch.Generator().manual_seed(0)
    xyz, feats = torch.randn(k, 3, generator=g), torch.randn(k, 3, M, generator=g)
    scales, rots, opac = torch.randn(k, 3, generator=g), torch.randn(k, 4, generator=g), torch.zeros(k, 1)
    model.xyz_gradient_accum += 1.0
    model.extend_from_pcd(xyz, feats, scales, rots, opac, kf_id=9)
    after = model.parameters()
    want_new = [xyz, feats[:, :, 0:1].transpose(1, 2), feats[:, :, 1:].transpose(1, 2), opac, scales, rots]
    for b, a, w in zip(before, after, want_new):
        assert a.shape[0] == n + k and a.is_leaf and a.requires_grad and a.is_contiguous()
        assert torch.equal(a[:n].detach(), b) and torch.equal(a[n:].detach(), w)
    assert model.get_features.shape == (n + k, M, 3)
    assert model.max_radii2D.shape == (n + k,) and model.xyz_gradient_accum.shape == (n + k, 1) and model.denom.shape == (n + k, 1)
    assert float(model.xyz_gradient_accum.abs().sum()) == 0 and float(model.max_radii2D.abs().sum()) == 0
    assert model.unique_kfIDs.tolist() == [3] * n + [9] * k and model.unique_kfIDs.dtype == torch.int32
    assert model.n_obs.tolist() == [0] * (n + k)
    if with_optimizer:
        for group, a, old in zip(model.optimizer.param_groups, after, mom):
            assert group["params"][0] is a
            st = model.optimizer.state[a]
            assert torch.equal(st["exp_avg"][:n], old) and float(st["exp_avg"][n:].abs().sum()) == 0
            assert st["exp_avg_sq"].shape == a.shape and float(st["exp_avg_sq"][n:].abs().sum()) == 0
        assert len(model.optimizer.state) == 6
        for p in after:
            p.grad = torch.ones_like(p)
        model.optimizer.step()  # runs on the grown state
        assert torch.isfinite(model._xyz).all() and not torch.equal(model._xyz[n:].detach(), xyz)


def test_extend_from_pcd_into_an_empty_model():
    from gaussian_splatting.scene.gaussian_model import GaussianModel

    model = GaussianModel(1)
    k, M = 6, 4
    model.extend_from_pcd(torch.ones(k, 3), torch.ones(k, 3, M), torch.zeros(k, 3), torch.ones(k, 4), torch.zeros(k, 1), kf_id=0)
    assert model.get_xyz.shape == (k, 3) and model.get_features.shape == (k, M, 3) and model.unique_kfIDs.tolist() == [0] * k
    model.init_lr(6.0)
    assert model.spatial_lr_scale == 6.0


def test_the_seeding_entry_points_refuse_cpu_tensors_and_bad_arguments():
    from gsaj import _lib, seeding

    with pytest.raises(_lib.GsajError, match="no CPU path"):
        seeding.median_depth(torch.ones(4, 4))
    with pytest.raises(_lib.GsajError, match="no CPU path"):
        seeding.seed_from_keyframe(torch.ones(3, 4, 4), torch.ones(4, 4), torch.eye(4), 1, 1, 0, 0, 1, 0.01)
    lib = _lib.load()
    assert lib.gsaj_version() >= 102
    assert lib.gsaj_seed_workspace_bytes(640, 480) >= 640 * 480 * 13
    assert lib.gsaj_seed_workspace_bytes(640, 480) < lib.gsaj_seed_workspace_bytes(1280, 720)
    assert lib.gsaj_depth_stats(0, 480, *([None] * 2), 0.95, None, None, 0.0, *([None] * 4)) == -1
    assert b"gsaj_depth_stats: invalid argument" in lib.gsaj_last_error()
    assert lib.gsaj_seed_select(640, 480, 1, None, 0.0, 100.0, 0.5, 0, 1, None) == -1  # downsample_factor < 1
    assert b"gsaj_seed_select: invalid argument" in lib.gsaj_last_error()
    assert lib.gsaj_seed_gaussians(-1, 640, 480, *([None] * 4), 1.0, 1.0, 0.0, 0.0, 0.01, 0, 1, 0, *([None] * 9)) == -1
    assert lib.gsaj_seed_gaussians(0, 640, 480, *([None] * 4), 1.0, 1.0, 0.0, 0.0, 0.01, 0, 1, 0, *([None] * 9)) == 0  # m == 0: a no-op
