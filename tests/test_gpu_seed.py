"""GPU: the keyframe seeding kernels (csrc/seed.hip, gsaj.seeding, the GaussianModel / slam_utils overlays) against the NumPy
restatement (tests/seed_restated.py) and the outputs recorded from the reference (tests/golden/median_depth_*.npz) -- never
against themselves -- plus one independent path (the rasteriser's preprocess sees every seed at its source pixel and depth) and
an end-to-end sanity run (a map seeded from a rendered keyframe re-renders that keyframe)."""
import glob
import os

import numpy as np
import pytest

import seed_restated as sr

# nothing here takes more than seconds: every test gets a time limit of its own (pytest-timeout, where it is installed)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("median_depth_"):-4] for p in glob.glob(os.path.join(GOLDEN, "median_depth_*.npz")))
DEV = "cuda:0"
ULP32 = 2.0 ** -23


def T(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def std_bound(std, n):
    """|device std - fp32(restated std)|: both are fp64 sums of n terms (relative error ~ n 2^-53 each, in different orders; the
    square root halves it) rounded ONCE to fp32 (half an ulp = 2^-24 relative each; the two roundings can fall either side of a
    tie, so one full ulp) -> (2^-23 + 2 n 2^-53) |std|.  At n = 921600 that is 1.19e-7 + 2.0e-10 relative."""
    return (ULP32 + 2.0 * n * 2.0 ** -53) * abs(std)


def check_stats(depth, opacity, mask, want=None):
    from gsaj import seeding

    med, std, valid, n = sr.median_depth(depth, opacity, mask) if want is None else want
    stats, dvalid = seeding.depth_stats(T(depth), T(opacity), T(mask), return_valid=True)
    stats = stats.cpu().numpy()
    assert int(stats[2]) == n and stats[3] == 0
    assert stats[0].tobytes() == np.float32(med).tobytes()
    assert np.array_equal(dvalid.cpu().numpy().reshape(valid.shape), valid)
    if n > 1:
        print("n_valid %d  median %.7g  std %.9g (restated %.9g, bound %.2e)" % (n, stats[0], stats[1], std, std_bound(std, n)))
        assert abs(float(stats[1]) - float(np.float32(std))) <= std_bound(std, n)
    return stats


@pytest.mark.parametrize("name", CASES)
def test_median_depth_on_the_reference_fixtures(name):
    from gsaj import seeding
    from utils.slam_utils import get_median_depth

    z = np.load(os.path.join(GOLDEN, "median_depth_%s.npz" % name))
    o = z["opacity"] if bool(z["use_opacity"]) else None
    m = z["mask"] if bool(z["use_mask"]) else None
    check_stats(z["depth"], o, m, want=(z["median"], float(z["std"]), z["valid"], int(z["n_valid"])))
    # the public forms: gsaj.seeding.median_depth and the overlay's get_median_depth with the reference's signature
    med, std, valid = get_median_depth(T(z["depth"]), T(o), T(m), return_std=True)
    assert med.cpu().numpy().tobytes() == z["median"].tobytes() and valid.shape == z["depth"].shape
    assert np.array_equal(valid.cpu().numpy(), z["valid"])
    assert abs(float(std) - float(z["std"])) <= std_bound(float(z["std"]), int(z["n_valid"]))
    assert seeding.median_depth(T(z["depth"]), T(o), T(m)).cpu().numpy().tobytes() == z["median"].tobytes()


@pytest.mark.parametrize("W,H", [(64, 48), (640, 480), (641, 479), (1280, 720)])
@pytest.mark.parametrize("variant", ["plain", "opacity_mask"])
def test_median_depth_against_the_restatement(W, H, variant):
    rng = np.random.default_rng(W * 7 + H)
    depth = (1.5 + 0.4 * np.sin(np.arange(W)[None, :] / 37.0) + rng.gamma(2.0, 0.5, (H, W))).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.2] = 0
    depth[rng.uniform(size=(H, W)) < 0.01] = -2.0
    depth[H // 2, : W // 2] = depth[H // 2, 0]  # a run of equal values
    o = m = None
    if variant == "opacity_mask":
        o = rng.uniform(0.85, 1.0, (H, W)).astype(np.float32)
        m = rng.uniform(size=(H, W)) < 0.6
    check_stats(depth, o, m)


def test_median_depth_edge_cases():
    H, W = 37, 53
    z = np.zeros((H, W), np.float32)
    s = check_stats(z, None, None)  # no valid pixel: the reference raises; the device answers 0, 0, n_valid 0
    assert s[0] == 0 and s[1] == 0 and s[2] == 0
    pm = z.copy()
    pm[::2] = -0.0  # +0 and -0 are both "not > 0"
    assert check_stats(pm, None, None)[2] == 0
    c = np.full((H, W), 2.5, np.float32)
    s = check_stats(c, None, None)  # all pixels equal: median 2.5, std exactly 0
    assert s[0] == 2.5 and s[1] == 0 and s[2] == H * W
    one = z.copy()
    one[3, 4] = 1.25
    s = check_stats(one, None, None)  # one valid pixel: torch.std is NaN
    assert s[0] == 1.25 and np.isnan(s[1]) and s[2] == 1
    two = z.copy()
    two[0, 0], two[H - 1, W - 1] = 3.0, 1.0
    s = check_stats(two, None, None)  # the LOWER median of two
    assert s[0] == 1.0


@pytest.mark.parametrize("W,H,with_noise", [(160, 120, True), (641, 479, True), (64, 48, False)])
def test_keyframe_depth_prior(W, H, with_noise):
    from gsaj import seeding

    rng = np.random.default_rng(W)
    depth = rng.normal(2.0, 0.5, (H, W)).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.05] = 0
    opacity = rng.uniform(0.9, 1.0, (H, W)).astype(np.float32)
    gt = rng.uniform(0, 0.5, (3, H, W)).astype(np.float32)
    gt[:, rng.uniform(size=(H, W)) < 0.1] = 0.001
    thr = 0.01
    noise = rng.normal(size=(H, W)).astype(np.float32) if with_noise else None
    want, margin, med, std32 = sr.keyframe_depth_prior(depth, opacity, gt, thr, noise)
    got, stats = seeding.keyframe_depth_prior(T(depth)[None], T(opacity)[None], T(gt), thr, T(noise), return_stats=True)
    got, stats = got.cpu().numpy(), stats.cpu().numpy()
    assert stats[0].tobytes() == med.tobytes()
    # the device's std may be the restated one's fp32 neighbour; then med +- std moves by up to an ulp of itself, and a pixel whose
    # depth is that close to a bound may fall on the other side: those pixels, and only those, may differ
    eps = 2 * ULP32 * (abs(float(med)) + abs(float(std32)))
    border = margin <= eps
    same_std = stats[1].tobytes() == std32.tobytes()
    assert abs(float(stats[1]) - float(std32)) <= std_bound(float(std32), int(stats[2]))
    # same std: the same fp32 operations on the same values, so the same bits everywhere.  A neighbouring std also moves the noise
    # scale by an ulp of 0.5 std, and the sum is rounded again: that much, no more, away from the borderline pixels
    tol = 0.0 if same_std else ULP32 * float(std32) * np.abs(noise if with_noise else 0.0) + 2 * ULP32 * np.abs(want)
    bad = np.abs(got.astype(np.float64) - want) > tol
    print("prior %dx%d: std bits %s; %d borderline pixels, %d differing pixels" % (W, H, "equal" if same_std else "an ulp apart",
                                                                                  int(border.sum()), int(bad.sum())))
    assert (bad <= border).all()  # every differing pixel is a verified borderline pixel
    assert (got[~sr.rgb_valid(gt, thr)] == 0).all()


def _keyframe(W, H, seed, band=False, valid_frac=0.8):
    rng = np.random.default_rng(seed)
    depth = (1.0 + rng.uniform(0, 4.0, (H, W))).astype(np.float32)
    depth[rng.uniform(size=(H, W)) > valid_frac] = 0
    depth[0, :5] = [100.0, 99.99, 150.0, -1.0, 1e-3]  # at / beyond depth_trunc: dropped; just below: kept
    if band:
        depth[: H // 3] = 0
        depth[2 * H // 3:] = 0
    image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    return depth, image


def _camera(W, H, orthonormal):
    from gsaj import synthetic as syn

    return syn.fixture_camera(noisy=True, orthonormal=orthonormal, W=W, H=H, fx=0.9 * W, fy=0.88 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)


def _seed(depth, image, cam, factor, seed, **kw):
    from gsaj import seeding

    w2c = T(cam["w2c"].astype(np.float32))
    return seeding.seed_from_keyframe(T(image), T(depth), w2c, cam["fx"], cam["fy"], cam["cx"], cam["cy"], factor, kw.pop("point_size", 0.01),
                                      seed=seed, return_pixels=True, **kw)


@pytest.mark.parametrize("W,H,factor,seed,band,masked", [
    (64, 48, 1, 0, False, False), (64, 48, 4, 1, False, True), (640, 480, 32, 0, False, False), (640, 480, 64, 3, True, False),
    (641, 479, 128, 4, False, True), (1280, 720, 32, 2, False, False), (160, 120, 2.5, 9, True, True), (64, 48, 4000, 0, False, False)])
def test_selection_equals_the_restatement_exactly(W, H, factor, seed, band, masked):
    depth, image = _keyframe(W, H, seed + W, band)
    gt, thr = (image.copy(), 0.6) if masked else (None, 0.0)
    cam = _camera(W, H, True)
    out = _seed(depth, image, cam, factor, seed, gt_image=T(gt), rgb_boundary_threshold=thr)
    want, nv = sr.select(sr.seed_valid(depth, gt, thr), factor, seed)
    pix = out[5].cpu().numpy()
    assert pix.size == want.size == int(nv * (1.0 / factor)) and np.array_equal(pix, want)
    assert out[0].shape == (want.size, 3) and out[1].shape == (want.size, 3, 1)
    if factor == 4000:
        assert want.size == 0  # n_valid < factor: m = 0, a successful no-op
    if factor == 1:
        assert want.size == nv
    flat = depth.reshape(-1)
    assert not np.isin(np.flatnonzero(flat >= 100.0), pix).any()  # at or beyond depth_trunc: never a seed
    if factor == 1 and not band and not masked:
        assert np.flatnonzero(flat == np.float32(99.99))[0] in pix  # just below it: one


@pytest.mark.parametrize("orthonormal", [True, False])
@pytest.mark.parametrize("adaptive,isotropic,sh_degree", [(False, False, 0), (True, True, 3), (True, False, 1)])
def test_seeded_parameters_against_the_restatement(orthonormal, adaptive, isotropic, sh_degree):
    import torch
    from oracle import knn_oracle

    W, H, factor, seed = 320, 240, 8, 5
    depth, image = _keyframe(W, H, 11)
    cam = _camera(W, H, orthonormal)
    ps = 0.01  # (adaptive: times the median of ALL pixels, ~2.9 here, stays below the cap of 0.05)
    exposure = (0.0, 0.0) if not adaptive else (0.13, -0.04)
    out = _seed(depth, image, cam, factor, seed, point_size=ps, adaptive_pointsize=adaptive, isotropic=isotropic, sh_degree=sh_degree,
                exposure_ab=T(np.array(exposure, np.float32)))
    xyz, feats, scales, rots, opac, pix = [t.cpu().numpy() for t in out]
    want_pix, _ = sr.select(sr.seed_valid(depth), factor, seed)
    assert np.array_equal(pix, want_pix) and pix.size > 1000
    m, M = pix.size, (sh_degree + 1) ** 2
    # xyz: two fp64 evaluations of the same expression on the same fp32 inputs, rounded once: 1 fp32 ulp of the largest magnitude
    # involved (the camera-space coordinates and the translation go through the sums, so cancellation is measured against them)
    w2c32 = cam["w2c"].astype(np.float32)
    pw = sr.backproject(depth, pix, W, w2c32, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    c2w = np.linalg.inv(w2c32.astype(np.float64))
    mag = np.maximum(np.abs(pw).max(axis=1), np.abs(c2w[:3, 3]).max())
    err = np.abs(xyz.astype(np.float64) - pw).max(axis=1)
    print("xyz: max error %.3g, max error / ulp bound %.3f" % (err.max(), (err / (ULP32 * mag)).max()))
    assert (err <= ULP32 * mag).all()
    # colour
    q, x = sr.quantised_colour(image, pix, exposure)
    assert feats.shape == (m, 3, M) and (feats[:, :, 1:] == 0).all()
    q_dev = np.rint((feats[:, :, 0].astype(np.float64) * sr.C0 + 0.5) * 255.0).astype(np.int64)
    if exposure == (0.0, 0.0):
        assert np.array_equal(q_dev, q)  # exact: exp(0) * image + 0 is the image
    else:
        dq = np.abs(q_dev - q.astype(np.int64))
        clear = np.abs(x - np.rint(x)) > 1e-3
        print("exposure %s: %d of %d colour bytes off by one, all within 1e-3 of an integer" % (exposure, int((dq > 0).sum()), dq.size))
        assert dq.max() <= 1 and (dq[clear] == 0).all()
    # f_dc = RGB2SH(q_dev / 255) to 2 ulp (a quotient against a product with the rounded reciprocal, see test_cpu_seed)
    want_dc = sr.rgb2sh(q_dev.astype(np.uint8))
    assert (np.abs(feats[:, :, 0].astype(np.float64) - want_dc) <= 2 * ULP32 * np.abs(want_dc) + 1e-12).all()
    # scales from the device's own xyz through the brute-force 3-NN: test_gpu_knn allows rtol 2e-5 on dist2, and
    # s = log(dist2 * point_size) / 2, so |ds| <= 1e-5, plus the fp32 roundings of the product, sqrt and log (4 ulp of |s|)
    psz = sr.adaptive_point_size(ps, depth) if adaptive else np.float32(ps)
    if adaptive:
        assert psz < 0.05  # (the case exercises the product, not the cap)
    want_s = sr.scales(knn_oracle.dist2(xyz), psz)
    assert scales.shape == (m, 1 if isotropic else 3) and (scales == scales[:, :1]).all()
    ds = np.abs(scales[:, 0].astype(np.float64) - want_s)
    print("scales: max |ds| %.3g" % ds.max())
    assert (ds <= 1e-5 + 4 * ULP32 * np.abs(want_s)).all()
    assert (rots == np.array([1, 0, 0, 0], np.float32)).all() and opac.shape == (m, 1) and (opac == 0).all()
    # twice the same bits; and a pose_state-shaped buffer serves as w2c and exposure_ab
    again = _seed(depth, image, cam, factor, seed, point_size=ps, adaptive_pointsize=adaptive, isotropic=isotropic, sh_degree=sh_degree,
                  exposure_ab=T(np.array(exposure, np.float32)))
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    from gsaj import seeding
    state = torch.zeros(80, device=DEV)
    state[:16] = T(w2c32).reshape(-1)
    state[33:35] = T(np.array(exposure, np.float32))
    via = seeding.seed_from_keyframe(T(image), T(depth), state, cam["fx"], cam["fy"], cam["cx"], cam["cy"], factor, ps, sh_degree=sh_degree,
                                     adaptive_pointsize=adaptive, isotropic=isotropic, exposure_ab=state[33:35], seed=seed)
    for a, b in zip(out[:5], via):
        assert torch.equal(a, b)


def test_fewer_than_four_seeds_keep_the_reference_scales():
    """dist2 keeps FLT_MAX terms when a point lacks three neighbours (gsaj_dist2), so the scales are huge or infinite, as upstream."""
    depth = np.zeros((48, 64), np.float32)
    depth[5, 7], depth[20, 30] = 1.0, 2.0
    out = _seed(depth, np.full((3, 48, 64), 0.5, np.float32), _camera(64, 48, True), 1, 0)
    assert out[0].shape == (2, 3) and bool((out[2] > 40).all())


@pytest.mark.parametrize("orthonormal", [True, False])
def test_the_rasteriser_sees_every_seed_at_its_pixel(orthonormal):
    """An independent path: the seeded map through the rasteriser's preprocess at the seeding pose (gsaj_debug_export)."""
    import helpers as hp
    from gsaj import rasterizer as C

    W, H, factor, seed = 160, 120, 4, 1
    depth, image = _keyframe(W, H, 21)
    depth[0, :5] = 0
    cam = _camera(W, H, orthonormal)
    out = _seed(depth, image, cam, factor, seed, point_size=0.05)
    xyz, feats, scales, rots, opac, pix = [t.cpu().numpy() for t in out]
    m = pix.size
    sc = dict(means3D=xyz, opacities=np.full((m, 1), 0.5, np.float32), scales=np.exp(scales), rotations=rots,
              shs=np.ascontiguousarray(feats.transpose(0, 2, 1)))
    fwd, _ = hp.gpu_forward(cam, sc, 0, kw=dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"]))
    R, _, radii, geom, binning, img = fwd[:6]
    dbg = {k: v.cpu().numpy() for k, v in C.debug_export(m, R, W, H, geom, binning, img).items()}
    assert (radii.cpu().numpy() > 0).all()
    u, v, d = (pix % W).astype(np.float64), (pix // W).astype(np.float64), depth.reshape(-1)[pix].astype(np.float64)
    g4 = 4 * 2.0 ** -24  # three products and three sums in fp32 per transformed coordinate
    w2c32 = cam["w2c"].astype(np.float32)
    pw = sr.backproject(depth, pix, W, w2c32, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ulp_in = ULP32 * np.maximum(np.abs(pw).max(axis=1), np.abs(np.linalg.inv(w2c32.astype(np.float64))[:3, 3]).max())  # the xyz bound above
    ph = np.concatenate([pw, np.ones((m, 1))], axis=1)

    def through(Mt, col):  # value and error bound of column `col` of [x y z 1] @ Mt (the rasteriser's transposed matrices)
        c = Mt.astype(np.float64)[:, col]
        return ph @ c, g4 * (np.abs(ph) @ np.abs(c)) + ulp_in * np.abs(c[:3]).sum()

    z, ez = through(cam["viewmatrix"], 2)
    err_d = np.abs(dbg["depths"] - d)
    print("depths: max |depth - source| %.3g (bound %.3g)" % (err_d.max(), ez.max()))
    assert (np.abs(z - d) <= ez).all() and (err_d <= 2 * ez + 2.0 ** -24 * d).all()
    hx, ex = through(cam["projmatrix"], 0)
    hy, ey = through(cam["projmatrix"], 1)
    hw, ew = through(cam["projmatrix"], 3)
    pwi = 1.0 / (hw + 1e-7)
    for S, h, e, col, pixc in ((W, hx, ex, 0, u), (H, hy, ey, 1, v)):
        ndc = h * pwi
        want = ((ndc + 1.0) * S - 1.0) * 0.5
        bound = 0.5 * S * ((e + np.abs(ndc) * ew) * np.abs(pwi) + 3 * 2.0 ** -24 * np.abs(ndc)) + 2.0 ** -24 * np.abs(want)
        got = dbg["means2D"][:, col].astype(np.float64)
        print("means2D[%d]: max error %.3g px (bound %.3g)" % (col, np.abs(got - want).max(), bound.max()))
        assert (np.abs(got - want) <= bound).all()
        # the offset between means2D and the integer pixel that ndc2Pix implies, from the projection matrix P (P^T row-major):
        # ndc = P00 x / z + P02 at w = z, pixel = ((ndc + 1) S - 1) / 2, and x / z = (u - c) / f
        P = cam["projmatrix_raw"].astype(np.float64).T
        f, c0 = (cam["fx"], cam["cx"]) if col == 0 else (cam["fy"], cam["cy"])
        slope = P[col, col] * S / (2.0 * f)
        offset = ((P[col, 2] + 1.0) * S - 1.0) * 0.5 - slope * c0
        assert abs(slope - 1.0) < 1e-6 and abs(offset + 0.5) < 1e-4
        spread = np.abs(got - (slope * pixc + offset))
        print("means2D[%d] - pixel: offset %.6f, spread %.3g px" % (col, offset, spread.max()))
        # (+ the fp32 rounding of the full projection matrix's entries, 2^-24 of terms of up to S / 2 pixels each: < 1e-4 px)
        assert (spread <= bound + 1e-4).all()


class _Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False


@pytest.mark.parametrize("orthonormal", [True, False])
def test_a_map_seeded_from_a_rendered_keyframe_renders_it_again(orthonormal):
    """End to end on a synthetic world.  Sanity inequalities only (they separate "splats in the right place" from "nothing or
    garbage", no tuned constant): colour L1 below the empty map's, median |depth / opacity - keyframe depth| over opaque pixels
    below the keyframe depth's standard deviation.  Then a second keyframe extends the map."""
    import torch
    from gaussian_splatting.gaussian_renderer import render
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj import synthetic as syn
    from gsaj.rasterizer import BatchContext
    from utils.camera_utils import Camera

    W, H = 160, 120
    cam = syn.fixture_camera(noisy=True, orthonormal=orthonormal, W=W, H=H, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    sc = syn.make_scene(6000, 3, cam, z_range=(1.0, 5.0), log_scale_range=(np.log(0.03), np.log(0.12)), sh_coeffs=1)
    world = GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"], sh_degree=0, device=DEV)
    view = Camera.from_synthetic(cam, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        kf = render(view, world, _Pipe, bg)
    colour, kdepth = kf["render"].detach().clamp(0, 1), torch.where(kf["opacity"] > 0.95, kf["depth"], torch.zeros_like(kf["depth"]))[0].detach()
    view.original_image, view.depth = colour, kdepth.cpu().numpy()
    cfg = {"Dataset": {"pcd_downsample": 2, "pcd_downsample_init": 2, "point_size": 1.0, "adaptive_pointsize": False, "sensor_type": "depth"}}
    model = GaussianModel(0, config=cfg)
    model.init_lr(6.0)
    model.extend_from_pcd_seq(view, kf_id=0, init=True)
    m0 = model.get_xyz.shape[0]
    assert m0 == int(int((kdepth > 0).sum()) * 0.5) and m0 > 1000
    with torch.no_grad():
        re = render(view, model, _Pipe, bg)
    l1_seeded = float((re["render"] - colour).abs().mean())
    l1_empty = float((bg[:, None, None] - colour).abs().mean())
    opaque = (re["opacity"][0] > 0.5) & (kdepth > 0)
    assert int(opaque.sum()) > 0
    derr = float(((re["depth"][0] / re["opacity"][0])[opaque] - kdepth[opaque]).abs().median())
    dstd = float(kdepth[kdepth > 0].std())
    print("seeded map (%d Gaussians): colour L1 %.4f (empty map %.4f); median depth error %.4g over %d opaque pixels (keyframe depth "
          "std %.4g)" % (m0, l1_seeded, l1_empty, derr, int(opaque.sum()), dstd))
    assert l1_seeded < l1_empty and derr < dstd
    # a second keyframe extends the EXISTING map
    before = [p.detach().clone() for p in model.parameters()]
    model.extend_from_pcd_seq(view, kf_id=1)
    m1 = model.get_xyz.shape[0] - m0
    assert m1 == m0  # same keyframe, same factor; another seed: another subset
    for b, a in zip(before, model.parameters()):
        assert torch.equal(a[:m0].detach(), b)
    assert not torch.equal(model.get_xyz[m0:].detach(), before[0])
    assert model.unique_kfIDs.tolist() == [0] * m0 + [1] * m1 and model.max_radii2D.shape == (m0 + m1,)
    with torch.no_grad():
        re2 = render(view, model, _Pipe, bg)
    assert torch.isfinite(re2["render"]).all() and int((re2["radii"] > 0).sum()) > m0
    bc = BatchContext(1, m0 + m1, W, H, 1, DEV)
    with torch.no_grad():
        st = bc.forward(bg, model.get_xyz, model.get_opacity, view.world_view_transform[None].contiguous(),
                        view.full_proj_transform[None].contiguous(), view.camera_center[None].contiguous(), cam["tanfovx"], cam["tanfovy"],
                        sh_degree=0, shs=model.get_features, scales=model.get_scaling, rotations=model.get_rotation)
    assert not any(ab for _, _, ab in st)
    assert torch.isfinite(bc.color).all() and float(bc.opacity.max()) > 0.5
