"""GPU parity of the dense analytic path (the reference's CPU/NumPy semantics) against the golden
vectors produced by the reference's own functions, and against the NumPy oracle at a larger N.
Tolerances: fp32 accumulations 5e-4 of the array's max (the reference sums 307 200 fp32 terms per
Gaussian in chunks of 1000; the kernels sum wave -> workgroup -> fp64), fp64 Jacobians 1e-9."""
import os

import numpy as np
import pytest

import dense_restated as dr
from gsaj import synthetic as syn
from oracle import dense_oracle as dor

pytestmark = pytest.mark.gpu
DENSE = ["dense_N1_64x48.npz", "dense_N15_64x48.npz", "dense_N15_64x48_ortho.npz", "dense_N64_64x48.npz",
         "dense_N15_640x480.npz"]
TOL = 5e-4


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


@pytest.mark.parametrize("name", DENSE)
def test_dense_golden(golden_dir, name):
    from gsaj import dense

    g = np.load(os.path.join(golden_dir, name))
    o = g["order"]
    N, W, H = int(g["N"]), int(g["W"]), int(g["H"])
    mu, S, z, c = dense.compute_gradients_2D(g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["opacities"][o, 0],
                                              g["seed_color"].astype(np.float32), g["seed_depth"].astype(np.float32))
    for got, want, nm in ((mu, g["grad_mu"], "mu"), (S, g["grad_Sigma"], "Sigma"), (z, g["grad_depth"], "depth"),
                          (c, g["grad_color"], "color")):
        assert _rel(got.cpu().numpy(), want) < TOL, (name, nm, _rel(got.cpu().numpy(), want))
    cam = syn.make_camera(g["w2c"], W=W, H=H, fx=float(g["fx"]), fy=float(g["fy"]), cx=float(g["cx"]), cy=float(g["cy"]))
    xyz_h = np.concatenate([g["means3D"].astype(np.float64), np.ones((N, 1))], 1)
    dmu, dcov = dense.compute_analytical_jacobians_all_gaussians(xyz_h, g["cov3D6"], cam["w2c"], cam["fx"], cam["fy"], W, H)
    assert np.allclose(dmu.cpu().numpy(), g["dmu_dtau"], rtol=1e-9, atol=1e-11)
    assert np.allclose(dcov.cpu().numpy(), g["dcov_dtau"], rtol=1e-8, atol=1e-9)
    # chain rule on the reference's own per-Gaussian gradients -> the reference's dL/dtau
    tau, parts = dense.assemble_dL_dtau(o, g["grad_mu"], g["grad_Sigma"], g["grad_depth"], g["grad_color"], dmu, dcov,
                                        g["means3D"], cam["w2c"], cam["campos"], g["shs"], 3)
    assert np.allclose(tau.cpu().numpy(), g["dL_dtau"], rtol=1e-8, atol=1e-8 * np.abs(g["dL_dtau"]).max())
    # end to end on the GPU: kernel gradients -> dL/dtau within the fp32 tolerance
    tau2, _ = dense.assemble_dL_dtau(o, mu, S, z, c, dmu, dcov, g["means3D"], cam["w2c"], cam["campos"], g["shs"], 3)
    assert _rel(tau2.cpu().numpy(), g["dL_dtau"]) < 2e-3
    assert mu.shape == (N, 2) and S.shape == (N, 2, 2) and z.shape == (N,)  # layout of Jacob_test_result/*.npy


def test_dense_kat_jacobians(golden_dir):
    from gsaj import dense

    g = np.load(os.path.join(golden_dir, "kat_pose_jacobian.npz"))
    for k in range(g["T_cw"].shape[0]):
        S = g["Sigma_w"][k]
        c6 = np.array([[S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]]])
        # fx = fy = 1, W = H = 2 -> unit scaling: raw Eq. 3 / Eq. 4 values
        dmu, dcov = dense.compute_analytical_jacobians_all_gaussians(g["mu_w"][k][None], c6, g["T_cw"][k], 1.0, 1.0, 2, 2)
        assert np.allclose(dmu.cpu().numpy()[0], g["dmu"][k], rtol=1e-10, atol=1e-12), k
        assert np.allclose(dcov.cpu().numpy()[0], g["dcov"][k], rtol=1e-9, atol=1e-11), k


def test_dense_large_n_vs_numpy_oracle_and_render():
    """N = 300 (three LDS chunks) on 160x120: kernels vs the NumPy oracle; forward compositor too."""
    from gsaj import dense

    W, H, N = 160, 120, 300
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=W, H=H, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
    sc = syn.make_scene(N, 31, cam, z_range=(1.0, 4.0), log_scale_range=(np.log(0.02), np.log(0.15)), margin=-0.05)
    cov6 = syn.covariance6(sc["scales"], sc["rotations"])
    m2, c2, dep = dor.project_gaussians(sc["means3D"], cov6, cam["w2c"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H)
    order = np.argsort(dep, kind="stable")
    dirs = dor.view_dirs(sc["means3D"].astype(np.float64), cam["campos"].astype(np.float64))
    col, _ = dor.colors_from_sh(sc["shs"].astype(np.float64), dirs, 3)
    m2, c2, dep, col, op = m2[order], c2[order], dep[order], col[order], sc["opacities"][order, 0]
    rng = np.random.default_rng(5)
    gc = rng.choice([-1.0, 0.0, 1.0], size=(H, W, 3)).astype(np.float32)
    gd = rng.choice([-1.0, 0.0, 1.0], size=(H, W)).astype(np.float32)
    want = dor.dense_backward(m2, c2, col, dep, op, gc, gd)
    got = dense.compute_gradients_2D(m2, c2, col, dep, op, gc, gd)
    for a, b in zip(got, want):
        assert _rel(a.cpu().numpy(), b) < TOL
    img, d = dense.render_projected(m2, c2, col, dep, op, H, W)
    img_ref, d_ref = dor.dense_render(m2, c2, col, dep, op, H, W)
    assert _rel(img.cpu().numpy(), img_ref) < 1e-4 and _rel(d.cpu().numpy(), d_ref) < 1e-4
    # bit-reproducible
    got2 = dense.compute_gradients_2D(m2, c2, col, dep, op, gc, gd)
    for a, b in zip(got, got2):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("name,naive", [("naive_N4_12x9.npz", False), ("naive_N4_12x9.npz", True), ("naive_edge_N5_12x9.npz", True)])
def test_naive_loop_goldens_on_the_device(golden_dir, name, naive):
    """Loss_Derivative_wrt_mu_and_cov.compute_gradients_2D (the O(HWN^2) loop) reproduced by the dense kernel: the plain golden
    in both modes (no edge case occurs in it), and the edge golden -- alpha >= 0.999 and abs(alpha) < 1e-8 entries -- in the
    naive-guard mode (GSAJ_DENSE_NAIVE_GUARDS)."""
    from gsaj import dense

    g = np.load(os.path.join(golden_dir, name))
    order = np.argsort(g["depth"], kind="stable")
    mu, S, _, _ = dense.compute_gradients_2D(g["mean_2D"][order], g["cov_2D"][order], g["color"][order], g["depth"][order],
                                             g["alpha"][order], g["seed_color"].astype(np.float32), g["seed_depth"].astype(np.float32),
                                             naive_guards=naive)
    inv = np.argsort(order)
    m_mu, m_S = np.abs(g["grad_mu"]).max(), np.abs(g["grad_Sigma"]).max()
    assert np.abs(mu.cpu().numpy()[inv] - g["grad_mu"]).max() < 3e-6 * m_mu
    assert np.abs(S.cpu().numpy()[inv] - g["grad_Sigma"]).max() < 3e-6 * m_S
    if name.startswith("naive_edge"):
        assert np.all(mu.cpu().numpy()[inv][3] == 0)  # the 1e-9-opacity entry is skipped entirely, as in the loop


@pytest.mark.parametrize("name", ["dense_normalised_N15_64x48.npz", "dense_normalised_N64_64x48.npz"])
def test_normalised_coordinate_variant_on_the_device(golden_dir, name):
    """a3, second producer: Loss_Derivative_script.py:820-979 (normalised image coordinates; GSAJ_DENSE_NORMALISED_COORDS) against
    the fixtures that function produced, and against the oracle on the same inputs."""
    from gsaj import dense
    from oracle import dense_oracle as dor

    g = np.load(os.path.join(golden_dir, name))
    intr = (float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"]))
    args = (g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["alpha"], g["seed_color"].astype(np.float32),
            g["seed_depth"].astype(np.float32))
    mu, S, z, c = (x.cpu().numpy() for x in dense.compute_gradients_2D(*args, normalised_intrinsics=intr))
    m_mu, m_S = np.abs(g["grad_mu"]).max(), np.abs(g["grad_Sigma"]).max()
    assert np.abs(mu - g["grad_mu"]).max() < 2e-5 * m_mu
    assert np.abs(S - g["grad_Sigma"]).max() < 2e-5 * m_S
    o_mu, o_S, o_z, o_c = dor.dense_backward(*args, normalised_intrinsics=intr)
    for got, want in ((mu, o_mu), (S, o_S), (z, o_z), (c, o_c)):
        assert np.abs(got - want).max() < 2e-5 * np.abs(want).max()
    with pytest.raises(Exception, match="NORMALISED_COORDS"):
        dense.compute_gradients_2D(*args, normalised_intrinsics=(0.0, 1.0, 0.0, 0.0))


def test_dense_render_reference_golden(golden_dir):
    """a10: rendered_Image_from_Projected_Gaussians_vectorized (compare.py:973-1018) -- the clipped image the reference hands to
    plt.imshow, recorded by tests/golden/make_goldens_r2.py (every 4th row / column + row and column sums of the full image)."""
    from gsaj import dense

    g = np.load(os.path.join(golden_dir, "dense_N15_640x480.npz"))
    r = np.load(os.path.join(golden_dir, "dense_render_N15_640x480.npz"))
    o = g["order"]
    img, _ = dense.render_projected(g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["opacities"][o, 0], 480, 640)
    img = np.clip(img.cpu().numpy(), 0.0, 1.0)
    assert np.abs(img[::4, ::4] - r["image_sub4"]).max() < 3e-6 * max(float(r["vmax"]), 1.0)
    assert np.abs(img.astype(np.float64).sum(axis=1) - r["row_sum"]).max() < 1e-5 * np.abs(r["row_sum"]).max()
    assert np.abs(img.astype(np.float64).sum(axis=0) - r["col_sum"]).max() < 1e-5 * np.abs(r["col_sum"]).max()


@pytest.mark.parametrize("name", DENSE)
def test_project_and_sort_golden(golden_dir, name):
    """a4 / a5 / a6 on the device: OrderGaussiansByDepth + GetImagePlaneMeanAndCovs (compute_cov2d, ndc2Pix, SH colours, view-space
    depth) against the arrays the reference's functions produced (tests/golden/make_goldens.py)."""
    from gsaj import dense

    g = np.load(os.path.join(golden_dir, name))
    cam = syn.make_camera(g["w2c"], W=int(g["W"]), H=int(g["H"]), fx=float(g["fx"]), fy=float(g["fy"]), cx=float(g["cx"]), cy=float(g["cy"]))
    pr = {k: v.cpu().numpy() for k, v in dense.project_and_sort(g["means3D"], g["cov3D6"], g["shs"], cam, 3).items()}
    np.testing.assert_array_equal(pr["order"], g["order"])
    assert np.allclose(pr["mean_2D"], g["mean_2D"], rtol=1e-6, atol=2e-5)   # the reference's P is fp32, the pixel values ~1e2
    assert np.allclose(pr["cov_2D"], g["cov_2D"], rtol=2e-6, atol=1e-6)
    assert np.allclose(pr["depth"], g["depth"], rtol=1e-7, atol=1e-7)
    assert np.allclose(pr["color"], g["color"], rtol=1e-9, atol=1e-10)
    assert np.allclose(pr["color_raw"], g["color_raw"][g["order"]], rtol=1e-9, atol=1e-10)


def test_depth_order_is_stable_and_keeps_points_behind_the_camera():
    """A.4: the NumPy path sorts ALL Gaussians by camera z (no z <= 0.2 cull) with Python's stable sort: ties keep index order."""
    from gsaj import dense

    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=64, H=48, fx=57.75, fy=57.75, cx=31.5, cy=23.5)
    sc = syn.make_scene(700, 8, cam, z_range=(-1.0, 3.0), margin=0.3)
    m = sc["means3D"].copy()
    m[100:110] = m[5]      # exact ties in depth
    m[400:420] = m[399]
    pr = dense.project_and_sort(m, syn.covariance6(sc["scales"], sc["rotations"]), sc["shs"], cam, 3)
    order, depth = pr["order"].cpu().numpy(), pr["depth"].cpu().numpy()
    z = (cam["viewmatrix"].astype(np.float64).T @ np.concatenate([m.astype(np.float64), np.ones((700, 1))], 1).T)[2]
    np.testing.assert_array_equal(order, np.argsort(z, kind="stable"))
    assert (depth[1:] >= depth[:-1]).all() and (depth < 0.2).sum() > 50 and sorted(order.tolist()) == list(range(700))


@pytest.mark.parametrize("name", ["dense_N15_64x48.npz", "dense_N15_640x480.npz", "dense_N64_64x48.npz"])
def test_jacobian_test_end_to_end(golden_dir, name):
    """gsaj.dense.jacobian_test: from world Gaussians + camera + ground truth to the four arrays of Jacob_test_result/ with no host
    step in between.  The golden seeds are sign patterns (the generator's `physical_seeds`); ground truth images that reproduce
    exactly those signs under l1_seeds are gt = render - seed (colour) and render - seed with gt > 0 (depth)."""
    from gsaj import dense

    g = np.load(os.path.join(golden_dir, name))
    W, H = int(g["W"]), int(g["H"])
    cam = syn.make_camera(g["w2c"], W=W, H=H, fx=float(g["fx"]), fy=float(g["fy"]), cx=float(g["cx"]), cy=float(g["cy"]))
    o = g["order"]
    img, dep = dense.render_projected(g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["opacities"][o, 0], H, W)
    img, dep = img.cpu().numpy(), dep.cpu().numpy()
    sc_, sd_ = g["seed_color"].astype(np.float32), g["seed_depth"].astype(np.float32)
    mask = (sc_ != 0).any(axis=-1) | (sd_ != 0)           # the generator's seeds are zero outside its own mask
    gt_c = img - sc_                                       # sign(render - gt) = seed, with a margin of 1
    gt_d = np.where(sd_ > 0, 0.5 * dep, np.where(sd_ < 0, 1.5 * dep + 1e-3, dep))   # same for depth, keeping gt > 0
    assert (gt_d[sd_ != 0] > 0).all()
    r = dense.jacobian_test(g["means3D"], g["cov3D6"], g["opacities"], g["shs"], cam, gt_c, gt_d, mask, 3)
    np.testing.assert_array_equal(r["order"].cpu().numpy(), o)
    for key, want in (("grad_mu_I_pixel", g["grad_mu"]), ("grad_Sigma_I_pixel", g["grad_Sigma"]), ("grad_depth_per_gaussian", g["grad_depth"])):
        assert _rel(r[key].cpu().numpy(), want) < TOL, (key, _rel(r[key].cpu().numpy(), want))
    assert _rel(r["dL_dtau"].cpu().numpy(), g["dL_dtau"]) < 2e-3
    assert r["grad_mu_I_pixel"].shape == (int(g["N"]), 2) and r["dL_dtau"].shape == (6,) and r["dL_dtau"].dtype == __import__("torch").float64


# ---- per-Gaussian / per-pixel parity against the fp64 restatement (tests/dense_restated.py) -----------------------------------------
# Every row and component is held to ITS OWN bound, MASS_TOL sum|term| + COND_K cond (derived in dense_restated's docstring), on
# generated cases that reach the chunk boundaries (N = 127 .. 129, 255 .. 257, 300), an image of fewer than 256 pixels, the ragged
# last workgroup, rows 6+ orders below their tensor's maximum (stack), the guards (saturated, offscreen; both guard modes) and
# ill-conditioned covariances (needles; once in normalised coordinates).  The worst err / bound per tensor goes into
# profiles/r09_dense_parity.json when GSAJ_WRITE_PARITY is set.  Found by these tests, on the kernel that formed S_i as fp64 total -
# fp64 prefix: behind a stack the difference is rounded at the size of the total and was the whole of dL/dalpha (stack-129-17x15:
# dL/dmu[1] of Gaussian 118 came out -7.8e-10 where it is 9.2e-48, every stack case alike), and the error measured on the device was
# about 1e-8 of the total, not 1e-16, so it reached ordinary rows of ill-conditioned Gaussians too (needles-128-16x16: dL/dSigma[1][1]
# of Gaussian 88 off by 3.5 %, 10.8 x its bound; needles-300-17x15 row 292; saturated-300-33x17 row 275, 2.75 x).  k_dense_bwd now keeps T_i from the forward
# walk and carries the suffix back to front as a recurrence.

REPEAT_RUN = dr.run_id((dr.CASES[8], False, "pixel"))   # stack-300-64x48: launched twice, identical bits


def _args(inp):
    return tuple(np.array(a) for a in dr.args_of(inp))


def _show(tag, ratios):
    print("%s err/bound %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))


@pytest.mark.parametrize("run", dr.runs(), ids=dr.run_id)
def test_dense_backward_per_gaussian_bounds(run):
    from gsaj import dense

    case, naive, variant = run
    inp, intr, r = dr.make_case(*case, naive=naive, variant=variant)
    got = dense.compute_gradients_2D(*_args(inp), naive_guards=naive, normalised_intrinsics=intr)
    have = dr.to10(*got)
    bd = dr.bound(r)
    ratios = {nm: float((np.abs(have - r["value"]) / bd)[:, s].max()) for nm, s in dr.TENSORS}
    _show(dr.run_id(run), ratios)
    dr.note("device_mi355x", "test_dense_backward_per_gaussian_bounds", dr.assert_dense_close(have, r, dr.run_id(run)))
    if dr.run_id(run) == REPEAT_RUN:
        again = dense.compute_gradients_2D(*_args(inp), naive_guards=naive, normalised_intrinsics=intr)
        for a, b in zip(got, again):
            assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("run", [x for x in dr.runs() if not x[1] and x[2] == "pixel"], ids=dr.run_id)
def test_dense_render_per_pixel_bounds(run):
    from gsaj import dense

    case, naive, variant = run
    inp, _, r = dr.make_case(*case)
    H, W = inp["grad_depth"].shape
    img, dep = dense.render_projected(*_args(inp)[:5], H, W)
    have = np.concatenate([img.cpu().numpy().reshape(H * W, 3), dep.cpu().numpy().reshape(H * W, 1)], axis=1).astype(np.float64)
    ratio = np.abs(have - r["render_value"]) / dr.bound(r, "render_")
    _show(dr.run_id(run), dict(color=ratio[:, :3].max(), depth=ratio[:, 3].max()))
    dr.note("device_mi355x", "test_dense_render_per_pixel_bounds", dr.assert_render_close(img, dep, r, dr.run_id(run)))


RECORDED = [(n, False, False) for n in DENSE] + [("dense_normalised_N15_64x48.npz", False, True), ("dense_normalised_N64_64x48.npz", False, True),
                                                  ("naive_N4_12x9.npz", False, False), ("naive_N4_12x9.npz", True, False),
                                                  ("naive_edge_N5_12x9.npz", True, False)]


def _recorded_inputs(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    f = np.float32
    if name.startswith("naive"):
        o = np.argsort(g["depth"], kind="stable")
        arrs = (g["mean_2D"][o], g["cov_2D"][o], g["color"][o], g["depth"][o], g["alpha"][o])
    elif "normalised" in name:
        arrs = (g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["alpha"])
    else:
        arrs = (g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["opacities"][g["order"], 0])
    return g, tuple(np.asarray(a).astype(f) for a in arrs) + (g["seed_color"].astype(f), g["seed_depth"].astype(f))


@pytest.mark.parametrize("name,naive,norm", RECORDED, ids=lambda v: str(v).replace(".npz", ""))
def test_recorded_inputs_per_gaussian_bounds(golden_dir, name, naive, norm):
    """The inputs of the committed goldens through the per-row comparator; dense_N15_640x480 is the one case with 1200 workgroups
    in the slab sum, and its render goes against the per-pixel bound as well."""
    from gsaj import dense

    g, args = _recorded_inputs(golden_dir, name)
    intr = (float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"])) if norm else None
    r = dr.restate(*args, naive_guards=naive, normalised_intrinsics=intr)
    got = dense.compute_gradients_2D(*args, naive_guards=naive, normalised_intrinsics=intr)
    have = dr.to10(*got)
    tag = "%s%s" % (name, "-naive" if naive else "")
    _show(tag, {nm: float((np.abs(have - r["value"]) / dr.bound(r))[:, s].max()) for nm, s in dr.TENSORS})
    dr.note("device_mi355x", "test_recorded_inputs_per_gaussian_bounds", dr.assert_dense_close(have, r, tag))
    if name == "dense_N15_640x480.npz":
        H, W = args[6].shape
        img, dep = dense.render_projected(*args[:5], H, W)
        dr.note("device_mi355x", "test_recorded_inputs_per_gaussian_bounds", {"render_" + k: v for k, v in dr.assert_render_close(img, dep, r, tag).items()})


@pytest.mark.parametrize("N", [255, 256, 257, 300])
def test_project_jacobians_tau_beyond_one_workgroup(N):
    """k_dense_project / k_dense_rank / k_dense_gather, k_pose_jacobians and k_dense_tau's strided loop past one workgroup (256 lanes,
    128 for the first and third), value by value against the fp64 functions of oracle/dense_oracle.py, with the tolerances
    test_project_and_sort_golden and test_dense_golden use for the same quantities; SH colours wide enough that channels clamp."""
    from gsaj import dense

    W, H = 64, 48
    cam = syn.fixture_camera(noisy=True, orthonormal=True, W=W, H=H, fx=57.75, fy=57.75, cx=31.5, cy=23.5)
    sc = syn.make_scene(N, 400 + N, cam, z_range=(1.0, 4.0), log_scale_range=(np.log(0.02), np.log(0.15)), margin=-0.05, sh_sigma=0.6)
    cov6 = syn.covariance6(sc["scales"], sc["rotations"]).astype(np.float32)
    m2, c2, dep = dor.project_gaussians(sc["means3D"], cov6, cam["w2c"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H)
    order = np.argsort(dep, kind="stable")
    dirs = dor.view_dirs(sc["means3D"].astype(np.float64), cam["campos"].astype(np.float64))
    col, raw = dor.colors_from_sh(sc["shs"].astype(np.float64), dirs, 3)
    assert (raw < 0).any() and (raw > 0).any()          # some channel is clamped
    pr = {k: v.cpu().numpy() for k, v in dense.project_and_sort(sc["means3D"], cov6, sc["shs"], cam, 3).items()}
    np.testing.assert_array_equal(pr["order"], order)
    assert np.allclose(pr["mean_2D"], m2[order], rtol=1e-6, atol=2e-5)
    assert np.allclose(pr["cov_2D"], c2[order], rtol=2e-6, atol=1e-6)
    assert np.allclose(pr["depth"], dep[order], rtol=1e-7, atol=1e-7)
    assert np.allclose(pr["color"], col[order], rtol=1e-9, atol=1e-10)
    assert np.allclose(pr["color_raw"], raw[order], rtol=1e-9, atol=1e-10)
    xyz_h = np.concatenate([sc["means3D"].astype(np.float64), np.ones((N, 1))], 1)
    dmu, dcov = dense.compute_analytical_jacobians_all_gaussians(xyz_h, cov6, cam["w2c"], cam["fx"], cam["fy"], W, H)
    dmu_ref, dcov_ref = dor.pose_jacobians_all(xyz_h, cov6, cam["w2c"], cam["fx"], cam["fy"], W, H)
    assert np.allclose(dmu.cpu().numpy(), dmu_ref, rtol=1e-9, atol=1e-11)
    assert np.allclose(dcov.cpu().numpy().reshape(N, 4, 6), dcov_ref, rtol=1e-8, atol=1e-9)
    rng = np.random.default_rng(N)
    gc = rng.choice([-1.0, 0.0, 1.0], size=(H, W, 3)).astype(np.float32)
    gd = rng.choice([-1.0, 0.0, 1.0], size=(H, W)).astype(np.float32)
    g = dense.compute_gradients_2D(pr["mean_2D"], pr["cov_2D"], pr["color"], pr["depth"], sc["opacities"][order, 0], gc, gd)
    tau, parts = dense.assemble_dL_dtau(order, *g, dmu, dcov, sc["means3D"], cam["w2c"], cam["campos"], sc["shs"], 3)
    gn = [x.cpu().numpy() for x in g]
    tau_ref, parts_ref = dor.assemble_dL_dtau(order, *gn, dmu_ref, dcov_ref, sc["means3D"], cam["w2c"], cam["campos"], sc["shs"], 3)
    assert np.allclose(tau.cpu().numpy(), tau_ref, rtol=1e-8, atol=1e-8 * np.abs(tau_ref).max())
    for k in ("mu", "cov", "depth", "sh"):
        assert np.allclose(parts[k].cpu().numpy(), parts_ref[k], rtol=1e-8, atol=1e-8 * np.abs(tau_ref).max()), k
    assert np.abs(parts_ref["sh"]).max() > 0


@pytest.mark.parametrize("name", ["dense_N1_64x48.npz", "dense_N15_64x48.npz", "dense_N15_64x48_ortho.npz", "dense_N64_64x48.npz"])
def test_dense_tau_end_to_end_within_propagated_bounds(golden_dir, name):
    """N <= 64, kernel gradients -> dL/dtau on the device against the restated gradients through the fp64 chain rule.  The chain is
    linear in the four gradient arrays, so sum |coefficient| x (the row's bound) is what two evaluations inside the per-row bounds
    may differ by; that replaces the constant 2e-3 (which stays for the recorded dL/dtau in test_dense_golden).  The fp64 chain itself
    is allowed the 1e-8 of the largest component test_dense_golden allows it."""
    from gsaj import dense

    g, args = _recorded_inputs(golden_dir, name)
    o, N, W, H = g["order"], int(g["N"]), int(g["W"]), int(g["H"])
    cam = syn.make_camera(g["w2c"], W=W, H=H, fx=float(g["fx"]), fy=float(g["fy"]), cx=float(g["cx"]), cy=float(g["cy"]))
    r = dr.restate(*args)
    got = dense.compute_gradients_2D(*args)
    xyz_h = np.concatenate([g["means3D"].astype(np.float64), np.ones((N, 1))], 1)
    dmu, dcov = dense.compute_analytical_jacobians_all_gaussians(xyz_h, g["cov3D6"], cam["w2c"], cam["fx"], cam["fy"], W, H)
    tau, _ = dense.assemble_dL_dtau(o, *got, dmu, dcov, g["means3D"], cam["w2c"], cam["campos"], g["shs"], 3)
    dmu_ref, dcov_ref = dor.pose_jacobians_all(xyz_h, g["cov3D6"], cam["w2c"], cam["fx"], cam["fy"], W, H)
    v = r["value"]
    tau_r, _ = dor.assemble_dL_dtau(o, v[:, 0:2], v[:, 2:6].reshape(N, 2, 2), v[:, 6], v[:, 7:10], dmu_ref, dcov_ref, g["means3D"],
                                    cam["w2c"], cam["campos"], g["shs"], 3)
    allowed = (dr.tau_bound(o, r, dmu_ref, dcov_ref, g["means3D"], cam["w2c"]) + dr.sh_tau_bound(o, r, g["means3D"], cam["campos"], g["shs"], 3)
               + 1e-8 * np.abs(tau_r).max())
    err = np.abs(tau.cpu().numpy() - tau_r)
    _show(name + " dL/dtau", {"tau%d" % k: err[k] / allowed[k] for k in range(6)})
    dr.note("device_mi355x", "test_dense_tau_end_to_end_within_propagated_bounds", {"dL_dtau": float((err / allowed).max())})
    assert (err <= allowed).all(), (name, err, allowed)
