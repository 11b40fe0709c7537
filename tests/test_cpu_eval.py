"""CPU: the NumPy restatement of the per-frame rendering metrics (tests/eval_restated.py) against the fixtures the reference's own
statements produced (tests/golden/eval_*.npz, make_eval_goldens.py), with canaries; the new C-ABI symbols and their argument errors;
the trajectory error (gsaj.evaluation.umeyama / ate); the host logic of utils.eval_utils with render and the launch replaced.
No kernel runs."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

import eval_restated as er

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "eval_*.npz")))
SCENES = ("noise_3x40x56", "gray_1x17x15", "identical_3x16x16", "black_gt_3x8x8", "tiny_3x5x7")


def accepts(z, r):
    """The comparator of this file: does the restatement's result r agree with the fixture z?  -> (ok, what failed)"""
    special = er.same_special(r["psnr"], z["psnr"])
    if special is None:
        if not abs(r["psnr"] - float(z["psnr"])) <= er.psnr_bound_reference(r["n"], r["psnr"]):
            return False, "psnr"
    elif not special:
        return False, "psnr (inf / NaN)"
    if not abs(r["ssim"] - float(z["ssim"])) < 5e-4:  # the bound of tests/test_cpu_ssim.py
        return False, "ssim"
    if r["n"] != int(z["n"]):
        return False, "n"
    if not np.array_equal(r["u8"], z["pred_u8"]):
        return False, "bytes"
    return True, ""


# ---- 1. the restatement against the reference's fixtures --------------------------------------------------------------------------
def test_fixtures_present_and_as_described():
    names = {os.path.basename(f) for f in FIXTURES}
    for case in SCENES:
        assert "eval_%s.npz" % case in names, case
    for f in FIXTURES:
        assert os.path.getsize(f) < 64 * 1024, f
    z = np.load(os.path.join(GOLDEN, "eval_noise_3x40x56.npz"))
    m = z["gt"] > 0
    kept = z["image"][m]
    assert (kept < 0).sum() > 100 and (kept > 1).sum() > 100  # the render leaves [0, 1] on elements the mask keeps
    assert 0.25 < 1 - m.mean() < 0.35
    assert (m.any(axis=0) != m.all(axis=0)).mean() > 0.5  # the mask differs by channel at most pixels
    assert np.isposinf(np.load(os.path.join(GOLDEN, "eval_identical_3x16x16.npz"))["psnr"])
    assert np.isnan(np.load(os.path.join(GOLDEN, "eval_black_gt_3x8x8.npz"))["psnr"])


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_restatement_matches_reference(path):
    z = np.load(path)
    r = er.evaluate(z["image"], z["gt"], reverse=True)
    ok, what = accepts(z, r)
    assert ok, (what, r["psnr"], z["psnr"], r["ssim"], z["ssim"], r["n"], z["n"])
    # the picture before the reference's channel swap is the reversal of what it appended
    plain = er.evaluate(z["image"], z["gt"], reverse=False, with_ssim=False)
    assert np.array_equal(plain["u8"], z["pred_u8"][:, :, ::-1])
    assert np.array_equal(r["x"], np.clip(z["image"], 0, 1))
    # the ground truth's picture follows the same byte rule: one fp32 multiply, truncation, channels reversed
    assert np.array_equal(er.evaluate(z["gt"], z["gt"], reverse=True, with_ssim=False)["u8"], z["gt_u8"])


@pytest.mark.parametrize("mutant", er.MUTANTS)
def test_comparator_rejects_the_mutant(mutant):
    rejected = []
    for path in FIXTURES:
        z = np.load(path)
        ok, what = accepts(z, er.evaluate(z["image"], z["gt"], reverse=True, mutate=mutant))
        if not ok:
            rejected.append((os.path.basename(path), what))
    assert rejected, mutant


def test_restatement_edge_cases():
    img = np.full((3, 4, 4), 0.5, np.float32)
    gt = np.full((3, 4, 4), 0.25, np.float32)
    img[1, 2, 3] = np.nan
    r = er.evaluate(img, gt)
    assert np.isnan(r["psnr"]) and np.isnan(r["x"][1, 2, 3]) and r["u8"][2, 3, 1] == 0 and r["u8"][0, 0, 0] == 127
    r = er.evaluate(np.full((1, 2, 2), 0.999, np.float32), np.ones((1, 2, 2), np.float32))
    assert r["u8"].max() == 254  # truncated, not rounded


# ---- 2. symbols and argument errors ---------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_argument_errors():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.gsaj_version() >= 106
    for name in ("gsaj_eval_workspace_bytes", "gsaj_eval_frame"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    wb = lib.gsaj_eval_workspace_bytes
    assert wb(3, 64, 48) < wb(3, 65, 48) <= wb(3, 65, 49) and wb(1, 64, 48) < wb(3, 64, 48) < wb(3, 640, 480)
    for C, W, H in ((3, 64, 48), (1, 17, 15), (3, 640, 480), (1, 1, 1)):
        assert wb(C, W, H) >= 4 * C * W * H + lib.gsaj_ssim_workspace_bytes(1, C, W, H)
    assert wb(0, 64, 48) == 0 and wb(3, -1, 48) == 0 and wb(3, 64, 0) == 0 and wb(3, 40000, 40000) == 0
    fake = 0x1000  # never dereferenced: every call below is rejected before any launch
    bad = [
        (0, 64, 48, 0, fake, fake, fake, fake, None, fake, None),
        (3, 0, 48, 0, fake, fake, fake, fake, None, fake, None),
        (3, 64, -2, 0, fake, fake, fake, fake, None, fake, None),
        (3, 40000, 40000, 0, fake, fake, fake, fake, None, fake, None),
        (3, 64, 48, 0, None, fake, fake, fake, None, fake, None),
        (3, 64, 48, 0, fake, None, fake, fake, None, fake, None),
        (3, 64, 48, 0, fake, fake, None, fake, None, fake, None),
        (3, 64, 48, 0, fake, fake, fake, None, None, fake, None),
        (3, 64, 48, 0, fake, fake, fake, fake, None, None, None),
        (3, 64, 48, 2, fake, fake, fake, fake, fake, fake, None),
        (3, 64, 48, -1, fake, fake, fake, fake, fake, fake, None),
    ]
    for args in bad:
        assert lib.gsaj_eval_frame(*args) == -1, args
        msg = lib.gsaj_last_error().decode()
        assert "gsaj_eval_frame" in msg and "invalid argument" in msg, msg


def test_python_layer_refuses_cpu_tensors():
    from gsaj import _lib
    from gsaj.evaluation import FrameEvaluator

    with pytest.raises(_lib.GsajError, match="no CPU path"):
        FrameEvaluator(16, 16, "cpu")


def test_overlay_image_utils_has_the_reference_names():
    from gaussian_splatting.utils import image_utils

    a = torch.tensor([[0.0, 0.5, 1.0, 1.0]])
    b = torch.tensor([[0.0, 0.0, 1.0, 0.0]])
    assert tuple(image_utils.mse(a, b).shape) == (1, 1) and float(image_utils.mse(a, b)) == 0.3125
    assert abs(float(image_utils.psnr(a, b)) - 20 * np.log10(1 / np.sqrt(0.3125))) < 1e-5
    from utils.eval_utils import eval_ate, eval_rendering, save_gaussians  # the reference's import line (slam.py)

    assert callable(eval_ate) and callable(eval_rendering) and callable(save_gaussians)


# ---- 3. trajectory error ----------------------------------------------------------------------------------------------------------
def _rotation(rng, angle=None):
    from scipy.spatial.transform import Rotation

    if angle is None:
        return Rotation.random(random_state=rng.integers(1 << 31)).as_matrix()
    v = rng.normal(size=3)
    return Rotation.from_rotvec(angle * v / np.linalg.norm(v)).as_matrix()


def _poses(positions, rng):
    out = []
    for p in positions:
        T = np.eye(4)
        T[:3, :3] = _rotation(rng)
        T[:3, 3] = p
        out.append(T)
    return out


def _trajectory(rng, n=40):
    t = np.linspace(0, 1, n)
    return np.stack([3 * np.cos(4 * t), 2 * np.sin(3 * t), 0.5 * t], axis=1) + rng.normal(0, 0.2, (n, 3))


@pytest.mark.parametrize("scale", [1.0, 1.7])
def test_ate_recovers_a_known_similarity(scale):
    from gsaj.evaluation import ate

    rng = np.random.default_rng(5)
    est = _trajectory(rng)
    R, t = _rotation(rng), rng.normal(0, 3, 3)
    gt = scale * est @ R.T + t
    extent = np.linalg.norm(gt.max(axis=0) - gt.min(axis=0))
    s = ate(_poses(gt, rng), _poses(est, rng), correct_scale=scale != 1.0)
    # measured: rmse / extent = 9.6e-17 (scale 1), 1.6e-16 (scale 1.7); the closed form is fp64, the bound leaves room for the SVD
    print("ate rmse / extent = %.3g" % (s["rmse"] / extent))
    assert s["rmse"] <= 1e-9 * extent
    assert np.abs(s["R"] - R).max() < 1e-9 and np.abs(s["t"] - t).max() < 1e-8 and abs(s["s"] - scale) < 1e-9
    if scale != 1.0:
        # the scale is estimated only when asked for
        assert ate(_poses(gt, rng), _poses(est, rng), correct_scale=False)["s"] == 1.0
        assert ate(_poses(gt, rng), _poses(est, rng), correct_scale=False)["rmse"] > 1e-2 * extent


@pytest.mark.parametrize("with_scale", [False, True])
def test_ate_alignment_is_a_minimum(with_scale):
    from gsaj.evaluation import ate

    rng = np.random.default_rng(6)
    est = _trajectory(rng)
    gt = 1.3 * est @ _rotation(rng).T + rng.normal(0, 3, 3) + rng.normal(0, 0.05, est.shape)
    s = ate(_poses(gt, rng), _poses(est, rng), correct_scale=with_scale)
    assert s["rmse"] > 1e-3

    def rmse(R, t, c):
        return float(np.sqrt(((gt - (c * est @ R.T + t)) ** 2).sum(axis=1).mean()))

    assert abs(rmse(s["R"], s["t"], s["s"]) - s["rmse"]) < 1e-12
    for k in range(200):
        mag = 10.0 ** rng.uniform(-6, -1)
        R = _rotation(rng, mag) @ s["R"] if k % 3 != 1 else s["R"]
        t = s["t"] + (mag * rng.normal(size=3) if k % 3 != 2 else 0.0)
        c = s["s"] * (1.0 + mag * rng.normal()) if with_scale else 1.0
        assert rmse(R, t, c) >= s["rmse"] * (1 - 1e-12), (k, mag)


def test_ate_rotation_agrees_with_scipy_and_is_proper_for_a_mirrored_set():
    from scipy.spatial.transform import Rotation

    from gsaj.evaluation import ate, umeyama

    rng = np.random.default_rng(7)
    est = _trajectory(rng)
    gt = est @ _rotation(rng).T + rng.normal(0, 3, 3) + rng.normal(0, 0.05, est.shape)
    s = ate(_poses(gt, rng), _poses(est, rng))
    rot, _ = Rotation.align_vectors(gt - gt.mean(axis=0), est - est.mean(axis=0))
    assert np.abs(rot.as_matrix() - s["R"]).max() < 1e-9
    mirrored = est * np.array([-1.0, 1.0, 1.0])
    for with_scale in (False, True):
        R, t, c = umeyama(mirrored.T, est.T, with_scale)
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and c > 0
    assert ate(_poses(est, rng), _poses(mirrored, rng))["rmse"] > 0.1  # a mirror image cannot be rotated onto the original


def _frames(n, rng, device="cpu"):
    frames = []
    for i in range(n):
        gt_T = np.eye(4)
        gt_T[:3, :3] = _rotation(rng)
        gt_T[:3, 3] = rng.normal(size=3)
        T = gt_T.copy()
        T[:3, 3] += rng.normal(0, 0.01, 3)
        f = types.SimpleNamespace(uid=i, R=torch.tensor(T[:3, :3], dtype=torch.float32), T=torch.tensor(T[:3, 3], dtype=torch.float32),
                                  R_gt=torch.tensor(gt_T[:3, :3], dtype=torch.float32), T_gt=torch.tensor(gt_T[:3, 3], dtype=torch.float32))
        frames.append(f)
    return frames


def test_eval_ate_writes_the_reference_files(tmp_path):
    from gsaj.evaluation import ate
    from utils.eval_utils import eval_ate

    rng = np.random.default_rng(8)
    frames = {i: f for i, f in enumerate(_frames(12, rng))}
    kf_ids = [0, 3, 4, 7, 11]
    rmse = eval_ate(frames, kf_ids, str(tmp_path), 25)
    trj = json.load(open(tmp_path / "plot" / "trj_0025.json"))
    assert list(trj) == ["trj_id", "trj_est", "trj_gt"] and trj["trj_id"] == kf_ids
    assert np.asarray(trj["trj_est"]).shape == (5, 4, 4) and np.asarray(trj["trj_gt"]).shape == (5, 4, 4)
    # camera-to-world: the inverse of [R | T]
    f = frames[3]
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = f.R_gt.numpy(), f.T_gt.numpy()
    assert np.abs(np.asarray(trj["trj_gt"][1]) @ w2c - np.eye(4)).max() < 1e-6
    stats = json.load(open(tmp_path / "plot" / "stats_0025.json"))
    assert set(stats) == {"rmse", "mean", "median", "std", "min", "max", "sse"}  # evo's APE.get_all_statistics
    want = ate(trj["trj_gt"], trj["trj_est"])
    assert stats["rmse"] == rmse == want["rmse"] and 0 < rmse < 0.05
    e = want["errors"]
    assert abs(stats["std"] - np.std(e)) < 1e-15 and abs(stats["sse"] - (e ** 2).sum()) < 1e-15 and stats["min"] <= stats["median"] <= stats["max"]
    assert eval_ate(frames, kf_ids, str(tmp_path), 25, final=True, monocular=True) <= rmse
    assert os.path.exists(tmp_path / "plot" / "trj_final.json") and os.path.exists(tmp_path / "plot" / "stats_final.json")


# ---- 4. host logic of eval_rendering and the evaluator's table, the launch replaced by the restatement -------------------------------
@pytest.fixture
def launches(monkeypatch):
    """gsaj.evaluation._launch replaced: records its arguments and writes the restatement's row into the (CPU) table."""
    import gsaj.evaluation as ge

    calls = []

    def fake(C, W, H, flags, image, gt, row, count, u8, ws):
        r = er.evaluate(image.numpy(), gt.numpy(), reverse=bool(flags & 1), with_ssim=False)
        calls.append(dict(shape=(C, H, W), flags=flags, image=image, n=r["n"]))
        with np.errstate(over="ignore"):
            row.copy_(torch.tensor([r["psnr"], 0.25 + 0.5 * r["frac"], r["mse"], r["frac"]], dtype=torch.float32))  # ("ssim": a stand-in)
        count.fill_(r["n"])
        if u8 is not None:
            u8.copy_(torch.from_numpy(r["u8"]))
        ge.FrameEvaluator.clamped(types.SimpleNamespace(_ws=ws, C=C, H=H, W=W)).copy_(torch.from_numpy(r["x"]))

    monkeypatch.setattr(ge, "_launch", fake)
    monkeypatch.setattr(ge, "_DEVICE_TYPES", ("cuda", "cpu"))
    return calls


def _pair(rng, shape=(3, 6, 8)):
    gt = rng.uniform(0, 1, shape).astype(np.float32)
    gt[rng.uniform(size=shape) < 0.2] = 0
    return torch.from_numpy((gt + rng.normal(0, 0.2, shape)).astype(np.float32)), torch.from_numpy(gt)


def test_add_refuses_what_the_kernel_does_not_take(launches):
    """The checks of add() come before the launch, so with the device types patched they run on CPU tensors everywhere."""
    import gsaj.evaluation as ge
    from gsaj import _lib

    ev = ge.FrameEvaluator(16, 12, "cpu")
    d = torch.rand(3, 12, 16)
    with pytest.raises(_lib.GsajError, match="no CPU path"):
        ev.add(d.numpy(), d)
    with pytest.raises(_lib.GsajError, match="no CPU path"):
        ev.add(d.to("meta"), d)
    with pytest.raises(_lib.GsajError, match="float32"):
        ev.add(d.double(), d)
    with pytest.raises(_lib.GsajError, match="float32"):
        ev.add(d, d.half())
    with pytest.raises(_lib.GsajError, match="shape"):
        ev.add(d[:, :8], d[:, :8])
    with pytest.raises(_lib.GsajError, match="shape"):
        ev.add(d[None], d[None])
    with pytest.raises(_lib.GsajError, match="contiguous"):
        ev.add(d.permute(0, 2, 1).contiguous().permute(0, 2, 1), d)
    with pytest.raises(_lib.GsajError, match="u8_out must be torch.uint8"):
        ev.add(d, d, u8_out=torch.zeros(12, 16, 3))
    with pytest.raises(_lib.GsajError, match="u8_out must have shape"):
        ev.add(d, d, u8_out=torch.zeros(3, 12, 16, dtype=torch.uint8))
    with pytest.raises(_lib.GsajError, match="reverse_channels"):
        ev.add(d, d, reverse_channels=True)
    assert ev.n == 0 and not launches
    with pytest.raises(_lib.GsajError, match="capacity"):
        ge.FrameEvaluator(16, 12, "cpu", capacity=0)
    assert ev.add(d, d) == 0 and len(launches) == 1


def test_table_grows_and_keeps_its_rows(launches):
    from gsaj.evaluation import FrameEvaluator

    rng = np.random.default_rng(9)
    pairs = [_pair(rng) for _ in range(11)]
    small, large = FrameEvaluator(8, 6, "cpu", capacity=2), FrameEvaluator(8, 6, "cpu", capacity=64)
    for i, (a, b) in enumerate(pairs):
        assert small.add(a, b) == i and large.add(a, b) == i
    assert small.capacity == 16 and large.capacity == 64 and small.n == 11
    (ts, cs), (tl, cl) = small.rows(), large.rows()
    assert ts.shape == (11, 4) and cs.dtype == np.uint32 and np.array_equal(ts, tl) and np.array_equal(cs, cl)
    assert [int(c) for c in cs] == [c["n"] for c in launches[0::2]]
    s = small.summary()
    assert set(s) == {"mean_psnr", "mean_ssim", "psnr", "ssim", "mse", "count"}
    assert s["mean_psnr"] == float(np.mean([float(v) for v in ts[:, 0]])) and s["count"] == [int(c) for c in cs]
    u8 = torch.zeros(6, 8, 3, dtype=torch.uint8)
    small.add(*pairs[0], u8_out=u8, reverse_channels=True)
    assert launches[-1]["flags"] == 1 and u8.any()
    assert np.isnan(FrameEvaluator(8, 6, "cpu").summary()["mean_psnr"])


@pytest.mark.parametrize("iteration", ["final", "before_opt", 3])
def test_eval_rendering_evaluates_the_reference_frames(launches, monkeypatch, tmp_path, iteration):
    import utils.eval_utils as eu

    rng = np.random.default_rng(10)
    n = 23
    pairs = [_pair(rng) for _ in range(n)]
    frames = [types.SimpleNamespace(uid=i) for i in range(n)]
    dataset = [(gt, None, None) for _, gt in pairs]
    rendered = []

    def fake_render(frame, gaussians, pipe, background):
        rendered.append(frame.uid)
        return {"render": pairs[frame.uid][0]}

    monkeypatch.setattr(eu, "render", fake_render)
    kf = [0, 10]
    pf = {}
    out = eu.eval_rendering(frames, None, dataset, str(tmp_path), None, None, kf, iteration=iteration, per_frame=pf)
    # interval 5 below len(frames) - 1 = 22 whatever `iteration` says (the reference's `or "before_opt"`), keyframes skipped
    assert rendered == [5, 15, 20] == pf["frame_idx"] and set(pf) == {"frame_idx", "psnr", "ssim", "mse", "count"}
    assert list(out) == ["mean_psnr", "mean_ssim", "mean_lpips"] and out["mean_lpips"] is None
    want = [er.evaluate(pairs[i][0].numpy(), pairs[i][1].numpy(), with_ssim=False) for i in rendered]
    assert pf["count"] == [r["n"] for r in want] and pf["psnr"] == [float(np.float32(r["psnr"])) for r in want]
    assert out["mean_psnr"] == float(np.mean([float(np.float32(r["psnr"])) for r in want]))
    assert out["mean_ssim"] == float(np.mean([float(np.float32(0.25 + 0.5 * r["frac"])) for r in want]))
    saved = json.load(open(tmp_path / "psnr" / str(iteration) / "final_result.json"))
    assert saved == out

    seen = []

    def lpips_fn(image, gt):
        seen.append((image.clone(), gt))
        return torch.tensor(0.25 * len(seen))

    out = eu.eval_rendering(frames, None, dataset, str(tmp_path), None, None, kf, iteration=iteration, lpips_fn=lpips_fn)
    assert out["mean_lpips"] == float(np.mean([0.25, 0.5, 0.75])) and len(seen) == 3
    assert torch.equal(seen[1][0], pairs[15][0].clamp(0, 1)) and seen[1][1] is pairs[15][1]  # the clamped image and the gt
    # frames[22] is the last one: a frame at a multiple of 5 equal to len(frames) - 1 is not reached
    del rendered[:]
    eu.eval_rendering(frames[:21], None, dataset, str(tmp_path), None, None, [], iteration=iteration)
    assert rendered == [0, 5, 10, 15]
    # nothing to evaluate: NaN means, empty lists, no evaluator
    pf = {}
    out = eu.eval_rendering(frames[:6], None, dataset, str(tmp_path), None, None, [0], iteration=iteration, per_frame=pf)
    assert np.isnan(out["mean_psnr"]) and np.isnan(out["mean_ssim"]) and pf["frame_idx"] == [] and pf["psnr"] == []
