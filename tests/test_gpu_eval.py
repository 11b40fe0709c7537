"""GPU: gsaj_eval_frame through gsaj.evaluation.FrameEvaluator against the NumPy restatement (tests/eval_restated.py) and the
reference's fixtures (tests/golden/eval_*.npz); both load widths; reproducibility; the growing table; utils.eval_utils.eval_rendering
end to end.

Bounds, u = 2^-24 (none of them comes from what the kernel gives):
  clamped plane, bytes, n   exact: each is one fp32 operation per element, or an integer.
  mse                       2 u relative: the fp64 sums of device and restatement differ by ~1e-16 relative whatever their order,
                            then ONE rounding to fp32 (u); the second u is room for a restatement sum that lands on a rounding tie.
  psnr                      32 u + 8 u |psnr| (eval_restated.psnr_bound_device): mse one rounding, the square root and the division one
                            each, log10f <= 2 ulp of its result, the final product one rounding, carried through 20 log10.
  ssim                      mean of tests/test_gpu_ssim.py's per-pixel map_bound.
The worst err / bound per column goes into profiles/r13_eval_parity.json when GSAJ_WRITE_PARITY is set.
"""
import glob
import json
import os

import numpy as np
import pytest

import eval_restated as er
from test_gpu_ssim import map_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "eval_*.npz")))
PARITY = os.path.join(ROOT, "profiles", "r13_eval_parity.json")
U = er.U
GUARD = 64  # floats (a multiple of 4: the guard keeps the 16-byte alignment of the allocation)
SENTINEL = -7.25
# C, H, W: one element; under one workgroup and no multiple of 4; whole workgroups exactly; gray and odd; odd with many workgroups;
# 900 workgroups, so that k_eval_finalize loops
SHAPES = [(1, 1, 1), (3, 5, 7), (3, 16, 16), (1, 17, 15), (3, 97, 131), (3, 480, 640)]
WORST = {}


def _dev():
    import torch

    return torch.device("cuda:0")


def make_pair(shape, seed):
    """A render that leaves [0, 1] on both sides and a ground truth with single channel values at 0 (about a fifth)."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.02, 1.0, shape).astype(np.float32)
    if gt.size > 1:
        gt[rng.uniform(size=shape) < 0.2] = 0.0
    image = (gt + rng.uniform(-0.35, 0.35, shape)).astype(np.float32)
    return image, gt


def guarded(a, offset, dtype=None):
    """a inside a sentinel-guarded device buffer, `offset` elements past a 16-byte-aligned address -> (buffer, view shaped like a)."""
    import torch

    dtype = dtype or torch.float32
    buf = torch.full((a.size + 2 * GUARD + 4,), SENTINEL if dtype == torch.float32 else 0xA5, dtype=dtype, device=_dev())
    view = buf[GUARD + offset:GUARD + offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


def guards_intact(buf, a, offset):
    import torch

    h = buf.cpu().numpy()
    fill = np.float32(SENTINEL) if buf.dtype == torch.float32 else np.uint8(0xA5)
    lo, hi = GUARD + offset, GUARD + offset + a.size
    return bool((h[:lo] == fill).all() and (h[hi:] == fill).all()), h[lo:hi].reshape(a.shape)


def note(case, ratios):
    slot = WORST.setdefault(case, {})
    for k, v in ratios.items():
        slot[k] = max(slot.get(k, 0.0), float(v))
    if os.environ.get("GSAJ_WRITE_PARITY"):
        doc = dict(what="worst |device - restatement| / bound per column of gsaj_eval_frame's row and per shape C x H x W, both load "
                        "widths (tests/test_gpu_eval.py); clamped plane, bytes and n are exact",
                   bounds=dict(mse="2 u relative", psnr="32 u + 8 u |psnr|", ssim="mean of test_gpu_ssim.map_bound", u="2^-24"),
                   worst_err_over_bound=WORST)
        with open(PARITY, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")


def compare(row, count, r, tag):
    """One device row against the restatement r -> err / bound per column (asserted <= 1)."""
    psnr, ssim, mse, frac = (float(v) for v in row)
    assert int(count) == r["n"], (tag, int(count), r["n"])
    assert frac == float(np.float32(r["frac"])), (tag, frac, r["frac"])
    ratios = {}
    if er.same_special(mse, r["mse"]) is None:
        ratios["mse"] = abs(mse - r["mse"]) / (2 * U * abs(r["mse"])) if r["mse"] else float(mse != 0)
    else:
        assert er.same_special(mse, r["mse"]), (tag, mse, r["mse"])
    if er.same_special(psnr, r["psnr"]) is None:
        ratios["psnr"] = abs(psnr - r["psnr"]) / er.psnr_bound_device(r["psnr"])
    else:
        assert er.same_special(psnr, r["psnr"]), (tag, psnr, r["psnr"])
    ratios["ssim"] = abs(ssim - r["ssim"]) / float(map_bound(r["ssim_partials"], r["ssim_map"]).mean())
    print("%s: psnr %.9g (want %.12g) mse %.9g (want %.12g) ssim %.9g (want %.12g) err/bound %s" % (tag, psnr, r["psnr"], mse, r["mse"], ssim, r["ssim"], ratios))
    for k, v in ratios.items():
        assert v <= 1.0, (tag, k, v)
    return ratios


# ---- 1. the device against the restatement, both load widths -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_device_matches_restatement(shape):
    import torch
    from gsaj.evaluation import FrameEvaluator

    C, H, W = shape
    image, gt = make_pair(shape, 100 + H)
    want = {rev: er.evaluate(image, gt, reverse=rev, with_ssim=not rev) for rev in (False, True)}
    r = want[False]
    assert 0 < r["n"] and (r["n"] < image.size or image.size == 1)
    ev = FrameEvaluator(W, H, _dev(), C=C, capacity=4)
    for offset in (0, 1):  # 16-byte aligned: 16 bytes per lane; 4 bytes past: a dword per lane
        ib, iv = guarded(image, offset)
        gb, gv = guarded(gt, offset)
        assert (iv.data_ptr() % 16 == 0) == (offset == 0) and gv.data_ptr() % 16 == iv.data_ptr() % 16
        for rev in (False, True):
            ub, uv = guarded(np.zeros((H, W, C), np.uint8), 3 * offset, torch.uint8)
            i = ev.add(iv, gv, u8_out=uv, reverse_channels=rev)
            x = ev.clamped().cpu().numpy()
            ok, u8 = guards_intact(ub, want[rev]["u8"], 3 * offset)
            assert ok, "bytes written outside image_u8"
            assert np.array_equal(u8, want[rev]["u8"]), (offset, rev)
            assert np.array_equal(x.view(np.uint32), r["x"].view(np.uint32)), (offset, rev)
        t, c = ev.rows()
        for j in (i - 1, i):
            note("%dx%dx%d" % shape, compare(t[j], c[j], r, "%dx%dx%d offset %d row %d" % (C, H, W, offset, j)))
        assert np.array_equal(t[i - 1].view(np.uint32), t[i].view(np.uint32))  # the bytes and their order do not touch the row
        for buf, a in ((ib, image), (gb, gt)):
            ok, inner = guards_intact(buf, a, offset)
            assert ok and np.array_equal(inner.view(np.uint32), a.view(np.uint32)), "an input or its guard was written"
    assert ev.n == 4 and ev.capacity == 4


# ---- 2. the reference's fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_fixtures_through_the_evaluator(path):
    import torch
    from gsaj.evaluation import FrameEvaluator

    z = np.load(path)
    image, gt = z["image"], z["gt"]
    C, H, W = image.shape
    ev = FrameEvaluator(W, H, _dev(), C=C)
    x, y = torch.from_numpy(image).to(_dev()), torch.from_numpy(gt).to(_dev())
    rev, plain = torch.zeros((H, W, C), dtype=torch.uint8, device=_dev()), torch.zeros((H, W, C), dtype=torch.uint8, device=_dev())
    ev.add(x, y, u8_out=rev, reverse_channels=True)
    ev.add(x, y, u8_out=plain)
    ev.add(x, y)
    t, c = ev.rows()
    assert np.array_equal(rev.cpu().numpy(), z["pred_u8"]) and np.array_equal(plain.cpu().numpy(), z["pred_u8"][:, :, ::-1])
    assert [int(v) for v in c] == [int(z["n"])] * 3
    assert np.array_equal(t[0].view(np.uint32), t[1].view(np.uint32)) and np.array_equal(t[0].view(np.uint32), t[2].view(np.uint32))
    r = er.evaluate(image, gt)
    psnr, ssim = float(t[0, 0]), float(t[0, 1])
    special = er.same_special(psnr, z["psnr"])
    if special is None:  # the fixture is the reference's fp32 arithmetic: allow both roundings
        assert abs(psnr - float(z["psnr"])) <= er.psnr_bound_reference(r["n"], r["psnr"]) + er.psnr_bound_device(r["psnr"]), (psnr, z["psnr"])
    else:
        assert special, (psnr, z["psnr"])  # inf (identical) and NaN (black gt) as such
    assert abs(ssim - float(z["ssim"])) <= 2 * map_bound(r["ssim_partials"], r["ssim_map"]).mean() + 1e-6, (ssim, z["ssim"])
    s = ev.summary()
    assert np.array_equal(s["psnr"], [psnr] * 3, equal_nan=True) and s["count"] == [int(z["n"])] * 3


def test_nan_in_the_render():
    import torch
    from gsaj.evaluation import FrameEvaluator

    image, gt = make_pair((3, 9, 11), 3)
    image[2, 4, 5] = np.nan
    r = er.evaluate(image, gt, with_ssim=False)
    assert gt[2, 4, 5] > 0 and r["u8"][4, 5, 2] == 0
    ev = FrameEvaluator(11, 9, _dev())
    u8 = torch.full((9, 11, 3), 9, dtype=torch.uint8, device=_dev())
    ev.add(torch.from_numpy(image).to(_dev()), torch.from_numpy(gt).to(_dev()), u8_out=u8)
    t, c = ev.rows()
    assert np.isnan(t[0, 0]) and np.isnan(t[0, 2]) and int(c[0]) == r["n"] and np.array_equal(u8.cpu().numpy(), r["u8"])
    assert np.isnan(ev.clamped().cpu().numpy()[2, 4, 5])


# ---- 3. reproducible; the workspace can be used again; the table grows ---------------------------------------------------------------
def test_two_runs_identical_bits_and_the_workspace_is_reusable():
    import torch
    from gsaj.evaluation import FrameEvaluator

    image, gt = make_pair((3, 97, 131), 21)
    other = make_pair((3, 97, 131), 22)
    x, y = torch.from_numpy(image).to(_dev()), torch.from_numpy(gt).to(_dev())
    tables = []
    for _ in range(2):
        ev = FrameEvaluator(131, 97, _dev())
        ev.add(x, y)
        ev.add(torch.from_numpy(other[0]).to(_dev()), torch.from_numpy(other[1]).to(_dev()))
        ev.add(x, y)  # the SSIM ticket was reset, the partials of the frame between are gone
        t, c = ev.rows()
        assert np.array_equal(t[0].view(np.uint32), t[2].view(np.uint32)) and c[0] == c[2]
        assert not np.array_equal(t[0], t[1])
        tables.append((t, c))
    assert np.array_equal(tables[0][0].view(np.uint32), tables[1][0].view(np.uint32)) and np.array_equal(tables[0][1], tables[1][1])


def test_300_rows_into_a_table_of_4_and_of_512():
    import torch
    from gsaj.evaluation import FrameEvaluator

    g = torch.Generator().manual_seed(5)
    images = (torch.rand(300, 3, 5, 7, generator=g) * 1.4 - 0.2).to(_dev())
    gts = torch.rand(300, 3, 5, 7, generator=g)
    gts[torch.rand(gts.shape, generator=g) < 0.2] = 0.0
    gts = gts.to(_dev())
    small, large = FrameEvaluator(7, 5, _dev(), capacity=4), FrameEvaluator(7, 5, _dev(), capacity=512)
    for k in range(300):
        assert small.add(images[k], gts[k]) == k == large.add(images[k], gts[k])
    assert small.capacity == 512 and large.capacity == 512 and small.n == 300
    (ts, cs), (tl, cl) = small.rows(), large.rows()
    assert ts.shape == (300, 4) and np.array_equal(ts.view(np.uint32), tl.view(np.uint32)) and np.array_equal(cs, cl)
    for k in (0, 3, 4, 255, 256, 299):  # rows on both sides of every growth
        r = er.evaluate(images[k].cpu().numpy(), gts[k].cpu().numpy())
        compare(ts[k], cs[k], r, "row %d" % k)


# ---- 4. eval_rendering end to end ----------------------------------------------------------------------------------------------------------
class _Pipe:
    convert_SHs_python = False
    compute_cov3D_python = False


def test_eval_rendering_end_to_end(tmp_path):
    import torch
    from gaussian_splatting.gaussian_renderer import render
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gaussian_splatting.utils.image_utils import psnr as torch_psnr
    from gsaj import ssim as gssim
    from gsaj import synthetic as syn
    from utils.camera_utils import Camera
    from utils.eval_utils import eval_rendering

    W, H = 100, 75
    kw = dict(W=W, H=H, fx=90.0, fy=90.0, cx=49.5, cy=37.0)
    cams = syn.keyframe_cameras(12, **kw)
    # (small Gaussians: about a quarter of the pixels stay background, exactly 0, so the mask is not trivial)
    sc = syn.make_scene(500, 7, cams[0], z_range=(1.0, 5.0), log_scale_range=(np.log(0.005), np.log(0.04)), sh_coeffs=1)
    model = GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"], sh_degree=0, device=_dev())
    bg = torch.zeros(3, device=_dev())
    frames = [Camera.from_synthetic(c, uid=i, device=_dev()) for i, c in enumerate(cams)]
    nudge = np.eye(4)
    nudge[0, 3], nudge[1, 3] = 0.01, -0.005  # the ground truth is the render from a slightly different pose
    dataset = []
    with torch.no_grad():
        for c in cams:
            view = Camera.from_synthetic(syn.make_camera(nudge @ c["w2c"], **kw), device=_dev())
            dataset.append((render(view, model, _Pipe, bg)["render"].detach().clone().contiguous(), None, None))
        pf = {}
        out = eval_rendering(frames, model, dataset, str(tmp_path), _Pipe, bg, [5], iteration="final", per_frame=pf)
        assert pf["frame_idx"] == [0, 10]  # interval 5 below len(frames) - 1 = 11, keyframe 5 skipped
        for k, idx in enumerate(pf["frame_idx"]):
            # the reference's statement, in torch on the same tensors
            gt_image = dataset[idx][0]
            image = torch.clamp(render(frames[idx], model, _Pipe, bg)["render"], 0.0, 1.0)
            mask = gt_image > 0
            n = int(mask.sum())
            assert 0 < n < mask.numel() and pf["count"][k] == n
            ps = float(torch_psnr(image[mask].unsqueeze(0), gt_image[mask].unsqueeze(0)))
            ss = float(gssim.ssim(image.unsqueeze(0), gt_image.unsqueeze(0)))
            got = pf["psnr"][k]
            assert 5.0 < ps < 60.0 and abs(got - ps) <= er.psnr_bound_reference(n, ps) + er.psnr_bound_device(ps), (idx, got, ps)
            assert pf["ssim"][k] == ss  # the same kernel on the same clamped image
    assert out["mean_psnr"] == float(np.mean(pf["psnr"])) and out["mean_ssim"] == float(np.mean(pf["ssim"]))
    assert out["mean_lpips"] is None and json.load(open(tmp_path / "psnr" / "final" / "final_result.json")) == out
