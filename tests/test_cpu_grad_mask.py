"""CPU: the NumPy restatement of the tracking gradient mask (tests/grad_mask_restated.py) and the torch mirrors of
utils/slam_utils.py against outputs recorded from the reference (tests/golden/grad_mask_*.npz, written by
tests/golden/make_grad_mask_goldens.py); canaries showing that the comparator rejects seven wrong restatements; the argument
errors of the C ABI that need no GPU.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

import grad_mask_restated as gr

CASES = ("noise_64x96", "noise_68x100", "noise_97x131", "noise_100x170", "checker_68x100", "dyadic_68x100", "bright_68x100")
THRESHOLDS = (1.1, 4.0)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return {name: dict(np.load(os.path.join(golden_dir, "grad_mask_%s.npz" % name))) for name in CASES}


def compare(got, rec, i, blocks):
    """The comparator: a restatement's result against the recorded reference output of threshold i.  Masks (and the 0 / 1 float
    image inside the blocks) must be equal EXACTLY; intensities and the leftover strips of block mode, which carry the reference's
    own conv2d rounding, within 16 * 2^-24 * max|gray| (grad_mask_restated.tolerance)."""
    bound = gr.tolerance(0.0, np.abs(rec["gray"]).max())
    assert np.abs(got["I"].astype(np.float64) - rec["intensity"]).max() <= bound, "intensity"
    if not blocks:
        want = rec["global_%d" % i]
        assert got["value"].dtype == np.bool_ and want.dtype == np.bool_
        assert np.array_equal(got["value"], want), "global mask: %d pixels differ" % int((got["value"] != want).sum())
        return
    want = rec["block_%d" % i]
    H, W = want.shape
    bh, bw = gr.block_shape(H, W)
    inside = np.zeros((H, W), bool)
    inside[:gr.GRID * bh, :gr.GRID * bw] = True
    assert got["value"].dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got["value"][inside], want[inside]), "blocks: %d pixels differ" % int((got["value"] != want)[inside].sum())
    if (~inside).any():
        assert np.abs(got["value"][~inside].astype(np.float64) - want[~inside]).max() <= bound, "leftover strip"
    assert np.array_equal(got["u8"], want.astype(np.uint8)), "byte mask"


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_recorded_reference(recorded, name):
    rec = recorded[name]
    assert np.array_equal(gr.make_scene(name.split("_")[0], *rec["image"].shape[1:]), rec["image"])  # the scenes are reproducible
    I, _, _, valid, gray = gr.intensity(rec["image"])
    assert np.array_equal(gray, rec["gray"]) and np.array_equal(valid, rec["valid"])
    for i, thr in enumerate(THRESHOLDS):
        assert float(rec["thresholds"][i]) == thr
        for blocks in (False, True):
            compare(gr.grad_mask(rec["image"], thr, blocks), rec, i, blocks)


def test_fixtures_exercise_what_they_are_for(recorded):
    """Zero-median blocks, quirk A, leftover strips, odd and even counts: a fixture that lost one of them would test less."""
    b = gr.grad_mask(recorded["noise_100x170"]["image"], 1.1, True)
    assert (b["t"][b["visited"]] == 0).any() and (~b["visited"]).sum() == 100 * 170 - 96 * 160
    q = gr.grad_mask(recorded["checker_68x100"]["image"], 4.0, True)
    assert (q["t"][q["visited"]] >= 1).any() and not q["value"][q["visited"]].any()
    assert gr.grad_mask(recorded["checker_68x100"]["image"], 1.1, True)["value"][q["visited"]].any()
    # intensities above a threshold of 1 or more: only quirk A zeroes them; and the leftover strips hold bytes of 1
    br = gr.grad_mask(recorded["bright_68x100"]["image"], 1.1, True)
    assert ((br["I"] > br["t"]) & (br["t"] >= 1) & br["visited"]).any() and not br["value"][br["visited"]].any()
    assert (br["u8"][~br["visited"]] == 1).any()
    assert gr.block_shape(100, 170) == (3, 5) and (68 * 100) % 2 == 0 and (97 * 131) % 2 == 1
    assert recorded["noise_68x100"]["intensity"].max() < 1  # images in [0, 1]: the strips' bytes are 0


MUTANTS = ("mutant_pad_zero", "mutant_strip_norm16", "mutant_upper_median", "mutant_ge", "mutant_no_quirk_a", "mutant_strip_zero",
           "mutant_ceil_blocks")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_comparator_rejects_wrong_restatements(recorded, mutant):
    rejected = []
    for name in CASES:
        for i, thr in enumerate(THRESHOLDS):
            for blocks in (False, True):
                try:
                    compare(gr.grad_mask(recorded[name]["image"], thr, blocks, **{mutant: True}), recorded[name], i, blocks)
                except AssertionError as e:
                    rejected.append((name, thr, blocks, str(e).split(":")[0]))
    assert rejected, "the comparator accepted %s on every fixture" % mutant
    if mutant in ("mutant_strip_norm16", "mutant_strip_zero"):  # the strips exist in block mode only, and not at 64 x 96
        assert all(blocks and name != "noise_64x96" for name, _, blocks, _ in rejected), rejected
        assert {name for name, _, _, _ in rejected} == set(CASES) - {"noise_64x96"}
    if mutant == "mutant_no_quirk_a":
        assert [r[:3] for r in rejected] == [("bright_68x100", 1.1, True)]
    if mutant == "mutant_pad_zero":
        assert len(rejected) == len(CASES) * 4  # the border of every image


@pytest.mark.parametrize("name", CASES)
def test_torch_mirrors_match_recorded_reference(recorded, name):
    from utils.slam_utils import image_gradient, image_gradient_mask

    rec = recorded[name]
    gray = torch.from_numpy(rec["image"]).mean(dim=0, keepdim=True)
    assert torch.equal(gray[0], torch.from_numpy(rec["gray"]))
    gv, gh = image_gradient(gray)
    mv, mh = image_gradient_mask(gray)
    assert gv.shape == gray.shape and gh.shape == gray.shape and mv.dtype == torch.bool
    bound = gr.tolerance(0.0, np.abs(rec["gray"]).max())
    assert np.abs(gv[0].numpy().astype(np.float64) - rec["gv"]).max() <= bound
    assert np.abs(gh[0].numpy().astype(np.float64) - rec["gh"]).max() <= bound
    assert np.array_equal(mv[0].numpy(), rec["valid"]) and torch.equal(mv, mh)
    inten = torch.sqrt((gv * mv) ** 2 + (gh * mh) ** 2)[0].numpy()
    assert np.abs(inten.astype(np.float64) - rec["intensity"]).max() <= bound
    for i, thr in enumerate(THRESHOLDS):  # the global form through the mirrors gives the recorded mask
        assert np.array_equal(inten > np.float32(gr.lower_median(inten) * np.float32(thr)), rec["global_%d" % i])


def test_depth_reg_mirror():
    from utils.slam_utils import depth_reg

    g = torch.Generator().manual_seed(3)
    gt = torch.rand(3, 12, 17, generator=g)
    depth = torch.rand(1, 12, 17, generator=g) + 0.5
    assert float(depth_reg(torch.full((1, 12, 17), 2.0), gt)) == 0.0  # a flat depth has no gradient
    val = depth_reg(depth, gt)
    assert val.dim() == 0 and float(val) > 0
    depth[0, 5, 5] = 0.0  # an invalid depth pixel removes its 3 x 3 neighbourhood from both means, nothing else
    from utils.slam_utils import image_gradient_mask
    assert int((~image_gradient_mask(depth)[0]).sum()) == 9 and torch.isfinite(depth_reg(depth, gt))


def test_argument_errors_need_no_gpu():
    from gsaj import _lib
    from gsaj.grad_mask import GradMask

    lib = _lib.load()
    assert lib.gsaj_grad_mask_workspace_bytes(640, 480) > 640 * 480 * 4 + lib.gsaj_seed_workspace_bytes(640, 480)
    assert lib.gsaj_grad_mask_workspace_bytes(1, 480) == 0
    fake = 4096  # never dereferenced: every call below returns before it launches anything
    assert lib.gsaj_grad_mask(31, 64, fake, 1.1, 1, fake, fake, fake, None) == -1  # empty blocks: the reference raises
    assert b"block mode needs W >= 32" in lib.gsaj_last_error()
    assert lib.gsaj_grad_mask(2080, 2080, fake, 1.1, 1, fake, fake, fake, None) == -1  # 65 x 65 = 4225 pixels per block
    assert b"exceeds" in lib.gsaj_last_error()
    assert lib.gsaj_grad_mask(64, 1, fake, 1.1, 0, fake, fake, fake, None) == -1
    assert lib.gsaj_grad_intensity(64, 64, None, fake, None) == -1
    with pytest.raises(_lib.GsajError, match="no CPU path"):
        GradMask(64, 64, "cpu")
