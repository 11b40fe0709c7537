"""CPU: the fp64 NumPy restatement of the reference SSIM / colour-refinement loss (tests/ssim_restated.py) against the fixtures
the reference produced under CPU autograd (tests/golden/ssim_*.npz, make_ssim_goldens.py); the new C-ABI symbols are exported
and reject invalid arguments before any launch; the Python layer refuses what the kernels do not cover.  No kernel runs."""
import glob
import os

import numpy as np
import pytest
import torch

import ssim_restated as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ssim_*.npz")))


def grad_err(g, ref):
    """max |g - ref| per pixel over max|ref| (the mean divides every gradient by N*C*H*W: raw values say nothing), with a floor
    of 1 / numel for a gradient that vanishes (identical images: S = 1 is a maximum)."""
    return float(np.abs(g - ref).max() / max(np.abs(ref).max(), 1.0 / ref.size))


def test_fixtures_present():
    names = {os.path.basename(f) for f in FIXTURES}
    for case in ("random_3x48x64", "smooth_3x40x56", "identical_3x32x32", "constant_3x24x40", "small_3x5x7", "batch_2x3x24x32",
                 "gray_1x40x36"):
        assert "ssim_%s.npz" % case in names, case
    for f in FIXTURES:
        assert os.path.getsize(f) < 250 * 1024, f


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[5:-4])
def test_restatement_matches_reference(path):
    z = np.load(path)
    a, b = z["img1"], z["img2"]
    a4, b4 = (a, b) if a.ndim == 4 else (a[None], b[None])
    s, sn, smap, g = sr.ssim(a4, b4)
    # the fixtures are the reference's fp32 arithmetic; 5e-4 / 1e-3 hold its rounding on near-constant planes (tests/test_gpu_ssim.py)
    assert abs(s - z["ssim"]) < 5e-4
    assert grad_err(g.reshape(a.shape), z["dssim"]) < 1e-3
    loss, l1, s2, gl = sr.refine_loss(a, b)
    assert abs(loss - z["loss"]) < 1e-4
    assert grad_err(gl, z["dloss"]) < 1e-3
    assert smap.shape == a4.shape and np.all(smap <= 1 + 1e-12)
    if a.ndim == 4:
        assert np.abs(sn - z["ssim_n"]).max() < 5e-4
        S, parts = sr.ssim_forward(a4, b4)
        wpix = (z["wn"].astype(np.float64) / (S[0].size))[:, None, None, None]
        assert grad_err(sr.ssim_backward(a4, b4, parts, wpix), z["dssim_n"]) < 1e-3


def test_blur_adjoint_is_the_transpose():
    rng = np.random.default_rng(3)
    for pad in ("zero", "edge"):
        for shift in (0, 1):
            x, y = rng.normal(size=(2, 2, 9, 13)), rng.normal(size=(2, 2, 9, 13))
            lhs = float((sr.blur(x, pad, shift) * y).sum())
            rhs = float((x * sr.blur_adjoint(y, pad, shift)).sum())
            assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs)), (pad, shift)


def test_restatement_gradient_by_finite_differences():
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 1, (1, 2, 9, 12))
    b = np.clip(a + rng.normal(0, 0.2, a.shape), 0, 1)
    _, _, _, g = sr.refine_loss(a, b)
    for idx in [(0, 0, 0, 0), (0, 1, 4, 6), (0, 1, 8, 11), (0, 0, 3, 11)]:
        e = np.zeros_like(a)
        e[idx] = 1e-6
        fd = (sr.refine_loss(a + e, b)[0] - sr.refine_loss(a - e, b)[0]) / 2e-6
        assert abs(fd - g[idx]) < 1e-6 * max(1.0, abs(g).max() * a.size), idx


def test_new_symbols_exported_and_argument_errors():
    from gsaj import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.gsaj_version() >= 101
    for name in ("gsaj_ssim_workspace_bytes", "gsaj_ssim_forward", "gsaj_ssim_backward", "gsaj_refine_loss_workspace_bytes",
                 "gsaj_refine_loss_seeds"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.gsaj_ssim_workspace_bytes(1, 3, 64, 48) < lib.gsaj_ssim_workspace_bytes(2, 3, 64, 48)
    assert lib.gsaj_ssim_workspace_bytes(1, 3, 64, 48) >= 3 * 4 * 3 * 64 * 48
    assert lib.gsaj_refine_loss_workspace_bytes(64, 48) == lib.gsaj_ssim_workspace_bytes(1, 3, 64, 48)
    assert lib.gsaj_ssim_workspace_bytes(0, 3, 64, 48) == 0
    fake = 0x1000  # never dereferenced: every call below is rejected before any launch
    bad = [
        ("gsaj_ssim_forward", (0, 3, 64, 48, fake, fake, fake, None, fake, None)),
        ("gsaj_ssim_forward", (1, 3, 64, 0, fake, fake, fake, None, fake, None)),
        ("gsaj_ssim_forward", (1, 3, 64, 48, None, fake, fake, None, fake, None)),
        ("gsaj_ssim_forward", (1, 3, 64, 48, fake, fake, None, None, fake, None)),
        ("gsaj_ssim_forward", (1, 3, 64, 48, fake, fake, fake, None, None, None)),
        ("gsaj_ssim_backward", (1, 0, 64, 48, fake, fake, fake, fake, fake, None)),
        ("gsaj_ssim_backward", (1, 3, 64, 48, fake, fake, None, fake, fake, None)),
        ("gsaj_ssim_backward", (1, 3, 64, 48, fake, fake, fake, None, fake, None)),
        ("gsaj_refine_loss_seeds", (64, 48, 1.5, fake, fake, fake, fake, fake, None)),
        ("gsaj_refine_loss_seeds", (-1, 48, 0.2, fake, fake, fake, fake, fake, None)),
        ("gsaj_refine_loss_seeds", (64, 48, 0.2, fake, None, fake, fake, fake, None)),
        ("gsaj_refine_loss_seeds", (64, 48, 0.2, fake, fake, fake, fake, None, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        msg = lib.gsaj_last_error().decode()
        assert name in msg and "invalid argument" in msg, msg


def test_python_layer_refuses_outside_the_kernel_domain():
    from gsaj import _lib, ssim as gssim

    a = torch.rand(3, 16, 16)
    with pytest.raises(_lib.GsajError, match="device"):
        gssim.ssim(a, a)  # CPU tensors: no CPU fallback
    from gsaj import losses

    with pytest.raises(_lib.GsajError, match="HIP device"):
        losses.RefinementLoss(16, 16, "cpu")
    if torch.cuda.is_available():
        d = a.cuda()
        with pytest.raises(_lib.GsajError, match="float32"):
            gssim.ssim(d.double(), d.double())
        with pytest.raises(_lib.GsajError, match="window_size"):
            gssim.ssim(d, d, window_size=7)
        with pytest.raises(_lib.GsajError, match="img2"):
            gssim.ssim(d, d.clone().requires_grad_(True))


def test_overlay_loss_utils_has_the_reference_names():
    from gaussian_splatting.utils import loss_utils

    for name in ("l1_loss", "l2_loss", "ssim"):
        assert callable(getattr(loss_utils, name))
    assert not hasattr(loss_utils, "l1_loss_weight")
    x, y = torch.tensor([0.0, 1.0, 3.0]), torch.tensor([1.0, 1.0, 1.0])
    assert float(loss_utils.l1_loss(x, y)) == 1.0
    assert abs(float(loss_utils.l2_loss(x, y)) - 5.0 / 3.0) < 1e-7
