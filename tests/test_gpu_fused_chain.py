"""GPU: the whole-window batched backward forms a (view, Gaussian)'s ten sums INSIDE k_chain_window (the row walk of k_gather_sums on
k_gather_sums' own grid of 64-row groups, no gsum round trip), the split sequence GSAJ_BWD_ONLY_COMPOSITE -> GSAJ_BWD_ONLY_CHAIN
goes through k_gather_sums and gsum as before.  Same additions in the same order: every output of the two must be the SAME BITS
(torch.equal, no tolerance) -- the summed per-Gaussian gradients, the per-view dL/dmean2D and dL/dtau rows, the per-view dL/dtau
sums -- and the sums summed again on demand after the fused call (BatchContext.view_sums) must be the bits the split sequence left
in the workspace.  Cases: the bench's cfg2 window; small scenes with K = 3 (partial group of views), K = 11 (second launch of 8
views, accumulating), Gaussian counts that are not multiples of 32 or 64, a view that sees nothing, both record formats, every
SH storage size."""
import numpy as np
import pytest

import helpers as hp
from gsaj import synthetic as syn

pytestmark = pytest.mark.gpu

OUTPUTS = ("mean2D", "opacity", "mean3D", "cov3D", "sh", "scale", "rot", "tau", "tau_all")


def _window(K, cams, sc, deg, record_bits, dLc, dLd, split, bg=(0.1, 0.2, 0.3)):
    """forward + backward of one window; -> (context, {name: clone of every gradient array}, [view_sums(v)])"""
    import torch
    from gsaj.rasterizer import BatchContext

    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    P, W, H, M = sc["means3D"].shape[0], cams[0]["W"], cams[0]["H"], sc["shs"].shape[1]
    kw = dict(sh_degree=deg, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    views, projs, cps = (t(np.stack([c[k] for c in cams])) for k in ("viewmatrix", "projmatrix", "campos"))
    praw, bgt, means = t(cams[0]["projmatrix_raw"]), t(np.array(bg)), t(sc["means3D"])
    bc = BatchContext(K, P, W, H, M, dev, record_bits=record_bits, per_gaussian_tau=True)
    st = bc.forward(bgt, means, t(sc["opacities"]), views, projs, cps, cams[0]["tanfovx"], cams[0]["tanfovy"], **kw)
    assert not any(ab for _, _, ab in st)
    g = bc.backward(bgt, means, views, projs, praw, cps, cams[0]["tanfovx"], cams[0]["tanfovy"], t(dLc), t(dLd), split=split, **kw)
    out = {n: g[n].clone() for n in OUTPUTS}
    # fused: summed again from the instance rows; split: what k_gather_sums left in the workspace for the chain
    sums = [bc.view_sums(v, stored=split) for v in range(K)]
    return bc, out, sums


def _assert_same_bits(K, cams, sc, deg, record_bits, dLc, dLd, bg=(0.1, 0.2, 0.3)):
    import torch

    bf, fused, sums_f = _window(K, cams, sc, deg, record_bits, dLc, dLd, False, bg)
    bs, split, sums_s = _window(K, cams, sc, deg, record_bits, dLc, dLd, True, bg)
    assert torch.equal(bf.radii, bs.radii)
    for n in OUTPUTS:
        assert torch.isfinite(fused[n]).all(), n
        assert torch.equal(fused[n], split[n]), "dL/d%s: fused and split backward differ (max |diff| %.3e of max %.3e)" % (
            n, float((fused[n] - split[n]).abs().max()), float(split[n].abs().max()))
    for v in range(K):
        assert torch.equal(sums_f[v], sums_s[v]), "view %d: the sums summed on demand differ from the ones the split backward stored" % v
    # (not vacuous: something was rendered and back-propagated)
    assert float(fused["mean3D"].abs().max()) > 0.0 and max(float(x.abs().max()) for x in sums_f) > 0.0
    return bf, fused


def _blind_camera(cam):
    """the same intrinsics, looking the other way: every Gaussian of the scene lies behind it"""
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])
    return syn.make_camera(flip @ cam["w2c"], **{k: cam[k] for k in ("W", "H", "fx", "fy", "cx", "cy")})


@pytest.mark.parametrize("K,P,coeffs,bits,blind", [(3, 1000, 16, 32, 1), (11, 1000, 16, 32, 9), (3, 77, 4, 16, None), (11, 2049, 1, 16, 0),
                                                   (8, 2500, 9, 32, 7), (1, 33, 16, 32, None)])
def test_fused_backward_equals_split_backward_bit_for_bit(K, P, coeffs, bits, blind):
    import torch  # noqa: F401

    W, H = 200, 150
    cam0 = hp.small_camera(W, H, f=0.8 * W, orthonormal=True)
    sc = syn.make_scene(P, 11 + P, cam0, z_range=(0.8, 3.0), log_scale_range=(np.log(0.01), np.log(0.2)), sh_coeffs=coeffs, margin=0.2)
    cams = syn.keyframe_cameras(K, radius=0.2, W=W, H=H, fx=cam0["fx"], fy=cam0["fy"], cx=cam0["cx"], cy=cam0["cy"])
    if blind is not None:
        cams[blind] = _blind_camera(cams[blind])
    deg = int(round(coeffs ** 0.5)) - 1
    seeds = [hp.seeds(c, seed=70 + k) for k, c in enumerate(cams)]
    dLc, dLd = np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds])
    bc, fused = _assert_same_bits(K, cams, sc, deg, bits, dLc, dLd)
    if blind is not None:
        assert int(bc.radii[blind].max()) == 0  # nothing visible in that view
        assert float(fused["mean2D"][blind].abs().max()) == 0.0 and float(fused["tau_all"][blind].abs().max()) == 0.0
    assert int((bc.radii > 0).sum()) > 0


@pytest.mark.parametrize("bits", [32, 16])
def test_fused_backward_equals_split_backward_on_the_bench_window(bits):
    """cfg2, the 8 keyframes and the pixel-gradient seeds bench.py runs (rank 0)."""
    K = 8
    cam0, sc = syn.config_scene("cfg2")
    cams = syn.keyframe_cameras(K, **{k: cam0[k] for k in ("W", "H", "fx", "fy", "cx", "cy")})
    W, H = cam0["W"], cam0["H"]
    rng = np.random.default_rng(1234)
    dLc = (rng.normal(size=(K, 3, H, W)) / (3 * H * W)).astype(np.float32)
    dLd = (rng.normal(size=(K, 1, H, W)) / (H * W)).astype(np.float32)
    _assert_same_bits(K, cams, sc, 3, bits, dLc, dLd, bg=(0.0, 0.0, 0.0))
