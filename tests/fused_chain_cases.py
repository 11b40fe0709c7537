"""The windows of tests/test_gpu_fused_chain.py and tools/backward_same_bits.py: one forward + backward of a BatchContext, whole-window
(the chain kernel sums the instance rows itself) or split (k_gather_sums, gsum, then the chain), and the cases both run.

SMALL: K = 3 (partial group of views), K = 11 (second launch of 8 views, accumulating), Gaussian counts that are not multiples of 32
or 64, a view that sees nothing, both record formats, every SH storage size.  bench_case: the bench's cfg2 window.  planted_case: the
smallest scene in which the row walk's corners all occur -- see there."""
import numpy as np

import helpers as hp
from gsaj import synthetic as syn

OUTPUTS = ("mean2D", "opacity", "mean3D", "cov3D", "sh", "scale", "rot", "tau", "tau_all")
SMALL = [(3, 1000, 16, 32, 1), (11, 1000, 16, 32, 9), (3, 77, 4, 16, None), (11, 2049, 1, 16, 0), (8, 2500, 9, 32, 7), (1, 33, 16, 32, None)]
PLANTED = (31, 32, 63, 64)   # the Gaussians of planted_case that touch every tile
BG = (0.1, 0.2, 0.3)


def window(K, cams, sc, deg, record_bits, dLc, dLd, split, bg=BG):
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


def blind_camera(cam):
    """the same intrinsics, looking the other way: every Gaussian of the scene lies behind it"""
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])
    return syn.make_camera(flip @ cam["w2c"], **{k: cam[k] for k in ("W", "H", "fx", "fy", "cx", "cy")})


def _pixel_seeds(cams):
    seeds = [hp.seeds(c, seed=70 + k) for k, c in enumerate(cams)]
    return np.stack([s[0] for s in seeds]), np.stack([s[1] for s in seeds])


def small_case(K, P, coeffs, bits, blind):
    """-> the arguments of window() up to `split`"""
    W, H = 200, 150
    cam0 = hp.small_camera(W, H, f=0.8 * W, orthonormal=True)
    sc = syn.make_scene(P, 11 + P, cam0, z_range=(0.8, 3.0), log_scale_range=(np.log(0.01), np.log(0.2)), sh_coeffs=coeffs, margin=0.2)
    cams = syn.keyframe_cameras(K, radius=0.2, W=W, H=H, fx=cam0["fx"], fy=cam0["fy"], cx=cam0["cx"], cy=cam0["cy"])
    if blind is not None:
        cams[blind] = blind_camera(cams[blind])
    return (K, cams, sc, int(round(coeffs ** 0.5)) - 1, bits) + _pixel_seeds(cams)


def bench_case(bits):
    """cfg2, the 8 keyframes and the pixel-gradient seeds bench.py runs (rank 0); its background is black"""
    K = 8
    cam0, sc = syn.config_scene("cfg2")
    cams = syn.keyframe_cameras(K, **{k: cam0[k] for k in ("W", "H", "fx", "fy", "cx", "cy")})
    W, H = cam0["W"], cam0["H"]
    rng = np.random.default_rng(1234)
    dLc = (rng.normal(size=(K, 3, H, W)) / (3 * H * W)).astype(np.float32)
    dLd = (rng.normal(size=(K, 1, H, W)) / (H * W)).astype(np.float32)
    return K, cams, sc, 3, bits, dLc, dLd


def planted_case():
    """224 x 176 (14 x 11 = 154 tiles), P = 96 (one and a half blocks of 64: the last chain workgroup is the first half of its block),
    K = 3 with view 1 seeing nothing.  The Gaussians PLANTED sit 2 m down the middle camera's axis with a 1 m scale (3 sigma = 270
    pixels: every tile) and little opacity, so what lies behind is still reached: runs of 154 rows span three 64-row groups, use the
    two-ahead flag prefetch, and lie on both sides of the half-block edge (31 | 32) and of the block edge (63 | 64).  The other
    Gaussians are a few pixels wide (a few tiles each) or off the frame."""
    K, P, W, H, coeffs = 3, 96, 224, 176, 4
    cam0 = hp.small_camera(W, H, f=0.8 * W, orthonormal=True)
    sc = syn.make_scene(P, 11 + P, cam0, z_range=(0.8, 3.0), log_scale_range=(np.log(0.01), np.log(0.04)), sh_coeffs=coeffs, margin=0.2)
    centre = (np.linalg.inv(cam0["w2c"]) @ np.array([0.0, 0.0, 2.0, 1.0]))[:3]
    for i in PLANTED:
        sc["means3D"][i] = centre
        sc["scales"][i] = 1.0
        sc["opacities"][i] = 0.05
    cams = syn.keyframe_cameras(K, radius=0.2, W=W, H=H, fx=cam0["fx"], fy=cam0["fy"], cx=cam0["cx"], cy=cam0["cy"])
    cams[1] = blind_camera(cams[1])
    return (K, cams, sc, 1, 32) + _pixel_seeds(cams)
