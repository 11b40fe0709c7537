"""The launches whose SIZE selects another code path of the binning front end (csrc/preprocess.hip: plan_preprocess picks bpw, the
256-Gaussian blocks a k_preprocess workgroup loops over; plan_scatter picks gpt, the blocks of a k_scatter_instances workgroup),
stated once for tests/test_cpu_launch_plan.py (which pins them through the library, on the CPU) and tests/test_gpu_launch_variants.py
(which runs them).  A variant of a 10^6-Gaussian window is reached at test size by batching many views of one small map: both
selectors look at P x views only."""
import functools
import math

import numpy as np

from gsaj import synthetic as syn

W, H = 80, 160  # 5 x 10 tiles: all eight row classes of the scatter exist and two of them (rows 8, 9) take a second row
CAPACITY = 65536  # instances per view the batched arenas are carved for (the scenes below stay under half of it: the GPU test asserts no view aborted)
MEMORY_CAP = 4 * 10 ** 9  # bytes of workspace the largest case may ask the library for

# id -> (P, K views in ONE call, SH coefficients stored (0: colors_precomp + cov3D_precomp), bpw, gpt, what runs)
CASES = {
    "bpw2_sh16": (65537, 32, 16, 2, 8, "k_preprocess<true,true>, two blocks per workgroup"),
    "bpw2_sh1": (65537, 32, 1, 2, 8, "k_preprocess<false,true>"),
    "bpw4_sh4": (65537, 64, 4, 4, 8, "k_preprocess<false,true>, four blocks"),
    "bpw8_sh16": (65537, 128, 16, 8, 8, "k_preprocess<true,true>, eight blocks"),
    "gpt9_sh1": (13000, 32, 1, 1, 9, "scatter workgroups of 9 blocks: the i0 + j < gpt tail with one block left"),
    "gpt10_sh4": (15000, 32, 4, 1, 10, "scatter workgroups of 10 blocks: the tail with two"),
    "gpt8_sh16": (17000, 32, 16, 1, 8, "scatter workgroups of 8 blocks, neither retry fits"),
    "bpw2_precomp": (65537, 32, 0, 2, 8, "k_preprocess<false,true> on precomputed colours and covariances"),
}
SINGLE_VIEW = (1, 4)  # (bpw, gpt) of ONE view of any of these maps: what the FrameContext every batched view is compared with runs


def plan(P, views, w=W, h=H):
    """The library's own answer (gsaj_debug_launch_plan): dict of gsaj.rasterizer.PLAN_FIELDS."""
    from gsaj import rasterizer as C

    return C.launch_plan(P, views, w, h)


def workspace_bytes(P, K, w=W, h=H, capacity=CAPACITY):
    """What the K blocks of the three workspaces of one batched call take, by the library's size queries."""
    from gsaj import _lib

    lib = _lib.load()
    return K * (lib.gsaj_geom_workspace_bytes(P) + lib.gsaj_image_workspace_bytes(w, h) + lib.gsaj_binning_workspace_bytes(capacity))


def pinned_ids(P):
    """The Gaussians every view must see: every index that is a multiple of 257 (one per 256-block, walking through the lanes,
    so every block of every workgroup's loop emits something) and P - 1 (at these P the only Gaussian of the last block)."""
    return np.unique(np.concatenate([np.arange(0, P, 257), [P - 1]]))


@functools.lru_cache(maxsize=None)
def window(P, K, coeffs):
    """-> (cameras [K], scene, pinned ids).  Small Gaussians (a few pixels) spread over twice the image in both directions, so
    about 70 % of them are culled in any one view and the arc of K cameras moves others in and out; the pinned ones sit in
    the middle of the first camera's image, which every camera of the arc keeps in view."""
    import helpers as hp

    cam0 = hp.small_camera(W, H, orthonormal=True)
    sc = syn.make_scene(P, 1000 + P + K, cam0, z_range=(1.0, 4.0), log_scale_range=(math.log(0.002), math.log(0.03)),
                        sh_coeffs=max(coeffs, 1), margin=0.5)
    ids = pinned_ids(P)
    rng = np.random.default_rng(P + K)
    u, v, z = rng.uniform(0.4 * W, 0.6 * W, ids.size), rng.uniform(0.3 * H, 0.7 * H, ids.size), rng.uniform(1.5, 4.0, ids.size)
    pc = np.stack([(u - cam0["cx"]) / cam0["fx"] * z, (v - cam0["cy"]) / cam0["fy"] * z, z, np.ones(ids.size)], axis=1)
    sc["means3D"][ids] = (pc @ np.linalg.inv(cam0["w2c"]).T)[:, :3].astype(np.float32)
    cams = syn.keyframe_cameras(K, W=W, H=H, fx=cam0["fx"], fy=cam0["fy"], cx=cam0["cx"], cy=cam0["cy"])
    return cams, sc, ids


def pixels(cam, means3D):
    """[n,3] (pixel x, pixel y, view depth) of world points under `cam`, in float64 (premise checks only)."""
    p = np.concatenate([np.asarray(means3D, np.float64), np.ones((len(means3D), 1))], axis=1) @ cam["w2c"].T
    return np.stack([cam["fx"] * p[:, 0] / p[:, 2] + cam["cx"], cam["fy"] * p[:, 1] / p[:, 2] + cam["cy"], p[:, 2]], axis=1)


# ---- the packed tile rectangle at the ends of its 10-bit fields: the widest and the tallest image a backward accepts -------------
BOUNDARY = {"x1023": (16384, 16), "y1023": (16, 16384)}  # id -> (W, H): 1024 x 1 and 1 x 1024 tiles


@functools.lru_cache(maxsize=None)
def boundary_scene(which):
    """-> (camera, scene): 3000 Gaussians over the whole strip (a 90-degree field of view along it), from sub-tile to a few tiles
    wide (sigma 0.6 .. 50 pixels before the perspective stretch).  The first three are small ones put 5 pixels from the far end
    of the strip, so that a tile rectangle starts in the last tile column (row) whatever the seed gives."""
    import helpers as hp

    w, h = BOUNDARY[which]
    side = max(w, h)
    cam = hp.small_camera(w, h, f=0.5 * side, orthonormal=True)
    sc = syn.make_scene(3000, 23 + (which == "y1023"), cam, z_range=(1.0, 4.0), log_scale_range=(math.log(0.0003), math.log(0.006)),
                        sh_coeffs=1, margin=0)
    z = np.array([1.5, 2.0, 3.0])
    along, across = np.full(3, side - 5.0), np.array([3.0, 8.0, 12.0])
    u, v = (along, across) if which == "x1023" else (across, along)
    pc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z, np.ones(3)], axis=1)
    sc["means3D"][:3] = (pc @ np.linalg.inv(cam["w2c"]).T)[:, :3].astype(np.float32)
    sc["scales"][:3] = np.float32(0.0003)
    return cam, sc
