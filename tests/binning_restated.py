"""Scenes with PRESCRIBED tile lists and the exact answer of the binning stage on them (k_scatter_instances, k_frame_scan and
k_tile_sort of csrc/preprocess.hip), in NumPy.  point_list and ranges are integers: the right answer is a stable sort of the
instances by (tile, depth bits, Gaussian id) -- one np.lexsort --, and nothing here has a tolerance.  Shared by
tests/test_cpu_binning.py (which ties this restatement to the project's oracle) and tests/test_gpu_binning.py."""
import functools
import math
import os
import re

import numpy as np

from gsaj import synthetic as syn

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gs-slam-analytica_jacobian_amd", "csrc")

# Tile-list lengths on every boundary of the tile sort: the 64-lane wave, the 128-key chunk lds_bitonic_sort skips padding by,
# every power of two up to the capacity classes of launch_tile_binning (128 .. 16384 keys of LDS), one below and one above each;
# empty tiles at the start and inside; 33000 = more than 256 output blocks of 128 keys in the last merge of sort_long_list.
SMALL = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
         0, 5, 300]
FULL = SMALL + [8191, 8192, 8193, 16383, 16384, 16385, 33000]
LAYOUT_GX = 7
F = 64.0  # focal length of the one-tile scenes, pixels

# what the layouts above (and the two scatter scenes of the tests) were designed for
DESIGN_CONSTANTS = dict(PRE_BLOCK=256, SORT_CAP=16384, GSAJ_SORT_128_MAX=1024, SCAT_CLS=8, SCAT_LDS_TILES=3411, SCAT_STAGE=4096,
                        LDS_TILES_MAX=8192)


def csrc_constants():
    """The #defines the binning stage branches on, read from the text of gsaj_common.h and preprocess.hip."""
    text = ""
    for name in ("gsaj_common.h", "preprocess.hip"):
        with open(os.path.join(CSRC, name)) as fh:
            text += fh.read() + "\n"
    out = {}
    for name in DESIGN_CONSTANTS:
        m = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)\b" % name, text, flags=re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


def one_tile_scene(lengths, gx=LAYOUT_GX, seed=0, depths="log"):
    """-> (cam, scene, tile [P] int64, z32 [P] float32): tile t of a gx-wide tile grid receives exactly lengths[t] Gaussians and
    every Gaussian touches exactly one tile.  The camera looks down +z with the identity view matrix, so a Gaussian's depth is
    its z, bit for bit; a Gaussian sits on the centre of its tile with an isotropic scale of one pixel (radius 4 or 5 of the 16
    pixels).  The tiles are dealt through a seeded permutation of the ids: a tile's ids are scattered over the whole id range,
    i.e. over many scatter workgroups.  depths="log": z log-uniform in [0.25, 4000] (depth bits over many exponents);
    depths="ties": z = round(64 u) / 64, u uniform in [0.5, 4] -- 225 distinct depths, so the lists are full of exact ties (a list of
    two or more has at least one), and chunk borders and merge-path splits fall inside runs of equal depth."""
    lengths = np.asarray(lengths, np.int64)
    gy = (lengths.size + gx - 1) // gx
    lengths = np.concatenate([lengths, np.zeros(gx * gy - lengths.size, np.int64)])
    W, H = 16 * gx, 16 * gy
    cam = syn.make_camera(np.eye(4), W=W, H=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    P = int(lengths.sum())
    rng = np.random.default_rng(seed)
    tile = np.empty(P, np.int64)
    tile[rng.permutation(P)] = np.repeat(np.arange(gx * gy), lengths)
    if depths == "log":
        z = np.exp(rng.uniform(math.log(0.25), math.log(4000.0), size=P))
    elif depths == "ties":
        z = np.round(rng.uniform(0.5, 4.0, size=P) * 64.0) / 64.0
        # (a list of two, three or five entries drawn from 225 depths would usually have no tie: the tile's two lowest ids share one)
        order = np.argsort(tile, kind="stable")
        start = np.cumsum(lengths) - lengths
        two = lengths >= 2
        z[order[start[two] + 1]] = z[order[start[two]]]
    else:
        raise KeyError(depths)
    z32 = z.astype(np.float32)
    z = z32.astype(np.float64)
    px, py = 16.0 * (tile % gx) + 7.5, 16.0 * (tile // gx) + 7.5
    means = np.stack([(px - cam["cx"]) / F * z, (py - cam["cy"]) / F * z, z], axis=1)
    f = np.float32
    sc = dict(means3D=means.astype(f), scales=np.repeat((z / F)[:, None], 3, axis=1).astype(f),
              rotations=np.tile(np.array([1.0, 0.0, 0.0, 0.0], f), (P, 1)), opacities=np.full((P, 1), 0.01, f),
              shs=rng.uniform(-1.0, 1.0, size=(P, 1, 3)).astype(f))
    assert np.array_equal(sc["means3D"][:, 2], z32)
    return cam, sc, tile, z32


def expected_lists(tile, z32, tiles=None):
    """-> (point_list [R] uint32, ranges [tiles, 2] int32) of instances (tile[i], z32[i], id i): per tile ascending depth BITS
    (the depths are positive floats: their bits order as they do), equal depths in ascending id order (the reference's stable
    radix sort of (tile | depth) keys over instances emitted in id order).  An empty tile's range is (0, 0)."""
    tile = np.asarray(tile, np.int64)
    z32 = np.ascontiguousarray(z32, np.float32)
    ids = np.arange(tile.size, dtype=np.int64)
    point_list = np.lexsort((ids, z32.view(np.uint32), tile)).astype(np.uint32)
    lengths = np.bincount(tile, minlength=tiles or 0)
    end = np.cumsum(lengths)
    ranges = np.stack([end - lengths, end], axis=1)
    ranges[lengths == 0] = 0
    return point_list, ranges.astype(np.int32)


def tile_rects(means2D, radii, gx, gy):
    """[P, 4] (x0, y0, x1, y1), the tile rectangle of k_preprocess (tile_rect in gsaj_common.h, whole frame): fp32 arithmetic,
    truncation towards zero, clamped to the grid.  A Gaussian with radius 0 was culled: an empty rectangle."""
    f = np.float32
    m = np.asarray(means2D, f)
    r = np.asarray(radii).astype(f)
    lo = lambda p, n: np.minimum(n, np.maximum(0, np.trunc((p - r) / f(16)).astype(np.int64)))  # noqa: E731
    hi = lambda p, n: np.minimum(n, np.maximum(0, np.trunc((p + r + f(15)) / f(16)).astype(np.int64)))  # noqa: E731
    rect = np.stack([lo(m[:, 0], gx), lo(m[:, 1], gy), hi(m[:, 0], gx), hi(m[:, 1], gy)], axis=1)
    rect[np.asarray(radii) <= 0] = 0
    return rect


def class_totals(rects, P, gx, gy, span=1024, classes=8):
    """[ceil(P / span), classes]: the instances a scatter workgroup handles -- those of `span` consecutive ids (gpt x 256
    Gaussians) whose tile row y belongs to row class y % classes -- from every Gaussian's tile rectangle."""
    rects = np.asarray(rects, np.int64)
    assert rects.shape == (P, 4) and rects[:, 2].max() <= gx and rects[:, 3].max() <= gy
    out = np.zeros(((P + span - 1) // span, classes), np.int64)
    blk = np.arange(P) // span
    for c in range(classes):
        # rows y in [y0, y1) with y % classes == c
        first = rects[:, 1] + (c - rects[:, 1]) % classes
        rows = np.maximum(0, (rects[:, 3] - first + classes - 1) // classes)
        np.add.at(out[:, c], blk, rows * (rects[:, 2] - rects[:, 0]))
    return out


@functools.lru_cache(maxsize=None)
def layout(name, depths, reverse=False):
    """The one-tile scene of a named layout with its exact answer, built once per session:
    dict(cam, sc, tile, z32, lengths, point_list, ranges, P, R, longest)."""
    lengths = list({"SMALL": SMALL, "FULL": FULL}[name])
    if reverse:
        lengths.reverse()
    cam, sc, tile, z32 = one_tile_scene(lengths, LAYOUT_GX, seed=len(lengths) + (depths == "ties"), depths=depths)
    tiles = (cam["W"] // 16) * (cam["H"] // 16)
    point_list, ranges = expected_lists(tile, z32, tiles)
    return dict(cam=cam, sc=sc, tile=tile, z32=z32, lengths=np.asarray(lengths), point_list=point_list, ranges=ranges,
                P=tile.size, R=tile.size, longest=max(lengths))


def scatter_scene(which):
    """S1: 4097 x 1 tiles -- ceil(gy / 8) * gx = 4097 class-local tiles, more than the scatter's LDS counters hold, while the
    4097 tiles still fit the LDS histogram of k_preprocess / k_frame_scan: k_scatter_instances takes its direct-global-atomics
    body.  S2: 8 x 8 tiles under 1100 screen-filling Gaussians: a scatter workgroup of 1024 Gaussians holds 8192 instances of
    every row class, twice the staging area, and the last workgroup (76 Gaussians) 608: both store paths in one launch.
    S3 .. S5, H1, H2: BUDGET_SCENES below.
    -> (cam, scene)"""
    import helpers as hp

    if which == "S1":
        cam = hp.small_camera(65552, 16, f=0.02 * 65552, orthonormal=True)
        sc = syn.make_scene(3000, 22, cam, z_range=(1.0, 4.0), log_scale_range=(math.log(0.002), math.log(0.3)), sh_coeffs=1, margin=0)
    elif which == "S2":
        cam = hp.small_camera(128, 128, f=0.8 * 128, orthonormal=True)
        sc = syn.make_scene(1100, 21, cam, z_range=(1.0, 2.0), log_scale_range=(math.log(0.5), math.log(2.0)), sh_coeffs=1,
                            opacity_range=(0.002, 0.01), margin=0)
    elif which in BUDGET_SCENES:
        W, H, P, _ = BUDGET_SCENES[which]
        f = 0.5 * max(W, H)
        cam = hp.small_camera(W, H, f=f, orthonormal=True)
        # sigma 0.5 .. 50 pixels at depth 1 (a quarter of that at depth 4): from inside one tile to some twenty tiles across
        sc = syn.make_scene(P, 30 + sorted(BUDGET_SCENES).index(which), cam, z_range=(1.0, 4.0),
                            log_scale_range=(math.log(2.0 / f), math.log(50.0 / f)), sh_coeffs=1, margin=0)
    else:
        raise KeyError(which)
    return cam, sc


# The far ends of the size classes whose launches request dynamic LDS that grows with the tile grid: the scatter's counters (12 bytes
# per class-local tile, ltiles = ceil(tile rows / 8) x tile columns, beside the 24 596 bytes k_scatter_instances declares: 3411 is
# the last ltiles at which both fit in 64 KB) and the tile histogram of k_preprocess / k_frame_scan (4 bytes per tile up to
# LDS_TILES_MAX = 8192).  id -> (W, H, Gaussians, backward run).  tests/test_cpu_lds_budget.py holds every premise to the library's plan.
#   S3  379 x 65 tiles, ltiles 9 x 379 = 3411: the last launch with LDS counters, every row class populated
#   S4  853 x 25 tiles, ltiles 4 x 853 = 3412: the first launch past the bound -- the global-atomics body on a grid with several
#       row classes (S1 has one row)
#   S5  240 x 135 tiles (3840 x 2160), ltiles 17 x 240 = 4080
#   H1  128 x 64 = 8192 tiles: the last LDS histogram
#   H2  241 x 34 = 8194 tiles: the first global histogram with the scatter still in LDS (ltiles 5 x 241 = 1205)
BUDGET_SCENES = {
    "S3": (6064, 1040, 3000, True),
    "S4": (13648, 400, 3000, True),
    "S5": (3840, 2160, 300, False),
    "H1": (2048, 1024, 3000, True),
    "H2": (3856, 544, 3000, True),
}
