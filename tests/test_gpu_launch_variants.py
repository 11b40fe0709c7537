"""GPU: every launch variant the binning front end selects by the SIZE of a launch (csrc/preprocess.hip), run at test-sized shapes.

plan_preprocess gives a k_preprocess workgroup bpw = 2, 4 or 8 blocks of 256 Gaussians once ceil(P / 256) x views reaches 8192 (the
MULTI instantiations: the block loop, its early end in the last workgroup, ONE histogram flush behind it, block_sums per block, the
scan's LDS words used again by the next block); plan_scatter gives a k_scatter_instances workgroup gpt = 8, 9 or 10 blocks (9 and
10: the i0 + j < gpt tail of its walk).  Both look at P x views only, so a 10^6-Gaussian window's variants are reached here by
batching 32 .. 128 views of one map of 13000 .. 65537 small Gaussians at 80 x 160 (tests/launch_variants.py), forward only: what
bpw and gpt change is what k_preprocess and k_scatter_instances leave behind, and every array of that is compared.

Each case asserts FIRST that the library's own plan for its launch is the variant in its id (gsaj_debug_launch_plan, the functions
the launchers call; tests/test_cpu_launch_plan.py pins the same table on the CPU), then compares
  - every view, bit for bit and on the device, with the single-view path of ONE FrameContext (bpw = 1, gpt = 4: also asserted): radii,
    n_touched, the three images, and tiles_touched, depths, means2D, conic_opacity, rgb, clamped, ranges, point_list[:R] of
    gsaj_debug_export (cov3D: view 0's copy, the only one a batched forward writes);
  - views 0, K // 2 and K - 1 with the CPU oracle: num_rendered, radii, tiles_touched, point_list, ranges exactly, colour and depth
    through helpers.assert_image_close (IMG_TOL), n_contrib through helpers.assert_counts_close.
BatchContext takes any K, so the cases go through it (streams = 1: two streams would halve the views per launch) and not through
the C ABI directly; its arena is sized by hand (launch_variants.CAPACITY) to keep the memory of the K = 128 case known in advance.

The packed tile rectangle (x0 | y0 << 10 | width << 20 in the splat row, unpacked by k_render_bwd alone) is run at the ends of its
fields: 16384 x 16 and 16 x 16384 pixels, the widest and tallest image a backward accepts, forward and backward against the oracle.

Measured on an MI355X (seconds of the whole test as pytest reports its call, the oracle's three views included; bytes = the K blocks
of the three workspaces by the library's size queries, launch_variants.workspace_bytes; R per view 30000 .. 32000 at P = 65537):
  bpw2_sh16     P 65537  K  32   0.53 GB   2.08 s  (the first test of the module: 2 s of it are the process's first HIP calls)
  bpw2_sh1      P 65537  K  32   0.53 GB   0.07 s
  bpw4_sh4      P 65537  K  64   1.07 GB   0.10 s
  bpw8_sh16     P 65537  K 128   2.14 GB   0.15 s  (the largest; test_cpu_launch_plan holds it under 4 GB)
  gpt9_sh1      P 13000  K  32   0.23 GB   0.03 s
  gpt10_sh4     P 15000  K  32   0.24 GB   0.03 s
  gpt8_sh16     P 17000  K  32   0.25 GB   0.04 s
  bpw2_precomp  P 65537  K  32   0.53 GB   0.10 s
  x1023 / y1023 (16384 x 16 / 16 x 16384, 3000 Gaussians, R = 15811 / 15685; largest x0 / y0 reached: 1023)   0.22 s / 0.21 s
The whole module: 3.4 s.
"""
import numpy as np
import pytest

import binning_restated as br
import helpers as hp
import launch_variants as lv

pytestmark = pytest.mark.gpu

EXPORTED = ("tiles_touched", "depths", "means2D", "conic_opacity", "rgb", "clamped", "ranges")  # + point_list[:R]; cov3D for view 0
IMAGES = ("radii", "n_touched", "color", "depth", "opacity")
BG = (0.1, 0.2, 0.3)


def _bits(x):
    """floats compared as their bits (a NaN equals itself, -0 differs from +0)"""
    import torch

    return x.view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("name", list(lv.CASES))
def test_variant(name):
    import torch
    from gsaj import rasterizer as C
    from gsaj.rasterizer import BatchContext, FrameContext
    from oracle import oracle as orc

    P, K, coeffs, bpw, gpt, _ = lv.CASES[name]
    W, H = lv.W, lv.H
    # ---- premises, before anything runs on the device
    pl = lv.plan(P, K)
    assert (pl["bpw"], pl["gpt"]) == (bpw, gpt), (name, pl)
    one = lv.plan(P, 1)
    assert (one["bpw"], one["gpt"]) == lv.SINGLE_VIEW, (name, one)
    nblk = (P + 255) // 256
    if bpw > 1:
        assert 0 < nblk - (pl["pre_workgroups"] - 1) * bpw < bpw  # the last workgroup leaves its loop early
        assert P - (nblk - 1) * 256 == 1                          # and its last block holds one Gaussian
    if gpt > 8:
        assert gpt % 4 != 0 and pl["scat_workgroups"] // 8 * gpt > nblk  # the tail of the walk, and blocks past P in the last workgroup
    cams, sc, pinned = lv.window(P, K, coeffs)
    assert pinned[-1] == P - 1 and lv.workspace_bytes(P, K) < lv.MEMORY_CAP
    for c in cams:  # the pinned Gaussians project well inside every view
        px = lv.pixels(c, sc["means3D"][pinned])
        assert px[:, 0].min() > 8 and px[:, 0].max() < W - 8 and px[:, 1].min() > 8 and px[:, 1].max() < H - 8 and px[:, 2].min() > 1.0

    precomp = coeffs == 0
    deg = 0 if precomp else int(round(coeffs ** 0.5)) - 1
    M = coeffs
    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    means, opac, bg = t(sc["means3D"]), t(sc["opacities"]), t(np.array(BG))
    # the oracle's answer for three views, once (its inputs -- the precomputed colours and covariances, if any -- are the device's)
    orc.set_threads(16)
    try:
        oracle = {k: hp.oracle_forward(cams[k], sc, deg, bg=BG, precomp=precomp) for k in sorted({0, K // 2, K - 1})}
    finally:
        orc.set_threads(1)
    kw = {n: t(v) for n, v in oracle[0][1].items() if n != "sh_degree"}
    views, projs, cps = (t(np.stack([c[k] for c in cams])) for k in ("viewmatrix", "projmatrix", "campos"))
    tanx, tany = cams[0]["tanfovx"], cams[0]["tanfovy"]

    # ---- the batched launch: K views in one call, the arena sized by hand, no host round trip inside
    bc = BatchContext(K, P, W, H, M, dev, has_scales=not precomp, streams=1)
    assert len(bc.groups) == 1
    bc.auto_grow = False
    bc._size(lv.CAPACITY)
    assert K * (bc.geom_stride + bc.img_stride + bc.bin_stride) == lv.workspace_bytes(P, K)
    bc.forward(bg, means, opac, views, projs, cps, tanx, tany, sh_degree=deg, sync=False, **kw)
    st = bc.status()
    assert not any(ab for _, _, ab in st), [k for k, s in enumerate(st) if s[2]]
    assert max(r for r, _, _ in st) <= lv.CAPACITY
    assert bool((bc.radii[:, torch.as_tensor(pinned, device=dev)] > 0).all())  # every block emits in every view

    # ---- every view against the single-view path: same bits, compared on the device, one flag per (view, array)
    names = IMAGES + EXPORTED + ("point_list", "cov3D")
    differs = torch.zeros((K, len(names)), dtype=torch.bool, device=dev)
    fc = FrameContext(P, W, H, M, dev, has_scales=not precomp)
    blk = lambda buf, stride, k: buf[k * stride:(k + 1) * stride]  # noqa: E731
    for k in range(K):
        Rk = fc.forward(bg, means, opac, views[k], projs[k], cps[k], tanx, tany, sh_degree=deg, sync=True, **kw)
        assert Rk == st[k][0] and fc.max_tile_list == st[k][1], (name, k, Rk, st[k])
        a = C.debug_export(P, bc.capacity, W, H, blk(bc.geom, bc.geom_stride, k), blk(bc.binning, bc.bin_stride, k), blk(bc.img, bc.img_stride, k))
        b = C.debug_export(P, Rk, W, H, fc.geom, fc.binning, fc.img)
        a["point_list"] = a["point_list"][:Rk]
        a.update(radii=bc.radii[k], n_touched=bc.n_touched[k], color=bc.color[k], depth=bc.depth[k], opacity=bc.opacity[k])
        b.update(radii=fc.radii, n_touched=fc.n_touched, color=fc.color, depth=fc.depth, opacity=fc.opacity)
        for j, n in enumerate(names):
            # (a batched forward writes view 0's cov3D only; with precomputed covariances / colours no forward writes cov3D / clamped)
            if (n == "cov3D" and (k > 0 or precomp)) or (n == "clamped" and precomp):
                continue
            differs[k, j] = (_bits(a[n]) != _bits(b[n])).any()
    differs = differs.cpu().numpy()
    assert not differs.any(), "%s: (view, array) that differ from the single-view path: %s" % (
        name, [(int(k), names[j]) for k, j in zip(*np.nonzero(differs))][:20])

    # ---- three views against the oracle
    for k, ((ref, ost), _) in oracle.items():
        tag = "variant/%s/view%d" % (name, k)
        assert st[k][0] == ref["num_rendered"], tag
        assert (ref["radii"][pinned] > 0).all(), tag  # (the lone Gaussian of the last block among them)
        np.testing.assert_array_equal(bc.radii[k].cpu().numpy(), ref["radii"], err_msg=tag)
        dbg = {n: v.cpu().numpy() for n, v in C.debug_export(P, bc.capacity, W, H, blk(bc.geom, bc.geom_stride, k),
                                                              blk(bc.binning, bc.bin_stride, k), blk(bc.img, bc.img_stride, k)).items()}
        np.testing.assert_array_equal(dbg["tiles_touched"], ost["tiles_touched"], err_msg=tag)
        np.testing.assert_array_equal(dbg["point_list"][:ref["num_rendered"]].astype(np.uint32), ost["point_list"], err_msg=tag)
        np.testing.assert_array_equal(dbg["ranges"], ost["ranges"], err_msg=tag)
        hp.assert_image_close(bc.color[k].cpu().numpy(), ref["color"], hp.IMG_TOL, st=ost, tag=tag + "/color")
        hp.assert_image_close(bc.depth[k].cpu().numpy(), ref["depth"], hp.IMG_TOL, st=ost, tag=tag + "/depth")
        hp.assert_image_close(bc.opacity[k].cpu().numpy(), ref["opacity"], hp.IMG_TOL, st=ost, tag=tag + "/opacity")
        hp.assert_counts_close(dbg["n_contrib"], ost["n_contrib"], ost, tag=tag + "/n_contrib")


@pytest.mark.parametrize("which", list(lv.BOUNDARY))
def test_packed_rectangle_at_the_ends_of_its_fields(which):
    """1024 x 1 and 1 x 1024 tiles: x0 (y0) of the packed rectangle runs up to 1023, all ten bits, in a forward AND the backward that
    unpacks it (the widest backward elsewhere in the suite has 129 tile columns).  Inside the packing's range: an ordinary test."""
    from gsaj import rasterizer as C

    cam, sc = lv.boundary_scene(which)
    P, W, H = sc["means3D"].shape[0], cam["W"], cam["H"]
    assert (W, H) == lv.BOUNDARY[which] and max(W, H) == 16384
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert max(gx, gy) == 1024 and min(gx, gy) == 1
    (ref, st), kw = hp.oracle_forward(cam, sc, 0)
    # premises, on the oracle's state: a rectangle starts in the last tile column (row); one that starts in the upper half of the
    # field (bit 9 set) spans two tiles or more
    rect = br.tile_rects(st["means2D"], st["radii"], gx, gy)
    a = 0 if which == "x1023" else 1
    seen = (rect[:, 2] > rect[:, 0]) & (rect[:, 3] > rect[:, 1])
    assert np.array_equal(seen, ref["radii"] > 0) and seen[:3].all()
    assert np.array_equal((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]), st["tiles_touched"])  # (the restated rectangles are the oracle's)
    start, span = rect[seen, a], (rect[:, a + 2] - rect[:, a])[seen]
    assert start.max() == 1023 and start.min() == 0, (start.min(), start.max())
    assert ((start >= 512) & (span >= 2)).any() and ((start & 256) > 0).any()
    print("%s: largest start %d, widest %d tiles, %d start at >= 512 and span >= 2; R = %d" % (
        which, start.max(), span.max(), int(((start >= 512) & (span >= 2)).sum()), ref["num_rendered"]))

    out, args = hp.gpu_forward(cam, sc, 0, kw=kw)
    R, color, radii, geom, binning, img, depth, opacity, n_touched = out
    assert R == ref["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["radii"])
    dbg = {k: v.cpu().numpy() for k, v in C.debug_export(P, R, W, H, geom, binning, img).items()}
    np.testing.assert_array_equal(dbg["tiles_touched"], st["tiles_touched"])
    np.testing.assert_array_equal(dbg["point_list"].astype(np.uint32), st["point_list"])
    np.testing.assert_array_equal(dbg["ranges"], st["ranges"])
    hp.assert_image_close(color.cpu().numpy(), ref["color"], hp.IMG_TOL, st=st, tag="rect_%s/color" % which)
    dLc, dLd = hp.seeds(cam, seed=31)
    hp.check_backward(cam, 0, out, args, st, dLc, dLd, "rect_%s" % which)
