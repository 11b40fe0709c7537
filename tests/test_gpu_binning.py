"""GPU: the binning stage (k_scatter_instances, k_frame_scan, k_tile_sort of csrc/preprocess.hip) against its exact answer, on
scenes whose tile lists are PRESCRIBED (tests/binning_restated.py; tests/test_cpu_binning.py ties them to the oracle): every
list length on a boundary of the sort -- the wave, the 128-key chunk, every power of two up to 16384, one below and one above each,
empty tiles, one list of 33000 -- under every capacity class of launch_tile_binning (128 / 256 / 512 threads, one launch or two,
lists inside the LDS or in chunks + merge passes, more than 64 KB of dynamic LDS), with depth bits spread over many exponents and
with exact ties everywhere; and the two bodies of the scatter no rendering scene of the suite reaches.  point_list and ranges are
integers: every comparison here is assert_array_equal."""
import functools

import numpy as np
import pytest

import binning_restated as br
import helpers as hp

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device_args(name, depths, reverse=False):
    import torch

    L = br.layout(name, depths, reverse)
    cam, sc = L["cam"], L["sc"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    return dict(bg=torch.zeros(3, device=dev), means3D=t(sc["means3D"]), opacities=t(sc["opacities"]), viewmatrix=t(cam["viewmatrix"]),
                projmatrix=t(cam["projmatrix"]), campos=t(cam["campos"]), tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], sh_degree=0,
                shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))


def _context(L):
    import torch
    from gsaj.rasterizer import FrameContext

    return FrameContext(L["P"], L["cam"]["W"], L["cam"]["H"], 1, torch.device("cuda:0"))


def _assert_exact(ctx, L, tag):
    """Everything the binning stage leaves behind, against the layout's own numbers (nothing the device returned is an input)."""
    from gsaj import rasterizer as C

    R, longest = ctx.status()  # (raises if the frame was aborted on the device)
    assert (R, longest) == (L["R"], L["longest"]), tag
    assert bool((ctx.radii > 0).all()), tag
    dbg = {k: v.cpu().numpy() for k, v in C.debug_export(L["P"], ctx.R, L["cam"]["W"], L["cam"]["H"], ctx.geom, ctx.binning, ctx.img).items()}
    assert np.all(dbg["tiles_touched"] == 1), tag
    np.testing.assert_array_equal(dbg["depths"].view(np.uint32), L["z32"].view(np.uint32), err_msg=tag)
    np.testing.assert_array_equal(dbg["ranges"], L["ranges"], err_msg=tag)
    got = dbg["point_list"][:R].astype(np.uint32)
    if not np.array_equal(got, L["point_list"]):  # name the tiles: the list length is what selects the path
        bad = [(int(n), int(np.count_nonzero(got[b:e] != L["point_list"][b:e]))) for (b, e), n in zip(L["ranges"], L["lengths"])
               if not np.array_equal(got[b:e], L["point_list"][b:e])]
        raise AssertionError("%s: point_list differs in the lists of (length, wrong entries) %s" % (tag, bad))


# tile_list_capacity of an asynchronous frame -> keys of LDS (the next power of two, 128 at least) -> the launch:
#      1 ->   128: 128 threads, long lists in chunks of T = 128; the 33000-entry list's last merge has 258 output blocks, so the
#                  merge-path split loop of sort_long_list (256 splits per step) takes its second step
#    300 ->   512
#   1024 ->  1024: the last 128-thread size
#   1025 ->  2048: 256 threads; the splits of a long list behind the keys
#   4096 ->  4096: 512 threads, two launches (pass 2 has 2048 keys); long lists in chunks of T = 2048, splits inside the capacity
#   8192 ->  8192
#   8193 -> 16384: more than 64 KB of dynamic LDS
#      0 -> 16384: the default
# "sync": forward(sync=True) as it is (the capacity comes from the longest list the host read back: 16384, the 33000-entry list in
# chunks of 8192); "forced": the same under FORCE_CHUNKED_SORT (128 keys)
CAPACITIES = [1, 300, 1024, 1025, 4096, 8192, 8193, 0, "sync", "forced"]


@pytest.mark.parametrize("depths", ["log", "ties"])
@pytest.mark.parametrize("c", CAPACITIES, ids=["cap%s" % c if isinstance(c, int) else c for c in CAPACITIES])
def test_every_length_under_every_capacity(c, depths):
    from gsaj import rasterizer as C

    L = br.layout("FULL", depths)
    args = _device_args("FULL", depths)
    ctx = _context(L)
    ctx.forward(**args, sync=True)  # sizes the arena
    if c == "forced":
        C.FORCE_CHUNKED_SORT = True
        try:
            ctx.forward(**args, sync=True)
        finally:
            C.FORCE_CHUNKED_SORT = False
    elif c != "sync":
        ctx.auto_grow = False  # (_grow_ahead would raise the capacity to the longest list it has seen)
        ctx.tile_list_capacity = c
        ctx.forward(**args, sync=False)
        assert ctx.tile_list_capacity == c
    _assert_exact(ctx, L, "FULL/%s/%s" % (depths, c))


@pytest.mark.parametrize("depths", ["log", "ties"])
def test_small_layout_through_the_drop_in_entry_point(depths):
    """SMALL through rasterize_gaussians (the synchronous path: longest list 4097 -> 8192 keys, two launches), against the
    restatement AND the oracle's own lists."""
    from gsaj import rasterizer as C

    L = br.layout("SMALL", depths)
    (ref, st), kw = hp.oracle_forward(L["cam"], L["sc"], 0)
    out, args = hp.gpu_forward(L["cam"], L["sc"], 0, kw=kw)
    R, color, radii, geom, binning, img, depth, opacity, n_touched = out
    assert R == L["R"] == ref["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["radii"])
    dbg = {k: v.cpu().numpy() for k, v in C.debug_export(L["P"], R, L["cam"]["W"], L["cam"]["H"], geom, binning, img).items()}
    assert np.all(dbg["tiles_touched"] == 1)
    np.testing.assert_array_equal(dbg["depths"].view(np.uint32), L["z32"].view(np.uint32))
    for want_pl, want_ranges in ((L["point_list"], L["ranges"]), (st["point_list"], st["ranges"])):
        np.testing.assert_array_equal(dbg["point_list"].astype(np.uint32), want_pl)
        np.testing.assert_array_equal(dbg["ranges"], want_ranges)


def test_a_context_forgets_the_previous_frames_lists():
    """One context, capacity fixed: FULL, then FULL with its lengths reversed over the tiles (same P, same R; the 33000-entry list
    moves from the last tile to the first, the empty tiles move too).  The second frame's lists are exact: tile counters, cursors
    and offsets are zeroed per frame, and nothing of a frame's lists survives into the next."""
    A, B = br.layout("FULL", "ties"), br.layout("FULL", "ties", True)
    assert A["P"] == B["P"] and not np.array_equal(A["ranges"], B["ranges"])
    ctx = _context(A)
    ctx.forward(**_device_args("FULL", "ties"), sync=True)
    ctx.auto_grow = False
    ctx.tile_list_capacity = 4096
    ctx.forward(**_device_args("FULL", "ties"), sync=False)
    _assert_exact(ctx, A, "first frame")
    ctx.forward(**_device_args("FULL", "ties", True), sync=False)
    _assert_exact(ctx, B, "second frame")
    ctx.forward(**_device_args("FULL", "ties"), sync=False)
    _assert_exact(ctx, A, "third frame")


def test_the_sort_clears_every_reached_flag():
    """The reverse compositor sets `reached` only for the instance rows it writes and the gather trusts the others to be clear:
    k_tile_sort clears a tile's flags in pass 0 / pass 1, whichever path then sorts the tile (short, pass 2's, long, empty)."""
    from gsaj import rasterizer as C

    L = br.layout("FULL", "log")
    args = _device_args("FULL", "log")
    ctx = _context(L)
    ctx.forward(**args, sync=True)
    ctx.auto_grow = False
    ctx.tile_list_capacity = 4096  # two launches, and the lists above 4096 take sort_long_list
    ctx.binning.fill_(0xFF)
    ctx.forward(**args, sync=False)
    _assert_exact(ctx, L, "arena filled with 0xFF")
    taken, reached = C.debug_export_taken(ctx.R, L["cam"]["W"], L["cam"]["H"], ctx.binning, ctx.img)
    reached = reached.cpu().numpy()[:L["R"]]
    assert reached.shape == (L["R"],) and not reached.any(), "%d reached flags survived the sort" % np.count_nonzero(reached)


def _scatter_parity(which, backward):
    from gsaj import rasterizer as C

    cam, sc = br.scatter_scene(which)
    P, W, H = sc["means3D"].shape[0], cam["W"], cam["H"]
    (ref, st), kw = hp.oracle_forward(cam, sc, 0)
    out, args = hp.gpu_forward(cam, sc, 0, kw=kw)
    R, color, radii, geom, binning, img, depth, opacity, n_touched = out
    assert R == ref["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), ref["radii"])
    dbg = {k: v.cpu().numpy() for k, v in C.debug_export(P, R, W, H, geom, binning, img).items()}
    np.testing.assert_array_equal(dbg["tiles_touched"], st["tiles_touched"])
    np.testing.assert_array_equal(dbg["point_list"].astype(np.uint32), st["point_list"])
    np.testing.assert_array_equal(dbg["ranges"], st["ranges"])
    hp.assert_image_close(color.cpu().numpy(), ref["color"], hp.IMG_TOL, st=st, tag="scatter_%s/color" % which)
    if backward:
        dLc, dLd = hp.seeds(cam, seed=21)
        hp.check_backward(cam, 0, out, args, st, dLc, dLd, "scatter_%s" % which)


def test_scatter_without_lds_counters():
    """Scene S1 (4097 x 1 tiles: more class-local tiles than SCAT_LDS_TILES): the direct-global-atomics body of
    k_scatter_instances.  Premises: test_cpu_binning.test_scene_s1_has_more_class_local_tiles_than_the_scatter_counters."""
    _scatter_parity("S1", backward=False)


def test_scatter_past_the_staging_area():
    """Scene S2: the first scatter workgroup of every row class holds 8192 instances (> SCAT_STAGE: stored directly), the second
    608 (staged).  Premises: test_cpu_binning.test_scene_s2_fills_and_overfills_the_staging_area.  Its 1100-entry lists of
    screen-filling Gaussians also go through the reverse compositor."""
    _scatter_parity("S2", backward=True)


@pytest.mark.parametrize("which", sorted(br.BUDGET_SCENES))
def test_the_far_end_of_every_lds_size_class(which):
    """binning_restated.BUDGET_SCENES: the last launch whose scatter counters fit the LDS beside what the kernel declares (S3), the
    first past it (S4) and a 3840 x 2160 frame (S5) -- both on the global-atomics body, over several row classes --, the last LDS
    tile histogram (H1) and the first global one with the scatter still in LDS (H2).  Through the synchronous entry point: a launch
    the runtime refuses is the library's error, not stale lists.  Premises (which body each launch takes, by the library's own plan
    and LDS figures): tests/test_cpu_lds_budget.py."""
    _scatter_parity(which, backward=br.BUDGET_SCENES[which][3])
