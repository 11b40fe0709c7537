"""GPU: the reverse compositor stages only the list entries the forward compositor took.

The forward leaves, per list position and 8x8 pixel quadrant, whether any pixel of the quadrant composited the entry
(BinWS.taken); the reverse compositor compacts the entries taken by at least one quadrant and walks those alone, 48 per round.
Scenes here are small and built so that most of a long list is dead (large 3-sigma squares, small alpha footprints), so that
whole 64-entry chunks of the forward are dead, so that the forward stops far before the end of its lists, so that the live
count sits on a round boundary, and so that quadrants lie outside the image.  Values are compared with the CPU oracle with the
comparators and tolerances of tests/helpers.py; the flags themselves with a NumPy restatement of "some pixel takes the entry"."""
import functools

import numpy as np
import pytest

import helpers as hp
from gsaj import synthetic as syn

pytestmark = pytest.mark.gpu

DEG = 3
# name: (W, H, P, seed, make_scene keywords)
SCENES = {
    "long_mostly_dead": (64, 48, 3000, 5, {}),
    "threshold_opacities": (64, 48, 3000, 6, dict(opacity_range=(0.004, 0.03))),
    "early_saturation": (48, 32, 2500, 8, dict(opacity_range=(0.6, 0.99), log_scale_range=(-3.9, -2.3))),
    "partial_tiles": (97, 61, 400, 3, {}),
}
FLAG_SCENES = ["long_mostly_dead", "threshold_opacities", "early_saturation"]


@functools.lru_cache(maxsize=None)
def _scene(name):
    W, H, P, seed, kw = SCENES[name]
    cam = hp.small_camera(W, H)
    return cam, syn.make_scene(P, seed, cam, **kw)


@functools.lru_cache(maxsize=None)
def _round_scene(P):
    """One 16x16 tile under P large Gaussians of opacity 0.02 at distinct depths: every entry is taken by all four quadrants, no
    pixel saturates (0.98^97 = 0.14), and the tile's list has exactly P entries."""
    cam = hp.small_camera(16, 16)
    sc = syn.make_scene(P, 40 + P, cam, z_range=(1.0, 2.0), log_scale_range=(np.log(1.5), np.log(3.0)), opacity_range=(0.02, 0.02),
                        margin=-0.3)
    return cam, sc


@functools.lru_cache(maxsize=None)
def _oracle(cam_key, name, P=None):
    cam, sc = _round_scene(P) if name == "round" else _scene(name)
    if cam_key is not None:
        cam = _window(name)[cam_key]
    return hp.oracle_forward(cam, sc, DEG, bg=hp.PARITY_BG)


@functools.lru_cache(maxsize=None)
def _window(name, K=3):
    cam, _ = _scene(name)
    return tuple(syn.keyframe_cameras(K, radius=0.2, **{k: cam[k] for k in ("W", "H", "fx", "fy", "cx", "cy")}))


def _single(name, P=None, tag=None):
    """forward + backward of one view against the oracle -> (forward outputs, oracle state, device gradients)."""
    cam, sc = _round_scene(P) if name == "round" else _scene(name)
    (ref, st), kw = _oracle(None, name, P)
    tag = tag or "live/" + name
    out, args = hp.gpu_forward(cam, sc, DEG, bg=hp.PARITY_BG, kw=kw)
    R, color, radii, geom, binning, img, depth, opacity, n_touched = out
    assert R == ref["num_rendered"]
    for nm, got in (("color", color), ("depth", depth), ("opacity", opacity)):
        hp.assert_image_close(got.cpu().numpy().reshape(ref[nm].shape), ref[nm], hp.IMG_TOL, st=st, tag=tag + "/" + nm)
    dLc, dLd = hp.seeds(cam, seed=1)
    g, _ = hp.check_backward(cam, DEG, out, args, st, dLc, dLd, tag)
    return out, args, st, g, (dLc, dLd)


def _batch_tensors(sc, cams, seed=70):
    import torch

    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    seeds = [hp.seeds(c, seed=seed + k) for k, c in enumerate(cams)]
    return dict(dev=dev, bg=t(np.asarray(hp.PARITY_BG)), means=t(sc["means3D"]), opac=t(sc["opacities"]),
                views=t(np.stack([c["viewmatrix"] for c in cams])), projs=t(np.stack([c["projmatrix"] for c in cams])),
                cps=t(np.stack([c["campos"] for c in cams])), praw=t(cams[0]["projmatrix_raw"]),
                dLc=t(np.stack([s[0] for s in seeds])), dLd=t(np.stack([s[1] for s in seeds])),
                geo=dict(sh_degree=DEG, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"])))


def _batch_run(bc, cams, a, sync=True):
    c0 = cams[0]
    bc.forward(a["bg"], a["means"], a["opac"], a["views"], a["projs"], a["cps"], c0["tanfovx"], c0["tanfovy"], sync=sync, **a["geo"])
    return bc.backward(a["bg"], a["means"], a["views"], a["projs"], a["praw"], a["cps"], c0["tanfovx"], c0["tanfovy"], a["dLc"], a["dLd"],
                       **a["geo"])


def _batch(name):
    """A window of K = 3 cameras through the batched entry points, every view against the oracle."""
    from gsaj.rasterizer import BatchContext
    from oracle import oracle as orc

    _, sc = _scene(name)
    cams = _window(name)
    K, P, M = len(cams), sc["means3D"].shape[0], sc["shs"].shape[1]
    a = _batch_tensors(sc, cams)
    bc = BatchContext(K, P, cams[0]["W"], cams[0]["H"], M, a["dev"], per_gaussian_tau=True)
    g = _batch_run(bc, cams, a)
    stt = bc.status()
    assert not any(ab for _, _, ab in stt)
    for k, cam in enumerate(cams):
        tag = "live/%s/kf%d" % (name, k)
        (ref, st), _ = _oracle(k, name)
        assert stt[k][0] == ref["num_rendered"]
        hp.assert_image_close(bc.color[k].cpu().numpy(), ref["color"], hp.IMG_TOL, st=st, tag=tag + "/color")
        dLc, dLd = a["dLc"][k].cpu().numpy(), a["dLd"][k].cpu().numpy()
        gref = orc.backward(st, dLc, dLd, cam["projmatrix_raw"])
        gref["error_model"] = orc.error_model(st, dLc, dLd, hp.BORDER_REL, hp.BORDER_REL_T)
        gv = hp.view_grads_from_sums(bc.view_sums(k).cpu().numpy(), g["tau"][k].cpu().numpy(), g["tau_all"][k].cpu().numpy())
        hp.assert_grads_close(gv, gref, tag, st=st, projmatrix_raw=cam["projmatrix_raw"])


@pytest.mark.parametrize("name", ["long_mostly_dead", "threshold_opacities", "early_saturation"])
def test_single_view_against_the_oracle(name):
    """Lists of ~360 entries of which 28 % / 19 % of the visited (quadrant, entry) pairs are live (the second with whole 64-entry
    chunks dead), and lists of ~650 entries of which the forward reaches a fraction before every pixel has saturated."""
    _single(name)


@pytest.mark.parametrize("name", ["long_mostly_dead", "threshold_opacities", "early_saturation"])
def test_window_of_three_views_against_the_oracle(name):
    _batch(name)


@pytest.mark.parametrize("P", [47, 48, 49, 96, 97])
def test_round_boundaries(P):
    """Live counts one below, at and one above one and two rounds of 48: every entry live in all four quadrants."""
    from gsaj import rasterizer as C

    out, _, st, _, _ = _single("round", P=P, tag="live/round%d" % P)
    R, W, H = out[0], 16, 16
    assert st["ranges"].shape[0] == 1 and int(st["ranges"][0][1] - st["ranges"][0][0]) == P == R
    assert int(st["n_contrib"].min()) > P - 8  # (no pixel stops early: the whole list is walked)
    taken, reached = C.debug_export_taken(R, W, H, out[4], out[5])
    taken = taken.cpu().numpy().view(np.uint32)
    last = int(st["n_contrib"].max())
    assert (taken[:last] == 0x01010101).all() and (taken[last:] == 0).all()
    assert int(reached.sum().item()) == last


def test_partial_tiles():
    """97 x 61: the last tile column and row have quadrants wholly outside the image (their forward waves never run)."""
    _single("partial_tiles")


def _frame_grads(fc, cam, sc, t, dLc, dLd, sync):
    import torch

    geo = dict(sh_degree=DEG, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    bg, view, proj, cp = t(np.asarray(hp.PARITY_BG)), t(cam["viewmatrix"]), t(cam["projmatrix"]), t(cam["campos"])
    fc.forward(bg, t(sc["means3D"]), t(sc["opacities"]), view, proj, cp, cam["tanfovx"], cam["tanfovy"], sync=sync, **geo)
    g = fc.backward(bg, t(sc["means3D"]), view, proj, t(cam["projmatrix_raw"]), cp, cam["tanfovx"], cam["tanfovy"], t(dLc), t(dLd), **geo)
    return {k: v.clone() for k, v in g.items() if torch.is_tensor(v)}


def test_stale_flags_single_view():
    """The binning arena that held the early-saturation scene (lists of ~650, most flags never written) is handed, with its
    capacity -- the same carving, so the same `taken` array -- to a context that renders the threshold-opacity scene (shorter
    lists, another camera and image size): every gradient equals the one a context with an arena of its own computes."""
    import torch
    from gsaj.rasterizer import FrameContext

    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)  # noqa: E731
    (camA, scA), (camB, scB) = _scene("early_saturation"), _scene("threshold_opacities")
    mk = lambda cam, sc: FrameContext(sc["means3D"].shape[0], cam["W"], cam["H"], sc["shs"].shape[1], dev, per_gaussian_tau=True)  # noqa: E731
    fa = mk(camA, scA)
    fa._ensure_binning(20000)  # (both scenes have fewer instances than the capacity this sizes the arena for)
    _frame_grads(fa, camA, scA, t, *hp.seeds(camA, seed=3), sync=True)
    _frame_grads(fa, camA, scA, t, *hp.seeds(camA, seed=3), sync=False)  # (carved for the capacity, as the next context carves it)
    dLc, dLd = hp.seeds(camB, seed=4)
    fb = mk(camB, scB)
    fb.binning, fb.capacity = fa.binning, fa.capacity
    got = _frame_grads(fb, camB, scB, t, dLc, dLd, sync=False)
    assert fb.status()[0] <= fb.capacity and fb.binning.data_ptr() == fa.binning.data_ptr()
    want = _frame_grads(mk(camB, scB), camB, scB, t, dLc, dLd, sync=True)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_stale_flags_window():
    """The same for a BatchContext with K = 3."""
    import torch
    from gsaj.rasterizer import BatchContext

    (_, scA), (_, scB) = _scene("early_saturation"), _scene("threshold_opacities")
    camsA, camsB = _window("early_saturation"), _window("threshold_opacities")
    aA, aB = _batch_tensors(scA, camsA), _batch_tensors(scB, camsB)
    mk = lambda cams, sc: BatchContext(3, sc["means3D"].shape[0], cams[0]["W"], cams[0]["H"], sc["shs"].shape[1], aA["dev"])  # noqa: E731
    ba = mk(camsA, scA)
    ba._size(36000)
    _batch_run(ba, camsA, aA)
    assert not any(ab for _, _, ab in ba.status())
    bb = mk(camsB, scB)
    bb.capacity, bb.bin_stride, bb.binning = ba.capacity, ba.bin_stride, ba.binning
    got = _batch_run(bb, camsB, aB, sync=False)
    assert not any(ab for _, _, ab in bb.status()) and bb.binning.data_ptr() == ba.binning.data_ptr()
    got = {k: v.clone() for k, v in got.items() if torch.is_tensor(v)}
    want = _batch_run(mk(camsB, scB), camsB, aB)
    for k in got:
        assert torch.equal(got[k], want[k]), k


def test_backward_twice_after_one_forward():
    """The sweep that forms the live list reads nothing a backward writes but its own output."""
    import torch

    cam, sc = _scene("threshold_opacities")
    (_, _), kw = _oracle(None, "threshold_opacities")
    out, args = hp.gpu_forward(cam, sc, DEG, bg=hp.PARITY_BG, kw=kw)
    dLc, dLd = hp.seeds(cam, seed=2)
    g1 = [x.clone() for x in hp.gpu_backward(cam, DEG, out, args, dLc, dLd)]
    g2 = hp.gpu_backward(cam, DEG, out, args, dLc, dLd)
    for nm, a, b in zip(hp.GRAD_NAMES, g1, g2):
        assert torch.equal(a, b), nm


@pytest.mark.parametrize("name", FLAG_SCENES)
def test_flags_equal_a_restatement_of_the_live_set(name):
    """The exported flags against NumPy on the device's own lists and last contributors and the oracle's means and conics: an
    entry is live in a quadrant if some pixel of it has position <= n_contrib, power <= 0 and alpha >= 1/255.  Entries that
    only a pixel within a relative 1e-4 of the alpha threshold (or 1e-6 of power = 0) decides are left out: at most 0.1 % of
    the visited (quadrant, entry) pairs."""
    from gsaj import rasterizer as C

    cam, sc = _scene(name)
    W, H, P = cam["W"], cam["H"], sc["means3D"].shape[0]
    (_, st), kw = _oracle(None, name)
    out, args = hp.gpu_forward(cam, sc, DEG, bg=hp.PARITY_BG, kw=kw)
    hp.gpu_backward(cam, DEG, out, args, *hp.seeds(cam, seed=1))
    R, geom, binning, img = out[0], out[3], out[4], out[5]
    dbg = {k: v.cpu().numpy() for k, v in C.debug_export(P, R, W, H, geom, binning, img).items()}
    taken, reached = (x.cpu().numpy() for x in C.debug_export_taken(R, W, H, binning, img))
    taken = taken.view(np.uint32)
    m2, co = st["means2D"].astype(np.float64), st["conic_opacity"].astype(np.float64)
    pl, rg, nc = dbg["point_list"].astype(np.int64), dbg["ranges"].astype(np.int64), dbg["n_contrib"].reshape(H, W).astype(np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    thr = 1.0 / 255.0
    visited = ambiguous = wrong = beyond = 0
    for tile in range(gx * gy):
        ty, tx = divmod(tile, gx)
        a, b = rg[tile]
        ids = pl[a:b]
        n = len(ids)
        if n == 0:
            continue
        mx, my, A, B, Cc, O = m2[ids, 0], m2[ids, 1], co[ids, 0], co[ids, 1], co[ids, 2], co[ids, 3]
        pos = np.arange(n)
        for q in range(4):
            X0, Y0 = tx * 16 + (q & 1) * 8, ty * 16 + (q >> 1) * 8
            ys, xs = np.mgrid[Y0:Y0 + 8, X0:X0 + 8]
            inside = (xs < W) & (ys < H)
            last = np.where(inside, nc[np.minimum(ys, H - 1), np.minimum(xs, W - 1)], 0)
            dx, dy = mx[None, None, :] - xs[:, :, None], my[None, None, :] - ys[:, :, None]
            power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
            alpha = O * np.exp(power)
            reach = pos[None, None, :] < last[:, :, None]
            sure = (reach & (power <= -1e-6) & (alpha >= thr * (1 + 1e-4))).any(axis=(0, 1))
            maybe = (reach & (power <= 1e-6) & (alpha >= thr * (1 - 1e-4))).any(axis=(0, 1))
            flag = ((taken[a:b] >> (8 * q)) & 0xff).astype(np.int64)
            wmax = int(last.max())
            visited += min(wmax, n)
            ambiguous += int((maybe & ~sure).sum())
            decided = sure | ~maybe
            wrong += int((flag[decided] != sure[decided].astype(np.int64)).sum())
            beyond += int((flag[wmax:] != 0).sum())
    print("%s: visited %d, left out %d (%.1e), wrong %d, beyond the last contributor %d; reached %d of %d rows"
          % (name, visited, ambiguous, ambiguous / max(visited, 1), wrong, beyond, int(reached.sum()), R))
    assert ambiguous <= 1e-3 * visited
    assert wrong == 0
    assert beyond == 0
    assert int(reached.sum()) == int((taken[:R] != 0).sum())
