"""GPU: the covisibility window (csrc/covis.hip, gsaj.covisibility.CovisibilityWindow) against the NumPy restatement
(tests/covis_restated.py) and the outcomes recorded from the reference (tests/golden/covis_prune.npz), and end to end behind the
rasteriser's n_touched, where the counts must equal the reference's torch statement on the same tensors and gsaj.keyframes must
decide alike from both.  Everything is an integer: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import covis_restated as cr
import helpers as hp
from gsaj import synthetic as syn

pytestmark = pytest.mark.gpu

GARBAGE = 0x7BADBEEF
LAYOUTS = {1: ([0], [31]), 3: ([0, 5, 31],), 8: (list(range(8)),), 11: (list(range(11)), [31, 0, 5, 17, 2, 9, 30, 12, 1, 22, 8])}


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev()) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device=_dev()).to(dtype)


def _words_t(words_u32):
    return _t(np.asarray(words_u32, np.uint32).view(np.int32))


def _words_np(t):
    return t.cpu().numpy().view(np.uint32)


def dev_pack(words_t, nt_t, slots, clear_mask):
    import torch
    from gsaj import _lib
    K, P = nt_t.shape
    _lib.check(_lib.load().gsaj_covis_pack(K, P, nt_t.data_ptr(), (ctypes.c_int * K)(*slots), clear_mask, words_t.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "gsaj_covis_pack")


def dev_query(words_t, cur_t, query_slot, slot_mask, out_t):
    import torch
    from gsaj import _lib
    _lib.check(_lib.load().gsaj_covis_query(words_t.numel(), words_t.data_ptr(), None if cur_t is None else cur_t.data_ptr(), query_slot,
                                            slot_mask, out_t.data_ptr(), torch.cuda.current_stream().cuda_stream), "gsaj_covis_query")
    return out_t.cpu().numpy()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000, 70001])
def test_pack_and_query_match_the_restatement(P):
    """One lane, the wave boundary from both sides, a ragged last workgroup, and enough workgroups (35 of 2048 Gaussians) that the
    cross-workgroup sum runs; rows of 1, 3, 8 and 11 views in contiguous and scattered slots, bit 31 among them."""
    import torch
    rng = np.random.default_rng(P)
    old = rng.integers(0, 2 ** 32, size=P, dtype=np.uint64).astype(np.uint32)
    out_t = torch.empty(65, dtype=torch.int32, device=_dev())
    for K, layouts in LAYOUTS.items():
        for slots in layouts:
            for density in (0.0, 0.5, 1.0):
                nt = cr.make_case(P, K, density, seed=1000 * K + int(10 * density))
                nt_t = _t(nt)
                # (a) keep the other bits of words full of garbage, (b) rebuild everything
                for clear in (0, 0x00F0F000, 0xFFFFFFFF):
                    words_t = _words_t(old)
                    dev_pack(words_t, nt_t, slots, clear)
                    want = cr.pack(old, nt, slots, clear)
                    assert_array_equal(_words_np(words_t), want, err_msg="pack K=%d slots=%s density=%g clear=%#x" % (K, slots, density, clear))
                mask = cr.bits_of(slots)
                for cur_density in (0.0, 0.5, 1.0):
                    cur = cr.make_case(P, 1, cur_density, seed=77 + K)[0]
                    out_t.fill_(GARBAGE)
                    got = dev_query(words_t, _t(cur), 0, mask, out_t)
                    assert_array_equal(got, cr.query(want, cur_n_touched=cur, slot_mask=mask), err_msg="query by cur K=%d slots=%s" % (K, slots))
                    assert_array_equal(dev_query(words_t, _t(cur), 0, mask, out_t), got, err_msg="the same query again")
                for qs in (slots[0], slots[-1]):
                    out_t.fill_(-1)
                    got = dev_query(words_t, None, qs, mask, out_t)
                    assert_array_equal(got, cr.query(want, query_slot=qs, slot_mask=mask), err_msg="query by slot %d" % qs)
                    assert got[qs] == got[32 + qs] == got[64]
                # a slot_mask that leaves a set slot out: zeros for it, the others as before
                part = mask & ~(1 << slots[-1])
                out_t.fill_(GARBAGE)
                got = dev_query(words_t, None, slots[0], part, out_t)
                assert_array_equal(got, cr.query(want, query_slot=slots[0], slot_mask=part))
                assert got[slots[-1]] == 0 and got[32 + slots[-1]] == 0


def test_window_slot_updates():
    import torch
    from gsaj import _lib
    from gsaj.covisibility import CovisibilityWindow

    P, K = 3001, 4
    nt = cr.make_case(P, K + 2, 0.5, 9)
    cw = CovisibilityWindow(P, _dev())
    cw.set_window([10, 11, 12, 13], _t(nt[:K]))
    words = cr.pack(np.zeros(P, np.uint32), nt[:K], [0, 1, 2, 3], 0xFFFFFFFF)
    assert_array_equal(_words_np(cw.words), words)
    # a new keyframe takes the lowest free slot and leaves the other bits alone; writing an id the window holds reuses its slot
    cw.set_keyframe(14, _t(nt[4]))
    words = cr.pack(words, nt[4:5], [4], 0)
    assert cw.slot_of[14] == 4
    assert_array_equal(_words_np(cw.words), words)
    cw.set_keyframe(11, _t(nt[5]))
    words = cr.pack(words, nt[5:6], [1], 0)
    assert_array_equal(_words_np(cw.words), words)
    # drop: excluded from the queries at once, bits cleared by the next pack, slot reused without stale bits
    cw.drop(12)
    per_kf, nq = cw.counts(kf_id=10)
    want = cr.query(words, query_slot=0, slot_mask=0b11011)
    assert sorted(per_kf) == [10, 11, 13, 14] and nq == want[64]
    assert_array_equal(cw.out.cpu().numpy(), want)
    for kf, s in ((10, 0), (11, 1), (13, 3), (14, 4)):
        assert per_kf[kf] == (int(want[s]), int(want[32 + s])) and all(type(v) is int for v in per_kf[kf])
    cw.set_keyframe(15, _t(np.zeros(P, np.int32)))  # an all-zero row: whatever survives in slot 2 would be stale
    assert cw.slot_of[15] == 2
    words = cr.pack(words, np.zeros((1, P), np.int32), [2], 1 << 2)
    assert_array_equal(_words_np(cw.words), words)
    assert not ((words >> np.uint32(2)) & 1).any()
    ref = cw.as_reference_dict()
    assert sorted(ref) == [10, 11, 13, 14, 15] and all(v.dtype == torch.int64 for v in ref.values())
    for kf, v in ref.items():
        assert_array_equal(v.cpu().numpy(), (words >> np.uint32(cw.slot_of[kf])) & 1)
    # round trip through the reference's dict
    cw2 = CovisibilityWindow(P, _dev()).from_reference_dict(ref)
    assert list(cw2.slot_of) == list(ref)
    for kf, v in cw2.as_reference_dict().items():
        assert torch.equal(v, ref[kf])
    # the 33rd keyframe
    cw3 = CovisibilityWindow(64, _dev())
    row = _t(np.ones(64, np.int32))
    for kf in range(32):
        cw3.set_keyframe(100 + kf, row)
    assert cw3.slot_mask == 0xFFFFFFFF and int(cw3.query(kf_id=131)[31]) == 64
    with pytest.raises(_lib.GsajError):
        cw3.set_keyframe(132, row)
    cw3.set_keyframe(105, row)  # an id the window holds is still fine


@pytest.mark.parametrize("mode,initialized", [(m, i) for m in ("odometry", "slam") for i in (False, True)])
def test_prune_mask_golden_and_compaction(golden_dir, mode, initialized):
    import torch
    from gsaj.covisibility import CovisibilityWindow

    g = np.load(os.path.join(golden_dir, "covis_prune.npz"))
    window = g["window"].tolist()
    K, P = g["n_touched"].shape
    cw = CovisibilityWindow(P, _dev())
    cw.set_window(window, _t(g["n_touched"]))
    cw.set_keyframe(99, _t(np.ones(P, np.int32)))  # a keyframe outside `window` must not count as an observation
    ids = _t(g["unique_kfIDs"])
    to_prune, n_pruned = cw.prune_mask(window, ids if mode == "slam" else None, mode, initialized)
    tag = "%s_%d" % (mode, int(initialized))
    assert to_prune.dtype == torch.uint8 and n_pruned.dtype == torch.int32
    assert_array_equal(to_prune.cpu().numpy(), g["to_prune_" + tag])
    assert_array_equal(cw.n_obs.cpu().numpy(), g["n_obs_" + tag])
    assert int(n_pruned) == int(g["to_prune_" + tag].sum())
    max_obs, kf_min = cr.prune_arguments(window, mode, initialized)
    want = cr.prune_mask(_words_np(cw.words), cr.bits_of(range(K)), None if kf_min is None else g["unique_kfIDs"], kf_min, max_obs)
    assert_array_equal(to_prune.cpu().numpy(), want[0])
    assert int(n_pruned) == want[2]
    # compaction: the same rows the reference keeps, occ_aware_visibility[idx][~to_prune]
    before = cw.as_reference_dict()
    keep = to_prune == 0
    cw.compact(keep)
    assert cw.P == P - int(n_pruned) and cw.to_prune.numel() == cw.P
    after = cw.as_reference_dict()
    for kf in window + [99]:
        assert torch.equal(after[kf], before[kf][keep])
    per_kf, nq = cw.counts(kf_id=window[0])  # the compacted window still answers
    assert nq == int(before[window[0]][keep].sum()) and per_kf[window[1]][0] == int((before[window[0]][keep] & before[window[1]][keep]).sum())


def test_prune_mask_more_than_one_workgroup():
    """P beyond 2048 x 256 lanes takes the grid-stride loop; ids and n_obs optional."""
    from gsaj.covisibility import CovisibilityWindow

    P, K = 2048 * 256 + 777, 5
    nt = cr.make_case(P, K, 0.5, 3)
    ids = np.random.default_rng(4).integers(0, 9, size=P).astype(np.int32)
    cw = CovisibilityWindow(P, _dev())
    cw.set_window([3, 8, 5, 1, 7], _t(nt))
    words = cr.pack(np.zeros(P, np.uint32), nt, list(range(K)), 0xFFFFFFFF)
    assert_array_equal(_words_np(cw.words), words)
    to_prune, n_pruned = cw.prune_mask([3, 8, 5, 7], _t(ids), "slam", True)  # slots 0 1 2 4; the third-newest id is 5
    want = cr.prune_mask(words, 0b10111, ids, 5, 3)
    assert_array_equal(to_prune.cpu().numpy(), want[0])
    assert_array_equal(cw.n_obs.cpu().numpy(), want[1])
    assert int(n_pruned) == want[2]
    cur = cr.make_case(P, 1, 0.5, 8)[0]
    assert_array_equal(cw.query(cur_n_touched=_t(cur)).cpu().numpy(), cr.query(words, cur_n_touched=cur, slot_mask=0b11111))


def _torch_counts(cur_vis, occ):
    """The reference's statement (utils/slam_frontend.py:218-224, 239-246) on the same device tensors."""
    import torch
    per_kf = {kf: (int(torch.logical_and(cur_vis, v).count_nonzero()), int(v.count_nonzero())) for kf, v in occ.items()}
    return per_kf, int(cur_vis.count_nonzero())


def test_end_to_end_behind_the_rasteriser():
    import torch
    from gsaj import keyframes as kfm
    from gsaj.covisibility import CovisibilityWindow
    from gsaj.rasterizer import BatchContext, FrameContext

    cam0, sc, deg = hp.make("p2000_160x120")
    K = 4
    cams = syn.keyframe_cameras(K + 1, W=cam0["W"], H=cam0["H"], fx=cam0["fx"], fy=cam0["fy"], cx=cam0["cx"], cy=cam0["cy"])
    dev = _dev()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    P, M = sc["means3D"].shape[0], sc["shs"].shape[1]
    bg = torch.zeros(3, device=dev)
    geo = dict(sh_degree=deg, shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    kf_cams, cur_cam = cams[:K], cams[K]
    bc = BatchContext(K, P, cam0["W"], cam0["H"], M, dev)
    bc.forward(bg, t(sc["means3D"]), t(sc["opacities"]), t(np.stack([c["viewmatrix"] for c in kf_cams])),
               t(np.stack([c["projmatrix"] for c in kf_cams])), t(np.stack([c["campos"] for c in kf_cams])), cam0["tanfovx"], cam0["tanfovy"], **geo)
    fc = FrameContext(P, cam0["W"], cam0["H"], M, dev)
    fc.forward(bg, t(sc["means3D"]), t(sc["opacities"]), t(cur_cam["viewmatrix"]), t(cur_cam["projmatrix"]), t(cur_cam["campos"]),
               cam0["tanfovx"], cam0["tanfovy"], **geo)
    window = [12, 9, 6, 3]  # newest first, as the front end keeps it
    cw = CovisibilityWindow(P, dev)
    cw.set_window(window, bc.n_touched)
    counts = cw.counts(cur_n_touched=fc.n_touched)
    occ = {kf: (bc.n_touched[k] > 0).long() for k, kf in enumerate(window)}  # slam_backend.py:240
    cur_vis = (fc.n_touched > 0).long()                                       # slam_frontend.py:414
    want = _torch_counts(cur_vis, occ)
    assert counts == want
    assert 0 < want[1] < P and all(0 < i < n for i, n in want[0].values()), "the scene must make the counts non-trivial"
    for kf, v in cw.as_reference_dict().items():
        assert torch.equal(v, occ[kf])
    # the union the reference forms with logical_or is |a| + |b| - |a & b|
    for kf, (inter, n) in counts[0].items():
        assert counts[1] + n - inter == int(torch.logical_or(cur_vis, occ[kf]).count_nonzero())
    # the decisions, fed from the device counts and from the torch counts
    poses = {kf: np.asarray(c["viewmatrix"], np.float32).reshape(4, 4).T for kf, c in zip(window + [15], kf_cams + [cur_cam])}
    base = dict(kf_translation=0.08, kf_min_translation=0.05, kf_overlap=0.9, kf_interval=2, single_thread=False)
    for extra in (dict(window_size=8, kf_cutoff=0.3), dict(window_size=4, kf_cutoff=0.3), dict(window_size=3, kf_cutoff=0.95), dict(window_size=4)):
        cfg = dict(base, **extra)
        for initialized in (False, True):
            got = (kfm.wants_keyframe(15, window, counts, poses, cfg, 2.0), kfm.add_to_window(15, counts, poses, window, cfg, initialized))
            ref = (kfm.wants_keyframe(15, window, want, poses, cfg, 2.0), kfm.add_to_window(15, want, poses, window, cfg, initialized))
            assert got == ref and type(got[0]) is bool and got[1][0][0] == 15
    assert len(kfm.add_to_window(15, counts, poses, window, dict(base, window_size=4), True)[0]) == 4


def test_argument_errors_raise():
    import torch
    from gsaj import _lib
    from gsaj.covisibility import CovisibilityWindow

    P = 500
    cw = CovisibilityWindow(P, _dev())
    ok = _t(cr.make_case(P, 2, 0.5, 1))
    cw.set_window([1, 2], ok)
    bad_rows = [ok.long(), ok.float(), ok[:, :-1], ok.cpu(), ok[0], ok.cpu().numpy()]
    for bad in bad_rows:
        with pytest.raises(_lib.GsajError):
            cw.set_window([1, 2], bad)
    for bad in (ok[0].long(), ok[0, :-1], ok[0].cpu(), ok, None):
        with pytest.raises(_lib.GsajError):
            cw.set_keyframe(3, bad)
    for bad in (ok[0].long(), ok[0, :-1], ok[0].cpu()):
        with pytest.raises(_lib.GsajError):
            cw.query(cur_n_touched=bad)
    for call in (lambda: cw.query(), lambda: cw.query(cur_n_touched=ok[0], kf_id=1), lambda: cw.query(kf_id=7), lambda: cw.drop(7),
                 lambda: cw.set_window([1, 1], ok), lambda: cw.set_window([], ok[:0]), lambda: cw.prune_mask([1, 2], None, "slam", True),
                 lambda: cw.prune_mask([1, 2], ok[0], "slam", True), lambda: cw.prune_mask([1, 2], ok[0].long(), "slam", False),
                 lambda: cw.prune_mask([1, 7], None, "odometry"), lambda: cw.prune_mask([1, 2], None, "other"),
                 lambda: cw.compact(torch.ones(P - 1, dtype=torch.bool, device=_dev())), lambda: cw.compact(torch.ones(P, dtype=torch.bool)),
                 lambda: cw.compact(torch.ones(P, dtype=torch.int32, device=_dev())), lambda: cw.from_reference_dict({}),
                 lambda: cw.from_reference_dict({1: ok[0].cpu()}), lambda: CovisibilityWindow(0, _dev())):
        with pytest.raises(_lib.GsajError):
            call()
    # the window still works after all of that
    assert cw.counts(kf_id=1)[1] == int((ok[0] > 0).sum())
