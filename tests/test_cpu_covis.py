"""CPU: the NumPy restatement of the covisibility kernels (tests/covis_restated.py) and the host decisions of gsaj.keyframes
against outcomes recorded from the reference's own statements (tests/golden/covis_prune.npz, kf_decisions.npz, written by
tests/golden/make_covis_goldens.py); the new C-ABI symbols and the argument errors that need no GPU.  No kernel is launched."""
import ctypes
import json
import os

import numpy as np
import pytest

import covis_restated as cr

MODES = [(m, i) for m in ("odometry", "slam") for i in (False, True)]


@pytest.fixture(scope="module")
def prune_rec(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "covis_prune.npz")))


@pytest.fixture(scope="module")
def decisions(golden_dir):
    z = np.load(os.path.join(golden_dir, "kf_decisions.npz"))
    return z, json.loads(str(z["cases"]))


def counts_of(z, name, meta):
    """What CovisibilityWindow.counts(cur_n_touched=...) returns for the case's vectors, through the restated pack and query."""
    cur, kf = z[name + "/cur"], z[name + "/kf"]
    ids = meta["kf_ids"]
    if not ids:
        return {}, int(np.count_nonzero(cur))
    words = cr.pack(np.zeros(cur.shape[0], np.uint32), kf.astype(np.int32), list(range(len(ids))), 0xFFFFFFFF)
    out = cr.query(words, cur_n_touched=cur.astype(np.int32), slot_mask=cr.bits_of(range(len(ids))))
    return {k: (int(out[s]), int(out[32 + s])) for s, k in enumerate(ids)}, int(out[64])


def test_fixtures_are_small(golden_dir):
    for f in ("covis_prune.npz", "kf_decisions.npz"):
        assert os.path.getsize(os.path.join(golden_dir, f)) < 64 * 1024, f


def test_make_case_values():
    nt = cr.make_case(5000, 3, 0.5, 1)
    assert nt.dtype == np.int32 and set(np.unique(nt)) == set(cr.TOUCH_VALUES.tolist())
    assert not cr.make_case(100, 2, 0.0, 1).any() and cr.make_case(100, 2, 1.0, 1).all()


@pytest.mark.parametrize("mode,initialized", MODES)
def test_restated_prune_mask_matches_the_reference(prune_rec, mode, initialized):
    g = prune_rec
    window = g["window"].tolist()
    assert np.array_equal(g["n_touched"], cr.make_case(g["n_touched"].shape[1], len(window), 0.35, 5))  # the inputs are reproducible
    words = cr.pack(np.zeros(g["n_touched"].shape[1], np.uint32), g["n_touched"], list(range(len(window))), 0xFFFFFFFF)
    for k in range(len(window)):  # the packed bits are the reference's visibility vectors
        assert np.array_equal((words >> np.uint32(k)) & 1, g["visibility"][k])
    max_obs, kf_min = cr.prune_arguments(window, mode, initialized)
    to_prune, n_obs, n = cr.prune_mask(words, cr.bits_of(range(len(window))), None if kf_min is None else g["unique_kfIDs"], kf_min, max_obs)
    tag = "%s_%d" % (mode, int(initialized))
    assert np.array_equal(to_prune, g["to_prune_" + tag]) and np.array_equal(n_obs, g["n_obs_" + tag])
    assert n == int(g["to_prune_" + tag].sum()) and 0 < n < to_prune.size


def test_restated_pack_keeps_and_clears():
    nt = cr.make_case(200, 3, 0.5, 2)
    w = cr.pack(np.full(200, 0xFFFFFFFF, np.uint32), nt, [0, 5, 31], 0)
    assert np.array_equal(w | np.uint32(cr.bits_of([0, 5, 31])), np.full(200, 0xFFFFFFFF, np.uint32))  # other bits kept
    assert np.array_equal((w >> np.uint32(31)) & 1, nt[2] > 0)
    w2 = cr.pack(w, nt[:1], [7], 1 << 5)
    assert not ((w2 >> np.uint32(5)) & 1).any() and np.array_equal((w2 >> np.uint32(7)) & 1, nt[0] > 0)
    out = cr.query(w2, query_slot=31, slot_mask=(1 << 7) | (1 << 31))
    assert out[31] == out[63] == out[64] == np.count_nonzero(nt[2]) and out[7] == np.count_nonzero((nt[0] > 0) & (nt[2] > 0))
    assert out[0] == out[32] == 0  # slot 0 is set in the words but outside slot_mask


def test_ratio_arithmetic_is_float32():
    from gsaj import keyframes as kfm

    assert not kfm._lt(kfm.ratio(9, 10), 0.9) and float(np.float32(9) / np.float32(10)) < 0.9  # (a double threshold decides otherwise)
    assert kfm._le(kfm.ratio(3, 10), 0.3) and kfm._le(kfm.ratio(2, 5), 0.4)
    nan = kfm.ratio(0, 0)
    assert np.isnan(nan) and not kfm._lt(nan, 0.9) and not kfm._le(nan, 0.4)


def test_decision_fixture_holds_the_cases_it_is_for(decisions):
    z, cases = decisions
    kinds = [c["kind"] for c in cases.values()]
    assert kinds.count("is_keyframe") >= 7 and kinds.count("wants_keyframe") >= 6 and kinds.count("add_to_window") >= 12
    assert cases["kf_ratio_exactly_at_overlap"]["decision"] is False and cases["kf_ratio_just_below_overlap"]["decision"] is True
    assert cases["add_ratio_exactly_at_cutoff"]["removed"] == 8 and cases["add_ratio_just_above_cutoff"]["removed"] is None
    assert cases["add_not_initialized_forces_0p4"]["removed"] == 8 and cases["add_initialized_same_counts"]["removed"] is None
    assert cases["add_two_below_cutoff_last_leaves"]["window_out"] == [20, 10, 9, 8]
    assert cases["add_cutoff_and_overflow_two_leave"]["window_out"] == [20, 10, 9, 7] and cases["add_cutoff_and_overflow_two_leave"]["removed"] == 6
    assert "kf_cutoff" not in cases["add_cutoff_absent_defaults_0p4"]["config"]
    assert cases["add_cutoff_absent_defaults_0p4"]["removed"] == 8 and cases["add_cutoff_0p3_same_counts"]["removed"] is None


def run_case(z, name, meta, counts):
    from gsaj import keyframes as kfm

    poses = {f: z[name + "/w2c"][i] for i, f in enumerate(meta["frames"])}
    cfg, cur, window = meta["config"], meta["cur"], meta["window"]
    if meta["kind"] == "is_keyframe":
        return dict(decision=kfm.is_keyframe(cur, window[0], counts, poses, cfg, meta["median_depth"]))
    if meta["kind"] == "wants_keyframe":
        return dict(decision=kfm.wants_keyframe(cur, window, counts, poses, cfg, meta["median_depth"]))
    w, removed = kfm.add_to_window(cur, counts, poses, window, cfg, meta["initialized"])
    return dict(window_out=w, removed=removed)


def test_keyframes_reproduce_every_recorded_decision(decisions):
    z, cases = decisions
    for name, meta in cases.items():
        before = list(meta["window"])
        got = run_case(z, name, meta, counts_of(z, name, meta))
        for key, val in got.items():
            assert type(val) in (bool, list, int, type(None)), (name, key, type(val))  # Python values, never tensors
            assert val == meta[key], (name, key, val, meta[key])
        assert meta["window"] == before  # the caller's window list is not modified


def test_new_symbols_exported_and_argument_errors():
    from gsaj import _lib

    lib = _lib.load()
    assert lib.gsaj_version() >= 103
    for name in ("gsaj_covis_pack", "gsaj_covis_query", "gsaj_covis_prune_mask"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    slots = lambda *s: (ctypes.c_int * len(s))(*s)  # noqa: E731
    fake = 4096  # never dereferenced: every call below is rejected before anything is launched
    bad = [lib.gsaj_covis_pack(1, 0, fake, slots(0), 0, fake, None), lib.gsaj_covis_pack(0, 10, fake, slots(0), 0, fake, None),
           lib.gsaj_covis_pack(33, 10, fake, slots(*range(33)), 0, fake, None), lib.gsaj_covis_pack(1, 10, fake, slots(32), 0, fake, None),
           lib.gsaj_covis_pack(1, 10, fake, slots(-1), 0, fake, None), lib.gsaj_covis_pack(2, 10, fake, slots(3, 3), 0, fake, None),
           lib.gsaj_covis_pack(1, 10, None, slots(0), 0, fake, None), lib.gsaj_covis_pack(1, 10, fake, slots(0), 0, None, None),
           lib.gsaj_covis_query(0, fake, fake, 0, 1, fake, None), lib.gsaj_covis_query(10, None, fake, 0, 1, fake, None),
           lib.gsaj_covis_query(10, fake, fake, 0, 1, None, None), lib.gsaj_covis_query(10, fake, None, 32, 1, fake, None),
           lib.gsaj_covis_query(10, fake, None, -1, 1, fake, None),
           lib.gsaj_covis_prune_mask(0, fake, 1, None, 0, 2, fake, None, fake, None),
           lib.gsaj_covis_prune_mask(10, None, 1, None, 0, 2, fake, None, fake, None),
           lib.gsaj_covis_prune_mask(10, fake, 1, None, 0, 2, None, None, fake, None),
           lib.gsaj_covis_prune_mask(10, fake, 1, None, 0, 2, fake, None, None, None)]
    assert bad == [-1] * len(bad), bad
    assert b"gsaj_covis_prune_mask" in lib.gsaj_last_error()


def test_window_needs_a_device():
    from gsaj import _lib
    from gsaj.covisibility import CovisibilityWindow

    with pytest.raises(_lib.GsajError):
        CovisibilityWindow(100, "cpu")
