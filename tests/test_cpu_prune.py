"""CPU: the C-ABI symbols of the row compaction (csrc/compact.hip) and the argument errors that need no GPU; the NumPy restatement
of the reference's prune_points (tests/prune_restated.py) against the outcome recorded from the reference's own statements
(tests/golden/prune_P120.npz, written by tests/golden/make_prune_goldens.py).  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest

import prune_restated as pr


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "prune_P120.npz"))


def test_fixture_is_small_and_holds_the_cases(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "prune_P120.npz")) < 200 * 1024
    for name, cols in (("aniso", 3), ("iso", 1)):
        rec = pr.case(golden, name)
        mask = rec["mask"]
        assert mask.shape == (120,) and mask[0] and mask[119] and 0.2 * 120 < mask.sum() < 0.4 * 120
        assert rec["in_scaling"].shape == (120, cols) and rec["in_f_rest"].shape == (120, 3, 3)
        assert all(float(rec["in_step_" + n]) == 3.0 for n in pr.NAMES)
        assert all(np.abs(rec["in_exp_avg_sq_" + n]).min() > 0 for n in pr.NAMES)  # three real steps: no moment is zero
        assert all(len(np.unique(rec["in_" + a])) > 2 for a in pr.AUX)


@pytest.mark.parametrize("name", ["aniso", "iso"])
def test_restated_prune_reproduces_the_reference(golden, name):
    rec = pr.case(golden, name)
    out = pr.prune(rec)
    want = sorted(k for k in rec if k.startswith("out_"))
    assert sorted(out) == want and len(want) == 6 * 4 + 5  # parameter, two moments and step of six groups; five bookkeeping tensors
    n = int((rec["mask"] == 0).sum())
    for k in want:
        assert out[k].dtype == rec[k].dtype and out[k].shape == rec[k].shape, k
        assert np.array_equal(pr.bits(out[k]), pr.bits(rec[k])), k
        if "_step_" not in k:
            assert out[k].shape[0] == n, k
    for nme in pr.NAMES:  # step is left alone
        assert float(rec["out_step_" + nme]) == float(rec["in_step_" + nme]) == 3.0


def test_new_symbols_exported_and_argument_errors():
    from gsaj import _lib

    lib = _lib.load()
    assert lib.gsaj_version() >= 104
    for name in ("gsaj_compact_workspace_bytes", "gsaj_compact_plan", "gsaj_compact_count", "gsaj_compact_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    nb = lambda P: (P + 255) // 256  # noqa: E731
    for P in (1, 256, 257, 10 ** 6):  # nb + O(1) words
        assert 4 * (nb(P) + 1) <= lib.gsaj_compact_workspace_bytes(P) <= 4 * (nb(P) + 1) + 512
    assert lib.gsaj_compact_workspace_bytes(0) == 0 and lib.gsaj_compact_workspace_bytes(-3) == 0

    fake = 4096  # never dereferenced: every call below is rejected before anything is launched
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)  # noqa: E731
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    n = ctypes.c_int(-7)
    rows = lib.gsaj_compact_rows
    bad = [lib.gsaj_compact_plan(0, fake, 1, fake, None), lib.gsaj_compact_plan(-1, fake, 1, fake, None),
           lib.gsaj_compact_plan(10, None, 1, fake, None), lib.gsaj_compact_plan(10, fake, 1, None, None),
           lib.gsaj_compact_count(None, None, ctypes.byref(n)), lib.gsaj_compact_count(fake, None, None),
           rows(0, 1, ptrs(fake), ptrs(2 * fake), ints(4), fake, None),
           rows(10, 0, ptrs(fake), ptrs(2 * fake), ints(4), fake, None),
           rows(10, 33, ptrs(*[fake] * 33), ptrs(*[2 * fake] * 33), ints(*[4] * 33), fake, None),
           rows(10, 1, None, ptrs(2 * fake), ints(4), fake, None), rows(10, 1, ptrs(fake), None, ints(4), fake, None),
           rows(10, 1, ptrs(fake), ptrs(2 * fake), None, fake, None), rows(10, 1, ptrs(fake), ptrs(2 * fake), ints(4), None, None),
           rows(10, 1, ptrs(None), ptrs(2 * fake), ints(4), fake, None), rows(10, 1, ptrs(fake), ptrs(None), ints(4), fake, None),
           rows(10, 2, ptrs(fake, fake), ptrs(2 * fake, 3 * fake), ints(4, 0), fake, None),
           rows(10, 2, ptrs(fake, fake), ptrs(2 * fake, 3 * fake), ints(4, -4), fake, None),
           rows(10, 1, ptrs(fake), ptrs(2 * fake), ints(6), fake, None), rows(10, 1, ptrs(fake), ptrs(2 * fake), ints(2), fake, None),
           rows(10, 1, ptrs(fake), ptrs(2 * fake), ints(4100), fake, None),
           rows(10, 2, ptrs(fake, 3 * fake), ptrs(2 * fake, 3 * fake), ints(4, 4), fake, None)]
    assert bad == [-1] * len(bad), bad
    assert b"gsaj_compact_rows" in lib.gsaj_last_error()
    assert n.value == -7
    lib.gsaj_compact_plan(0, fake, 1, fake, None)
    assert b"gsaj_compact_plan" in lib.gsaj_last_error()
    lib.gsaj_compact_count(None, None, ctypes.byref(n))
    assert b"gsaj_compact_count" in lib.gsaj_last_error()


def test_plan_refuses_a_host_mask():
    import torch
    from gsaj import _lib
    from gsaj.pruning import CompactPlan

    for bad in (torch.ones(10, dtype=torch.bool), torch.ones(10, dtype=torch.uint8), np.ones(10, bool), None):
        with pytest.raises(_lib.GsajError):
            CompactPlan(bad)


def test_model_has_prune_points():
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from gsaj.covisibility import CovisibilityWindow

    assert callable(getattr(GaussianModel, "prune_points", None)) and callable(getattr(CovisibilityWindow, "compact_plan", None))
