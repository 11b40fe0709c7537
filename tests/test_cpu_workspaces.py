"""CPU: every workspace size function, and the offsets the ABI exports, pinned to recorded values over a ladder that sits on every
rounding edge.  No kernel is launched: the size functions are pure host code (csrc/workspace.h: a Carver over a null base).

tests/golden/workspace_bytes.json was recorded with record() below from a library built from the commit BEFORE the layouts moved
onto csrc/workspace.h (GSAJ_LIB_PATH pointing at that build), the motion-stereo entries from the commit before its entry points'
checks moved to csrc/sgm.h:

    python -c "import sys; sys.path.insert(0, 'tests'); import test_cpu_workspaces as t; t.write_golden()"

A layout change that is meant to move a size re-records it with the same line; one that is not meant to fails here.  The second
half asserts the relations the entry points rely on: a batched workspace is K blocks of view_stride(one view), and every stride
is a multiple of 256."""
import ctypes
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")

WH = [(1, 1), (15, 15), (16, 16), (17, 17), (33, 17), (64, 48), (640, 480)]
P = [0, 1, 31, 32, 33, 255, 256, 257, 1000]
R = [0, 1, 63, 64, 65, 100000]
K = [1, 3]


def _x(*axes):
    """Cartesian product of the axes; an axis of tuples contributes its members flat."""
    return [sum(((a,) if not isinstance(a, tuple) else a for a in row), ()) for row in itertools.product(*axes)]


# name -> argument tuples.  Every function of the CONTRACTS table of tests/test_gpu_memory_contracts.py is here (checked below),
# with one illegal value for each that has a "returns 0" (or 512) branch, and negative counts where the function maps them.
CASES = {
    "gsaj_geom_workspace_bytes": _x(P + [-5]),
    "gsaj_image_workspace_bytes": _x(WH),
    "gsaj_binning_workspace_bytes": _x(R + [-1]),
    "gsaj_loss_workspace_bytes": _x(WH),
    "gsaj_fused_loss_workspace_bytes": _x(WH),
    "gsaj_fused_loss_batch_workspace_bytes": _x([0, -2] + K, WH),
    "gsaj_isotropic_workspace_bytes": _x(P),
    "gsaj_ssim_workspace_bytes": _x([1, 2, 16], [1, 3, 4], WH) + [(0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, 0)],
    "gsaj_refine_loss_workspace_bytes": _x(WH) + [(0, 5)],
    "gsaj_pose_jac_workspace_bytes": _x(P + [-5], WH),
    "gsaj_pose_jac_batch_workspace_bytes": _x([0, -2] + K, P + [-5], [(1, 1), (640, 480)]),
    "gsaj_pyramid_bytes": _x(WH, [1, 2, 4], [(0, 0), (1, 0), (0, 1), (1, 1)]) + [(64, 48, 0, 1, 1), (64, 48, 5, 1, 1), (0, 48, 1, 1, 1)],
    "gsaj_dist2_workspace_bytes": _x(P + [2047, 2048, 2049, -1]),
    "gsaj_seed_workspace_bytes": _x(WH) + [(0, 0), (-1, 4), (65536, 32768)],
    "gsaj_grad_mask_workspace_bytes": _x(WH) + [(2, 2), (1, 9), (65536, 32768)],
    "gsaj_compact_workspace_bytes": _x(P + [-1]),
    "gsaj_densify_workspace_bytes": _x(P, [1, 2, 4]) + [(1000, 0), (1000, 5), (-1, 2)],
    "gsaj_eval_workspace_bytes": _x([1, 3, 4], WH) + [(0, 16, 16), (3, 0, 16), (3, 16, 0)],
    "gsaj_dense_workspace_bytes": _x([0, 1, 15, 1000, -3], WH),
    "gsaj_dense_project_workspace_bytes": _x(P + [-3]),
    # what the ABI exports beside the sizes: the partial rows a caller sizes its own buffers by
    "gsaj_pose_jac_partial_rows": _x(WH),
    "gsaj_rgbd_align_partial_rows": _x(WH) + [(2, 2)],
}
STEREO = _x(WH + [(129, 3), (4096, 2)], [16, 64, 128], [4, 8]) + [(64, 48, 24, 4), (64, 48, 16, 5), (4097, 1, 16, 4)]
MOTION_STEREO = _x(WH + [(129, 3), (4096, 2)], [16, 64, 128], [4, 8]) + [(64, 48, 24, 4), (64, 48, 16, 5), (0, 48, 16, 4)]   # (1, 1) is legal here
# the two matchers: size function -> (offsets function, how many offsets it gives, the ladder)
MATCHERS = {"gsaj_stereo_workspace_bytes": ("gsaj_debug_stereo_offsets", 2, STEREO),
            "gsaj_motion_stereo_bytes": ("gsaj_debug_motion_stereo_offsets", 3, MOTION_STEREO)}
PYRAMID_LEVELS = [a + (l,) for a in CASES["gsaj_pyramid_bytes"] for l in (1, 2, 4)]


def _key(args):
    return ",".join(str(a) for a in args)


def record(lib):
    """{function: {"a,b,..": value}} of the library at hand: the sizes, gsaj_stereo_workspace_bytes / gsaj_debug_stereo_offsets as
    [rc, bytes, cost_off, sum_off], gsaj_motion_stereo_bytes / gsaj_debug_motion_stereo_offsets as [rc, bytes, pc_off, cost_off, sum_off]
    and gsaj_pyramid_level as [rc, W_l, H_l, color_off, depth_off, mask_off]."""
    out = {name: {_key(a): int(getattr(lib, name)(*a)) for a in cases} for name, cases in CASES.items()}
    for size_fn, (offsets_fn, n_offs, ladder) in MATCHERS.items():
        st = out[size_fn] = {}
        for a in ladder:
            n, offs = ctypes.c_size_t(0), [ctypes.c_size_t(0) for _ in range(n_offs)]
            rc = getattr(lib, size_fn)(*a, ctypes.byref(n))
            rc2 = getattr(lib, offsets_fn)(*a, *[ctypes.byref(o) for o in offs])
            assert rc == rc2, a
            st[_key(a)] = [rc, n.value] + [o.value for o in offs]
    lv = out["gsaj_pyramid_level"] = {}
    for a in PYRAMID_LEVELS:
        wl, hl = ctypes.c_int(0), ctypes.c_int(0)
        offs = [ctypes.c_size_t(0) for _ in range(3)]
        rc = lib.gsaj_pyramid_level(*a, ctypes.byref(wl), ctypes.byref(hl), *[ctypes.byref(o) for o in offs])
        lv[_key(a)] = [rc, wl.value, hl.value] + ([o.value for o in offs] if rc == 0 else [0, 0, 0])
    return out


def write_golden():
    from gsaj import _lib
    with open(GOLDEN, "w") as fh:
        json.dump(record(_lib.load()), fh, indent=0, sort_keys=True)
        fh.write("\n")


@pytest.fixture(scope="module")
def lib():
    from gsaj import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _mismatches(got, want):
    bad = []
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in sorted(want):
        assert sorted(got[name]) == sorted(want[name]), "%s: the ladder and the recorded cases differ" % name
        bad += ["%s(%s) = %r, recorded %r" % (name, k, got[name][k], v) for k, v in sorted(want[name].items()) if got[name][k] != v]
    return bad


def test_every_size_and_exported_offset_is_the_recorded_one(lib, golden):
    bad = _mismatches(record(lib), golden)
    assert not bad, "%d value(s) moved:\n  %s" % (len(bad), "\n  ".join(bad[:40]))


def test_every_contract_row_is_on_the_ladder():
    import test_gpu_memory_contracts as mc
    missing = [n for n in mc.CONTRACTS if n not in CASES and n not in MATCHERS]
    assert not missing, missing


def test_the_ladder_is_not_trivial(golden):
    """Legal cases give sizes, illegal ones the recorded 0 / 512 / error code -- the golden file holds both kinds for every function
    that has such a branch."""
    for name in ("gsaj_ssim_workspace_bytes", "gsaj_refine_loss_workspace_bytes", "gsaj_pyramid_bytes", "gsaj_seed_workspace_bytes",
                 "gsaj_grad_mask_workspace_bytes", "gsaj_compact_workspace_bytes", "gsaj_densify_workspace_bytes",
                 "gsaj_eval_workspace_bytes"):
        vals = list(golden[name].values())
        assert 0 in vals and max(vals) > 0, name
    assert golden["gsaj_dist2_workspace_bytes"]["0"] == 512 and golden["gsaj_dist2_workspace_bytes"]["-1"] == 512
    for name in MATCHERS:
        st = list(golden[name].values())
        assert any(v[0] == 0 and v[1] > 0 for v in st) and any(v[0] != 0 for v in st), name
    assert sum(len(v) for v in golden.values()) == sum(len(c) for c in CASES.values()) + len(STEREO) + len(MOTION_STEREO) + len(PYRAMID_LEVELS)


def test_one_altered_number_is_noticed(lib, golden):
    """Canary: any single recorded size moved by 256 bytes fails the comparison, and only that entry is named."""
    got = record(lib)
    for name in sorted(golden):
        k = sorted(golden[name])[len(golden[name]) // 2]
        bent = json.loads(json.dumps(golden))
        if isinstance(bent[name][k], list):
            bent[name][k][1] += 256
        else:
            bent[name][k] += 256
        bad = _mismatches(got, bent)
        assert len(bad) == 1 and bad[0].startswith("%s(%s)" % (name, k)), (name, k, bad)


def _stride(n):
    return (n + 255) // 256 * 256


def test_batched_sizes_are_k_view_strides(lib):
    """Where the ABI says "K consecutive blocks": gsaj_fused_loss_batch_workspace_bytes is K x view_stride(the single form's size);
    gsaj_pose_jac_batch_workspace_bytes is K x the derivative rows alone (the batched forms keep no partial rows), and those rows
    are the single form's size less its partial rows and its 256 bytes of base slack."""
    for k in K + [0]:
        for w, h in WH:
            assert lib.gsaj_fused_loss_batch_workspace_bytes(k, w, h) == k * _stride(lib.gsaj_fused_loss_workspace_bytes(w, h))
            for p in P:
                # (4 * 32: GSAJ_GN_PARTIAL_FLOATS floats a partial row)
                rows = lib.gsaj_pose_jac_workspace_bytes(p, w, h) - 256 - _stride(4 * 32 * lib.gsaj_pose_jac_partial_rows(w, h))
                assert rows > 0 and rows % 256 == 0
                assert lib.gsaj_pose_jac_batch_workspace_bytes(k, p, w, h) == k * rows


def test_every_stride_is_a_multiple_of_256(lib):
    """The per-view strides of the batched launches: the geometry, image and binning blocks are their size functions' values as they
    are (api.hip: carve()), the loss and fused-loss blocks view_stride of theirs (gsaj/losses.py restates that rule)."""
    for p in P:
        assert lib.gsaj_geom_workspace_bytes(p) % 256 == 0
        assert lib.gsaj_pose_jac_batch_workspace_bytes(1, p, 64, 48) % 256 == 0
    for r in R:
        assert lib.gsaj_binning_workspace_bytes(r) % 256 == 0
    for w, h in WH:
        assert lib.gsaj_image_workspace_bytes(w, h) % 256 == 0
        assert lib.gsaj_fused_loss_batch_workspace_bytes(1, w, h) % 256 == 0
