"""GPU: every entry point under the guarded allocator of tests/guards.py -- where the kernels write and which stale bytes they read.

For each operation: one unguarded run whose outputs are kept, then, for both fills (0xFF: NaN / -1 / huge counters; 0x5A: plausible
floats and counters), three runs under the guard on inputs A, B, A -- B differs from A everywhere, and is a smaller problem where
the workspace's contract allows one -- with
  (a) every front and tail band of every workspace and output intact after every run;
  (b) the outputs of the first run bitwise those of the unguarded run (device against device, same inputs: the kernels are
      bit-reproducible, include/gsaj.h);
  (c) no fp32 / int32 output taken from torch.empty still holding the fill -- for byte and int16 outputs (b) under BOTH fills says
      the same, since an unwritten element cannot equal the unguarded value under two different fills;
  (d) the third run bitwise the first: tickets, cursors, select state and flags a call leaves behind.
Workspaces whose contract is "no initialisation needed" are poisoned again before every run; "zeroed once" workspaces are zeroed
when allocated and then only reused, and (d) is their poisoning.

CONTRACTS is the table: one row per size function (gsaj_*_bytes) with the line of include/gsaj.h its contract comes from.  tests/test_cpu_guards.py fails if a size function of gsaj/_lib.py has no row, if a quoted line moved, or if a
named test is missing.

Operations that turned out not to be bit-reproducible between two runs (compared at their own GPU test's tolerance instead):
  none.

Wrapper routes the guard does not see (tests/guards.py): PoseTrackerBatch's torch.stack state and the trackers' cloned ground truth;
the pose-step tests therefore go through the C ABI on guarded states.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import guards
import helpers as hp
from gsaj import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name of the size function -> where include/gsaj.h states the workspace's contract (line, a phrase of that line), the contract
# ("none": no initialisation needed, poisoned before every run; "zeroed once": zeroed when allocated, then only reused), and the
# tests below that run it under guard
CONTRACTS = {
    "gsaj_geom_workspace_bytes": dict(line=65, quote="no initialisation needed", init="none",
                                      tests=["test_rasteriser_forward_backward_export", "test_fused_loss_single_and_batch"]),
    "gsaj_image_workspace_bytes": dict(line=67, quote="zeroed once", init="zeroed once",
                                       tests=["test_rasteriser_forward_backward_export", "test_arena_cap_aborts_inside_the_arena"]),
    "gsaj_binning_workspace_bytes": dict(line=73, quote="no initialisation needed", init="none",
                                         tests=["test_rasteriser_forward_backward_export", "test_chunk_and_merge_sort_path",
                                                "test_arena_cap_aborts_inside_the_arena"]),
    "gsaj_loss_workspace_bytes": dict(line=299, quote="ZEROED ONCE", init="zeroed once", tests=["test_loss_seeds_single_and_batch"]),
    "gsaj_fused_loss_workspace_bytes": dict(line=322, quote="bytes, no", init="none", tests=["test_fused_loss_single_and_batch"]),
    "gsaj_fused_loss_batch_workspace_bytes": dict(line=361, quote="no initialisation needed", init="none",
                                                  tests=["test_fused_loss_single_and_batch"]),
    "gsaj_isotropic_workspace_bytes": dict(line=402, quote="ZEROED ONCE", init="zeroed once", tests=["test_loss_seeds_single_and_batch"]),
    "gsaj_ssim_workspace_bytes": dict(line=410, quote="ZEROED", init="zeroed once", tests=["test_ssim_forward_backward"]),
    "gsaj_refine_loss_workspace_bytes": dict(line=423, quote="zeroed once", init="zeroed once", tests=["test_refine_loss"]),
    "gsaj_pose_jac_workspace_bytes": dict(line=482, quote="no initialisation needed", init="none", tests=["test_gauss_newton_single_view"]),
    "gsaj_pose_jac_batch_workspace_bytes": dict(line=573, quote="no initialisation needed", init="none",
                                                tests=["test_gauss_newton_window_and_select"]),
    "gsaj_pyramid_bytes": dict(line=633, quote="no initialisation needed", init="none", tests=["test_pyramid_build"]),
    "gsaj_stereo_workspace_bytes": dict(line=742, quote="S is zeroed on the stream inside the call", init="none", tests=["test_stereo_match"]),
    "gsaj_dist2_workspace_bytes": dict(line=768, quote="no initialisation needed", init="none", tests=["test_knn", "test_seeding"]),
    "gsaj_seed_workspace_bytes": dict(line=782, quote="no initialisation needed", init="none", tests=["test_seeding"]),
    "gsaj_grad_mask_workspace_bytes": dict(line=841, quote="bytes, no", init="none", tests=["test_grad_mask"]),
    "gsaj_compact_workspace_bytes": dict(line=896, quote="no initialisation needed", init="none", tests=["test_compaction"]),
    "gsaj_densify_workspace_bytes": dict(line=953, quote="no initialisation needed", init="none", tests=["test_densify"]),
    "gsaj_eval_workspace_bytes": dict(line=1036, quote="ZEROED ONCE", init="zeroed once", tests=["test_eval_frame"]),
    "gsaj_dense_workspace_bytes": dict(line=1047, quote="no initialisation needed", init="none", tests=["test_dense_path"]),
    "gsaj_dense_project_workspace_bytes": dict(line=1072, quote="project_ws", init="none", tests=["test_dense_path"]),
    "gsaj_motion_stereo_bytes": dict(line=1289, quote="no initialisation needed (S is zeroed on the stream", init="none", tests=["test_motion_stereo"]),
}


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def _lib():
    from gsaj import _lib as L
    return L.load()


def _ck(rc, what):
    from gsaj import _lib as L
    return L.check(rc, what)


def _stream():
    import torch
    return torch.cuda.current_stream(DEV).cuda_stream


def _t(a, dtype=None):
    """An INPUT on the device: torch.as_tensor is not a guarded route."""
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.as_tensor(a, device=DEV)


def _f(a):
    return _t(a, np.float32)


def E(*shape, dtype=None):
    """An OUTPUT or workspace: torch.empty, so under the guard it is fenced and poisoned."""
    import torch
    return torch.empty(shape, dtype=dtype or torch.float32, device=DEV)


def Z(*shape, dtype=None):
    import torch
    return torch.zeros(shape, dtype=dtype or torch.float32, device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    import torch
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().copy()


def _snap(out):
    return {k: (tuple(v.shape), str(v.dtype), v.element_size(), _bits(v)) for k, v in out.items() if v is not None}


def _assert_same(got, ref, where):
    assert sorted(got) == sorted(ref), (where, sorted(got), sorted(ref))
    for k, (shape, dtype, item, bits) in ref.items():
        g = got[k]
        assert g[0] == shape and g[1] == dtype, "%s: %s is %s %s, the unguarded run's is %s %s" % (where, k, g[1], g[0], dtype, shape)
        if not np.array_equal(g[3], bits):
            bad = np.flatnonzero((g[3] != bits).reshape(-1, item).any(axis=1))
            raise AssertionError("%s: %s (%s %s) differs from the unguarded run in %d of %d elements, flat indices %d .. %d"
                                 % (where, k, dtype, list(shape), bad.size, bits.size // item, bad[0], bad[-1]))


def _assert_written(g, out, where, skip=()):
    """(c): outputs this run took from torch.empty under the guard hold no fill.  4- and 8-byte elements only (module docstring)."""
    for k, v in out.items():
        if v is None or k in skip or v.element_size() < 4 or not v.is_contiguous() or v.numel() == 0:
            continue
        try:
            a = g.allocation_of(v)
        except KeyError:
            continue
        if a.kind == "empty":
            g.assert_fully_written(v, "%s: %s" % (where, k))


def _contract(monkeypatch, op, A, B, tag, skip_written=()):
    """op(inp, st) -> {name: output tensor}.  st persists over the three runs of one guard: op keeps its workspaces in it, lists under
    st["scratch"] (a list or a callable returning one) those whose contract is "none", and may call st["poison"](t) between two
    entry points that share no state."""
    import torch

    ref = _snap(op(A, {"poison": lambda t: None}))
    torch.cuda.synchronize()
    for fill in guards.FILLS:
        with guards.guarded(monkeypatch, fill) as g:
            st = {"poison": g.refill}
            for run, inp in (("A", A), ("B", B), ("A again", A)):
                sc = st.get("scratch", ())
                for t in (sc() if callable(sc) else sc):
                    g.refill(t)
                out = op(inp, st)
                torch.cuda.synchronize()
                where = "%s, fill 0x%02X, run %s" % (tag, fill, run)
                bad = g.damaged()
                assert not bad, "%s: guard bands damaged:\n  %s" % (where, "\n  ".join(bad))   # (a)
                if run != "B":
                    _assert_same(_snap(out), ref, where)                                         # (b), (d)
                    _assert_written(g, out, where, skip_written)                                 # (c)
            assert g.allocations, "%s: nothing was allocated under the guard" % tag


def _rng(*seed):
    return np.random.default_rng(list(seed))


# ---- k-NN ---------------------------------------------------------------------------------------------------------------------------
def _op_knn(pts, st):
    import torch
    L, P = _lib(), pts.shape[0]
    if "ws" not in st:
        st["ws"] = E(L.gsaj_dist2_workspace_bytes(P), dtype=torch.uint8)   # sized for A; B is smaller
        st["scratch"] = [st["ws"]]
    out, codes, idx = E(P), E(P, dtype=torch.int32), E(P, dtype=torch.int32)
    _ck(L.gsaj_dist2(P, _p(pts), _p(out), _p(st["ws"]), _stream()), "gsaj_dist2")
    _ck(L.gsaj_debug_dist2_order(P, _p(st["ws"]), _p(codes), _p(idx), _stream()), "gsaj_debug_dist2_order")
    return dict(mean_dists=out, codes=codes, idx=idx)


@pytest.mark.parametrize("P", [1, 4, 257, 2049])
def test_knn(monkeypatch, P):
    """The last 256-point box and the last 2048-key radix tile hold one point; the ticket k_knn_bbox resets for its successor."""
    A = _f(_rng(P).uniform(-2, 3, (P, 3)))
    B = _f(_rng(P, 1).uniform(-1, 1, (max(1, P // 2), 3)))
    _contract(monkeypatch, _op_knn, A, B, "k-NN P=%d" % P)


# ---- SSIM, refine loss, eval -------------------------------------------------------------------------------------------------------
def _op_ssim(inp, st):
    import torch
    img, gt, up = inp
    L = _lib()
    N, C, H, W = img.shape
    if "ws" not in st:
        st["ws"] = Z(L.gsaj_ssim_workspace_bytes(N, C, W, H), dtype=torch.uint8)   # zeroed once
    out, smap, dimg = E(N + 1), E(N, C, H, W), E(N, C, H, W)
    _ck(L.gsaj_ssim_forward(N, C, W, H, _p(img), _p(gt), _p(out), _p(smap), _p(st["ws"]), _stream()), "gsaj_ssim_forward")
    _ck(L.gsaj_ssim_backward(N, C, W, H, _p(img), _p(gt), _p(up), _p(dimg), _p(st["ws"]), _stream()), "gsaj_ssim_backward")
    return dict(ssim_out=out, ssim_map=smap, dL_dimg=dimg)


@pytest.mark.parametrize("N,C,H,W", [(1, 3, 5, 7), (1, 1, 40, 36), (2, 3, 24, 32)])
def test_ssim_forward_backward(monkeypatch, N, C, H, W):
    """A window wider than the image, one plane, a batch.  B has A's shape: the workspace is zeroed once for one shape."""
    def pair(s):
        r = _rng(N, C, H, W, s)
        return _f(r.uniform(0, 1, (N, C, H, W))), _f(r.uniform(0, 1, (N, C, H, W))), _f(r.normal(size=N + 1))
    _contract(monkeypatch, _op_ssim, pair(0), pair(1), "ssim %dx%dx%dx%d" % (N, C, H, W))


def _op_refine(inp, st):
    import torch
    img, gt = inp
    L = _lib()
    _, H, W = img.shape
    if "ws" not in st:
        st["ws"] = Z(L.gsaj_refine_loss_workspace_bytes(W, H), dtype=torch.uint8)
    d, s = E(3, H, W), E(3)
    _ck(L.gsaj_refine_loss_seeds(W, H, 0.2, _p(img), _p(gt), _p(d), _p(s), _p(st["ws"]), _stream()), "gsaj_refine_loss_seeds")
    return dict(dL_dcolor=d, scalars=s)


@pytest.mark.parametrize("H,W", [(5, 7), (40, 36), (24, 32)])
def test_refine_loss(monkeypatch, H, W):
    def pair(s):
        r = _rng(H, W, s)
        return _f(r.uniform(0, 1, (3, H, W))), _f(r.uniform(0, 1, (3, H, W)))
    _contract(monkeypatch, _op_refine, pair(0), pair(1), "refine loss %dx%d" % (W, H))


def _op_eval(inp, st):
    import torch
    img, gt = inp
    L = _lib()
    C, H, W = img.shape
    if "ws" not in st:
        st["ws"] = Z(L.gsaj_eval_workspace_bytes(C, W, H), dtype=torch.uint8)
    row, cnt, u8 = E(4), E(1, dtype=torch.int32), E(H, W, C, dtype=torch.uint8)
    _ck(L.gsaj_eval_frame(C, W, H, 1 if C == 3 else 0, _p(img), _p(gt), _p(row), _p(cnt), _p(u8), _p(st["ws"]), _stream()), "gsaj_eval_frame")
    off = (-st["ws"].data_ptr()) % 256
    x = st["ws"][off:off + 4 * C * H * W].view(torch.float32)   # the clamped image the header says stays readable
    return dict(row=row, count=cnt, image_u8=u8, clamped=x)


@pytest.mark.parametrize("C,H,W", [(3, 5, 7), (1, 17, 15)])
def test_eval_frame(monkeypatch, C, H, W):
    """"Nothing but out_row, out_count, image_u8 and eval_ws is written" (include/gsaj.h): the bands of all four."""
    def pair(s):
        r = _rng(C, H, W, s)
        return _f(r.uniform(-0.2, 1.2, (C, H, W))), _f(np.where(r.uniform(size=(C, H, W)) < 0.2, 0.0, r.uniform(0, 1, (C, H, W))))
    _contract(monkeypatch, _op_eval, pair(0), pair(1), "eval %dx%dx%d" % (C, H, W))


# ---- gradient mask ----------------------------------------------------------------------------------------------------------------
def _op_grad_mask(inp, st):
    import torch
    img, blocks = inp
    L = _lib()
    _, H, W = img.shape
    if "ws" not in st:
        st["ws"] = E(L.gsaj_grad_mask_workspace_bytes(W, H), dtype=torch.uint8)
        st["scratch"] = [st["ws"]]
    inten, u8, f32 = E(H, W), E(H, W, dtype=torch.uint8), E(H, W)
    _ck(L.gsaj_grad_intensity(W, H, _p(img), _p(inten), _stream()), "gsaj_grad_intensity")
    _ck(L.gsaj_grad_mask(W, H, _p(img), 1.1, blocks, _p(u8), _p(f32), _p(st["ws"]), _stream()), "gsaj_grad_mask")
    return dict(intensity=inten, mask_u8=u8, mask_f32=f32)


@pytest.mark.parametrize("blocks", [0, 1], ids=["frame", "blocks"])
@pytest.mark.parametrize("H,W", [(68, 100), (97, 131)])
def test_grad_mask(monkeypatch, H, W, blocks):
    """Remainders of the 64 x 16 tiles; in block mode the strips the 32 x 32 grid leaves over (they keep the intensity)."""
    img = lambda h, w, s: _f(_rng(h, w, s).uniform(0, 1, (3, h, w)))  # noqa: E731
    _contract(monkeypatch, _op_grad_mask, (img(H, W, 0), blocks), (img(64, 96, 1), blocks), "grad mask %dx%d blocks=%d" % (W, H, blocks))


# ---- image pyramid -----------------------------------------------------------------------------------------------------------------
def _op_pyramid(inp, st):
    import torch
    from gsaj.pyramid import ImagePyramid
    color, depth, mask = inp
    _, H, W = color.shape
    if "pyr" not in st:
        st["pyr"] = ImagePyramid(W, H, 3, DEV, has_depth=depth is not None, has_mask=mask is not None)
        st["scratch"] = [st["pyr"].buf]
    pyr = st["pyr"]
    pyr.build(color, depth, mask)
    out, planes = {}, torch.zeros(pyr.buf.numel(), dtype=torch.bool)
    for l in range(1, 4):
        wl, hl, co, do, mo = pyr._lv[l]
        out["color%d" % l] = pyr.color(l)
        planes[co:co + 12 * wl * hl] = True
        if depth is not None:
            out["depth%d" % l] = pyr.depth(l)
            planes[do:do + 4 * wl * hl] = True
        if mask is not None:
            out["mask%d" % l] = pyr.mask(l)
            planes[mo:mo + wl * hl] = True
    st["between"] = pyr.buf.cpu()[~planes]   # "the bytes between planes are never written"
    return out


@pytest.mark.parametrize("planes", ["color", "color+depth+mask"])
def test_pyramid_build(monkeypatch, planes):
    """97 x 61, three levels: odd sizes at every level (48 x 30, 24 x 15, 12 x 7).  The bytes between the planes keep the fill."""
    W, H = 97, 61

    def frame(s):
        r = _rng(s)
        d = np.where(r.uniform(size=(H, W)) < 0.15, 0.0, r.uniform(0.5, 4.0, (H, W)))
        m = (r.uniform(size=(H, W)) < 0.3).astype(np.uint8) * r.integers(1, 256, (H, W)).astype(np.uint8)
        full = planes != "color"
        return _f(r.uniform(0, 1, (3, H, W))), (_f(d) if full else None), (_t(m, np.uint8) if full else None)

    seen = []

    def op(inp, st):
        out = _op_pyramid(inp, st)
        seen.append(st["between"])
        return out

    _contract(monkeypatch, op, frame(0), frame(1), "pyramid " + planes)
    for k, fill in enumerate(guards.FILLS):   # runs 0 is the unguarded one, then three per fill
        for b in seen[1 + 3 * k:4 + 3 * k]:
            assert b.numel() > 0 and bool((b == fill).all()), "pyramid %s: %d byte(s) between the planes were written" % (planes, int((b != fill).sum()))


def _op_relevel(inp, st):
    init, proj = inp
    out = {}
    for n in (_lib().gsaj_gn_state_floats(), _lib().gsaj_gn8_state_floats()):
        s = E(n)   # exactly the state's floats: the joint form's two extra slots must not be written in the 6-form
        s.copy_(init[:n])
        _ck(_lib().gsaj_pose_gn_relevel(_p(s), n, _p(proj), 1e-3, None, _stream()), "gsaj_pose_gn_relevel")
        out["state%d" % n] = s
    return out


def test_pyramid_relevel(monkeypatch):
    """gsaj_pose_gn_relevel on states of exactly GSAJ_GN_STATE_FLOATS / GSAJ_GN8_STATE_FLOATS floats, one with an accepted pose and one
    without."""
    cams = syn.keyframe_cameras(2, radius=0.25, W=97, H=61, fx=85.0, fy=85.0, cx=48.0, cy=30.0)

    def case(k, accepted):
        r = _rng(k)
        s = r.normal(size=152)
        s[0:16] = np.ascontiguousarray(cams[k]["viewmatrix"].T).reshape(-1)
        s[88:104] = np.ascontiguousarray(cams[1 - k]["viewmatrix"].T).reshape(-1)
        s[82] = accepted
        return _f(s), _f(cams[k]["projmatrix_raw"])

    _contract(monkeypatch, _op_relevel, case(0, 1.0), case(1, 0.0), "relevel")


# ---- ingest, rectify ---------------------------------------------------------------------------------------------------------------
def _op_ingest(inp, st):
    import torch
    src, depth, maps, W, H, C = inp
    L = _lib()
    Hs, stride = src.shape
    Ws = (stride - 8) // C   # rows are padded by 8 bytes
    color, dep = E(3, H, W), E(H, W)
    mx, my = (None, None) if maps is None else maps
    _ck(L.gsaj_frame_ingest(W, H, Ws, Hs, C, stride, _p(src), _p(mx), _p(my), _p(depth), depth.shape[1], 5000.0, 0, _p(color), _p(dep),
                            _stream()), "gsaj_frame_ingest")
    out = dict(color=color, depth=dep)
    if C == 1:
        rect, rc = E(H, W + 5, dtype=torch.uint8), E(3, H, W)   # padded output rows: the pad must keep the fill
        _ck(L.gsaj_rectify_u8(W, H, Ws, Hs, stride, _p(src), _p(mx), _p(my), _p(rect), W + 5, _p(rc), _stream()), "gsaj_rectify_u8")
        out.update(rect=rect[:, :W].contiguous(), rect_color=rc)
        st["pad"] = rect[:, W:].cpu()
    return out


@pytest.mark.parametrize("remap", [False, True], ids=["direct", "remap"])
@pytest.mark.parametrize("W,H,C", [(37, 11, 3), (40, 9, 3), (40, 9, 1), (37, 11, 1), (36, 7, 4)])
def test_ingest_and_rectify(monkeypatch, W, H, C, remap):
    """W % 4 != 0 (one thread per pixel) and W % 4 == 0 (four pixels per thread, 16-byte stores) with padded source and depth rows:
    the last store of a row, and of the image, at the exact end of out_color and out_depth."""
    Ws, Hs = (W + 6, H + 3) if remap else (W, H)

    def frame(s):
        r = _rng(W, H, C, s)
        src = r.integers(0, 256, (Hs, Ws * C + 8), dtype=np.uint8)
        depth = r.integers(0, 65536, (H, W + 4), dtype=np.uint16).view(np.uint8)   # rows padded by 8 bytes
        maps = None
        if remap:
            u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
            mx, my = u * (Ws / W) + r.uniform(-2, 2, (H, W)), v * (Hs / H) + r.uniform(-2, 2, (H, W))
            mx[0, 0], my[-1, -1] = np.nan, np.inf
            maps = (_f(mx), _f(my))
        return _t(src), _t(depth), maps, W, H, C

    pads = []

    def op(inp, st):
        out = _op_ingest(inp, st)
        pads.append(st.get("pad"))
        return out

    _contract(monkeypatch, op, frame(0), frame(1), "ingest %dx%dx%d remap=%d" % (W, H, C, remap))
    if C == 1:
        for k, fill in enumerate(guards.FILLS):
            for pad in pads[1 + 3 * k:4 + 3 * k]:
                assert bool((pad == fill).all()), "gsaj_rectify_u8 wrote into the padding of its output rows"


# ---- stereo ------------------------------------------------------------------------------------------------------------------------
def _op_stereo(inp, st):
    from gsaj.stereo import StereoMatcher
    left, right, paths = inp
    H, W = left.shape
    if "m" not in st:
        st["m"] = StereoMatcher(W, H, DEV, num_disparities=16, block_radius=2, paths=paths)
        st["scratch"] = [st["m"].workspace]
    m = st["m"]
    disp = E(H, W, dtype=__import__("torch").int16)
    depth = E(H, W)
    m(left, right, bf=47.9, out_disp16=disp, out_depth=depth)
    # (only columns x >= D of the cost volume carry a result: tests/test_gpu_stereo.py)
    return dict(disp16=disp, depth=depth, cost=m.cost_volume()[:, 16:].contiguous(), sums=m.sums())


@pytest.mark.parametrize("paths", [4, 8])
def test_stereo_match(monkeypatch, paths):
    """96 x 40, D = 16: the cost volume and S end at the workspace's exact end; S is summed into and must start from the call's own
    zeroes, not from the fill."""
    from test_gpu_stereo import _pair

    la, ra = _pair(96, 40, 16, seed=5)
    lb, rb = _pair(96, 40, 16, seed=6)
    _contract(monkeypatch, _op_stereo, (_t(la), _t(ra), paths), (_t(lb[::-1].copy()), _t(rb[::-1].copy()), paths), "stereo paths=%d" % paths)


# ---- motion stereo -------------------------------------------------------------------------------------------------------------------
def _op_sweep(inp, st):
    import torch
    from gsaj import MotionStereo

    c, D, paths = inp
    cam = c["cam"]
    H, W = c["ref"].shape
    key = ("m", W, H, D)
    if key not in st:
        st[key] = MotionStereo(W, H, DEV, cam["fx"], cam["fy"], cam["cx"], cam["cy"], num_hypotheses=D, block_radius=2, paths=paths)
        st.setdefault("all", []).append(st[key].workspace)
        st["scratch"] = lambda: st["all"]
    m = st[key]
    idx16 = E(H, W, dtype=torch.int16)
    depth = E(H, W)
    m(c["dev"][0], c["dev"][1], c["dev"][2], c["dev"][3], 0.2, 0.7, out_idx16=idx16, out_depth=depth)
    return dict(idx16=idx16, depth=depth, grad=m.gradient_bytes(), pc=m.pixel_costs(), cost=m.cost_volume(), sums=m.sums())


def _sweep_inputs(W, H, motion):
    import sweep_restated as sw

    c = dict(sw.case(W, H, motion))
    c["dev"] = [_t(c[k]) for k in ("ref", "src", "ref_w2c", "src_w2c")]   # inputs: not a guarded route
    return c


@pytest.mark.parametrize("paths", [4, 8])
def test_motion_stereo(monkeypatch, paths):
    """A: 96 x 40, D = 32; B: 65 x 33, D = 16 -- a smaller image with fewer hypotheses on an object of its own: the sizes of a
    MotionStereo are fixed when it is made.  pc, C and S end at the workspace's exact end; S is summed into and must start from the
    call's own zeroes, not from the fill."""
    A, B = _sweep_inputs(96, 40, "forward"), _sweep_inputs(65, 33, "mixed")
    _contract(monkeypatch, _op_sweep, (A, 32, paths), (B, 16, paths), "motion stereo paths=%d" % paths)


# ---- seeding and depth statistics ---------------------------------------------------------------------------------------------------
def _op_seed(inp, st):
    import torch
    depth, opacity, mask, gt, noise, w2c, ab = inp
    L = _lib()
    H, W = depth.shape
    if "ws" not in st:
        st["ws"] = E(L.gsaj_seed_workspace_bytes(W, H), dtype=torch.uint8)   # sized for A; B is smaller
        st["scratch"] = [st["ws"]]
    ws, s = st["ws"], _stream()
    out = {}
    stats, valid = E(4), E(H, W, dtype=torch.uint8)
    _ck(L.gsaj_depth_stats(W, H, _p(depth), _p(opacity), 0.9, _p(mask), _p(gt), 0.3, _p(stats), _p(valid), _p(ws), s), "gsaj_depth_stats")
    out.update(stats=stats, valid=valid)
    st["poison"](ws)
    stats2 = E(4)
    _ck(L.gsaj_depth_stats(W, H, _p(depth), None, 0.0, None, None, 0.0, _p(stats2), None, _p(ws), s), "gsaj_depth_stats")
    out.update(stats_plain=stats2)
    st["poison"](ws)
    prior, pstats = E(H, W), E(4)
    _ck(L.gsaj_keyframe_depth_prior(W, H, _p(depth), _p(opacity), _p(gt), 0.3, _p(noise), _p(prior), _p(pstats), _p(ws), s),
        "gsaj_keyframe_depth_prior")
    out.update(prior=prior, prior_stats=pstats)
    st["poison"](ws)
    _ck(L.gsaj_seed_select(W, H, _p(depth), _p(gt), 0.3, 5.0, 3.0, 7, _p(ws), s), "gsaj_seed_select")
    nv, m = ctypes.c_int(0), ctypes.c_int(0)
    _ck(L.gsaj_seed_count(_p(ws), s, ctypes.byref(nv), ctypes.byref(m)), "gsaj_seed_count")
    m = m.value
    assert 3 < m < nv.value
    for iso in (0, 1):   # two initialisations follow one selection: the state it left is read, not consumed
        xyz, fdc, frest, sc, rot, op = E(m, 3), E(m, 3), E(m, 9), E(m, 1 if iso else 3), E(m, 4), E(m)
        knn = E(L.gsaj_dist2_workspace_bytes(m), dtype=torch.uint8)
        _ck(L.gsaj_seed_gaussians(m, W, H, _p(depth), _p(gt), _p(ab), _p(w2c), 0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5, 0.01, 1 - iso, 4, iso,
                                  _p(xyz), _p(fdc), _p(frest), _p(sc), _p(rot), _p(op), _p(ws), _p(knn), s), "gsaj_seed_gaussians")
        out.update({"xyz%d" % iso: xyz, "f_dc%d" % iso: fdc, "f_rest%d" % iso: frest, "scaling%d" % iso: sc, "rotation%d" % iso: rot,
                    "opacity%d" % iso: op})
    px = E(m, dtype=torch.int32)
    _ck(L.gsaj_debug_seed_pixels(W, H, m, _p(ws), _p(px), s), "gsaj_debug_seed_pixels")
    out.update(pixels=px, counts=_t(np.array([nv.value, m], np.int32)))
    return out


@pytest.mark.parametrize("golden", ["median_depth_mask_odd", "median_depth_plain_even", "median_depth_both_even"])
def test_seeding(monkeypatch, golden):
    """The depth images of the median_depth goldens (17 x 23: an odd pixel count; 24 x 32 and 48 x 64: even), then a smaller frame in
    the same workspace, then the first again: the radix-select state and the selection's counters."""
    def frame(depth, s):
        H, W = depth.shape
        r = _rng(H, W, s)
        w2c = np.eye(4)
        w2c[:3, 3] = (0.1, -0.2, 0.3)
        return (_f(depth), _f(r.uniform(0.8, 1.0, (H, W))), _t((r.uniform(size=(H, W)) < 0.7).astype(np.uint8) * 255), _f(r.uniform(0, 1, (3, H, W))),
                _f(r.normal(size=(H, W))), _f(w2c.reshape(-1)), _f([0.05, -0.02]))

    d = np.load(os.path.join(GOLDEN, golden + ".npz"))["depth"][0]
    r = _rng(7)
    small = np.where(r.uniform(size=(13, 19)) < 0.2, 0.0, r.uniform(0.2, 6.0, (13, 19)))
    _contract(monkeypatch, _op_seed, frame(d, 0), frame(small, 1), "seeding " + golden)


# ---- compaction, densification -------------------------------------------------------------------------------------------------------
def _op_compact(inp, st):
    import torch
    mask, remove, tensors = inp
    L, P = _lib(), mask.shape[0]
    if "ws" not in st:
        st["ws"] = E(L.gsaj_compact_workspace_bytes(P), dtype=torch.uint8)   # sized for A; B is smaller
        st["scratch"] = [st["ws"]]
    ws = st["ws"]
    _ck(L.gsaj_compact_plan(P, _p(mask), remove, _p(ws), _stream()), "gsaj_compact_plan")
    n = ctypes.c_int(-1)
    _ck(L.gsaj_compact_count(_p(ws), _stream(), ctypes.byref(n)), "gsaj_compact_count")
    n = n.value
    outs = [E(n, *t.shape[1:], dtype=t.dtype) for t in tensors]   # exactly n_kept rows
    if n > 0:
        k = len(tensors)
        src, dst = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors]), (ctypes.c_void_p * k)(*[t.data_ptr() for t in outs])
        rb = (ctypes.c_int * k)(*[(t.numel() // P) * t.element_size() for t in tensors])
        for _ in range(2):   # several moves may follow one plan
            _ck(L.gsaj_compact_rows(P, k, src, dst, rb, _p(ws), _stream()), "gsaj_compact_rows")
    out = {"t%d" % i: o for i, o in enumerate(outs)}
    out["n_kept"] = _t(np.array([n], np.int32))
    return out


@pytest.mark.parametrize("P,kind", [(1, "all"), (120, "random"), (300, "random"), (300, "all"), (257, "none"), (513, "edges")])
def test_compaction(monkeypatch, P, kind):
    """Destinations of exactly n_kept rows (4, 12, 180 and 4096 bytes wide); P = 1; every row kept; no row kept; kept rows at the
    edges of the 256-row blocks."""
    import torch

    def case(P, kind, s):
        r = _rng(P, s)
        rows = np.arange(P)
        keep = {"all": np.ones(P, bool), "none": np.zeros(P, bool), "random": r.uniform(size=P) < 0.6,
                "edges": (rows % 256 == 0) | (rows % 256 == 255) | (rows == P - 1)}[kind]
        remove = int(s % 2)
        mask = (keep != bool(remove)).astype(np.uint8) * r.integers(1, 256, P).astype(np.uint8)
        tensors = [torch.arange(P * w, dtype=torch.int32, device=DEV).view(P, w) * 41 + s for w in (1, 3, 45, 1024)]
        return _t(mask), remove, tensors

    _contract(monkeypatch, _op_compact, case(P, kind, 0), case(max(1, P // 2), "random" if P > 1 else "all", 1), "compact P=%d %s" % (P, kind))


def _op_densify(inp, st):
    import torch
    from gsaj.densify import DensifyPlan
    from test_gpu_densify_prune import EXTENT, MAX_GRAD, MIN_OPACITY
    d, N, xyz, rot = inp
    P = d["scaling"].shape[0]
    plan = DensifyPlan(_f(d["accum"]), _f(d["denom"]), _f(d["scaling"]), _f(d["opacity"]), MAX_GRAD, MIN_OPACITY, EXTENT, d["max_screen_size"], N=N)
    sc = _f(d["scaling"])
    tensors = [xyz, sc, torch.arange(P * 45, dtype=torch.int32, device=DEV).view(P, 45), torch.arange(P, dtype=torch.int32, device=DEV)]
    dx, ds, wide, rows = plan.apply(tensors, ["parent", "parent", "zeros", "parent"])   # outputs of exactly P'' rows
    plan.children(xyz, sc, rot, dx, ds, seed=1234)
    noise = E(N, P, 3)
    _ck(_lib().gsaj_densify_noise(P, N, 1234, _p(noise), _stream()), "gsaj_densify_noise")
    return dict(code=plan.code, xyz=dx, scaling=ds, wide=wide, rows=rows, noise=noise, counts=_t(np.array(plan.counts, np.int32)))


@pytest.mark.parametrize("P,S,N,pat", [(1, 3, 2, "all_split"), (150, 3, 2, "random"), (300, 1, 4, "random"), (300, 3, 2, "all_pruned"),
                                       (513, 3, 3, "block_edges")])
def test_densify(monkeypatch, P, S, N, pat):
    """gsaj.densify.DensifyPlan: the plan's workspace and code, destinations of exactly P'' rows, the children written into them.  The
    wrapper makes a workspace per plan, so the third run checks determinism, not reuse."""
    from test_gpu_densify_prune import make_inputs

    def case(P, pat, s):
        r = _rng(P, s)
        return make_inputs(P, S, N, pat, s), N, _f(r.normal(size=(P, 3))), _f(r.normal(size=(P, 4)))

    _contract(monkeypatch, _op_densify, case(P, pat, 3), case(max(1, P - 37), "random", 4), "densify P=%d S=%d N=%d %s" % (P, S, N, pat))


# ---- map step ----------------------------------------------------------------------------------------------------------------------
def _op_map_step(inp, st):
    from gsaj import map_step as ms
    P, M, S, init, grads, radii = inp
    widths = (3, 3, 3 * (M - 1), 1, S, 4)
    buf = E(init.numel())          # ONE allocation: 18 field views packed tight, so an overrun of one lands in its neighbour or a band
    buf.copy_(init)
    views, off = [], 0
    for _ in range(3):
        group = []
        for w in widths:
            group.append(buf[off:off + P * w])
            off += P * w
        views.append(group)
    assert off == buf.numel()
    ss, bc = zip(*[ms.adam_scalars(lr, 0.9, 0.999, 1.0) for lr in (1e-3, 2e-3, 1e-4, 5e-2, 1e-3, 1e-3)])
    ms.launch(P, M, S, views[0], views[1], views[2], grads, ss, bc, [False] * 6, 0.9, 0.999, 1e-15)
    ms.launch(P, M, S, views[0], views[1], views[2], grads, ss, bc, [False] * 6, 0.9, 0.999, 1e-15, flags=ms.RESET_NONVISIBLE, radii=radii,
              reset=ms.reset_value(0.4))
    return dict(state=buf)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("P", [7, 301])
def test_map_step(monkeypatch, P, M, S):
    """P odd: the field views start at addresses that are 4-byte aligned only, so the 16-byte path must fall back; every parameter and
    moment sits tight against the next.  A step, then a step with the non-visible opacity reset."""
    def case(s):
        r = _rng(P, M, S, s)
        n = P * (3 + 3 + 3 * (M - 1) + 1 + S + 4)
        init = np.concatenate([r.normal(size=n), r.normal(size=n) * 0.01, r.uniform(0, 1e-4, n)])
        grads = [_f(r.normal(size=(P, 3))), _f(r.normal(size=(P, M, 3))), _f(r.normal(size=P)), _f(r.normal(size=(P, 3))), _f(r.normal(size=(P, 4)))]
        return P, M, S, _f(init), grads, _t(r.integers(-1, 3, (2, P)), np.int32)

    _contract(monkeypatch, _op_map_step, case(0), case(1), "map step P=%d M=%d S=%d" % (P, M, S))


# ---- covisibility ------------------------------------------------------------------------------------------------------------------
def _op_covis(inp, st):
    from gsaj.covisibility import CovisibilityWindow
    nt, cur, ids = inp
    K, P = nt.shape
    if "cw" not in st:
        st["cw"] = CovisibilityWindow(P, DEV)
    cw = st["cw"]
    for t in (cw.words, cw.out, cw.n_pruned, cw.to_prune, cw.n_obs):   # the header: rebuilt / overwritten / zeroed inside the call
        st["poison"](t)
    window = list(range(10, 10 + K))
    cw.set_window(window, nt)
    q = cw.query(cur_n_touched=cur).clone()
    q2 = cw.query(kf_id=window[1]).clone()
    to_prune, n_pruned = cw.prune_mask(window, ids, "slam", True)
    return dict(words=cw.words, query=q, query_kf=q2, to_prune=to_prune, n_pruned=n_pruned, n_obs=cw.n_obs)


def test_covisibility(monkeypatch):
    """P = 200: `out` and `n_pruned` are zeroed inside the calls and the words rebuilt without being read, so all of them start as fill."""
    def case(s):
        r = _rng(s)
        return _t(r.integers(0, 3, (5, 200)), np.int32), _t(r.integers(0, 2, 200), np.int32), _t(r.integers(8, 16, 200), np.int32)
    _contract(monkeypatch, _op_covis, case(0), case(1), "covisibility")


# ---- dense analytic path -------------------------------------------------------------------------------------------------------------
def _op_dense(inp, st):
    from gsaj import dense
    g, cam, gt_c, gt_d, mask = inp
    r = dense.jacobian_test(g["means3D"], g["cov3D6"], g["opacities"], g["shs"], cam, gt_c, gt_d, mask, 3)
    pr = r["projected"]
    return dict(grad_mu=r["grad_mu_I_pixel"], grad_Sigma=r["grad_Sigma_I_pixel"], grad_depth=r["grad_depth_per_gaussian"],
                grad_color=r["grad_color_per_gaussian"], dL_dtau=r["dL_dtau"], order=r["order"], **{"tau_" + k: v for k, v in r["dL_dtau_parts"].items()},
                color=r["rendered_color"], depth=r["rendered_depth"], mean_2D=pr["mean_2D"], cov_2D=pr["cov_2D"], pcolor=pr["color"],
                color_raw=pr["color_raw"], pdepth=pr["depth"])


@pytest.mark.parametrize("name", ["dense_N1_64x48", "dense_N15_64x48"])
def test_dense_path(monkeypatch, name):
    """gsaj_dense_project / _render / _backward / gsaj_pose_jacobians / gsaj_dense_tau on the goldens' Gaussians: the per-block partials
    of the dense backward, N = 1.  The wrapper makes its workspaces per call (third run: determinism)."""
    def case(name, s):
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        W, H = int(g["W"]), int(g["H"])
        cam = syn.make_camera(g["w2c"], W=W, H=H, fx=float(g["fx"]), fy=float(g["fy"]), cx=float(g["cx"]), cy=float(g["cy"]))
        r = _rng(s)
        return g, cam, r.uniform(0, 1, (H, W, 3)).astype(np.float32), r.uniform(0.3, 3.0, (H, W)).astype(np.float32), r.uniform(size=(H, W)) < 0.8

    _contract(monkeypatch, _op_dense, case(name, 0), case("dense_N15_64x48" if name.endswith("N1_64x48") else "dense_N1_64x48", 1), name)


# ---- pose step -----------------------------------------------------------------------------------------------------------------------
def _op_pose_step(inp, st):
    init, tau, dexp, active, proj = inp
    L, K = _lib(), init.shape[0]
    states = E(K, 80)
    states.copy_(init)
    single = E(80)
    single.copy_(init[0])
    lr = (0.003, 0.001, 0.01, 0.01, 0.9, 0.999, 1e-8, 1e-4)
    for it in range(3):
        _ck(L.gsaj_pose_adam_step_batch(K, _p(tau[it]), _p(dexp[it]), _p(active), *lr, _p(proj), _p(states), None, 0, _stream()),
            "gsaj_pose_adam_step_batch")
        _ck(L.gsaj_pose_adam_step(_p(tau[it][0]), _p(dexp[it][0]), *lr, _p(proj), _p(single), None, _stream()), "gsaj_pose_adam_step")
    return dict(states=states, single=single)


def test_pose_step(monkeypatch):
    """K = 5 with an active mask: the masked states stay bit for bit, the stepped ones equal the single-pose call's, and nothing
    outside the [K, 80] states is written."""
    import torch
    from gsaj.pose_step import PoseTracker

    cams = syn.keyframe_cameras(5, radius=0.25, W=97, H=61, fx=85.0, fy=85.0, cx=48.0, cy=30.0)

    def case(s):
        r = _rng(s)
        init = torch.stack([PoseTracker(np.ascontiguousarray(c["viewmatrix"].T), c["projmatrix_raw"], DEV).state for c in cams])
        return (init, _f(r.normal(size=(3, 5, 6)) * 0.1), _f(r.normal(size=(3, 5, 2)) * 0.1), _t(np.array([1, 0, 255, 1, 0], np.uint8)),
                _f(cams[0]["projmatrix_raw"]))

    A = case(0)
    seen = {}

    def op(inp, st):
        out = _op_pose_step(inp, st)
        if inp is A:
            seen["states"], seen["single"] = out["states"].clone(), out["single"].clone()
        return out

    _contract(monkeypatch, op, A, case(1), "pose step")
    assert torch.equal(seen["states"][[1, 4]], A[0][[1, 4]]), "a masked pose state was touched"
    assert torch.equal(seen["states"][0], seen["single"]) and not torch.equal(seen["states"][0], A[0][0])


# ---- the rasteriser through the C ABI -------------------------------------------------------------------------------------------------
def _scene_inputs(name=None, cam=None, sc=None, deg=3, mod=1.0, seed=0):
    if name is not None:
        cam, sc, deg = hp.make(name)
        mod = hp.scale_modifier(name)
    dLc, dLd = hp.seeds(cam, seed)
    d = {k: _f(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    d.update({k: _f(cam[k]) for k in ("viewmatrix", "projmatrix", "projmatrix_raw", "campos")})
    d.update(bg=_f(hp.PARITY_BG), dLc=_f(dLc), dLd=_f(dLd), W=cam["W"], H=cam["H"], tan=(float(cam["tanfovx"]), float(cam["tanfovy"])),
             deg=deg, mod=float(mod), P=sc["means3D"].shape[0], M=sc["shs"].shape[1])
    return d


def _op_raster(inp, st):
    """gsaj_forward_preprocess / _num_rendered / _render, gsaj_debug_export, gsaj_rasterize_backward with EVERY output from torch.empty
    (the wrappers' torch.zeros outputs would hide an unwritten row) and a binning workspace of exactly gsaj_binning_workspace_bytes(R)."""
    import torch
    d, flags, chunked = inp
    L, s = _lib(), _stream()
    P, M, W, H, deg = d["P"], d["M"], d["W"], d["H"], d["deg"]
    if "geom" not in st:
        st["geom"] = E(L.gsaj_geom_workspace_bytes(P), dtype=torch.uint8)          # sized for A; B has fewer Gaussians
        st["img"] = Z(L.gsaj_image_workspace_bytes(W, H), dtype=torch.uint8)        # zeroed once
        st["scratch"] = [st["geom"]]
    geom, img = st["geom"], st["img"]
    color, depth, opac = E(3, H, W), E(1, H, W), E(1, H, W)
    radii, touched = E(P, dtype=torch.int32), E(P, dtype=torch.int32)
    scene_f = (_p(d["means3D"]), _p(d["shs"]), None, _p(d["opacities"]), _p(d["scales"]), d["mod"], _p(d["rotations"]), None)
    _ck(L.gsaj_forward_preprocess(P, deg, M, W, H, *scene_f, _p(d["viewmatrix"]), _p(d["projmatrix"]), _p(d["campos"]), *d["tan"], 0,
                                  _p(radii), _p(touched), _p(geom), _p(img), s), "gsaj_forward_preprocess")
    R, mt = ctypes.c_int(0), ctypes.c_int(0)
    _ck(L.gsaj_forward_num_rendered(W, H, _p(img), s, ctypes.byref(R), ctypes.byref(mt)), "gsaj_forward_num_rendered")
    R = R.value
    nbytes = L.gsaj_binning_workspace_bytes(R)
    binning = E(nbytes, dtype=torch.uint8)
    _ck(L.gsaj_forward_render(P, R, -1 if chunked else mt.value, W, H, _p(d["bg"]), None, _p(radii), _p(geom), _p(binning), nbytes, _p(img),
                              _p(color), _p(depth), _p(opac), _p(touched), flags, s), "gsaj_forward_render")
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    i32, u8 = torch.int32, torch.uint8
    ex = dict(means2D=E(P, 2), depths=E(P), cov3D=E(P, 6), conic_opacity=E(P, 4), rgb=E(P, 3), clamped=E(P, 3, dtype=u8),
              tiles_touched=E(P, dtype=i32), point_list=E(max(R, 1), dtype=i32), ranges=E(tiles, 2, dtype=i32), final_T=E(H, W),
              n_contrib=E(H, W, dtype=i32))
    _ck(L.gsaj_debug_export(P, R, W, H, _p(geom), _p(binning), _p(img), *[_p(ex[k]) for k in (
        "means2D", "depths", "cov3D", "conic_opacity", "rgb", "clamped", "tiles_touched", "point_list", "ranges", "final_T", "n_contrib")], s),
        "gsaj_debug_export")
    g = dict(mean2D=E(P, 3), conic=E(P, 2, 2), dopacity=E(P, 1), dcolor=E(P, 3), ddepth=E(P, 1), mean3D=E(P, 3), dcov3D=E(P, 6), sh=E(P, M, 3),
             scale=E(P, 3), rot=E(P, 4), tau=E(P, 6), tau_sum=E(6))
    scene_b = (_p(d["means3D"]), _p(d["shs"]), None, _p(d["scales"]), d["mod"], _p(d["rotations"]), None)
    _ck(L.gsaj_rasterize_backward(P, deg, M, R, _p(d["bg"]), W, H, *scene_b, _p(d["viewmatrix"]), _p(d["projmatrix"]), _p(d["projmatrix_raw"]),
                                  _p(d["campos"]), *d["tan"], _p(radii), _p(geom), _p(binning), _p(img), _p(d["dLc"]), _p(d["dLd"]),
                                  *[_p(g[k]) for k in ("mean2D", "conic", "dopacity", "dcolor", "ddepth", "mean3D", "dcov3D", "sh", "scale", "rot",
                                                       "tau", "tau_sum")], s), "gsaj_rasterize_backward")
    st["R"], st["max_list"] = R, mt.value
    # the geometry rows of a culled Gaussian hold nothing the header promises: the export is compared where the Gaussian is visible
    vis = radii > 0
    for k in ("means2D", "depths", "cov3D", "conic_opacity", "rgb", "clamped"):
        ex[k] = torch.where(vis.view(-1, *([1] * (ex[k].dim() - 1))), ex[k], torch.zeros_like(ex[k]))
    ex["point_list"] = ex["point_list"][:R].contiguous()
    out = dict(color=color, depth=depth, opacity=opac, radii=radii, n_touched=touched)
    out.update(ex)
    out.update(g)
    return out


def _single_gaussian():
    cam = hp.small_camera(33, 17)
    sc = syn.make_scene(1, 1, cam, z_range=(1.0, 1.2), log_scale_range=(math.log(0.05), math.log(0.1)), opacity_range=(0.8, 0.9), margin=-0.3)
    return cam, sc


RASTER = {
    # A: the scene; B: another scene of fewer Gaussians on the same image size (the image workspace is zeroed once for one size)
    "canary_97x61": lambda: (_scene_inputs("canary_97x61"), _scene_inputs(cam=hp.make("canary_97x61")[0], sc=syn.make_scene(
        257, 12, hp.make("canary_97x61")[0], z_range=(0.5, 2.0), log_scale_range=(math.log(0.03), math.log(0.3))), seed=1)),
    "p300_behind_64x48": lambda: (_scene_inputs("p300_behind_64x48"), _scene_inputs(cam=hp.make("p300_behind_64x48")[0], sc=syn.make_scene(
        130, 6, hp.make("p300_behind_64x48")[0], z_range=(-1.0, 2.0), log_scale_range=(math.log(0.02), math.log(0.2)), margin=0.6), seed=1)),
    "p1_33x17": lambda: (_scene_inputs(cam=_single_gaussian()[0], sc=_single_gaussian()[1]),
                         _scene_inputs(cam=_single_gaussian()[0], sc=syn.make_scene(1, 3, _single_gaussian()[0], z_range=(2.0, 2.5)), seed=1)),
}


@pytest.mark.parametrize("record_bits", [32, 16])
@pytest.mark.parametrize("scene", sorted(RASTER))
def test_rasteriser_forward_backward_export(monkeypatch, scene, record_bits):
    """Partial tiles on both edges (97 x 61), culled rows (Gaussians behind the camera: their output rows are zeros, written by the
    kernels), a single Gaussian; fp32 and fp16 records."""
    A, B = RASTER[scene]()
    flags = 1 if record_bits == 16 else 0
    seen = {}

    def op(inp, st):
        out = _op_raster(inp, st)
        if inp[0] is A:
            seen.update(R=st["R"], culled=int((out["radii"] == 0).sum()), radii=out["radii"].clone(), sh=out["sh"].clone(), tau=out["tau"].clone())
        return out

    _contract(monkeypatch, op, (A, flags, False), (B, flags, False), "rasteriser %s fp%d" % (scene, record_bits))
    assert seen["R"] > 0, "the scene renders nothing"
    if scene == "p300_behind_64x48":
        assert seen["culled"] > 20, seen["culled"]
        gone = seen["radii"] == 0
        assert not bool(seen["sh"][gone].any()) and not bool(seen["tau"][gone].any()), "a culled Gaussian's gradient rows are not zeros"


def test_chunk_and_merge_sort_path(monkeypatch):
    """The "FULL" layout of tests/test_gpu_binning.py (tile lists of every length up to 33000 entries) through sort_long_list:
    max_tile_list < 0, what FORCE_CHUNKED_SORT passes, sends every list longer than 128 entries through 128-key chunks and the in-place
    merge.  B: the same lengths reversed over the tiles, tied depths."""
    import binning_restated as br

    def scene(depths, reverse, seed):
        L = br.layout("FULL", depths, reverse)
        return _scene_inputs(cam=L["cam"], sc=L["sc"], deg=0, seed=seed), L

    (A, LA), (B, _) = scene("log", False, 0), scene("ties", True, 1)
    seen = {}

    def op(inp, st):
        out = _op_raster(inp, st)
        if inp[0] is A:
            seen.update(max_list=st["max_list"], R=st["R"], point_list=out["point_list"].cpu().numpy().astype(np.uint32))
        return out

    _contract(monkeypatch, op, (A, 0, True), (B, 0, True), "chunk + merge sort")
    assert (seen["R"], seen["max_list"]) == (LA["R"], LA["longest"]) and LA["longest"] > 4096
    np.testing.assert_array_equal(seen["point_list"], LA["point_list"])


# ---- the loss seeds, single and batch, and the isotropic term ----------------------------------------------------------------------------
def _loss_images(K, H, W, s):
    r = _rng(K, H, W, s)
    gt_d = np.where(r.uniform(size=(K, H, W)) < 0.1, 0.0, r.uniform(0.5, 4.0, (K, H, W)))
    return dict(color=_f(r.uniform(0, 1, (K, 3, H, W))), depth=_f(r.uniform(0.5, 4.0, (K, 1, H, W))), opacity=_f(r.uniform(0.5, 1.0, (K, 1, H, W))),
                gt_color=_f(r.uniform(0, 1, (K, 3, H, W))), gt_depth=_f(gt_d), mask=_t(r.choice(np.array([0, 1, 255], np.uint8), size=(K, H, W))),
                ea=_f(r.normal(size=K) * 0.05), eb=_f(r.normal(size=K) * 0.05), scales=_f(r.uniform(0.01, 0.2, (301, 3))))


def _op_loss(inp, st):
    import torch
    L, s = _lib(), _stream()
    K, _, H, W = inp["color"].shape
    if "ws" not in st:
        stride = (L.gsaj_loss_workspace_bytes(W, H) + 255) & ~255
        st["ws"] = Z(L.gsaj_loss_workspace_bytes(W, H), dtype=torch.uint8)       # all three zeroed once
        st["ws_batch"] = Z(K * stride, dtype=torch.uint8)
        st["ws_iso"] = Z(L.gsaj_isotropic_workspace_bytes(301), dtype=torch.uint8)
    out = {}
    for name, flags in (("tracking", 1), ("mapping", 0)):
        dc, dd, do, sc = E(3, H, W), E(1, H, W), E(1, H, W), E(5)
        _ck(L.gsaj_loss_seeds(W, H, flags, 0.9, 0.01, _p(inp["color"][0]), _p(inp["depth"][0]), _p(inp["opacity"][0]), _p(inp["gt_color"][0]),
                              _p(inp["gt_depth"][0]), _p(inp["mask"][0]) if flags else None, _p(inp["ea"][0:1]), _p(inp["eb"][0:1]), _p(dc), _p(dd), _p(do),
                              _p(sc), _p(st["ws"]), s), "gsaj_loss_seeds")
        out.update({name + "_dL_dcolor": dc, name + "_dL_ddepth": dd, name + "_dL_dopacity": do, name + "_scalars": sc})
    dc, dd, sc = E(K, 3, H, W), E(K, 1, H, W), E(K, 5)
    _ck(L.gsaj_loss_seeds_batch(K, W, H, 0, 0.9, 0.01, _p(inp["color"]), _p(inp["depth"]), _p(inp["opacity"]), _p(inp["gt_color"]), _p(inp["gt_depth"]),
                                None, _p(inp["ea"]), _p(inp["eb"]), _p(dc), _p(dd), None, _p(sc), _p(st["ws_batch"]), s), "gsaj_loss_seeds_batch")
    out.update(batch_dL_dcolor=dc, batch_dL_ddepth=dd, batch_scalars=sc)
    ds, il = E(301, 3), E(1)
    _ck(L.gsaj_isotropic_loss(301, 3, 10.0, _p(inp["scales"]), _p(ds), 0, _p(il), _p(st["ws_iso"]), s), "gsaj_isotropic_loss")
    out.update(iso_dL_dscales=ds, iso_loss=il)
    return out


@pytest.mark.parametrize("H,W", [(48, 64), (61, 97)])
def test_loss_seeds_single_and_batch(monkeypatch, H, W):
    """gsaj_loss_seeds (tracking and mapping), gsaj_loss_seeds_batch K = 3 and gsaj_isotropic_loss (P = 301) with every seed image from
    torch.empty: 97 x 61 ends in a partial last block of loss partials.  The workspaces hold tickets: zeroed once, then only reused."""
    _contract(monkeypatch, _op_loss, _loss_images(3, H, W, 0), _loss_images(3, H, W, 1), "loss seeds %dx%d" % (W, H))


# ---- the loss fused into the compositors -----------------------------------------------------------------------------------------------
def _window(K, W, H, P, seed):
    f = 0.875 * W
    cams = syn.keyframe_cameras(K, radius=0.25, W=W, H=H, fx=f, fy=f, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    sc = syn.make_scene(P, seed, cams[K // 2], z_range=(1.0, 4.0), log_scale_range=(math.log(0.02), math.log(0.1)))
    views, projs, cps = (_f(np.stack([c[k] for c in cams])) for k in ("viewmatrix", "projmatrix", "campos"))
    kw = dict(sh_degree=3, shs=_f(sc["shs"]), scales=_f(sc["scales"]), rotations=_f(sc["rotations"]))
    return dict(cams=cams, views=views, projs=projs, cps=cps, kw=kw, means=_f(sc["means3D"]), opac=_f(sc["opacities"]), bg=_f(hp.PARITY_BG),
                praw=_f(cams[0]["projmatrix_raw"]), tan=(cams[0]["tanfovx"], cams[0]["tanfovy"]), M=sc["shs"].shape[1], P=P, K=K, W=W, H=H)


def _grads(g):
    import torch
    return {"g_" + k: v for k, v in g.items() if torch.is_tensor(v) and k not in ("tau_every_window",)}


def _op_fused(inp, st):
    import torch
    from gsaj.rasterizer import BatchContext, FrameContext
    w, im = inp
    K, P, W, H, M = w["K"], w["P"], w["W"], w["H"], w["M"]
    if "fc" not in st:
        st["fc"] = FrameContext(P, W, H, M, DEV, per_gaussian_tau=True)
        st["bc"] = BatchContext(K, P, W, H, M, DEV, per_gaussian_tau=True)
        st["fc"].auto_grow = st["bc"].auto_grow = False
        st["scratch"] = lambda: [t for c in (st["fc"], st["bc"]) for t in (c.geom, c.binning, getattr(c, "loss_ws", None)) if t is not None]
    fc, bc = st["fc"], st["bc"]
    out = {}
    v = K // 2
    one = (w["views"][v], w["projs"][v], w["cps"][v]) + w["tan"]
    fc.forward(w["bg"], w["means"], w["opac"], *one, sync=True, **w["kw"])
    sc1 = E(5)
    FL = dict(flags=1, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=im["gt_color"][v], gt_depth=im["gt_depth"][v],
              grad_mask=im["mask"][v].reshape(-1), exposure_a=im["ea"][v:v + 1], exposure_b=im["eb"][v:v + 1], scalars=sc1)
    fc.forward_loss(FL, w["bg"], w["means"], w["opac"], *one, **w["kw"])
    g1 = fc.backward_loss(FL, w["bg"], w["means"], one[0], one[1], w["praw"], one[2], *w["tan"], **w["kw"])
    fc.status()
    out.update(color1=fc.color, depth1=fc.depth, opacity1=fc.opacity, radii1=fc.radii, n_touched1=fc.n_touched, scalars1=sc1)
    out.update({k + "1": t for k, t in _grads(g1).items()})
    bc.forward(w["bg"], w["means"], w["opac"], w["views"], w["projs"], w["cps"], *w["tan"], sync=True, **w["kw"])
    scK, dx = E(K, 5), E(K, 2)
    FLK = dict(flags=0, alpha=0.9, rgb_boundary_threshold=0.01, gt_color=im["gt_color"], gt_depth=im["gt_depth"], grad_mask=None,
               exposure_a=im["ea"], exposure_b=im["eb"], scalars=scK, dexposure=dx)
    bc.forward_loss(FLK, w["bg"], w["means"], w["opac"], w["views"], w["projs"], w["cps"], *w["tan"], **w["kw"])
    gK = bc.backward_loss(FLK, w["bg"], w["means"], w["views"], w["projs"], w["praw"], w["cps"], *w["tan"], **w["kw"])
    assert bc.clear_aborts() == 0
    out.update(colorK=bc.color, depthK=bc.depth, opacityK=bc.opacity, radiiK=bc.radii, n_touchedK=bc.n_touched, scalarsK=scK, dexposureK=dx)
    out.update({k + "K": t for k, t in _grads(gK).items()})
    return out


@pytest.mark.parametrize("H,W", [(48, 64), (61, 97)])
def test_fused_loss_single_and_batch(monkeypatch, H, W):
    """gsaj_rasterize_forward_loss / _backward_loss on a FrameContext and the batched pair on a BatchContext, K = 3, P = 301: the loss
    partial slots of a partial last block, the K blocks of every workspace side by side."""
    wa, wb = _window(3, W, H, 301, 11), _window(3, W, H, 301, 12)
    _contract(monkeypatch, _op_fused, (wa, _loss_images(3, H, W, 0)), (wb, _loss_images(3, H, W, 1)), "fused loss %dx%d" % (W, H))


# ---- Gauss-Newton: pose Jacobians, normal equations, the LM step, the selection ------------------------------------------------------------
def _gn_frame(w, s):
    """Ground truth = what view 0's camera sees, so that the solve from view 1's pose has something to find; B: noise."""
    import torch
    from gsaj.rasterizer import FrameContext
    c = FrameContext(w["P"], w["W"], w["H"], w["M"], DEV)
    c.forward(w["bg"], w["means"], w["opac"], w["views"][0], w["projs"][0], w["cps"][0], *w["tan"], sync=True, **w["kw"])
    r = _rng(s)
    gt_c = (c.color + _f(r.normal(size=tuple(c.color.shape)) * 0.02 * s)).contiguous()
    gt_d = (c.depth[0] * _f(np.where(r.uniform(size=tuple(c.depth[0].shape)) < 0.1, 0.0, 1.0))).contiguous()
    mask = _t((r.uniform(size=(1, w["H"], w["W"])) < 0.8).astype(np.uint8))
    torch.cuda.synchronize()
    return gt_c, gt_d, mask


def _op_gn_single(inp, st):
    import gsaj
    w, frame, start, joint = inp
    if "tr" not in st:
        tr = st["tr"] = gsaj.GaussNewtonTracker(w["P"], w["W"], w["H"], w["M"], DEV, start, w["praw"], *w["tan"], w["bg"], w["means"], w["opac"], alpha=0.9,
                                                irls_delta=0.01, solve_exposure=joint, **w["kw"])
        tr.ctx.auto_grow = False
        own = "gn8_partials" if joint else "gn_partials"
        st["scratch"] = lambda: [t for t in (tr.ctx.geom, tr.ctx.binning, getattr(tr.ctx, "jac_ws", None), getattr(tr.ctx, own, None)) if t is not None]
    tr = st["tr"]
    tr.ctx.capacity = 0   # every run starts with the synchronous iteration that sizes the arena
    tr.set_frame(frame[0], frame[1], frame[2], w2c=start)
    assert tr.iterate(3) == 3
    rows = tr.ctx.gn8_partials if joint else tr.ctx.gn_partials
    return dict(state=tr.state, partials=rows, color=tr.ctx.color, depth=tr.ctx.depth, radii=tr.ctx.radii)


@pytest.mark.parametrize("joint", [False, True], ids=["pose", "pose+exposure"])
def test_gauss_newton_single_view(monkeypatch, joint):
    """gsaj_rasterize_pose_jacobian_loss[8] and gsaj_pose_gn[8]_step at 97 x 61 with P = 301 (no multiple of 64): the rows of jac_ws and of
    gn_partials -- both poisoned before every run, the header says every slot of every row is written."""
    w = _window(3, 97, 61, 301, 11)
    starts = [np.ascontiguousarray(c["viewmatrix"].T) for c in w["cams"]]
    A = (w, _gn_frame(w, 1), starts[1], joint)
    B = (w, _gn_frame(w, 9), starts[2], joint)
    _contract(monkeypatch, _op_gn_single, A, B, "Gauss-Newton single, joint=%s" % joint)


def _op_gn_window(inp, st):
    import gsaj
    w, frame, starts, joint = inp
    K = w["K"]
    if "win" not in st:
        win = st["win"] = gsaj.GaussNewtonWindow(K, w["P"], w["W"], w["H"], w["M"], DEV, np.stack(starts), w["praw"], *w["tan"], w["bg"], w["means"],
                                                 w["opac"], alpha=0.9, irls_delta=0.01, solve_exposure=joint, **w["kw"])
        win.ctx.auto_grow = False
        own = "gn8_partials" if joint else "gn_partials"
        st["scratch"] = lambda: [t for t in (win.ctx.geom, win.ctx.binning, getattr(win.ctx, "jac_ws", None), getattr(win.ctx, own, None))
                                 if t is not None]
    win = st["win"]
    win._sized = False
    win.set_frame(frame[0], frame[1], frame[2], w2cs=np.stack(starts))
    win.active[1] = 0   # a masked view: rendered, its state untouched
    assert win.iterate(3) == 3
    st["poison"](win._best)
    best = win.best()
    rows = win.ctx.gn8_partials if joint else win.ctx.gn_partials
    return dict(state=win.state, partials=rows, color=win.ctx.color, best=win._best, best_host=_t(np.array([best[0]], np.int32)))


@pytest.mark.parametrize("joint", [False, True], ids=["pose", "pose+exposure"])
def test_gauss_newton_window_and_select(monkeypatch, joint):
    """The batched forms, K = 3 with one view masked, and gsaj_pose_gn_select: K blocks of jac_ws and of the partial rows side by side."""
    w = _window(3, 97, 61, 301, 11)
    starts = [np.ascontiguousarray(c["viewmatrix"].T) for c in w["cams"]]
    A = (w, _gn_frame(w, 1), starts, joint)
    B = (w, _gn_frame(w, 9), starts[::-1], joint)
    seen = {}

    def op(inp, st):
        out = _op_gn_window(inp, st)
        if inp is A:
            seen["best"] = int(out["best_host"][0])
            seen["masked"] = out["state"][1].clone()
        return out

    _contract(monkeypatch, op, A, B, "Gauss-Newton window, joint=%s" % joint)
    assert seen["best"] in (0, 2), seen["best"]
    assert float(seen["masked"][83]) == 0.0 and float(seen["masked"][84]) == 0.0, "the masked view's state was stepped"


# ---- the arena cap -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", guards.FILLS)
def test_arena_cap_aborts_inside_the_arena(monkeypatch, fill):
    """An asynchronous frame that needs a few hundred instances more than its arena holds: the designed device-abort path of
    tests/test_gpu_arena_watch.py.  The arena is guarded and its tail band is as large as the whole un-capped arena would be, so every
    write a broken cap could make lands in memory this test owns.  The frame reports aborted, the band is intact, and the next frame
    with enough capacity is bitwise the frame a fresh context renders."""
    import torch
    from gsaj import _lib as L
    from gsaj.rasterizer import FrameContext

    w = _window(1, 97, 61, 400, 11)
    args = (w["bg"], w["means"], w["opac"], w["views"][0], w["projs"][0], w["cps"][0]) + w["tan"]
    ref = FrameContext(w["P"], w["W"], w["H"], w["M"], DEV)
    R = ref.forward(*args, sync=True, **w["kw"])
    assert R > 1000, R
    lib = _lib()
    cap = R - 300
    capped, full = lib.gsaj_binning_workspace_bytes(cap), lib.gsaj_binning_workspace_bytes(R)
    tail = lambda shape, dtype, kind: full if shape == (capped,) else 0  # noqa: E731
    with guards.guarded(monkeypatch, fill, tail_bytes=tail) as g:
        ctx = FrameContext(w["P"], w["W"], w["H"], w["M"], DEV)
        ctx.auto_grow = False
        ctx.capacity = cap
        ctx.binning = torch.empty(capped, dtype=torch.uint8, device=DEV)
        assert g.allocation_of(ctx.binning).tail == full
        ctx.forward(*args, sync=False, **w["kw"])
        torch.cuda.synchronize()
        g.check()
        with pytest.raises(L.GsajError, match="aborted"):
            ctx.status()
        assert not bool(ctx.color.any()), "an aborted first frame wrote an image"
        assert ctx.forward(*args, sync=True, **w["kw"]) == R
        torch.cuda.synchronize()
        g.check()
        for n in ("color", "depth", "opacity", "radii", "n_touched"):
            assert torch.equal(getattr(ctx, n), getattr(ref, n)), "%s after the aborted frame differs from a fresh context's" % n
