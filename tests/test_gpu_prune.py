"""GPU: the row compaction (csrc/compact.hip, gsaj.pruning.CompactPlan) against torch's t[keep] on the same tensors, the overlay
GaussianModel.prune_points against the outcome recorded from the reference (tests/golden/prune_P120.npz) and against a twin pruned
with the reference's torch statement, CovisibilityWindow.compact_plan against compact, and a pruned model through the rasteriser.
Pure data movement: every comparison is torch.equal on int32 views, so NaN payloads count."""
import ctypes
import os

import numpy as np
import pytest

import helpers as hp
import prune_restated as pr

pytestmark = pytest.mark.gpu

SENT = 0x5E471E15          # what the 64 dwords either side of every destination hold
ROW_BYTES = (4, 8, 12, 16, 36, 96, 180, 4096)
NAMES = pr.NAMES
FIELDS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")


def _dev():
    import torch
    return torch.device("cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _i32(t):
    """The tensor's bytes as int32 (a row is a multiple of 4 bytes)."""
    import torch
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.int32) if t.numel() else torch.empty(0, dtype=torch.int32, device=t.device)


def same_bits(a, b):
    import torch
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(_i32(a), _i32(b))


def pattern(t, P, w):
    """int32 [P, w]: element (row, col) of tensor t holds 41 (row w + col) + t, unique over (tensor, row, column) for t < 41 while
    41 P w < 2^32 (int32 arithmetic wraps; every P and w below stays under that)."""
    import torch
    assert t < 41 and 41 * P * w < 2 ** 32
    return (torch.arange(P * w, dtype=torch.int32, device=_dev()) * 41 + t).view(P, w)


def keep_sets(P):
    """name -> bool [P] numpy: the rows that stay."""
    rng = np.random.default_rng(P)
    r = np.arange(P)
    sets = {"all": np.ones(P, bool), "none": np.zeros(P, bool), "first": r == 0, "last": r == P - 1, "alternating": r % 2 == 1}
    if P >= 768:
        sets["one_block_between_empty"] = (r >= 256) & (r < 512)
    if P >= 512:
        sets["one_block_removed"] = ~((r >= 256) & (r < 512))
    for f in (0.01, 0.5, 0.99):
        sets["random_%g" % f] = rng.uniform(size=P) < f
    return sets


def mask_bytes(keep, remove, seed):
    """uint8 [P] with the set bytes drawn from {1, 2, 255}: a kernel that tests == 1 shows."""
    import torch
    setb = ~keep if remove else keep
    vals = np.random.default_rng(seed).choice(np.array([1, 2, 255], np.uint8), size=keep.size)
    return torch.as_tensor(np.where(setb, vals, 0).astype(np.uint8), device=_dev())


def c_plan(P, mask, remove):
    import torch
    from gsaj import _lib
    lib = _lib.load()
    ws = torch.empty(lib.gsaj_compact_workspace_bytes(P), dtype=torch.uint8, device=_dev())
    _lib.check(lib.gsaj_compact_plan(P, mask.data_ptr(), remove, ws.data_ptr(), _stream()), "gsaj_compact_plan")
    n = ctypes.c_int(-1)
    _lib.check(lib.gsaj_compact_count(ws.data_ptr(), _stream(), ctypes.byref(n)), "gsaj_compact_count")
    return ws, n.value


def c_rows(P, srcs, n_kept, ws):
    """gsaj_compact_rows into destinations that sit inside larger buffers: 64 sentinel dwords in front (65 for every odd entry, so
    that its destination is only 4-byte aligned) and 64 behind.  -> [(buffer, dwords in front, dwords of the destination)]."""
    import torch
    from gsaj import _lib
    bufs = []
    for k, s in enumerate(srcs):
        front, n = 64 + (k & 1), n_kept * s.shape[1]
        bufs.append((torch.full((front + n + 64,), SENT, dtype=torch.int32, device=_dev()), front, n))
    cnt = len(srcs)
    src = (ctypes.c_void_p * cnt)(*[s.data_ptr() for s in srcs])
    dst = (ctypes.c_void_p * cnt)(*[b.data_ptr() + 4 * front for b, front, _ in bufs])
    rb = (ctypes.c_int * cnt)(*[4 * s.shape[1] for s in srcs])
    _lib.check(_lib.load().gsaj_compact_rows(P, cnt, src, dst, rb, ws.data_ptr(), _stream()), "gsaj_compact_rows")
    return bufs


def check_rows(P, srcs, keep_t, n_kept, ws, tag):
    import torch
    first = c_rows(P, srcs, n_kept, ws)
    again = c_rows(P, srcs, n_kept, ws)  # a second launch on the same plan
    for k, (s, (buf, front, n), (buf2, _, _)) in enumerate(zip(srcs, first, again)):
        assert torch.equal(buf[front:front + n], s[keep_t].reshape(-1)), "%s: entry %d (%d bytes per row)" % (tag, k, 4 * s.shape[1])
        assert bool((buf[:front] == SENT).all()) and bool((buf[front + n:] == SENT).all()), "%s: entry %d wrote outside its rows" % (tag, k)
        assert torch.equal(buf, buf2), "%s: entry %d differs between two runs" % (tag, k)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000, 70001, 524288 + 777])
def test_rows_match_torch_indexing(P):
    """One lane, the wave and the workgroup boundary from both sides, ragged last blocks, and 2 052 blocks: more than one pass of
    the scan's 1024-lane workgroup.  Tables of exactly 32 entries over every row size, and one-entry tables of each size (the 4096
    byte rows stay out of the 32-entry table of the two large sizes and of the largest size altogether: 2 GB a tensor)."""
    import torch
    widths = [rb // 4 for rb in ROW_BYTES]
    table_w = widths if P <= 1000 else widths[:-1]
    table = [pattern(t, P, table_w[t % len(table_w)]) for t in range(32)]
    single_w = widths if P <= 70001 else widths[:-1]
    singles = {w: (table[table_w.index(w)] if w in table_w else pattern(40, P, w)) for w in single_w}
    for name, keep in keep_sets(P).items():
        keep_t = torch.as_tensor(keep, device=_dev())
        for remove in (0, 1):
            tag = "P=%d %s remove=%d" % (P, name, remove)
            mask = mask_bytes(keep, remove, seed=P + remove)
            mask0 = mask.clone()
            ws, n_kept = c_plan(P, mask, remove)
            assert n_kept == int(keep.sum()), tag
            if n_kept == 0:  # legal: no destination exists, nothing is launched (gsaj.pruning returns empty tensors)
                continue
            check_rows(P, table, keep_t, n_kept, ws, tag)
            if remove == 0:
                for w, s in singles.items():
                    check_rows(P, [s], keep_t, n_kept, ws, tag + " single")
            assert torch.equal(mask, mask0), tag
    for t, s in enumerate(table):  # the sources are what they were
        assert torch.equal(s, pattern(t, P, s.shape[1]))


def test_apply_batches_and_dtypes():
    """apply() with 40 tensors takes two launches; int64 rows, 3-D rows, a bool mask; the empty result; the errors."""
    import torch
    from gsaj import _lib
    from gsaj.pruning import CompactPlan

    P, dev = 1000, _dev()
    keep = np.random.default_rng(7).uniform(size=P) < 0.7
    keep_t = torch.as_tensor(keep, device=dev)
    shapes = [((P,), torch.int64), ((P, 15, 3), torch.float32), ((P, 1), torch.float32), ((P,), torch.int32), ((P, 2), torch.float64),
              ((P, 4), torch.uint8), ((P, 2), torch.bfloat16), ((P, 3), torch.float32)]
    tensors = []
    for k in range(40):
        shape, dtype = shapes[k % len(shapes)]
        raw = pattern(k, P, int(np.prod(shape[1:], dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size() // 4)
        tensors.append(raw.view(dtype).view(shape))
    nan = torch.tensor([0x7FC12345, -1, 0x7F800001], dtype=torch.int32, device=dev).view(torch.float32)  # NaN payloads travel
    tensors[2][5:8, 0] = nan
    keep_t[5:8] = True
    for mask, remove in ((keep_t, False), (~keep_t, True), ((~keep_t).to(torch.uint8) * 255, True)):
        plan = CompactPlan(mask, remove=remove)
        outs = plan.apply(*tensors)
        assert plan.launches == 2 and plan.n_kept == int(keep_t.sum()) and len(outs) == 40
        for t, o in zip(tensors, outs):
            assert same_bits(o, t[keep_t])
        assert same_bits(plan.apply(tensors[0])[0], tensors[0][keep_t]) and plan.launches == 3  # several applies follow one plan
        assert torch.equal(plan.keep_mask(), keep_t)
    # n_kept handed in: the same result and no read
    lib = _lib.load()
    reads = []
    real = lib.gsaj_compact_count
    try:
        lib.gsaj_compact_count = lambda *a: reads.append(a) or real(*a)
        plan = CompactPlan(keep_t, remove=False, n_kept=int(keep_t.sum()))
        assert same_bits(plan.apply(tensors[1])[0], tensors[1][keep_t]) and reads == []
        assert same_bits(CompactPlan(keep_t, remove=False).apply(tensors[1])[0], tensors[1][keep_t]) and len(reads) == 1
    finally:
        lib.gsaj_compact_count = real
    # nothing kept
    plan = CompactPlan(torch.ones(P, dtype=torch.bool, device=dev))
    outs = plan.apply(tensors[0], tensors[1])
    assert plan.n_kept == 0 and plan.launches == 0 and tuple(outs[0].shape) == (0,) and tuple(outs[1].shape) == (0, 15, 3)
    assert outs[0].dtype == torch.int64 and outs[1].dtype == torch.float32
    # the errors
    plan = CompactPlan(keep_t, remove=False)
    f = torch.zeros(P, 6, device=dev)
    bad = [f[:, ::2], f.t().contiguous().t(), f.cpu(), f[:-1], torch.zeros(P, 3, dtype=torch.uint8, device=dev),
           torch.zeros(P, 1, dtype=torch.float16, device=dev), torch.zeros(P, 1025, device=dev), torch.zeros(P, 0, device=dev), None]
    for b in bad:
        with pytest.raises(_lib.GsajError):
            plan.apply(tensors[0], b)
    for m in (keep_t.float(), keep_t.view(P // 2, 2), keep_t[:0], keep_t.cpu()):
        with pytest.raises(_lib.GsajError):
            CompactPlan(m)
    with pytest.raises(_lib.GsajError):
        CompactPlan(keep_t, n_kept=P + 1)


# ---- the model --------------------------------------------------------------------------------------------------------------
def build_model(params, moments=None, step=None, aux=None, ids_on_device=False, optimizer=True):
    """An overlay GaussianModel of the given raw parameters (name -> array), with a torch.optim.Adam of the six named groups whose
    state is set to `moments` (name -> (exp_avg, exp_avg_sq)) when given."""
    import torch
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    dev = _dev()
    m = GaussianModel(1)
    for n in NAMES:
        setattr(m, FIELDS[n], torch.as_tensor(np.ascontiguousarray(params[n]), device=dev).clone().requires_grad_(True))
    m._init_aux()
    for a, v in (aux or {}).items():
        on_dev = a not in ("unique_kfIDs", "n_obs") or ids_on_device
        setattr(m, a, torch.as_tensor(np.ascontiguousarray(v), device=dev if on_dev else "cpu").clone())
    if optimizer:
        m.optimizer = torch.optim.Adam([dict(params=[getattr(m, FIELDS[n])], lr=1e-3 * (k + 1), name=n) for k, n in enumerate(NAMES)],
                                       lr=0.0, eps=1e-15)
        if moments is not None:
            for n in NAMES:
                m.optimizer.state[getattr(m, FIELDS[n])] = dict(step=torch.tensor(float(step)),
                                                                exp_avg=torch.as_tensor(moments[n][0], device=dev).clone(),
                                                                exp_avg_sq=torch.as_tensor(moments[n][1], device=dev).clone())
    return m


def adam_steps(m, count, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    for _ in range(count):
        for n in NAMES:
            p = getattr(m, FIELDS[n])
            p.grad = torch.randn(p.shape, generator=gen).to(p.device)
        m.optimizer.step()


def torch_prune(m, mask):
    """The reference's statement (gaussian_model.py:559-597) in torch on the overlay model's tensors."""
    import torch
    keep = ~mask
    if m.optimizer is not None:
        for group in m.optimizer.param_groups:
            p = group["params"][0]
            st = m.optimizer.state.get(p, None)
            new = p.detach()[keep].requires_grad_(True)
            if st is not None:
                st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]
                del m.optimizer.state[p]
                m.optimizer.state[new] = st
            group["params"][0] = new
            setattr(m, FIELDS[group["name"]], new)
    else:
        for n in NAMES:
            setattr(m, FIELDS[n], getattr(m, FIELDS[n]).detach()[keep].requires_grad_(True))
    m.xyz_gradient_accum, m.denom, m.max_radii2D = m.xyz_gradient_accum[keep], m.denom[keep], m.max_radii2D[keep]
    m.unique_kfIDs = m.unique_kfIDs[keep.to(m.unique_kfIDs.device)]
    m.n_obs = m.n_obs[keep.to(m.n_obs.device)]


def assert_models_equal(a, b, tag):
    for n in NAMES:
        pa, pb = getattr(a, FIELDS[n]), getattr(b, FIELDS[n])
        assert same_bits(pa, pb), (tag, n)
        assert pa.is_leaf and pa.requires_grad
        if a.optimizer is not None:
            ga = [g for g in a.optimizer.param_groups if g["name"] == n][0]
            assert ga["params"][0] is pa and len(a.optimizer.state) == len(b.optimizer.state), (tag, n)
            sa, sb = a.optimizer.state.get(pa), b.optimizer.state.get(pb)
            assert (sa is None) == (sb is None), (tag, n)
            if sa is not None:
                assert sorted(sa) == sorted(sb) and float(sa["step"]) == float(sb["step"]), (tag, n)
                assert same_bits(sa["exp_avg"], sb["exp_avg"]) and same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), (tag, n)
    for x in pr.AUX:
        ta, tb = getattr(a, x), getattr(b, x)
        assert ta.device == tb.device and same_bits(ta, tb), (tag, x)


@pytest.mark.parametrize("name", ["aniso", "iso"])
def test_model_reproduces_the_reference_golden(golden_dir, name):
    import torch
    rec = pr.case(np.load(os.path.join(golden_dir, "prune_P120.npz")), name)
    m = build_model({n: rec["in_" + n] for n in NAMES}, {n: (rec["in_exp_avg_" + n], rec["in_exp_avg_sq_" + n]) for n in NAMES},
                    step=rec["in_step_xyz"], aux={a: rec["in_" + a] for a in pr.AUX})
    mask = torch.as_tensor(rec["mask"], device=_dev())
    plan = m.prune_points(mask)
    assert plan.n_kept == int((~rec["mask"]).sum()) and plan.launches == 1
    for n in NAMES:
        p = getattr(m, FIELDS[n])
        st = m.optimizer.state[p]
        assert p.is_leaf and p.requires_grad and m.optimizer.param_groups[NAMES.index(n)]["params"][0] is p
        for got, key in ((p, "out_" + n), (st["exp_avg"], "out_exp_avg_" + n), (st["exp_avg_sq"], "out_exp_avg_sq_" + n)):
            assert same_bits(got, torch.as_tensor(rec[key], device=_dev())), key
        assert float(st["step"]) == float(rec["out_step_" + n]) == 3.0
    assert len(m.optimizer.state) == 6
    for a in pr.AUX:
        got = getattr(m, a)
        assert got.device.type == ("cpu" if a in ("unique_kfIDs", "n_obs") else "cuda")
        assert same_bits(got.cpu(), torch.as_tensor(rec["out_" + a])), a


def _twins(P, seed, steps=3, optimizer=True, ids_on_device=False):
    rng = np.random.default_rng(seed)
    shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 3, 3), opacity=(P, 1), scaling=(P, 3), rotation=(P, 4))
    params = {n: rng.normal(size=s).astype(np.float32) for n, s in shapes.items()}
    aux = dict(xyz_gradient_accum=rng.uniform(size=(P, 1)).astype(np.float32), denom=rng.integers(0, 5, (P, 1)).astype(np.float32),
               max_radii2D=rng.integers(0, 30, P).astype(np.float32), unique_kfIDs=rng.integers(0, 9, P).astype(np.int32),
               n_obs=rng.integers(0, 6, P).astype(np.int32))
    twins = [build_model(params, aux=aux, ids_on_device=ids_on_device, optimizer=optimizer) for _ in range(2)]
    if optimizer and steps:
        for m in twins:
            adam_steps(m, steps, seed=seed + 1)
    return twins


@pytest.mark.parametrize("ids_on_device", [False, True])
def test_model_against_the_torch_statement(ids_on_device):
    import torch
    P = 1000
    a, b = _twins(P, 11, ids_on_device=ids_on_device)
    mask = torch.as_tensor(np.random.default_rng(12).uniform(size=P) < 0.3, device=_dev())
    plan = a.prune_points(mask)
    torch_prune(b, mask)
    assert plan.launches == 1 and a._xyz.shape[0] == P - int(mask.sum())
    assert a.unique_kfIDs.device.type == ("cuda" if ids_on_device else "cpu")
    assert_models_equal(a, b, "pruned")
    for n in NAMES:
        assert float(a.optimizer.state[getattr(a, FIELDS[n])]["step"]) == 3.0
    for m in (a, b):  # the optimizer goes on as if nothing had happened
        adam_steps(m, 1, seed=99)
    assert_models_equal(a, b, "one more step")
    assert float(a.optimizer.state[a._xyz]["step"]) == 4.0


@pytest.mark.parametrize("kind", ["no_optimizer", "empty_state", "n_kept_given", "nothing_kept"])
def test_model_variants(kind):
    import torch
    from gsaj import _lib
    P = 1000
    a, b = _twins(P, 21, steps=0 if kind == "empty_state" else 3, optimizer=kind != "no_optimizer")
    mask = torch.as_tensor(np.random.default_rng(22).uniform(size=P) < 0.3, device=_dev())
    if kind == "nothing_kept":
        mask[:] = True
    if kind == "n_kept_given":
        lib, reads = _lib.load(), []
        real = lib.gsaj_compact_count
        try:
            lib.gsaj_compact_count = lambda *args: reads.append(args) or real(*args)
            a.prune_points(mask.to(torch.uint8), n_kept=P - int(mask.sum()))
        finally:
            lib.gsaj_compact_count = real
        assert reads == []
    else:
        a.prune_points(mask)
    torch_prune(b, mask)
    assert_models_equal(a, b, kind)
    if kind == "empty_state":
        assert len(a.optimizer.state) == 0
        for m in (a, b):
            adam_steps(m, 1, seed=5)
        assert_models_equal(a, b, kind + " first step")
    if kind == "nothing_kept":
        assert tuple(a._features_rest.shape) == (0, 3, 3) and tuple(a.max_radii2D.shape) == (0,) and tuple(a.n_obs.shape) == (0,)
        assert tuple(a.optimizer.state[a._xyz]["exp_avg"].shape) == (0, 3)


# ---- the covisibility window ------------------------------------------------------------------------------------------------
def test_covisibility_compact_plan_equals_compact(golden_dir):
    import torch
    from gsaj.covisibility import CovisibilityWindow
    from gsaj.pruning import CompactPlan

    g = np.load(os.path.join(golden_dir, "covis_prune.npz"))
    window = g["window"].tolist()
    K, P = g["n_touched"].shape
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=_dev())  # noqa: E731
    cw = CovisibilityWindow(P, _dev())
    cw.set_window(window, t(g["n_touched"]))
    to_prune, n_pruned = cw.prune_mask(window, t(g["unique_kfIDs"]), "slam", True)
    assert 0 < int(n_pruned) < P
    twin = CovisibilityWindow(P, _dev())
    twin.words, twin.slot_of = cw.words.clone(), dict(cw.slot_of)
    plan = CompactPlan(to_prune, remove=True, n_kept=P - int(n_pruned))
    cw.compact_plan(plan)
    twin.compact(to_prune == 0)
    assert cw.P == twin.P == P - int(n_pruned) and torch.equal(cw.words, twin.words) and cw.words.dtype == twin.words.dtype
    assert cw.to_prune.numel() == cw.P and cw.n_obs.numel() == cw.P
    for kf in window[:2]:
        assert cw.counts(kf_id=kf) == twin.counts(kf_id=kf)
    from gsaj import _lib
    with pytest.raises(_lib.GsajError):
        cw.compact_plan(plan)  # a plan of the old size


def test_back_end_flow_prune_mask_prune_points_compact_plan():
    """The flow INTEGRATION.md 3f states: prune_mask -> prune_points(to_prune) -> compact_plan(plan), against the torch statement."""
    import torch
    import covis_restated as cr
    from gsaj.covisibility import CovisibilityWindow

    P, K, dev = 1000, 4, _dev()
    a, b = _twins(P, 31)
    window = [12, 9, 6, 3]
    cw, twin = CovisibilityWindow(P, dev), CovisibilityWindow(P, dev)
    nt = torch.as_tensor(cr.make_case(P, K, 0.5, 2), device=dev)
    for w in (cw, twin):
        w.set_window(window, nt)
    kf_ids = a.unique_kfIDs.to(dev)
    to_prune, n_pruned = cw.prune_mask(window, kf_ids, "slam", True)
    removed = to_prune.bool().clone()
    assert 0 < int(n_pruned) < P
    plan = a.prune_points(to_prune)
    cw.compact_plan(plan)
    torch_prune(b, removed)
    twin.compact(~removed)
    assert_models_equal(a, b, "flow")
    assert cw.P == twin.P == a._xyz.shape[0] and torch.equal(cw.words, twin.words)
    assert cw.counts(kf_id=12) == twin.counts(kf_id=12)
    cw.prune_mask(window, a.unique_kfIDs.to(dev), "slam", True)  # the compacted window and model go on together


# ---- through the rasteriser -------------------------------------------------------------------------------------------------
def test_pruned_model_renders_like_the_indexed_one():
    import torch
    from gaussian_splatting.gaussian_renderer import render
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from utils.camera_utils import Camera

    cam, sc, deg = hp.make("p300_behind_64x48")
    dev = "cuda:0"
    P = sc["means3D"].shape[0]
    mk = lambda: GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"],  # noqa: E731
                                              sh_degree=deg, device=dev)
    a, b = mk(), mk()
    mask = torch.as_tensor(np.random.default_rng(3).uniform(size=P) < 0.3, device=dev)
    a.prune_points(mask)
    for n in NAMES:
        setattr(b, FIELDS[n], getattr(b, FIELDS[n]).detach()[~mask].requires_grad_(True))
    view = Camera.from_synthetic(cam, device=dev)

    class Pipe:
        convert_SHs_python = False
        compute_cov3D_python = False

    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    ra, rb = render(view, a, Pipe, bg), render(view, b, Pipe, bg)
    assert a._xyz.shape[0] == P - int(mask.sum()) and int((ra["radii"] > 0).sum()) > 0
    for key in ("render", "depth", "radii", "n_touched"):
        assert same_bits(ra[key], rb[key]), key
