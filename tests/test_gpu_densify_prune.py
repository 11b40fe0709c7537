"""GPU: clone, split and prune of the map from one plan (csrc/densify_prune.hip, gsaj.densify.DensifyPlan) against the NumPy
restatement of the reference (tests/densify_restated.py) on generated inputs that keep a 1e-4 margin from every threshold, the
exact ties, a prune-only plan against gsaj.pruning.CompactPlan (one row mover under both), the overlay
GaussianModel.densify_and_prune against the outcome recorded from the reference (tests/golden/densify_prune_P150.npz) and against
a twin densified with the reference's statement in torch, the counter-based noise, the covisibility window and a densified model
through the rasteriser.  Everything copied, zeroed or counted is compared with torch.equal on int32 views; the children's xyz and
_scaling against the fp64 restatement within the bounds derived there.  The worst err / bound of each goes into
profiles/r08_densify_parity.json when GSAJ_WRITE_PARITY is set."""
import ctypes
import json
import os

import numpy as np
import pytest

import densify_restated as dr
import helpers as hp

pytestmark = pytest.mark.gpu

SENT = 0x5E471E15          # what the 64 dwords either side of every destination hold
ROW_BYTES = (4, 8, 12, 16, 36, 96, 180, 4096)
NAMES = dr.NAMES
FIELDS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY = 5.0, 0.01, 0.25, 0.3   # t_dense = 0.05, t_big = 0.5
PATTERNS = ("nothing", "all_clone", "all_split", "all_pruned", "random", "block_edges")
WORST = {}                 # name -> worst err / bound seen in this session


def _dev():
    import torch
    return torch.device("cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _i32(t):
    import torch
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.int32) if t.numel() else torch.empty(0, dtype=torch.int32, device=t.device)


def same_bits(a, b):
    import torch
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(_i32(a), _i32(b))


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    if os.environ.get("GSAJ_WRITE_PARITY"):
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08_densify_parity.json")
        with open(path, "w") as fh:
            json.dump({"what": "worst |device - fp64 restatement| / bound over tests/test_gpu_densify_prune.py", "worst_err_over_bound": WORST},
                      fh, indent=1, sort_keys=True)


def pattern(t, P, w):
    """int32 [P, w]: element (row, col) of tensor t holds 41 (row w + col) + t + 1: unique over (tensor, row, column), never 0."""
    import torch
    assert t < 40 and 41 * P * w < 2 ** 32
    return (torch.arange(P * w, dtype=torch.int32, device=_dev()) * 41 + t + 1).view(P, w)


# ---- inputs with a margin -------------------------------------------------------------------------------------------------------
def make_inputs(P, S, N, pat, seed):
    """accum, denom [P,1], scaling [P,S], opacity [P,1] (numpy fp32) and max_screen_size of one pattern.  Every g, m, child m and o
    is at least 1e-4 (relative) from its threshold: the classes are drawn from ranges that end well short of them, and the few
    child scales that land near t_big are moved."""
    rng = np.random.default_rng(seed)
    r = np.arange(P)
    want_g = {"nothing": np.zeros(P, bool), "all_clone": np.ones(P, bool), "all_split": np.ones(P, bool), "all_pruned": rng.uniform(size=P) < 0.5,
              "random": rng.uniform(size=P) < 0.4, "block_edges": (r % 256 == 0) | (r % 256 == 255) | (r == P - 1)}[pat]
    large = {"nothing": rng.uniform(size=P) < 0.5, "all_clone": np.zeros(P, bool), "all_split": np.ones(P, bool),
             "all_pruned": rng.uniform(size=P) < 0.5, "random": rng.uniform(size=P) < 0.5, "block_edges": (r // 256 + r) % 2 == 0}[pat]
    huge = (rng.uniform(size=P) < 0.15) & large if pat == "random" else np.zeros(P, bool)
    faint = {"all_pruned": np.ones(P, bool), "random": rng.uniform(size=P) < 0.1}.get(pat, np.zeros(P, bool))
    denom = rng.integers(1, 5, P).astype(np.float32)
    g = np.where(want_g, rng.uniform(0.3, 0.9, P), rng.uniform(0.0, 0.2, P))
    if pat == "random":  # signs: the clone rule takes |g|, the split rule g
        g = np.where(rng.uniform(size=P) < 0.1, -g, g)
    accum = (g * denom).astype(np.float32)
    if pat == "random":  # rows never seen: 0 / 0
        unseen = rng.uniform(size=P) < 0.1
        accum[unseen], denom[unseen] = 0.0, 0.0
    top = np.where(huge, rng.uniform(0.8, 2.5, P), np.where(large, rng.uniform(0.07, 0.3, P), rng.uniform(0.004, 0.04, P)))
    e = top[:, None] * np.concatenate([np.ones((P, 1)), rng.uniform(0.2, 1.0, (P, S - 1))], axis=1)
    e = np.take_along_axis(e, rng.permuted(np.tile(np.arange(S), (P, 1)), axis=1), axis=1)
    scaling = np.log(e).astype(np.float32)
    for _ in range(8):  # child scales near t_big: shrink the row a little
        mc = np.exp(scaling.astype(np.float64)).max(axis=1) / float(np.float32(0.8 * N))
        near = np.abs(mc - 0.5) < 1e-3
        if not near.any():
            break
        scaling[near] -= np.float32(0.01)
    opacity = np.where(faint, rng.uniform(-3.0, -1.2, P), rng.uniform(-0.4, 3.0, P)).astype(np.float32)
    th = dr.thresholds(MAX_GRAD, MIN_OPACITY, EXTENT, 20, PERCENT_DENSE, N)
    gq, m, mc, o = dr.quantities(accum[:, None], denom[:, None], scaling, opacity[:, None], N)
    far = lambda v, t: (np.abs(np.asarray(v, np.float64) - float(t)) >= 1e-4 * float(t)).all()  # noqa: E731
    assert far(np.abs(gq), th["thr"]) and far(m, th["t_d"]) and far(m, th["t_b"]) and far(mc, th["t_b"]) and far(o, th["min_o"])
    return dict(accum=accum[:, None], denom=denom[:, None], scaling=scaling, opacity=opacity[:, None],
                max_screen_size=20 if pat in ("random", "block_edges") else None)


def c_plan(P, S, N, stages, accum, denom, n_grads, scaling, opacity, max_screen_size, max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=EXTENT):
    import torch
    from gsaj import _lib
    from gsaj.densify import thresholds
    lib = _lib.load()
    thr, t_d, t_b, min_o, rule, size_all = thresholds(max_grad, min_opacity, extent, max_screen_size, PERCENT_DENSE)
    ws = torch.empty(lib.gsaj_densify_workspace_bytes(P, N), dtype=torch.uint8, device=_dev())
    code = torch.full((P + 64,), 0xEE, dtype=torch.uint8, device=_dev())
    _lib.check(lib.gsaj_densify_plan(P, S, N, stages, accum.data_ptr(), None if denom is None else denom.data_ptr(), n_grads, scaling.data_ptr(),
                                     opacity.data_ptr(), thr, t_d, t_b, min_o, int(rule), int(size_all), code.data_ptr(), ws.data_ptr(), _stream()),
               "gsaj_densify_plan")
    c = (ctypes.c_int * 4)(-1, -1, -1, -1)
    _lib.check(lib.gsaj_densify_counts(ws.data_ptr(), _stream(), c), "gsaj_densify_counts")
    assert bool((code[P:] == 0xEE).all())
    return ws, code[:P], tuple(c)


def c_rows(P, N, srcs, zero_new, n_out, code, ws):
    """gsaj_densify_rows into destinations inside larger buffers: 64 sentinel dwords in front (65 for every odd entry, so that its
    destination is only 4-byte aligned) and 64 behind.  -> [(buffer, dwords in front, dwords of the destination)]."""
    import torch
    from gsaj import _lib
    bufs = []
    for k, s in enumerate(srcs):
        front, n = 64 + (k & 1), n_out * s.shape[1]
        bufs.append((torch.full((front + n + 64,), SENT, dtype=torch.int32, device=_dev()), front, n))
    cnt = len(srcs)
    src = (ctypes.c_void_p * cnt)(*[s.data_ptr() for s in srcs])
    dst = (ctypes.c_void_p * cnt)(*[b.data_ptr() + 4 * front for b, front, _ in bufs])
    rb = (ctypes.c_int * cnt)(*[4 * s.shape[1] for s in srcs])
    zn = (ctypes.c_int * cnt)(*[int(z) for z in zero_new])
    _lib.check(_lib.load().gsaj_densify_rows(P, N, cnt, src, dst, rb, zn, code.data_ptr(), ws.data_ptr(), _stream()), "gsaj_densify_rows")
    return bufs


def check_rows(P, N, srcs, zero_new, src_t, new_t, code, ws, tag):
    import torch
    n_out = int(src_t.numel())
    first = c_rows(P, N, srcs, zero_new, n_out, code, ws)
    again = c_rows(P, N, srcs, zero_new, n_out, code, ws)  # a second launch on the same plan
    for k, (s, zn, (buf, front, n), (buf2, _, _)) in enumerate(zip(srcs, zero_new, first, again)):
        want = s[src_t]
        if zn:
            want = want.clone()
            want[new_t] = 0
        assert torch.equal(buf[front:front + n], want.reshape(-1)), "%s: entry %d (%d bytes per row, zero_new=%d)" % (tag, k, 4 * s.shape[1], zn)
        assert bool((buf[:front] == SENT).all()) and bool((buf[front + n:] == SENT).all()), "%s: entry %d wrote outside its rows" % (tag, k)
        assert torch.equal(buf, buf2), "%s: entry %d differs between two runs" % (tag, k)


def check_children(P, S, N, inp, code, ws, src, kind, tag, noise=None, seed=0):
    """gsaj_densify_children into sentinel-guarded copies: child rows within the bounds, every other row and the guards untouched."""
    import torch
    from gsaj import _lib
    rng = np.random.default_rng(P + S + N)
    xyz = rng.normal(size=(P, 3)).astype(np.float32) * 3
    rot = rng.normal(size=(P, 4)).astype(np.float32)
    z = rng.standard_normal((N, P, 3)).astype(np.float32) if noise is None else noise
    n_out = len(src)
    bufs = {}
    for name, cols, front in (("xyz", 3, 64), ("scaling", S, 65)):
        bufs[name] = (torch.full((front + n_out * cols + 64,), SENT, dtype=torch.int32, device=_dev()), front, n_out * cols)
    xyz_t, sc_t, rot_t, z_t = _t(xyz), _t(inp["scaling"]), _t(rot), _t(z)
    dx, ds = (bufs[k][0].data_ptr() + 4 * bufs[k][1] for k in ("xyz", "scaling"))
    _lib.check(_lib.load().gsaj_densify_children(P, S, N, xyz_t.data_ptr(), sc_t.data_ptr(), rot_t.data_ptr(), z_t.data_ptr(), seed,
                                                 code.data_ptr(), ws.data_ptr(), dx, ds, _stream()), "gsaj_densify_children")
    cx, bx, cs, bs = dr.children(xyz, inp["scaling"], rot, z, N)
    ch = kind >= 2
    for name, cols, want, bound in (("xyz", 3, cx, bx), ("scaling", S, cs, bs)):
        buf, front, n = bufs[name]
        got = buf[front:front + n].view(torch.float32).view(n_out, cols).cpu().numpy()
        raw = buf[front:front + n].view(n_out, cols).cpu().numpy()
        assert bool((buf[:front] == SENT).all()) and bool((buf[front + n:] == SENT).all()), (tag, name)
        assert (raw[~ch] == SENT).all(), (tag, name, "a row that is no child was written")
        if ch.any():
            err = np.abs(got[ch].astype(np.float64) - want[kind[ch] - 2, src[ch]])
            ratio = err / bound[kind[ch] - 2, src[ch]]
            note("child_" + name, ratio.max())
            assert (ratio <= 1.0).all(), (tag, name, float(ratio.max()))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000, 70001])
def test_plan_rows_children_match_the_restatement(P):
    """One lane, the wave and the workgroup boundary from both sides, ragged last blocks, and 274 blocks x (2 + N) counters: more
    than one pass of the scan's 1024-lane workgroup.  S = 3 and 1, N = 1, 2, 4, every pattern; tables of 23 entries over the row
    sizes with both new-row modes, and one-entry tables of each size (4096-byte rows up to P = 1000)."""
    import torch
    widths = [rb // 4 for rb in ROW_BYTES]
    table_w = widths if P <= 1000 else widths[:-1]
    table = [pattern(t, P, table_w[t % len(table_w)]) for t in range(23)]
    zero_new = [t % 3 == 1 for t in range(23)]
    combos = [(3, 2), (1, 1), (3, 4), (1, 2), (3, 1), (1, 4)] if P <= 1000 else [(3, 2), (1, 4)]
    for S, N in combos:
        for pat in PATTERNS:
            tag = "P=%d S=%d N=%d %s" % (P, S, N, pat)
            inp = make_inputs(P, S, N, pat, seed=1000 * S + 10 * N + P)
            th = dr.thresholds(MAX_GRAD, MIN_OPACITY, EXTENT, inp["max_screen_size"], PERCENT_DENSE, N)
            code_want = dr.classify(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], th, N)
            src, kind = dr.order(code_want, N)
            dev_in = {k: _t(inp[k]) for k in ("accum", "denom", "scaling", "opacity")}
            keep = {k: v.clone() for k, v in dev_in.items()}
            ws, code, counts = c_plan(P, S, N, dr.ALL, dev_in["accum"], dev_in["denom"], P, dev_in["scaling"], dev_in["opacity"], inp["max_screen_size"])
            assert torch.equal(code, _t(code_want)), tag
            n0, n1, n2 = int((code_want & 1 != 0).sum()), int((code_want & 2 != 0).sum()), int((code_want & 4 != 0).sum())
            assert counts == (n0, n1, n2, n0 + n1 + N * n2) and counts[3] == len(src), (tag, counts)
            if pat == "all_pruned":
                assert counts[3] == 0, tag
            if pat == "all_clone":
                assert counts[:3] == (P, P, 0), tag
            if pat == "all_split":
                assert counts[:3] == (0, 0, P), tag
            if pat == "block_edges" and P > 2:
                assert n1 + n2 >= 2 * (P // 256), tag
            if counts[3] == 0:  # legal: no destination exists, nothing is launched (gsaj.densify returns empty tensors)
                continue
            code0 = code.clone()
            src_t, new_t = _t(src), _t(kind > 0)
            check_rows(P, N, table, zero_new, src_t, new_t, code, ws, tag)
            singles = table_w if (S, N) == (3, 2) and pat == "random" else [3]
            for w in singles:
                for zn in (False, True):
                    check_rows(P, N, [table[table_w.index(w)] if w in table_w else pattern(30, P, w)], [zn], src_t, new_t, code, ws, tag + " single")
            check_children(P, S, N, inp, code, ws, src, kind, tag)
            assert torch.equal(code, code0) and all(torch.equal(dev_in[k], keep[k]) for k in keep), tag
    for t, s in enumerate(table):  # the sources are what they were
        assert torch.equal(s, pattern(t, P, s.shape[1]))


@pytest.mark.parametrize("P", [257, 1000])
def test_stage_subsets(P):
    """CLONE alone and SPLIT alone (the reference's densify_and_clone / densify_and_split), gradients handed in directly, the
    split's shorter than the map (padded_grad)."""
    import torch
    S, N = 3, 2
    inp = make_inputs(P, S, N, "random", seed=P)
    with np.errstate(all="ignore"):
        g = (inp["accum"] / inp["denom"]).astype(np.float32)
    g[np.isnan(g)] = 0
    th = dr.thresholds(MAX_GRAD, MIN_OPACITY, EXTENT, None, PERCENT_DENSE, N)
    table = [pattern(t, P, w) for t, w in enumerate((3, 1, 9, 4))]
    for stages, n_grads in ((dr.CLONE, P), (dr.SPLIT, P), (dr.SPLIT, P - 100), (dr.CLONE | dr.SPLIT, P), (dr.PRUNE, P), (0, P)):
        tag = "P=%d stages=%d n_grads=%d" % (P, stages, n_grads)
        gp = g.copy()
        gp[n_grads:] = 0
        code_want = dr.classify(gp, None, inp["scaling"], inp["opacity"], th, N, stages=stages)
        src, kind = dr.order(code_want, N)
        g_t, sc_t, op_t = _t(g[:n_grads]), _t(inp["scaling"]), _t(inp["opacity"])
        ws, code, counts = c_plan(P, S, N, stages, g_t, None, n_grads, sc_t, op_t, None)
        assert torch.equal(code, _t(code_want)) and counts[3] == len(src), tag
        if stages == dr.CLONE:
            assert counts[0] == P and counts[1] > 0 and counts[2] == 0, tag
        if stages == dr.SPLIT and n_grads == P:
            assert counts[0] < P and counts[1] == 0 and counts[2] > 0, tag
        if stages == 0:
            assert counts == (P, 0, 0, P), tag
        check_rows(P, N, table, [False, True, False, True], _t(src), _t(kind > 0), code, ws, tag)


@pytest.mark.parametrize("P", [255, 256, 257, 1000])
def test_a_prune_only_plan_moves_what_the_compact_plan_moves(P):
    """The two wrappers over the one mover (csrc/row_move.h) agree.  Opacity logits of +2 / -2 against min_opacity = 0.3 make the
    prune rule keep a known set: with two blocks or more the first block whole (the straight copy), with three or more the second
    block not at all, and two rows of three everywhere else, the ragged last block included.  A DensifyPlan of the PRUNE stage
    alone (no gradients, no size rule) then has to give the tensors CompactPlan gives for that set, which are t[keep], bit for
    bit, for rows of 4, 12, 180 and 4096 bytes, and counts of (kept, 0, 0, kept)."""
    import torch
    from gsaj.densify import PRUNE, DensifyPlan
    from gsaj.pruning import CompactPlan
    r = torch.arange(P, device=_dev())
    nb = (P + 255) // 256
    keep = r % 3 != 1  # (P = 257: the one row of the last block goes)
    if nb >= 2:
        keep[:256] = True
    if nb >= 3:
        keep[256:512] = False
    n_kept = int(keep.sum())
    assert 0 < n_kept < P
    opacity = torch.where(keep, 2.0, -2.0).to(torch.float32).view(P, 1)
    scaling = torch.full((P, 3), -3.0, device=_dev())
    tensors = [pattern(t, P, w) for t, w in enumerate((1, 3, 45, 1024))]
    dn = DensifyPlan(torch.empty(0, dtype=torch.float32, device=_dev()), None, scaling, opacity, MAX_GRAD, MIN_OPACITY, EXTENT, None,
                     percent_dense=PERCENT_DENSE, stages=PRUNE)
    assert dn.counts == (n_kept, 0, 0, n_kept), (P, dn.counts)
    cp = CompactPlan(keep, remove=False)
    assert cp.n_kept == n_kept
    got_dn, got_cp = dn.apply(tensors), cp.apply(*tensors)
    assert dn.launches == 1 and cp.launches == 1
    for t, a, b in zip(tensors, got_dn, got_cp):
        assert same_bits(a, b), "P=%d: rows of %d bytes differ between the two plans" % (P, 4 * t.shape[1])
        assert same_bits(a, t[keep]), "P=%d: rows of %d bytes are not t[keep]" % (P, 4 * t.shape[1])


def test_exact_ties():
    """scaling = 0 with t_dense = 1: clone, not split.  opacity = 0 with min_opacity = 0.5: not pruned.  g exactly the threshold:
    selected.  0 / 0: not selected.  accum > 0 over denom = 0: selected (inf)."""
    import torch
    P, S, N = 5, 3, 2
    accum = np.array([0.9, 0.5, 0.0, 0.3, 0.1], np.float32)[:, None]
    denom = np.array([1.0, 2.0, 0.0, 0.0, 1.0], np.float32)[:, None]
    scaling = np.array([[0, 0, 0], [0, -1, -2], [0, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    opacity = np.zeros((P, 1), np.float32)
    ws, code, counts = c_plan(P, S, N, dr.ALL, _t(accum), _t(denom), P, _t(scaling), _t(opacity), None, max_grad=0.25, min_opacity=0.5, extent=100.0)
    #        row 0: g over, m == t_dense: clone | row 1: g == threshold: clone | row 2: 0/0 | row 3: inf, m = e > 1: split | row 4: below
    assert code.cpu().tolist() == [1 | 2, 1 | 2, 1, 4, 1] and counts == (4, 2, 1, 8)
    th = dr.thresholds(0.25, 0.5, 100.0, None, 0.01, N)
    assert dr.classify(accum, denom, scaling, opacity, th, N).tolist() == code.cpu().tolist()
    # extent 10 with the size rule: t_dense = 0.1, t_big = 1.  Rows 0, 1 split (children of 1 / 1.6 stay); row 2: m == t_big
    # stays (the rule is >); row 3 splits and its children of e / 1.6 > 1 go; a negative max_screen_size removes everything
    ws, code, counts = c_plan(P, S, N, dr.ALL, _t(accum), _t(denom), P, _t(scaling), _t(opacity), 20, max_grad=0.25, min_opacity=0.5, extent=10.0)
    assert code.cpu().tolist() == [4, 4, 1, 0, 1] and counts == (2, 0, 2, 6)
    ws, code, counts = c_plan(P, S, N, dr.ALL, _t(accum), _t(denom), P, _t(scaling), _t(opacity), -1, max_grad=0.25, min_opacity=0.5, extent=100.0)
    assert code.cpu().tolist() == [0] * P and counts == (0, 0, 0, 0)


# ---- the model --------------------------------------------------------------------------------------------------------------
def build_model(params, moments=None, step=None, aux=None, ids_on_device=False, optimizer=True):
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
        m.optimizer = torch.optim.Adam([dict(params=[getattr(m, FIELDS[n])], lr=1e-4 * (k + 1), name=n) for k, n in enumerate(NAMES)],
                                       lr=0.0, eps=1e-15)
        if moments is not None:
            for n in NAMES:
                m.optimizer.state[getattr(m, FIELDS[n])] = dict(step=torch.tensor(float(step)),
                                                                exp_avg=torch.as_tensor(moments[n][0], device=dev).clone(),
                                                                exp_avg_sq=torch.as_tensor(moments[n][1], device=dev).clone())
    return m


def golden_model(rec, **kw):
    return build_model({n: rec["in_" + n] for n in NAMES}, {n: (rec["in_exp_avg_" + n], rec["in_exp_avg_sq_" + n]) for n in NAMES},
                       step=rec["in_step_xyz"], aux={a: rec["in_" + a] for a in dr.AUX}, **kw)


def adam_step(m, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    for n in NAMES:
        p = getattr(m, FIELDS[n])
        p.grad = torch.randn(p.shape, generator=gen).to(p.device)
    m.optimizer.step()


def _torch_append(m, new, id_rows):
    """New rows behind every parameter, zero moments behind every Adam moment, zeroed statistics, the parents' ids."""
    import torch
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        st = m.optimizer.state.pop(p, None)
        grown = torch.cat((p.detach(), new[group["name"]]), dim=0).requires_grad_(True)
        if st is not None:
            for key in ("exp_avg", "exp_avg_sq"):
                st[key] = torch.cat((st[key], torch.zeros_like(new[group["name"]])), dim=0)
            m.optimizer.state[grown] = st
        group["params"][0] = grown
        setattr(m, FIELDS[group["name"]], grown)
    n, dev = m._xyz.shape[0], m._xyz.device
    m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.zeros((n, 1), device=dev), torch.zeros((n, 1), device=dev), torch.zeros((n,), device=dev)
    for a in ("unique_kfIDs", "n_obs"):
        t = getattr(m, a)
        setattr(m, a, torch.cat((t, t[id_rows.to(t.device)])).int())


def _torch_prune(m, mask):
    keep = ~mask
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        st = m.optimizer.state.pop(p, None)
        new = p.detach()[keep].requires_grad_(True)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]
            m.optimizer.state[new] = st
        group["params"][0] = new
        setattr(m, FIELDS[group["name"]], new)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = m.xyz_gradient_accum[keep], m.denom[keep], m.max_radii2D[keep]
    m.unique_kfIDs = m.unique_kfIDs[keep.to(m.unique_kfIDs.device)]
    m.n_obs = m.n_obs[keep.to(m.n_obs.device)]


def torch_densify_and_prune(m, max_grad, min_opacity, extent, max_screen_size, noise, N=2):
    """The reference's statement (gaussian_model.py:599-765) in torch on the overlay model's tensors, the normal draws taken from
    noise [N,P,3] by source row."""
    import torch
    from gaussian_splatting.utils.general_utils import build_rotation
    with torch.no_grad():
        P = m._xyz.shape[0]
        grads = m.xyz_gradient_accum / m.denom
        grads[grads.isnan()] = 0.0
        sel = (torch.norm(grads, dim=-1) >= max_grad) & (m.get_scaling.max(dim=1).values <= m.percent_dense * extent)
        _torch_append(m, {n: getattr(m, FIELDS[n]).detach()[sel] for n in NAMES}, sel)
        padded = torch.zeros(m._xyz.shape[0], device=m._xyz.device)
        padded[:P] = grads.squeeze()
        sel = (padded >= max_grad) & (m.get_scaling.max(dim=1).values > m.percent_dense * extent)
        assert not bool(sel[P:].any())
        stds = m.get_scaling[sel].repeat(N, 1)
        samples = stds * noise[:, sel[:P]].reshape(-1, 3)
        rots = build_rotation(m._rotation[sel]).repeat(N, 1, 1)
        new = {n: getattr(m, FIELDS[n]).detach()[sel].repeat(N, *([1] * (getattr(m, FIELDS[n]).dim() - 1))) for n in NAMES}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + m._xyz[sel].repeat(N, 1)
        new["scaling"] = torch.log(m.get_scaling[sel].repeat(N, 1) / (0.8 * N))
        _torch_append(m, new, sel.nonzero().squeeze(1).repeat(N))
        _torch_prune(m, torch.cat((sel, torch.zeros(N * int(sel.sum()), dtype=torch.bool, device=sel.device))))
        gone = (m.get_opacity < min_opacity).squeeze(1)
        if max_screen_size:
            gone = gone | (m.max_radii2D > max_screen_size) | (m.get_scaling.max(dim=1).values > 0.1 * extent)
        _torch_prune(m, gone)


def assert_model_matches(m, want, bounds, tag, prefix="out_"):
    """The model against arrays name -> value (fp64 where computed): copied rows bit for bit, children within the bounds."""
    import torch
    for n in NAMES:
        p = getattr(m, FIELDS[n])
        assert p.is_leaf and p.requires_grad and [g for g in m.optimizer.param_groups if g["name"] == n][0]["params"][0] is p, (tag, n)
        got = p.detach().cpu().numpy()
        w = want[prefix + n]
        assert got.shape == w.shape, (tag, n, got.shape, w.shape)
        b = bounds.get(n)
        if b is None:
            assert np.array_equal(dr.bits(got), dr.bits(np.asarray(w, np.float32))), (tag, n)
        else:
            copied = b == 0
            assert np.array_equal(dr.bits(got)[copied], dr.bits(np.asarray(w, np.float32))[copied]), (tag, n)
            if (~copied).any():
                ratio = np.abs(got.astype(np.float64) - w)[~copied] / b[~copied]
                note("model_" + n, ratio.max())
                assert (ratio <= 1.0).all(), (tag, n, float(ratio.max()))


@pytest.mark.parametrize("ids_on_device", [False, True])
@pytest.mark.parametrize("name", ["aniso", "iso", "aniso_size", "iso_size", "children_pruned", "nothing", "ties"])
def test_model_reproduces_the_reference_golden(golden_dir, name, ids_on_device):
    """The goldens through the device model with their noise handed in: against the restatement, against the reference's record,
    and against a twin densified by the torch statement; then one more Adam step on both."""
    import torch
    rec = dr.case(np.load(os.path.join(golden_dir, "densify_prune_P150.npz")), name)
    size = float(rec["max_screen_size"]) or None
    args = (float(rec["max_grad"]), float(rec["min_opacity"]), float(rec["extent"]), size)
    a, b = golden_model(rec, ids_on_device=ids_on_device), golden_model(rec, ids_on_device=ids_on_device)
    noise = _t(rec["z"])
    seed0 = a.seed
    plan = a.densify_and_prune(*args, noise=noise)
    torch_densify_and_prune(b, *args, noise)
    out = dr.densify(rec)
    assert a.seed == seed0 and plan.counts[3] == len(out["src"]) == rec["out_xyz"].shape[0] and plan.launches == (2 if plan.counts[2] else 1)
    assert np.array_equal(plan.source_rows().cpu().numpy(), out["src"].astype(np.int32))
    bounds = {"xyz": out["bound_xyz"], "scaling": out["bound_scaling"]}
    assert_model_matches(a, out, bounds, name + " restated")
    copied = out["kind"] < 2
    for n in NAMES:  # the reference's record: copied rows bit for bit, its fp32 children within twice the bound of ours
        got, ref = getattr(a, FIELDS[n]).detach().cpu().numpy(), rec["out_" + n]
        assert np.array_equal(dr.bits(got)[copied], dr.bits(ref)[copied]), n
        if n in bounds and (~copied).any():
            assert (np.abs(got.astype(np.float64) - ref)[~copied] <= 2 * bounds[n][~copied]).all(), n
        st = a.optimizer.state[getattr(a, FIELDS[n])]
        for key in ("exp_avg", "exp_avg_sq"):
            assert same_bits(st[key].cpu(), torch.as_tensor(rec["out_%s_%s" % (key, n)])), (key, n)
        assert float(st["step"]) == float(rec["out_step_" + n]) == 3.0 and sorted(st) == ["exp_avg", "exp_avg_sq", "step"]
    assert len(a.optimizer.state) == 6
    for x in dr.AUX:
        got = getattr(a, x)
        assert got.device.type == ("cuda" if x not in ("unique_kfIDs", "n_obs") or ids_on_device else "cpu"), x
        assert same_bits(got.cpu(), torch.as_tensor(rec["out_" + x])), x

    def against_twin(tag):
        for n in NAMES:
            pa, pb = getattr(a, FIELDS[n]).detach(), getattr(b, FIELDS[n]).detach()
            assert pa.shape == pb.shape, (tag, n)
            c = torch.as_tensor(copied, device=pa.device)
            assert torch.equal(_i32(pa[c]), _i32(pb[c])), (tag, n)
            if n in bounds and (~copied).any():  # both sides are fp32: each within its bound of the fp64 value, one ulp each for the step
                slack = 2 * bounds[n][~copied] + 2 * dr.EPS * np.abs(pb[~c].cpu().numpy())
                assert (np.abs(pa[~c].cpu().numpy().astype(np.float64) - pb[~c].cpu().numpy()) <= slack).all(), (tag, n)
            elif (~copied).any():
                assert torch.equal(_i32(pa), _i32(pb)), (tag, n)
            sa, sb = a.optimizer.state[getattr(a, FIELDS[n])], b.optimizer.state[getattr(b, FIELDS[n])]
            assert float(sa["step"]) == float(sb["step"]), (tag, n)
            assert same_bits(sa["exp_avg"], sb["exp_avg"]) and same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), (tag, n)
        for x in dr.AUX:
            assert same_bits(getattr(a, x).cpu(), getattr(b, x).cpu()), (tag, x)

    against_twin(name)
    if plan.counts[3]:
        for m in (a, b):
            adam_step(m, seed=99)
        against_twin(name + " one more step")
        assert float(a.optimizer.state[a._xyz]["step"]) == 4.0


def _random_model(P, seed, S=3, f_rest_cols=3, optimizer=True):
    inp = make_inputs(P, S, 2, "random", seed)
    rng = np.random.default_rng(seed)
    params = dict(xyz=rng.normal(size=(P, 3)).astype(np.float32), f_dc=rng.normal(size=(P, 1, 3)).astype(np.float32),
                  f_rest=rng.normal(size=(P, f_rest_cols, 3)).astype(np.float32), opacity=inp["opacity"], scaling=inp["scaling"],
                  rotation=rng.normal(size=(P, 4)).astype(np.float32))
    aux = dict(xyz_gradient_accum=inp["accum"], denom=inp["denom"], max_radii2D=rng.integers(0, 30, P).astype(np.float32),
               unique_kfIDs=rng.integers(0, 9, P).astype(np.int32), n_obs=rng.integers(0, 6, P).astype(np.int32))
    m = build_model(params, aux=aux, optimizer=optimizer)
    if optimizer:
        adam_step(m, seed)
        with_stats = _t(inp["accum"]), _t(inp["denom"])
        m.xyz_gradient_accum, m.denom = with_stats
    return m, inp


@pytest.mark.parametrize("kind", ["no_optimizer", "counts_given", "nothing_left", "sh_degree_0", "clone_then_split", "wrong_group"])
def test_model_variants(kind):
    import torch
    from gsaj import _lib
    P = 1000
    a, inp = _random_model(P, 5, optimizer=kind != "no_optimizer", f_rest_cols=0 if kind == "sh_degree_0" else 3)
    b, _ = _random_model(P, 5, optimizer=kind != "no_optimizer", f_rest_cols=0 if kind == "sh_degree_0" else 3)
    th = dr.thresholds(MAX_GRAD, MIN_OPACITY, EXTENT, 20, PERCENT_DENSE, 2)
    sc0, op0 = a._scaling.detach().cpu().numpy(), a._opacity.detach().cpu().numpy()
    code = dr.classify(inp["accum"], inp["denom"], sc0, op0, th, 2)
    src, kindv = dr.order(code, 2)
    if kind == "wrong_group":
        a.optimizer.param_groups[2]["params"][0] = torch.zeros(P, 3, 3, device=_dev(), requires_grad=True)
        with pytest.raises(_lib.GsajError):
            a.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, seed=1)
        return
    if kind == "nothing_left":
        plan = a.densify_and_prune(MAX_GRAD, 1.5, EXTENT, 20, seed=1)  # no opacity reaches 1.5
        assert plan.counts == (0, 0, 0, 0) and plan.launches == 0
        assert tuple(a._features_rest.shape) == (0, 3, 3) and tuple(a.max_radii2D.shape) == (0,) and tuple(a.n_obs.shape) == (0,)
        assert tuple(a.optimizer.state[a._xyz]["exp_avg"].shape) == (0, 3) and a._xyz.requires_grad
        return
    if kind == "clone_then_split":  # the reference's two public methods, one after the other, as densify_and_prune calls them
        with np.errstate(all="ignore"):
            g = (inp["accum"] / inp["denom"]).astype(np.float32)
        g[np.isnan(g)] = 0
        g_t = _t(g)
        seed0 = a.seed
        p1 = a.densify_and_clone(g_t, MAX_GRAD, EXTENT)
        p2 = a.densify_and_split(g_t, MAX_GRAD, EXTENT)
        assert a.seed == seed0 + 1
        c = dr.classify(g, None, sc0, op0, th, 2, stages=dr.CLONE | dr.SPLIT)
        s2, k2 = dr.order(c, 2)
        assert p1.counts[:3] == (P, int((c & 2 != 0).sum()), 0) and p2.counts[2] == int((c & 4 != 0).sum())
        assert a._xyz.shape[0] == len(s2)
        cp = _t(k2 < 2)
        assert torch.equal(_i32(a._rotation.detach()), _i32(b._rotation.detach()[_t(s2)]))
        assert torch.equal(_i32(a._xyz.detach()[cp]), _i32(b._xyz.detach()[_t(s2)][cp]))
        assert np.array_equal(a.unique_kfIDs.numpy(), b.unique_kfIDs.numpy()[s2]) and not a.denom.any()
        return
    reads = []
    if kind == "counts_given":
        lib = _lib.load()
        real = lib.gsaj_densify_counts
        n0, n1, n2 = (int((code & bit != 0).sum()) for bit in (1, 2, 4))
        try:
            lib.gsaj_densify_counts = lambda *args: reads.append(args) or real(*args)
            plan = a.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, seed=7, counts=(n0, n1, n2, n0 + n1 + 2 * n2))
        finally:
            lib.gsaj_densify_counts = real
        assert reads == []
        with pytest.raises(_lib.GsajError):
            b.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, seed=7, counts=(n0, n1, n2, n0 + n1 + 2 * n2 + 1))
    else:
        plan = a.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, seed=7)
    assert plan.launches == 2 and plan.counts[3] == len(src) and a._xyz.shape[0] == len(src)
    src_t, cp = _t(src), _t(kindv < 2)
    for n in NAMES:
        pa, pb = getattr(a, FIELDS[n]).detach(), getattr(b, FIELDS[n]).detach()[src_t]
        assert pa.shape == pb.shape and pa.dtype == pb.dtype, (kind, n)
        if n in ("xyz", "scaling"):
            assert torch.equal(_i32(pa[cp]), _i32(pb[cp])), (kind, n)
        else:
            assert torch.equal(_i32(pa), _i32(pb)), (kind, n)
        if a.optimizer is not None:
            sa, sb = a.optimizer.state[getattr(a, FIELDS[n])], b.optimizer.state[getattr(b, FIELDS[n])]
            for key in ("exp_avg", "exp_avg_sq"):
                w = sb[key][src_t].clone()
                w[_t(kindv > 0)] = 0
                assert same_bits(sa[key], w), (kind, n, key)
    if kind == "sh_degree_0":
        assert tuple(a._features_rest.shape) == (len(src), 0, 3) and a._features_rest.requires_grad
    assert not a.xyz_gradient_accum.any() and not a.denom.any() and not a.max_radii2D.any() and tuple(a.denom.shape) == (len(src), 1)
    assert np.array_equal(a.n_obs.numpy(), b.n_obs.numpy()[src]) and a.n_obs.dtype == torch.int32


# ---- the generated noise --------------------------------------------------------------------------------------------------------
def test_generated_noise():
    import torch
    from gsaj.densify import DensifyPlan, densify_noise
    P, N, seed = 3000, 4, 0x9E3779B97F4A7C15
    z = densify_noise(P, N, seed)
    want, r = dr.normals(P, N, seed)
    ratio = np.abs(z.cpu().numpy().astype(np.float64) - want) / (32 * dr.EPS * (1 + r))
    note("z", ratio.max())
    assert tuple(z.shape) == (N, P, 3) and (ratio <= 1.0).all(), float(ratio.max())
    assert torch.equal(_i32(z), _i32(densify_noise(P, N, seed))) and not torch.equal(_i32(z), _i32(densify_noise(P, N, seed + 1)))
    assert not torch.equal(_i32(z), _i32(densify_noise(P, N, seed ^ (1 << 40))))  # the high word of the seed is in the key
    for P2 in (1, 257, 2999):  # row i's draws do not depend on P (nor on where the row sits in a workgroup's grid)
        assert torch.equal(_i32(densify_noise(P2, N, seed)), _i32(z[:, :P2].contiguous()))
    assert torch.equal(_i32(densify_noise(P, 2, seed)), _i32(z[:2].contiguous()))

    # children drawn inside the kernel == children computed from that noise handed back in, bit for bit
    inp = make_inputs(P, 3, N, "random", seed=77)
    rng = np.random.default_rng(78)
    xyz, rot = _t(rng.normal(size=(P, 3)).astype(np.float32)), _t(rng.normal(size=(P, 4)).astype(np.float32))
    sc = _t(inp["scaling"])
    plan = DensifyPlan(_t(inp["accum"]), _t(inp["denom"]), sc, _t(inp["opacity"]), MAX_GRAD, MIN_OPACITY, EXTENT, 20, N=N)
    outs = []
    for kw in (dict(seed=seed), dict(noise=z), dict(seed=seed), dict(seed=seed + 1)):
        dx, ds = plan.apply([xyz, sc])
        plan.children(xyz, sc, rot, dx, ds, **kw)
        outs.append((dx, ds))
    assert plan.counts[2] > 100
    assert torch.equal(_i32(outs[0][0]), _i32(outs[1][0])) and torch.equal(_i32(outs[0][1]), _i32(outs[1][1]))
    assert torch.equal(_i32(outs[0][0]), _i32(outs[2][0])) and not torch.equal(_i32(outs[0][0]), _i32(outs[3][0]))
    assert torch.equal(_i32(outs[0][1]), _i32(outs[3][1]))  # the log-scales take no noise


# ---- the covisibility window ------------------------------------------------------------------------------------------------
def test_covisibility_densify_plan_equals_the_torch_statement():
    import torch
    from gsaj import _lib
    from gsaj.covisibility import CovisibilityWindow
    P, dev = 1000, _dev()
    a, inp = _random_model(P, 9)
    cw = CovisibilityWindow(P, dev)
    nt = torch.as_tensor((np.random.default_rng(10).uniform(size=(4, P)) < 0.5).astype(np.int32), device=dev)
    cw.set_window([12, 9, 6, 3], nt)
    words = cw.words.clone()
    plan = a.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, seed=3)
    cw.densify_plan(plan)
    th = dr.thresholds(MAX_GRAD, MIN_OPACITY, EXTENT, 20, PERCENT_DENSE, 2)
    code = dr.classify(inp["accum"], inp["denom"], inp["scaling"], inp["opacity"], th, 2)
    kept = _t(code & 1 != 0)
    want = torch.cat((words[kept], torch.zeros(plan.counts[3] - int(kept.sum()), dtype=words.dtype, device=dev)))
    assert cw.P == plan.counts[3] == a._xyz.shape[0] and torch.equal(cw.words, want) and cw.words.dtype == words.dtype
    assert cw.to_prune.numel() == cw.P and cw.n_obs.numel() == cw.P
    assert cw.counts(kf_id=12)[1] == int(((want >> cw.slot_of[12]) & 1).sum())
    with pytest.raises(_lib.GsajError):
        cw.densify_plan(plan)  # a plan of the old size


# ---- through the rasteriser -------------------------------------------------------------------------------------------------
def test_densified_model_renders_and_differs_only_where_rows_changed():
    """The footprint of a set of rows is where rendering them alone leaves any opacity.  Outside the footprint of the parent's
    changed rows (cloned, split, pruned) and of the new rows, the densified model's image is the parent's, bit for bit."""
    import torch
    from gaussian_splatting.gaussian_renderer import render
    from gaussian_splatting.scene.gaussian_model import GaussianModel
    from utils.camera_utils import Camera

    cam, sc, deg = hp.make("p2000_160x120")
    dev = "cuda:0"
    P = sc["means3D"].shape[0]
    mk = lambda: GaussianModel.from_activated(sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["shs"],  # noqa: E731
                                              sh_degree=deg, device=dev)
    a, b = mk(), mk()
    view = Camera.from_synthetic(cam, device=dev)

    class Pipe:
        convert_SHs_python = False
        compute_cov3D_python = False

    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    with torch.no_grad():
        rb = render(view, b, Pipe, bg)
    radii = rb["radii"].cpu().numpy()
    vis = np.flatnonzero(radii > 0)
    chosen = vis[np.argsort(radii[vis], kind="stable")[:12]]  # the smallest footprints: half will be cloned, half split
    big = np.exp(b._scaling.detach().cpu().numpy().astype(np.float64)).max(axis=1)
    extent = float(np.sort(big[chosen])[5] + np.sort(big[chosen])[6]) / 2 / 0.01  # t_dense between the 6th and the 7th
    accum = np.zeros((P, 1), np.float32)
    accum[chosen] = 1.0
    a.xyz_gradient_accum, a.denom, a.max_radii2D = _t(accum), torch.ones(P, 1, device=dev), torch.zeros(P, device=dev)
    plan = a.densify_and_prune(0.5, 0.0, extent, None, seed=11)
    n0, n1, n2, n_out = plan.counts
    assert n1 >= 1 and n2 >= 1 and n1 + n2 == 12 and n0 == P - n2 and n_out == P + n1 + n2
    with torch.no_grad():
        ra = render(view, a, Pipe, bg)
        old_rows = torch.zeros(P, dtype=torch.bool, device=dev)
        old_rows[_t(chosen)] = True
        new_rows = torch.zeros(n_out, dtype=torch.bool, device=dev)
        new_rows[n0:] = True
        foot = (render(view, b, Pipe, bg, mask=old_rows)["opacity"] > 0) | (render(view, a, Pipe, bg, mask=new_rows)["opacity"] > 0)
    foot = foot.reshape(foot.shape[-2:])
    assert int((ra["radii"] > 0).sum()) > 0 and 0 < int(foot.sum()) < foot.numel() // 2
    for key in ("render", "depth", "opacity"):
        ia, ib = ra[key], rb[key]
        outside = (~foot).expand_as(ia)
        assert torch.equal(ia[outside].view(torch.int32), ib[outside].view(torch.int32)), key
    assert not torch.equal(ra["render"], rb["render"])
    assert torch.equal(ra["radii"][:n0], rb["radii"][_t(dr.order(plan.code.cpu().numpy(), 2)[0][:n0])])
