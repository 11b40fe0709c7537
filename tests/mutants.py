"""Mutant outputs for the comparator canaries (tests/test_cpu_comparator_canaries.py): what a kernel with a given bug would
return, built on the CPU from the oracle, with the names and shapes of helpers.gpu_forward / gpu_backward (NumPy).

A forward output is a dict(color, depth, opacity, n_contrib, n_touched); a backward output is a 12-tuple in helpers.GRAD_NAMES
order.  Three ways to build one: state surgery (a changed copy of the oracle state through oracle.render / oracle.backward /
oracle.chain), linearity (the compositor sums are linear in the pixel seeds: a backward with the seeds masked to one tile is
that tile's share of every Gaussian) and the oracle's opt-in mutant walks (gsaj_oracle.c, MUTANT_*).  Every frame is rendered
as test_gpu_tiled.test_forward_and_backward_parity renders it (SH colours, helpers.PARITY_BG, the scene's scale modifier,
seeds helpers.seeds(cam, seed=1)); its control is what the MI355X returned for it (tests/golden/device_<scene>.npz)."""
import functools
import os

import numpy as np

import helpers as hp
from oracle import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MUTANT_LATE_STOP, MUTANT_NO_ALPHA_CLAMP, MUTANT_TOUCHED_NO_CUTOFF, MUTANT_DG_ZERO_CLAMPED = 1, 2, 3, 4  # gsaj_oracle.c
CHAIN_IN = ("dL_dmean2D", "dL_dconic", "dL_dcolor", "dL_ddepth")


class Frame:
    """One scene of helpers.SCENES through the oracle: state, outputs, seeds, the oracle's backward with its error model."""

    def __init__(self, name, bg=hp.PARITY_BG, record_bits=32, shs=None, scene=None, seed=1):
        """scene=(cam, scene, SH degree) with scale modifier 1 instead of helpers.SCENES[name]; seed: of helpers.seeds."""
        self.name = name
        if scene is None:
            (self.cam, self.sc, self.deg), self.mod = hp.make(name), hp.scale_modifier(name)
        else:
            (self.cam, self.sc, self.deg), self.mod = scene, 1.0
        if shs is not None:
            self.sc = dict(self.sc, shs=shs(self.sc["shs"]))
        self.bg = np.asarray(bg, np.float32)
        (self.ref, self.st), _ = hp.oracle_forward(self.cam, self.sc, self.deg, bg=bg, record_bits=record_bits, scale_modifier=self.mod)
        self.praw = self.cam["projmatrix_raw"]
        self.dLc, self.dLd = hp.seeds(self.cam, seed=seed)
        self.gref = orc.backward(self.st, self.dLc, self.dLd, self.praw)
        self.gref["error_model"] = orc.error_model(self.st, self.dLc, self.dLd, hp.BORDER_REL, hp.BORDER_REL_T)
        self.P = self.st["P"]
        self.clean = self.gref["error_model"]["flip_budget"].max(axis=1) == 0
        self.visible = self.ref["radii"] > 0
        self._shares = None  # tile_shares(self)

    def fwd(self):
        return dict(color=self.ref["color"], depth=self.ref["depth"], opacity=self.ref["opacity"], n_contrib=self.st["n_contrib"],
                    n_touched=self.ref["n_touched"])

    def grads(self, g=None):
        g = self.gref if g is None else g
        return tuple(g[nm] for nm in hp.GRAD_NAMES)

    def bound10(self):
        """(A)'s per-Gaussian, per-component bound (the arithmetic of helpers.assert_grads_close)."""
        em = self.gref["error_model"]
        want = hp.compositor_sums(self.gref, self.P)
        return (hp.MASS_TOL * em["term_mass"] + hp.COND_K * em["cond_slack"] + hp.FLIP_K * em["flip_budget"]
                + 1e-9 * np.abs(want).max(axis=0, keepdims=True) + 1e-37)


@functools.lru_cache(maxsize=None)
def frame(name):
    """A frame of test_gpu_tiled.test_forward_and_backward_parity[name-False], or, for "random/<id>", of
    test_gpu_random.test_random_scene_parity[<id>] (its background, its seeds)."""
    if name.startswith("random/"):
        import test_gpu_random as tr

        case = dict(zip(tr.CASE_IDS, tr.CASES))[name[len("random/"):]]
        return Frame(name, bg=tr.RANDOM_BG, scene=tr.random_case_scene(case), seed=case[3])
    return Frame(name)


def device(name):
    """The recorded device outputs of `name`: (forward dict, 12-tuple of gradients)."""
    d = np.load(os.path.join(GOLDEN, "device_%s.npz" % name))
    fwd = dict(color=d["color"], depth=d["depth"], opacity=d["opacity"], n_contrib=d["n_contrib"].astype(np.uint32),
               n_touched=d["n_touched"], radii=d["radii"], num_rendered=int(d["num_rendered"]))
    return fwd, tuple(d[nm] if nm in d.files else None for nm in hp.GRAD_NAMES)


# ---- the comparators, as the GPU parity tests call them ------------------------------------------------------------------------
def check_forward(fr, out, which=("image", "counts", "touched")):
    if "image" in which:
        for nm in ("color", "depth", "opacity"):
            hp.assert_image_close(out[nm].reshape(fr.ref[nm].shape), fr.ref[nm], hp.IMG_TOL, st=fr.st, tag="(image) %s" % nm)
    if "counts" in which:
        hp.assert_counts_close(out["n_contrib"], fr.st["n_contrib"], fr.st, tag="(counts)")
    if "touched" in which:
        hp.assert_touched_close(out["n_touched"], fr.ref["n_touched"], fr.st, tag="(touched)")


def check_backward(fr, g, layers=("A", "B", "C"), **kw):
    return hp.assert_grads_close(g, fr.gref, fr.name, st=fr.st, projmatrix_raw=fr.praw, layers=layers, **kw)


def image_margin(fr, out):
    """Worst image error over IMG_TOL at pixels the oracle's walk does not flag borderline (>= 1: the image check rejects)."""
    border = fr.gref["error_model"]["border_mask"]
    worst = 0.0
    for nm in ("color", "depth", "opacity"):
        want = fr.ref[nm].astype(np.float64)
        err = np.abs(out[nm].reshape(want.shape) - want) / (np.abs(want).max() + 1e-30)
        worst = max(worst, float(err.reshape(-1, *border.shape)[:, ~border].max(initial=0.0)) / hp.IMG_TOL)
    return worst


# ---- forward mutants -----------------------------------------------------------------------------------------------------------
def _render(fr, st, bg=None, mutant=0):
    img = orc.render(st, fr.bg if bg is None else bg, mutant=mutant)
    return dict(color=img["color"], depth=img["depth"], opacity=img["opacity"], n_contrib=img["n_contrib"], n_touched=img["n_touched"])


def f1_half_pixel(fr):
    st = dict(fr.st, means2D=(fr.st["means2D"] - np.float32(0.5)).astype(np.float32))
    return _render(fr, st)


def f2_late_stop(fr):
    return _render(fr, fr.st, mutant=MUTANT_LATE_STOP)


def f3_no_alpha_clamp(fr):
    return _render(fr, fr.st, mutant=MUTANT_NO_ALPHA_CLAMP)


def f4_no_background(fr):
    return _render(fr, fr.st, bg=np.zeros(3, np.float32))


def f5_ragged_column_lost(fr):
    out = {k: v.copy() for k, v in fr.fwd().items()}
    x0 = 16 * ((fr.st["W"] + 15) // 16 - 1)
    for k in ("color", "depth", "opacity"):
        out[k][..., x0:] = 0.0
    out["n_contrib"][:, x0:] = 0
    return out


def longest_tile(fr):
    r = fr.st["ranges"]
    return int(np.argmax(r[:, 1] - r[:, 0]))


def f6_list_short(fr):
    ranges = fr.st["ranges"].copy()
    ranges[longest_tile(fr), 1] -= 1
    return _render(fr, dict(fr.st, ranges=ranges))


def f7_touched_no_cutoff(fr):
    return _render(fr, fr.st, mutant=MUTANT_TOUCHED_NO_CUTOFF)


def f8_other_record_bits(fr, bits):
    """The same frame through the oracle's other record mode (16: fp16 rounding of conic, opacity and colour)."""
    other = Frame(fr.name, bg=fr.bg, record_bits=bits)
    return other, dict(other.fwd()), other.grads()


def f10_depth_half(fr):
    """Depths stored at half precision in the compositor's records (the fp16 record mode rounds conic, opacity and colour only)."""
    return _render(fr, dict(fr.st, depths=orc.round_to_half(fr.st["depths"])))


def f9_one_pixel(fr, k, px):
    out = {kk: v.copy() for kk, v in fr.fwd().items()}
    py_, px_ = px
    out["color"][0, py_, px_] += np.float32(k * hp.IMG_TOL * np.abs(fr.ref["color"]).max())
    return out


def f9_borderline_pixels(fr, pixels):
    out = {kk: v.copy() for kk, v in fr.fwd().items()}
    for py_, px_ in pixels:
        out["color"][0, py_, px_] += np.float32(0.5 * hp.IMG_FLIP_BOUND * np.abs(fr.ref["color"]).max())
    return out


# ---- backward mutants ----------------------------------------------------------------------------------------------------------
def with_sums(fr, g, st=None):
    """A full gradient dict from the compositor sums of `g` and the oracle's fp32 chain on them (what a device with those sums
    and a correct chain returns)."""
    g = {k: np.asarray(v) for k, v in g.items() if k != "error_model"}
    g.update(orc.chain(fr.st if st is None else st, *(g[k] for k in CHAIN_IN), fr.praw))
    return g


def _copy_sums(fr):
    return {k: fr.gref[k].copy() for k in CHAIN_IN + ("dL_dopacity",)}


def a1_conic_offdiag_x2(fr):
    s = _copy_sums(fr)
    s["dL_dconic"] = s["dL_dconic"].reshape(fr.P, 4)
    s["dL_dconic"][:, 1] *= 2
    s["dL_dconic"] = s["dL_dconic"].reshape(fr.P, 2, 2)
    return fr.grads(with_sums(fr, s))


def a2_no_background_term(fr):
    st = dict(fr.st, inputs=dict(fr.st["inputs"], bg=np.zeros(3, np.float32)))
    g = orc.backward(st, fr.dLc, fr.dLd, fr.praw)
    return fr.grads(g)


def a3_depth_seed_ignored(fr):
    return fr.grads(orc.backward(fr.st, fr.dLc, np.zeros_like(fr.dLd), fr.praw))


def a4_dG_zero_where_clamped(fr):
    return fr.grads(orc.backward(fr.st, fr.dLc, fr.dLd, fr.praw, mutant=MUTANT_DG_ZERO_CLAMPED))


def a5_walk_one_past(fr):
    r = fr.st["ranges"]
    W, H = fr.st["W"], fr.st["H"]
    gx = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * gx + xs // 16
    n_list = (r[:, 1] - r[:, 0])[tile]
    st = dict(fr.st, n_contrib=np.minimum(fr.st["n_contrib"].astype(np.int64) + 1, n_list).astype(np.uint32))
    return fr.grads(orc.backward(st, fr.dLc, fr.dLd, fr.praw))


def tile_shares(fr):
    """[tiles, P, 10]: every tile's share of every Gaussian's ten compositor sums in frame `fr` (a backward with the seeds masked
    to the tile), computed once per Frame."""
    if fr._shares is not None:
        return fr._shares
    W, H = fr.st["W"], fr.st["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    out = np.zeros((gx * gy, fr.P, 10))
    for t in range(gx * gy):
        m = np.zeros((H, W), np.float32)
        ty, tx = divmod(t, gx)
        m[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = 1.0
        g = orc.backward(fr.st, fr.dLc * m, fr.dLd * m, fr.praw)
        out[t] = hp.compositor_sums(g, fr.P)
    fr._shares = out
    return out


def lost_share_ratio(fr, gid):
    """Per tile: how far (A) is exceeded when tile t's share of Gaussian gid is lost (worst component, err / bound)."""
    return (np.abs(tile_shares(fr)[:, gid, :]) / fr.bound10()[gid]).max(axis=1)


def a6_lost_atomic(fr, gid, tile):
    s = _copy_sums(fr)
    share = tile_shares(fr)[tile, gid]
    s["dL_dmean2D"] = s["dL_dmean2D"].copy()
    s["dL_dmean2D"][gid, :2] -= share[0:2].astype(np.float32)
    cn = s["dL_dconic"].reshape(fr.P, 4).copy()
    cn[gid, [0, 1, 3]] -= share[2:5].astype(np.float32)
    s["dL_dconic"] = cn.reshape(fr.P, 2, 2)
    s["dL_dopacity"] = s["dL_dopacity"].copy()
    s["dL_dopacity"][gid, 0] -= np.float32(share[5])
    s["dL_dcolor"] = s["dL_dcolor"].copy()
    s["dL_dcolor"][gid] -= share[6:9].astype(np.float32)
    s["dL_ddepth"] = s["dL_ddepth"].copy()
    s["dL_ddepth"][gid, 0] -= np.float32(share[9])
    return fr.grads(with_sums(fr, s))


def a7_one_sum_off(fr, gid, comp, k):
    """Compositor sum `comp` (order of helpers.compositor_sums) of Gaussian gid moved by k times its own (A) bound."""
    s = _copy_sums(fr)
    d = k * fr.bound10()[gid, comp]
    if comp < 2:
        s["dL_dmean2D"] = s["dL_dmean2D"].copy()
        s["dL_dmean2D"][gid, comp] += d
    elif comp < 5:
        cn = s["dL_dconic"].reshape(fr.P, 4).copy()
        cn[gid, (0, 1, 3)[comp - 2]] += d
        s["dL_dconic"] = cn.reshape(fr.P, 2, 2)
    elif comp == 5:
        s["dL_dopacity"] = s["dL_dopacity"].copy()
        s["dL_dopacity"][gid, 0] += d
    elif comp < 9:
        s["dL_dcolor"] = s["dL_dcolor"].copy()
        s["dL_dcolor"][gid, comp - 6] += d
    else:
        s["dL_ddepth"] = s["dL_ddepth"].copy()
        s["dL_ddepth"][gid, 0] += d
    return fr.grads(with_sums(fr, s))


def _edit(g, **repl):
    g = list(g)
    for nm, f in repl.items():
        i = hp.GRAD_NAMES.index(nm)
        g[i] = f(np.array(g[i]))
    return tuple(g)


def b1_tau_halves_swapped(g):
    return _edit(g, dL_dtau=lambda x: x[:, [3, 4, 5, 0, 1, 2]], dL_dtau_sum=lambda x: x[[3, 4, 5, 0, 1, 2]])


def b1_tau_sign(g, comp):
    def flip_rows(x):
        x[:, comp] = -x[:, comp]
        return x

    def flip_sum(x):
        x[comp] = -x[comp]
        return x
    return _edit(g, dL_dtau=flip_rows, dL_dtau_sum=flip_sum)


def _chain_mutant(fr, st):
    return fr.grads(dict(fr.gref, **orc.chain(st, *(fr.gref[k] for k in CHAIN_IN), fr.praw)))


def b2_sh_clamp_ignored(fr):
    return _chain_mutant(fr, dict(fr.st, clamped=np.zeros_like(fr.st["clamped"])))


def b3_view_rotation_transposed(fr):
    vm = fr.st["inputs"]["viewmatrix"].reshape(4, 4).copy()
    vm[:3, :3] = vm[:3, :3].T.copy()
    return _chain_mutant(fr, dict(fr.st, inputs=dict(fr.st["inputs"], viewmatrix=np.ascontiguousarray(vm.reshape(16)))))


def b4_rows_exchanged(g, i, j):
    def swap(x):
        x[[i, j]] = x[[j, i]]
        return x
    return _edit(g, **{nm: swap for nm in hp.CHAIN_NAMES})


def b5_scale_modifier_ignored(fr):
    return _chain_mutant(fr, dict(fr.st, inputs=dict(fr.st["inputs"], scale_modifier=1.0)))


def b8_campos_half(fr):
    """The chain evaluates the SH basis with the camera position read at half precision (the view direction is slightly off)."""
    return _chain_mutant(fr, dict(fr.st, inputs=dict(fr.st["inputs"], campos=orc.round_to_half(fr.st["inputs"]["campos"]))))


def b9_scale_modifier_half(fr):
    """The chain reads the scale modifier at half precision (0.8 -> 0.7998)."""
    return _chain_mutant(fr, dict(fr.st, inputs=dict(fr.st["inputs"], scale_modifier=float(orc.round_to_half(fr.mod)))))


def b6_chain_on_half_sums(fr, g):
    """The per-Gaussian chain reads the compositor sums through a half-precision buffer (the sums reported stay fp32)."""
    g = dict(zip(hp.GRAD_NAMES, g))
    half = [orc.round_to_half(np.asarray(g[k], np.float32)) for k in CHAIN_IN]
    return fr.grads(dict(g, **orc.chain(fr.st, *half, fr.praw)))


def b7_one_row_off(fr, g, nm, gid, k):
    """Row gid of chain output nm moved by k times what (B) allows it (its largest component; the sums stay as they are)."""
    g = list(g)
    i = hp.GRAD_NAMES.index(nm)
    x = np.array(g[i], np.float64).reshape(fr.P, -1)
    truth, sens, noise32, _ = hp.chain_sensitivity(fr.st, tuple(np.asarray(g[hp.GRAD_NAMES.index(k)]) for k in CHAIN_IN), fr.praw)
    t = truth[nm].reshape(fr.P, -1)
    scale = np.maximum(np.abs(t).max(axis=1), hp.CHAIN_FLOOR * np.abs(t).max())
    allowed = np.maximum(np.maximum(hp.CHAIN_ROW_TOL * scale, hp.CHAIN_COND_K * sens[nm]), hp.CHAIN_K * noise32[nm])
    c = int(np.argmax(np.abs(t[gid])))
    x[gid] = t[gid]
    x[gid, c] += k * allowed[gid]
    g[i] = x.reshape(np.shape(g[i])).astype(np.float32)
    return tuple(g)


def uniform_colour(shs):
    """A map painted in one colour (tools/fuzz_uniform.py): SH DC only, the same for every Gaussian."""
    shs = np.zeros_like(shs)
    shs[:, 0, :] = np.array([0.7, -0.2, 0.4], np.float32)
    return shs
