"""NumPy restatement of the reference's densify_and_prune (gaussian_splatting/scene/gaussian_model.py:599-765: densify_and_clone,
densify_and_split, densification_postfix, cat_tensors_to_optimizer and the two prune_points) as ONE classification of the source
rows and one ordered emission, and of the counter-based normal generator of csrc/densify_prune.hip (Philox4x32-10, Box-Muller).
Decisions are taken on the fp32 inputs (the gradient quotient in fp32, which is exactly rounded everywhere; exp and sigmoid in
fp64, so fixtures keep a margin from every threshold); the children are computed in fp64.  MUTANTS lists deliberate mistakes the
golden must reject.  Shared by the CPU test and the GPU tests."""
import numpy as np

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
AUX = ("xyz_gradient_accum", "denom", "max_radii2D", "unique_kfIDs", "n_obs")
CLONE, SPLIT, PRUNE = 1, 2, 4
ALL = 7
EPS = 2.0 ** -24
MUTANTS = ("grad_gt", "clone_lt", "interleaved", "clones_last", "moments_copied", "stats_kept", "divisor_08", "children_exempt",
           "size_rule_always")


def case(z, name):
    """The arrays of one case of densify_prune_P150.npz without their prefix."""
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def cases(z):
    return sorted({k.split("/")[0] for k in z.files})


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize % 4 else a.view(np.int32)


def f32(x):
    return np.float32(x)


def thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense, N):
    """Formed in double, rounded to fp32 once."""
    size_rule = bool(max_screen_size)
    return dict(thr=f32(max_grad), t_d=f32(float(percent_dense) * float(extent)), t_b=f32(0.1 * float(extent)), min_o=f32(min_opacity),
                d=f32(0.8 * N), size_rule=size_rule, size_all=bool(size_rule and f32(0.0) > f32(max_screen_size)))


def quantities(accum, denom, scaling, opacity, N, n_grads=None):
    """g (fp32), m, child m, o (fp64 on the fp32 inputs) of every row."""
    P = scaling.shape[0]
    if denom is None:
        g = np.zeros(P, np.float32)
        g[:np.asarray(accum).size] = np.asarray(accum, np.float32).reshape(-1)
    else:
        with np.errstate(all="ignore"):
            g = (np.asarray(accum, np.float32).reshape(-1) / np.asarray(denom, np.float32).reshape(-1)).astype(np.float32)
        g[np.isnan(g)] = 0.0
    e = np.exp(scaling.astype(np.float64))
    m = e.max(axis=1)
    mc = np.exp(np.log(e / np.float64(f32(0.8 * N)))).max(axis=1)
    o = 1.0 / (1.0 + np.exp(-opacity.astype(np.float64).reshape(-1)))
    return g, m, mc, o


def classify(accum, denom, scaling, opacity, th, N, stages=ALL, mutant=None):
    """The code byte of every row: bit 0 original emitted, bit 1 clone, bit 2 children."""
    g, m, mc, o = quantities(accum, denom, scaling, opacity, N)
    ge = (lambda a, b: a > b) if mutant == "grad_gt" else (lambda a, b: a >= b)
    le = (lambda a, b: a < b) if mutant == "clone_lt" else (lambda a, b: a <= b)
    clone = ge(np.abs(g), th["thr"]) & le(m, th["t_d"]) if stages & CLONE else np.zeros(len(g), bool)
    split = ge(g, th["thr"]) & (m > th["t_d"]) if stages & SPLIT else np.zeros(len(g), bool)
    gone = np.zeros(len(g), bool)
    child_gone = np.zeros(len(g), bool)
    if stages & PRUNE:
        faint = o < th["min_o"]
        rule = th["size_rule"] or mutant == "size_rule_always"
        gone = faint | (rule & (th["size_all"] | (m > th["t_b"])))
        child_gone = faint | (rule & (th["size_all"] | (mc > th["t_b"])))
        if mutant == "children_exempt":
            child_gone[:] = False
    return ((~split & ~gone) * 1 + (clone & ~gone) * 2 + (split & ~child_gone) * 4).astype(np.uint8)


def order(code, N, mutant=None):
    """(source row, kind) of every output row; kind 0 original, 1 clone, 2 + n child of copy n."""
    rows = lambda bit: np.flatnonzero(code & bit)  # noqa: E731
    orig, clones, kids = rows(1), rows(2), rows(4)
    if mutant == "interleaved":
        ch = [(np.repeat(kids, N), np.tile(2 + np.arange(N), len(kids)))]
    else:
        ch = [(kids, np.full(len(kids), 2 + n)) for n in range(N)]
    segs = [(orig, np.zeros(len(orig), int))] + ([(clones, np.ones(len(clones), int))] if mutant != "clones_last" else []) + ch \
        + ([(clones, np.ones(len(clones), int))] if mutant == "clones_last" else [])
    return np.concatenate([s for s, _ in segs]).astype(np.int64), np.concatenate([k for _, k in segs]).astype(np.int64)


def rotation_matrices(q):
    q = q.astype(np.float64)
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def children(xyz, scaling, rotation, z, N, mutant=None):
    """fp64 children of EVERY source row and copy: (xyz [N,P,3], its bound, scaling [N,P,S], its bound).  z [N,P,3]."""
    e = np.exp(scaling.astype(np.float64))
    v = e[None, :, :] * z.astype(np.float64)          # [N,P,3] (S = 1 broadcasts)
    R = rotation_matrices(rotation)
    mu = xyz.astype(np.float64)
    cx = np.einsum("pcj,npj->npc", R, v) + mu[None]
    # 16 eps (|mu_c| + sum_j |R_cj| |v_j|) covers errors RELATIVE to each term.  An entry of R also carries an ABSOLUTE error that
    # does not shrink with the entry when 1 - 2 (y^2 + z^2) or x y - r z cancels: each normalised component is within 4 eps
    # (sum of four squares, sqrt, division), a product of two within 9 eps |ab|, a sum of two products within 10 eps (|ab| + |cd|)
    # with |ab| + |cd| <= 1, doubled, plus one eps for "1 -": at most 21 eps, taken as 24 eps, times |v_j|.  The reference's own
    # fp32 children need it (golden case "ties", row 35: R_22 = 0.06 against |v_2| = 24.6).
    bx = 16 * EPS * (np.abs(mu)[None] + np.einsum("pcj,npj->npc", np.abs(R), np.abs(v))) + 24 * EPS * np.abs(v).sum(axis=2)[:, :, None]
    d = np.float64(f32(0.8 if mutant == "divisor_08" else 0.8 * N))
    cs = np.broadcast_to(np.log(e / d)[None], (N,) + e.shape).copy()
    bs = 8 * EPS * np.maximum(1.0, np.abs(cs))
    return cx, bx, cs, bs


def densify(rec, N=2, stages=ALL, mutant=None, noise=None):
    """in_* of a record + its scalars -> out_* as the reference leaves them, the children in fp64, plus "src" / "kind" (the
    origin of every output row) and "bound_xyz" / "bound_scaling" (zero on copied rows)."""
    th = thresholds(float(rec["max_grad"]), float(rec["min_opacity"]), float(rec["extent"]), float(rec["max_screen_size"]),
                    float(rec["percent_dense"]), N)
    code = classify(rec["in_xyz_gradient_accum"], rec["in_denom"], rec["in_scaling"], rec["in_opacity"], th, N, stages, mutant)
    src, kind = order(code, N, mutant)
    new = kind > 0
    out = {"code": code, "src": src, "kind": kind}
    for n in NAMES:
        out["out_" + n] = rec["in_" + n][src]
        for pre in ("exp_avg_", "exp_avg_sq_"):
            if "in_" + pre + n in rec:
                v = rec["in_" + pre + n][src].copy()
                if mutant != "moments_copied":
                    v[new] = 0
                out["out_" + pre + n] = v
                out["out_step_" + n] = rec["in_step_" + n]
    z = rec["z"] if noise is None else noise
    cx, bx, cs, bs = children(rec["in_xyz"], rec["in_scaling"], rec["in_rotation"], z, N, mutant)
    out["out_xyz"] = out["out_xyz"].astype(np.float64)
    out["out_scaling"] = out["out_scaling"].astype(np.float64)
    out["bound_xyz"] = np.zeros_like(out["out_xyz"])
    out["bound_scaling"] = np.zeros_like(out["out_scaling"])
    ch = kind >= 2
    out["out_xyz"][ch], out["bound_xyz"][ch] = cx[kind[ch] - 2, src[ch]], bx[kind[ch] - 2, src[ch]]
    out["out_scaling"][ch], out["bound_scaling"][ch] = cs[kind[ch] - 2, src[ch]], bs[kind[ch] - 2, src[ch]]
    n = len(src)
    for a, shape in (("xyz_gradient_accum", (n, 1)), ("denom", (n, 1)), ("max_radii2D", (n,))):
        out["out_" + a] = rec["in_" + a][src].astype(np.float32).reshape(shape) if mutant == "stats_kept" else np.zeros(shape, np.float32)
    for a in ("unique_kfIDs", "n_obs"):
        out["out_" + a] = rec["in_" + a][src].astype(np.int32)
    return out


def mismatches(out, rec):
    """Names of the out_* arrays of the record the restated outcome does not reproduce: copied tensors bit for bit, the children
    within their bounds."""
    bad = []
    for k in sorted(k for k in rec if k.startswith("out_")):
        if k not in out or out[k].shape != rec[k].shape:
            bad.append(k)
        elif k in ("out_xyz", "out_scaling"):
            b = out["bound_" + k[4:]]
            copied = b == 0
            if not np.array_equal(bits(out[k].astype(np.float32))[copied], bits(rec[k])[copied]) or \
                    not (np.abs(out[k] - rec[k].astype(np.float64)) <= b)[~copied].all():
                bad.append(k)
        elif not np.array_equal(bits(np.asarray(out[k], rec[k].dtype)), bits(rec[k])):
            bad.append(k)
    return bad


# ---- Philox4x32-10 + Box-Muller -------------------------------------------------------------------------------------------
def philox4x32(counter, key, rounds=10):
    """counter [...,4], key [...,2] (uint32 values) -> [...,4] uint32."""
    c = [np.asarray(counter[..., k], np.uint64) for k in range(4)]
    k0, k1 = np.asarray(key[..., 0], np.uint64), np.asarray(key[..., 1], np.uint64)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=-1).astype(np.uint32)


def normals(P, N, seed, rows=None):
    """z [N,P,3] fp64 of the generator and the Box-Muller radius r [N,P,3] behind each component (for the bound 32 eps (1 + r))."""
    i = np.arange(P, dtype=np.uint64) if rows is None else np.asarray(rows, np.uint64)
    ctr = np.zeros((N, len(i), 4), np.uint64)
    ctr[..., 0] = i[None, :]
    ctr[..., 1] = np.arange(N, dtype=np.uint64)[:, None]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    x = philox4x32(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,))).astype(np.float64)
    u1a, u2a = (np.floor(x[..., 0] / 512) + 0.5) * 2.0 ** -23, np.floor(x[..., 1] / 256) * 2.0 ** -24
    u1b, u2b = (np.floor(x[..., 2] / 512) + 0.5) * 2.0 ** -23, np.floor(x[..., 3] / 256) * 2.0 ** -24
    ra, rb = np.sqrt(-2 * np.log(u1a)), np.sqrt(-2 * np.log(u1b))
    z = np.stack([ra * np.cos(2 * np.pi * u2a), ra * np.sin(2 * np.pi * u2a), rb * np.cos(2 * np.pi * u2b)], axis=-1)
    return z, np.stack([ra, ra, rb], axis=-1)
