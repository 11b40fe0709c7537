"""The workgroup-count ladder of the five kernels that end with the last-workgroup hand-off (csrc/last_block.h), their inputs A and B,
the comparators, and the two wrong sums a broken hand-off would give.  TEST INFRASTRUCTURE ONLY; shared by
tests/test_gpu_last_block.py (the device, A then B then A on one workspace) and tests/test_cpu_last_block.py (the comparators reject a
partial that is left out and a partial that comes from B, at every rung).

G = number of workgroups: 1 (the arriver is itself last), 2, 256 (one full trip of the last workgroup's 256-wide load loop), 257 and
513 (one and two trips with a ragged end).  k_isotropic's tail has no strided loop: 1, 2, 257.  k_ssim_fwd's loop runs per image over
that image's workgroups: 1, 2, 288, 765, and 288 per image at N = 2.

A and B are CLEARLY different, so that one workgroup's partial of B inside the sum for A stands out at the bounds the suite already
has: B has another exposure (loss), scales 64 x larger (isotropic), a far worse reconstruction (SSIM), another extent (bounding box) and
other rows (dL/dtau).  No bound here is new except the one of dL/dtau, derived at assert_tau_sum."""
import functools

import numpy as np

import loss_restated as lr
import ssim_restated as sr
from test_gpu_ssim import map_bound  # the bound of tests/test_gpu_ssim.py, not a copy

F = np.float32

# ---- k_loss_seeds: 1024 pixels per workgroup ------------------------------------------------------------------------------------------
LOSS_SIZES = ((32, 32), (33, 32), (512, 512), (512, 513), (1024, 513))   # (W, H): G = 1, 2, 256, 257, 513


def wrong_rungs(G):
    """The workgroups whose partial the wrong sums lose: the last and one from the middle."""
    return sorted({G - 1, G // 2})


@functools.lru_cache(maxsize=None)
def loss_frames(W, H):
    """(A, B): tracking frames with a mask and every planted gate; B with exposure b = -0.5, whose residuals are several times A's."""
    return (lr.make_frame(W, H, lr.TRACKING, True, 71, exposure="ab"), lr.make_frame(W, H, lr.TRACKING, True, 72, exposure="negb"))


def loss_wrong_scalars(A, B, k):
    """-> (dropped, stale): the five scalars of A with workgroup k's partial left out, and with B's partial of workgroup k in its place
    (every scalar is linear in the four sums, and A and B share alpha and the image size)."""
    a_drop = lr.restate_frame(A, mutant="drop_partial", drop=k)["value"]
    b_drop = lr.restate_frame(B, mutant="drop_partial", drop=k)["value"]
    b_full = B["want"]["value"]
    return ({s: a_drop[s] for s in lr.SCALARS}, {s: a_drop[s] + (b_full[s] - b_drop[s]) for s in lr.SCALARS})


# ---- k_isotropic: 256 rows per workgroup ----------------------------------------------------------------------------------------------
ISO_P = (256, 257, 65537)   # G = 1, 2, 257
ISO_BLOCK = 256


@functools.lru_cache(maxsize=None)
def iso_cases(P):
    """(A, B), each dict(scales [P,3] fp32, want): log-uniform scales, B's 64 x larger.  A row with a component within lr.GUARD eps of
    the row's mean (where fp32 could see another sign) is replaced by (1, 2, 4) / 64, never skipped; the margin is asserted."""
    out = []
    for seed, mul in ((0, 1.0), (1, 64.0)):
        rng = np.random.default_rng(977 * P + seed)
        s = (mul * np.exp(rng.uniform(np.log(0.01), np.log(0.2), (P, 3)))).astype(F)
        w = lr.iso_restate(s, lr.ISO_WEIGHT)
        s[(w["abs_d"] < 2 * lr.GUARD * lr.EPS * w["mean"]).any(axis=1)] = mul * np.array([1, 2, 4], F) / F(64)
        want = lr.iso_restate(s, lr.ISO_WEIGHT)
        assert (want["abs_d"] >= lr.GUARD * lr.EPS * want["mean"]).all()
        s.setflags(write=False)
        out.append(dict(scales=s, want=want))
    return tuple(out)


def iso_partials(case):
    """Per-workgroup sums of |s - mean| (float64), and k: loss = k * their sum."""
    P, C = case["scales"].shape
    d = case["want"]["abs_d"].sum(axis=1)
    n = -(-P // ISO_BLOCK)
    return np.pad(d, (0, n * ISO_BLOCK - P)).reshape(n, ISO_BLOCK).sum(axis=1), float(F(lr.ISO_WEIGHT)) / (P * C)


def iso_wrong_losses(A, B, k):
    pa, ka = iso_partials(A)
    pb, _ = iso_partials(B)
    return ka * (pa.sum() - pa[k]), ka * (pa.sum() - pa[k] + pb[k])


# ---- k_ssim_fwd: one 32x16 tile of one plane per workgroup ----------------------------------------------------------------------------
SSIM_CASES = ((1, 1, 32, 16), (1, 1, 64, 16), (1, 3, 384, 128), (1, 3, 544, 240), (2, 3, 384, 128))   # (N, C, W, H): G per image 1, 2, 288, 765, 288
SSIM_TW, SSIM_TH = 32, 16


@functools.lru_cache(maxsize=None)
def ssim_pairs(N, C, W, H):
    """(A, B), each dict(x, y [N,C,H,W] fp32, S64, bound): textured images (no flat patch: the bound of tests/test_gpu_ssim.py grows
    like 1 / sigma^2) and a reconstruction with noise 0.03 (A) or 0.3 (B: a far lower SSIM)."""
    out = []
    for seed, noise in ((11, 0.03), (12, 0.3)):
        rng = np.random.default_rng(1000 * seed + 7 * W + H + N)
        x = np.clip(0.5 + 0.25 * rng.normal(size=(N, C, H, W)), 0, 1).astype(F)
        y = np.clip(x + noise * rng.normal(size=x.shape), 0, 1).astype(F)
        S64, parts = sr.ssim_forward(x, y)
        for a in (x, y, S64):
            a.setflags(write=False)
        out.append(dict(x=x, y=y, S64=S64, bound=map_bound(parts, S64)))
    return tuple(out)


def assert_ssim_means(out, case, tag):
    """out [N+1]: the per-image means and the mean over everything, each within the mean of the per-pixel bound (test_gpu_ssim.py)."""
    S64, bound = case["S64"], case["bound"]
    N = S64.shape[0]
    out = np.asarray(out, np.float64)
    for n in range(N):
        assert abs(out[n] - S64[n].mean()) <= bound[n].mean(), "%s: image %d: got %.9e want %.9e, bound %.3e" % (
            tag, n, out[n], S64[n].mean(), bound[n].mean())
    assert abs(out[N] - S64.mean()) <= bound.mean(), "%s: mean: got %.9e want %.9e, bound %.3e" % (tag, out[N], S64.mean(), bound.mean())


def ssim_partials(case):
    """[N, workgroups per image] sums of S over each workgroup's tile (float64), in blockIdx order: plane, tile row, tile column."""
    S = case["S64"]
    N, C, H, W = S.shape
    gy, gx = -(-H // SSIM_TH), -(-W // SSIM_TW)
    Sp = np.zeros((N, C, gy * SSIM_TH, gx * SSIM_TW))
    Sp[:, :, :H, :W] = S
    return Sp.reshape(N, C, gy, SSIM_TH, gx, SSIM_TW).sum(axis=(3, 5)).reshape(N, C * gy * gx)


def ssim_out_from_partials(part, case):
    N, C, H, W = case["S64"].shape
    return np.concatenate([part.sum(axis=1) / (C * H * W), [part.sum() / (N * C * H * W)]])


# ---- k_knn_bbox: 256 points per workgroup ---------------------------------------------------------------------------------------------
KNN_N = (256, 257, 65536, 65537, 131073)   # G = 1, 2, 256, 257, 513
KNN_BLOCK = 256


@functools.lru_cache(maxsize=None)
def knn_points(n):
    """(A, B) [n,3] fp32.  The first point of the last workgroup is the maximum of every axis, the first point of the middle
    workgroup (where that is another one) the minimum: a box that lacks either workgroup's partial is another box.  B: another extent."""
    out = []
    G = -(-n // KNN_BLOCK)
    for seed, ext, far in ((21, 1.0, 5.0), (22, 3.0, 7.0)):
        p = np.random.default_rng(seed + n).uniform(-ext, ext, (n, 3)).astype(F)
        p[(G - 1) * KNN_BLOCK] = far
        if G // 2 != G - 1:
            p[(G // 2) * KNN_BLOCK] = -far
        p.setflags(write=False)
        out.append(p)
    return tuple(out)


def knn_box_partials(p):
    """[G,6] per-workgroup {min xyz, max xyz}, each including the origin as k_knn_bbox's do."""
    G = -(-p.shape[0] // KNN_BLOCK)
    return np.stack([np.concatenate([np.minimum(p[b * KNN_BLOCK:(b + 1) * KNN_BLOCK].min(axis=0), 0),
                                     np.maximum(p[b * KNN_BLOCK:(b + 1) * KNN_BLOCK].max(axis=0), 0)]) for b in range(G)]).astype(F)


def knn_box(partials):
    """The fold of the partials: exact, min and max do not depend on the order.  The last workgroup starts from the origin too."""
    return np.concatenate([np.minimum(partials[:, :3].min(axis=0), 0), np.maximum(partials[:, 3:].max(axis=0), 0)]).astype(F)


def _spread(x):
    x = x.astype(np.uint32)
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def knn_order(p, box):
    """(codes_sorted, idx_sorted) as k_knn_morton and the stable radix sort give them for this box: fp32 arithmetic, one rounding per
    operation as in the kernel, 10 bits per axis interleaved, ties in index order."""
    with np.errstate(all="ignore"):
        q = [((p[:, a] - box[a]) / (box[3 + a] - box[a])) * F(1023) for a in range(3)]
        assert all(v.dtype == F for v in q)
        c = [_spread(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64).clip(0, 2 ** 32 - 1)) for v in q]
    codes = (c[0] | (c[1] << 1) | (c[2] << 2)).astype(np.int64)
    idx = np.argsort(codes, kind="stable")
    return codes[idx], idx.astype(np.int64)


def assert_knn_order(codes, idx, p, box, tag):
    """The brute-force order check of tests/test_gpu_knn.py (ascending codes, a permutation, ties in index order), made exact: the
    codes are the ones of THIS box."""
    codes, idx = np.asarray(codes).astype(np.int64), np.asarray(idx).astype(np.int64)
    n = p.shape[0]
    assert (np.diff(codes) >= 0).all() and np.array_equal(np.sort(idx), np.arange(n)), tag
    assert (np.diff(idx)[np.diff(codes) == 0] > 0).all(), tag
    wc, wi = knn_order(p, box)
    bad = np.flatnonzero(codes != wc)
    assert bad.size == 0, "%s: %d of %d codes are not the ones of the points' bounding box (first at %d)" % (
        tag, bad.size, n, int(bad[0]) if bad.size else -1)
    assert np.array_equal(idx, wi), tag


# ---- k_gaussian_bwd: 64 Gaussians per workgroup (one wave) ----------------------------------------------------------------------------
BWD_P = (64, 65, 16384, 16385, 32769)   # G = 1, 2, 256, 257, 513
BWD_BLOCK = 64
BWD_W, BWD_H = 64, 48


def assert_tau_sum(tau_sum, tau, tag):
    """dL_dtau_sum [6] against the float64 column sums of the same call's dL_dtau [P,6].  Bound 7 x 2^-24 x sum|column|: a row's value
    passes six fp32 additions of the wave butterfly and the final rounding to fp32; the sums over workgroups are fp64, whose own
    rounding is far below that."""
    t = np.asarray(tau, np.float64)
    got, want, mass = np.asarray(tau_sum, np.float64), t.sum(axis=0), np.abs(t).sum(axis=0)
    assert got.shape == (6,) and np.isfinite(got).all(), (tag, got)
    bound = 7 * 2.0 ** -24 * mass
    for k in range(6):
        print("%s: dL_dtau_sum[%d] got %.9e want %.9e err %.3e bound %.3e" % (tag, k, got[k], want[k], abs(got[k] - want[k]), bound[k]))
    bad = np.flatnonzero(np.abs(got - want) > bound)
    assert bad.size == 0, "%s: dL_dtau_sum%s: got %s want %s, bound %s" % (tag, bad, got[bad], want[bad], bound[bad])


@functools.lru_cache(maxsize=None)
def tau_rows(P):
    """(A, B) [P,6] fp32 stand-ins for dL/dtau rows on the CPU: A with a mean of its own per column, B four times larger."""
    rng = np.random.default_rng(31 + P)
    A = (rng.normal(size=(P, 6)) + np.array([1, -1, 2, -2, 0.5, -0.5])).astype(F)
    B = (4 * rng.normal(size=(P, 6)) - 3).astype(F)
    return A, B


def tau_partials(t):
    """[G,6]: a workgroup's partial as its wave forms it, the fp32 xor butterfly over its 64 rows (lane 0's result)."""
    P = t.shape[0]
    G = -(-P // BWD_BLOCK)
    v = np.zeros((G * BWD_BLOCK, 6), F)
    v[:P] = t
    v = v.reshape(G, BWD_BLOCK, 6)
    lane = np.arange(BWD_BLOCK)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    assert v.dtype == F
    return v[:, 0]
