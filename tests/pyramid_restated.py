"""NumPy restatements (float32, one rounding per operation) of csrc/pyramid.hip -- k_pyramid level by level, and k_gn_relevel on the
dict state of gn_restated.lm_new_state / gn8_restated.lm8_new_state -- with the comparator the GPU tests use and a `mutant=` switch
for the canaries.  TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_pyramid.py, tests/test_gpu_pyramid.py and
tests/test_gpu_gn_pyramid.py.

  pyramid               levels 1..L of (colour [3,H,W], depth [H,W] or None, mask [H,W] or None): include/gsaj.h's three rules
  assert_pyramid_equal  the raw bits of every plane of every level
  planted               a frame with every depth case of the rules planted at an even and an odd block position and on a corner of
                        the 32 x 32 block one workgroup owns
  relevel               gsaj_pose_gn_relevel on the dict state -> (state, the projection matrix its camera matrices are from)

Mutants: "partial_block_averaged" (an odd last column / row is averaged over the children that exist instead of dropped),
"invalid_depth_as_zero_in_mean" (the depth sum divided by 4 whatever the number of valid children), "no_edge_test" (a pixel across a
depth discontinuity keeps its mean), "mask_and" (AND of the children's masks); "relevel_keeps_proposal" (the unjudged proposal
survives the relevel), "relevel_keeps_accepted_loss" (the coarse level's loss stays the baseline), "relevel_old_projection" (the
camera matrices keep the previous level's projection)."""
import numpy as np

F = np.float32
PYRAMID_MUTANTS = ("partial_block_averaged", "invalid_depth_as_zero_in_mean", "no_edge_test", "mask_and")
RELEVEL_MUTANTS = ("relevel_keeps_proposal", "relevel_keeps_accepted_loss", "relevel_old_projection")
MAX_LEVELS = 4
R_N = np.array([0.0, 1.0, 0.5, F(1.0 / 3.0), 0.25], F)   # r[n]; n = 0 never multiplies


def _children(a, fill):
    """The four children p00, p01, p10, p11 of every pixel of the next level: whole 2 x 2 blocks only (fill None), or -- the
    partial-block mutant -- the last odd column / row padded with `fill`."""
    H, W = a.shape[-2:]
    if fill is None:
        a = a[..., :H // 2 * 2, :W // 2 * 2]
    else:
        pad = [(0, 0)] * (a.ndim - 2) + [(0, H % 2), (0, W % 2)]
        a = np.pad(a, pad, constant_values=fill)
    return a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]


def _color_down(c, mutant):
    if mutant == "partial_block_averaged":
        kids = np.stack(_children(c, np.nan))   # (whole blocks: the rule itself; the padded ones: the mean of what exists)
        whole = (F(0.25) * ((kids[0] + kids[1]) + (kids[2] + kids[3]))).astype(F)
        return np.where(np.isnan(whole), np.nanmean(kids, axis=0), whole).astype(F)
    p00, p01, p10, p11 = _children(c, None)
    return (F(0.25) * ((p00 + p01) + (p10 + p11))).astype(F)


def _depth_down(d, ratio, mutant):
    kids = np.stack(_children(d, F(0.0) if mutant == "partial_block_averaged" else None)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = kids > F(0.0)                 # NaN and negatives are not
        s, n = np.zeros(kids.shape[1:], F), np.zeros(kids.shape[1:], np.int64)
        for i in range(4):                    # p00, p01, p10, p11, skipping invalid ones
            s = np.where(valid[i], np.where(n > 0, s + kids[i], kids[i]), s).astype(F)
            n = n + valid[i]
        dmin = np.where(valid, kids, np.inf).min(axis=0).astype(F)
        dmax = np.where(valid, kids, -np.inf).max(axis=0).astype(F)
        edge = (dmax - dmin).astype(F) > (F(ratio) * dmin).astype(F)
        if mutant == "no_edge_test":
            edge = np.zeros_like(edge)
        mean = (s * (F(0.25) if mutant == "invalid_depth_as_zero_in_mean" else R_N[n])).astype(F)
    return np.where((n == 0) | edge, F(0.0), mean).astype(F)


def _mask_down(m, mutant):
    p = [(k != 0) for k in _children(m, 0 if mutant == "partial_block_averaged" else None)]
    out = (p[0] & p[1] & p[2] & p[3]) if mutant == "mask_and" else (p[0] | p[1] | p[2] | p[3])
    return out.astype(np.uint8)


def pyramid(color, depth, mask, levels, depth_edge_ratio, mutant=None):
    """-> [level 1, ..., level L], each dict(color [3,H_l,W_l] float32, depth [H_l,W_l] float32 or None, mask [H_l,W_l] uint8 or None)."""
    assert mutant is None or mutant in PYRAMID_MUTANTS, mutant
    assert 1 <= levels <= MAX_LEVELS
    c = np.asarray(color, F)
    d = None if depth is None else np.asarray(depth, F).reshape(c.shape[1:])
    m = None if mask is None else np.asarray(mask, np.uint8).reshape(c.shape[1:])
    out = []
    for _ in range(levels):
        c = _color_down(c, mutant)
        d = None if d is None else _depth_down(d, depth_edge_ratio, mutant)
        m = None if m is None else _mask_down(m, mutant)
        out.append(dict(color=c, depth=d, mask=m))
    return out


def assert_pyramid_equal(got, want, tag):
    """The comparator of the GPU tests: every plane of every level, shape and raw bits."""
    assert len(got) == len(want), (tag, len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want), start=1):
        for key, bits in (("color", np.uint32), ("depth", np.uint32), ("mask", np.uint8)):
            if w[key] is None:
                assert g[key] is None, "%s: level %d has a %s plane it should not have" % (tag, l, key)
                continue
            have, v = np.ascontiguousarray(g[key]), np.ascontiguousarray(w[key])
            assert have.shape == v.shape and have.dtype == v.dtype, "%s: level %d %s is %s %s, want %s %s" % (tag, l, key, have.dtype, have.shape, v.dtype, v.shape)
            same = have.view(bits) == v.view(bits)
            assert same.all(), "%s: level %d %s differs at %d of %d elements, first at %s: got %r want %r" % (
                tag, l, key, int((~same).sum()), same.size, np.argwhere(~same)[0], have[~same][0], v[~same][0])


# ---- planted depth cases ----------------------------------------------------------------------------------------------------------
PLANTED_RATIO = 0.125          # exactly representable, and so is every spread below
ULP = F(2.0 ** -23)            # one ulp in [1, 2)
_NAN = F(np.nan)
DEPTH_CASES = (                # name, the children p00 p01 p10 p11
    ("four_valid", (1.0, 1.03125, 1.0625, 1.09375)),
    ("three_valid", (1.0, 0.0, 1.0625, 1.03125)),
    ("two_valid", (0.0, 1.0, 0.0, 1.0625)),
    ("one_valid", (0.0, 0.0, 1.5, 0.0)),
    ("none_valid", (0.0, 0.0, 0.0, 0.0)),
    ("nan_child", (1.0, _NAN, 1.0625, 1.03125)),
    ("negative_child", (1.0, 1.03125, -1.0625, 1.09375)),
    ("spread_just_inside", (1.0, F(1.125) - ULP, 1.0625, 1.03125)),
    ("spread_just_outside", (1.0, F(1.125) + ULP, 1.0625, 1.03125)),
    ("spread_equal", (1.0, 1.125, 1.0625, 1.03125)),
)
# what the rules give at level 1, written out by hand (sums in the order p00, p01, p10, p11 over the valid children)
DEPTH_EXPECTED = dict(
    four_valid=F(F(F(F(1.0) + F(1.03125)) + F(1.0625)) + F(1.09375)) * F(0.25),
    three_valid=F(F(F(1.0) + F(1.0625)) + F(1.03125)) * F(1.0 / 3.0),
    two_valid=F(F(1.0) + F(1.0625)) * F(0.5),
    one_valid=F(1.5),
    none_valid=F(0.0),
    nan_child=F(F(F(1.0) + F(1.0625)) + F(1.03125)) * F(1.0 / 3.0),
    negative_child=F(F(F(1.0) + F(1.03125)) + F(1.09375)) * F(1.0 / 3.0),
    spread_just_inside=F(F(F(F(1.0) + (F(1.125) - ULP)) + F(1.0625)) + F(1.03125)) * F(0.25),
    spread_just_outside=F(0.0),
    spread_equal=F(F(F(F(1.0) + F(1.125)) + F(1.0625)) + F(1.03125)) * F(0.25),
)
# level-1 positions (x1, y1): case i at an even and at an odd position, and on a corner of a workgroup's 16 x 16 tile of level 1
_CORNERS = ((15, 15), (16, 16), (31, 15), (32, 16), (47, 15), (48, 16), (63, 15), (64, 16), (15, 31), (16, 32))


def planted_positions():
    """name -> [(x1, y1) even, odd, workgroup-block corner]."""
    return {name: [(2 + 4 * i, 4), (3 + 4 * i, 9), _CORNERS[i]] for i, (name, _) in enumerate(DEPTH_CASES)}


def planted(W=162, H=122, seed=5):
    """-> (color [3,H,W], depth [H,W], mask [H,W] uint8): a random colour image, a smooth valid depth (no discontinuity anywhere at
    PLANTED_RATIO) with DEPTH_CASES planted at planted_positions(), a random mask with an all-zero and an all-one 8 x 8 block.  W = 162:
    level 1 is 81 wide, so level 2 drops a column."""
    rng = np.random.default_rng(seed)
    color = rng.random((3, H, W), dtype=F)
    ys, xs = np.mgrid[0:H, 0:W]
    depth = (F(2.0) + F(0.001) * xs.astype(F) + F(0.002) * ys.astype(F)).astype(F)
    for name, kids in DEPTH_CASES:
        for (x1, y1) in planted_positions()[name]:
            assert 2 * x1 + 1 < W and 2 * y1 + 1 < H
            depth[2 * y1:2 * y1 + 2, 2 * x1:2 * x1 + 2] = np.asarray(kids, F).reshape(2, 2)
    mask = (rng.random((H, W)) < 0.3).astype(np.uint8) * np.uint8(255)   # (any non-zero byte is set)
    mask[40:48, 8:16] = 0
    mask[40:48, 24:32] = 1
    return color, depth, mask


# ---- the Levenberg-Marquardt state at the next resolution ----------------------------------------------------------------------------
def relevel(state, projection_old, projection_next, lambda_init, skip=0, mutant=None):
    """gsaj_pose_gn_relevel on a gn_restated / gn8_restated dict state (updated in place) -> (state, the projection matrix the packed
    state's camera matrices are to be formed with: gn_restated.pack_state(state, that))."""
    assert mutant is None or mutant in RELEVEL_MUTANTS, mutant
    st = state
    if skip:
        return st, projection_old
    joint = "exposure" in st
    if st["has"] and mutant != "relevel_keeps_proposal":
        st["w2c"] = st["acc_w2c"].copy()
        if joint:
            st["exposure"] = st["acc_exposure"].copy()
    st["lam"] = float(F(lambda_init))
    if mutant != "relevel_keeps_accepted_loss":
        st["acc_loss"], st["has"] = 0.0, False
    st["acc_w2c"] = st["w2c"].copy()
    st["H"], st["g"] = np.zeros_like(st["H"]), np.zeros_like(st["g"])
    st["tau"], st["converged"] = np.zeros(6), False
    if joint:
        st["acc_exposure"], st["dexposure"] = st["exposure"].copy(), np.zeros(2)
    return st, (projection_old if mutant == "relevel_old_projection" else projection_next)


def assert_relevelled(dev_state, tag):
    """What the state comparators of gn_restated / gn8_restated do not look at: the fields a relevel zeroes are zero, bit for bit."""
    s = np.asarray(dev_state, F)
    joint = s.size == 152
    assert s[82] == 0 and s[81] == 0, (tag, s[81], s[82])
    assert not s[70:78].any() and not s[85:88].any(), (tag, s[70:78], s[85:88])
    assert not s[104:(148 if joint else 131)].any(), "%s: the accepted H and g are not zeroed" % tag
    assert np.array_equal(s[88:104], s[0:16]), "%s: the accepted W2C is not the W2C" % tag
    if joint:
        assert not s[78:80].any() and np.array_equal(s[148:150], s[33:35]), (tag, s[78:80], s[148:150], s[33:35])
