"""GPU: csrc/pyramid.hip against tests/pyramid_restated.py.  k_pyramid: the raw bits of every plane of every level, at the smallest
shapes at which the kernel can go wrong (one pixel, odd sizes, dropped remainders, more than one 32 x 32 workgroup block in both
directions, both the 8-byte and the scalar load path), the planted depth cases, the padding between planes, run-to-run equality and a
non-default stream.  k_gn_relevel: the state against the restatement within the comparators of the step kernels' tests."""
import numpy as np
import pytest

import gn8_restated as g8
import gn_restated as gn
import pyramid_restated as pr
from gsaj import synthetic as syn

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
SHAPES = ((2, 2, 1), (7, 5, 1), (33, 17, 4), (67, 35, 4), (97, 61, 3), (160, 120, 3))   # W, H, L
LM = dict(lambda_init=1e-3, nu=4.0, lambda_min=1e-7, lambda_max=1e7, converged_threshold=1e-4)


def _frame(W, H, seed):
    """Random colour; a depth with invalid pixels of every kind sprinkled in (zeros, negatives, NaN, an all-invalid block) and
    steps that make some pixels straddle a discontinuity; a random mask with empty and full regions."""
    rng = np.random.default_rng(seed)
    color = rng.random((3, H, W), dtype=F)
    depth = (1.0 + 2.0 * rng.random((H, W))).astype(F)
    depth[rng.random((H, W)) < 0.5] = F(2.0)          # (flat regions: spreads below the ratio)
    depth[rng.random((H, W)) < 0.15] = F(0.0)
    depth[rng.random((H, W)) < 0.03] = F(-1.5)
    depth[rng.random((H, W)) < 0.03] = F(np.nan)
    depth[H // 3:H // 3 + 9, W // 3:W // 3 + 9] = F(0.0)
    depth[:, W // 2:] *= F(1.5)
    mask = (rng.random((H, W)) < 0.2).astype(np.uint8) * np.uint8(3)
    mask[:H // 2, :W // 4] = 0
    return color, depth, mask


def _build(torch, W, H, L, color, depth, mask, ratio, stream=None):
    """-> (ImagePyramid, its levels as the restatement returns them), the allocation pre-filled with SENTINEL."""
    from gsaj.pyramid import ImagePyramid

    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    pyr = ImagePyramid(W, H, L, dev, has_depth=depth is not None, has_mask=mask is not None)
    pyr.buf.fill_(SENTINEL)
    args = (t(color), t(depth), t(mask))
    if stream is None:
        pyr.build(*args, depth_edge_ratio=ratio)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            pyr.build(*args, depth_edge_ratio=ratio)
        stream.synchronize()
    return pyr, _levels(pyr)


def _levels(pyr):
    return [dict(color=pyr.color(l).cpu().numpy(), depth=pyr.depth(l).cpu().numpy() if pyr.has_depth else None,
                 mask=pyr.mask(l)[0].cpu().numpy() if pyr.has_mask else None) for l in range(1, pyr.levels + 1)]


def _assert_padding_untouched(pyr, tag):
    buf = pyr.buf.cpu().numpy()
    written = np.zeros(buf.size, bool)
    for l in range(1, pyr.levels + 1):
        wl, hl, co, do, mo = pyr._lv[l]
        for off, nbytes, has in ((co, 12 * wl * hl, True), (do, 4 * wl * hl, pyr.has_depth), (mo, wl * hl, pyr.has_mask)):
            if has:
                assert off % 256 == 0 and not written[off:off + nbytes].any(), (tag, l, off)
                written[off:off + nbytes] = True
    assert written.any() and (buf[~written] == SENTINEL).all(), "%s: bytes between the level planes were written" % tag


@pytest.mark.parametrize("planes", ["depth+mask", "colour", "depth"])
@pytest.mark.parametrize("W,H,L", SHAPES, ids=["%dx%d-L%d" % s for s in SHAPES])
def test_pyramid_bits_against_the_restatement(W, H, L, planes):
    import torch

    color, depth, mask = _frame(W, H, seed=W * 1000 + H)
    depth = depth if planes != "colour" else None
    mask = mask if planes == "depth+mask" else None
    pyr, got = _build(torch, W, H, L, color, depth, mask, 0.1)
    want = pr.pyramid(color, depth, mask, L, 0.1)
    assert [g["color"].shape for g in got] == [(3, H >> l, W >> l) for l in range(1, L + 1)]
    pr.assert_pyramid_equal(got, want, "%dx%d L=%d %s" % (W, H, L, planes))
    _assert_padding_untouched(pyr, "%dx%d L=%d %s" % (W, H, L, planes))
    if depth is not None and W >= 33:   # the frame exercises the rules: valid, invalid and edge pixels all occur at level 1
        d1 = want[0]["depth"]
        assert (d1 > 0).any() and (d1 == 0).any()
        assert not np.array_equal(d1, pr.pyramid(color, depth, mask, 1, 0.1, mutant="no_edge_test")[0]["depth"])


def test_planted_depth_cases_at_even_odd_and_workgroup_corner_positions():
    import torch

    color, depth, mask = pr.planted()
    H, W = depth.shape
    _, got = _build(torch, W, H, 3, color, depth, mask, pr.PLANTED_RATIO)
    for name, positions in pr.planted_positions().items():
        want = F(pr.DEPTH_EXPECTED[name])
        for (x1, y1) in positions:
            have = got[0]["depth"][y1, x1]
            assert have.view(np.uint32) == want.view(np.uint32), "%s at level-1 pixel (%d, %d): got %r want %r" % (name, x1, y1, have, want)
    # an invalid level-1 pixel is an invalid child of level 2: the mean there is over the three others
    x1, y1 = pr.planted_positions()["none_valid"][0]
    kids = got[0]["depth"][y1 // 2 * 2:y1 // 2 * 2 + 2, x1 // 2 * 2:x1 // 2 * 2 + 2].reshape(-1)
    assert (kids > 0).sum() == 3
    s = F(0.0)
    for k in kids[kids > 0]:
        s = F(s + k)
    assert got[1]["depth"][y1 // 2, x1 // 2].view(np.uint32) == F(s * F(1.0 / 3.0)).view(np.uint32)
    pr.assert_pyramid_equal(got, pr.pyramid(color, depth, mask, 3, pr.PLANTED_RATIO), "planted")


def test_pyramid_is_the_same_bits_run_to_run_and_on_another_stream():
    import torch

    W, H, L = 67, 35, 4
    color, depth, mask = _frame(W, H, seed=3)
    first, _ = _build(torch, W, H, L, color, depth, mask, 0.1)
    again, _ = _build(torch, W, H, L, color, depth, mask, 0.1)
    other, _ = _build(torch, W, H, L, color, depth, mask, 0.1, stream=torch.cuda.Stream())
    assert torch.equal(first.buf, again.buf) and torch.equal(first.buf, other.buf)


# ---- gsaj_pose_gn_relevel ------------------------------------------------------------------------------------------------------------
def _rows(rng, joint, H, g, loss, n=23):
    """n partial rows whose sum is (H, g, loss, ...), in the row format of the form."""
    if joint:
        tot = np.zeros(64)
        tot[:36], tot[36:44], tot[44:47] = [H[k, l] for (k, l) in g8.SYM8], g, [loss, 0.7 * loss, 0.3 * loss]
    else:
        tot = np.zeros(32)
        tot[:21], tot[21:27], tot[27:30] = [H[k, l] for (k, l) in gn.SYM6], g, [loss, 0.7 * loss, 0.3 * loss]
    return np.ascontiguousarray(rng.dirichlet(np.ones(n), size=tot.size).T * tot[None, :], dtype=F)


class _Solver:
    """A device state and its restated twin, stepped together."""

    def __init__(self, torch, joint, seed):
        from gsaj import _lib
        self.torch, self.joint, self.lib, self.dev = torch, joint, _lib.load(), torch.device("cuda:0")
        self.rng = np.random.default_rng(seed)
        self.cam = syn.fixture_camera(noisy=True, orthonormal=True, W=160, H=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
        w2c0 = np.ascontiguousarray(self.cam["viewmatrix"].T).astype(F)
        self.proj = np.asarray(self.cam["projmatrix_raw"], F).reshape(4, 4)
        # the next level's camera: half the resolution of a frame whose width is no multiple of 2, so that it differs in every entry
        self.proj_next = np.asarray(syn.make_camera(self.cam["w2c"], W=80, H=60, fx=70.0, fy=70.0, cx=39.5, cy=29.5)["projmatrix_raw"], F).reshape(4, 4)
        self.proj_next[0, 0] *= F(1.0125)
        assert np.abs(self.proj_next - self.proj).max() > 1e-3
        n = 8 if joint else 6
        self.state = torch.zeros(152 if joint else 136, dtype=torch.float32, device=self.dev)
        self.state[0:16] = torch.as_tensor(w2c0.reshape(16), device=self.dev)
        if joint:
            self.state[33], self.state[34] = 0.1, -0.02
            self.want = g8.lm8_new_state(w2c0, LM["lambda_init"], exposure=(0.1, -0.02))
        else:
            self.want = gn.lm_new_state(w2c0, LM["lambda_init"])
        A = self.rng.normal(size=(50, n))
        self.H = A.T @ A
        self.n = n

    def t(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def step(self, loss, proj):
        from gsaj import _lib
        rows = _rows(self.rng, self.joint, self.H, self.rng.normal(size=self.n) * 0.05, loss)
        tot = rows.astype(np.float64).sum(axis=0)
        fn, name = (self.lib.gsaj_pose_gn8_step, "gsaj_pose_gn8_step") if self.joint else (self.lib.gsaj_pose_gn_step, "gsaj_pose_gn_step")
        d_rows, d_proj = self.t(rows), self.t(proj)   # (held until the call is made: a freed block is handed out again at once)
        _lib.check(fn(d_rows.data_ptr(), rows.shape[0], LM["lambda_init"], LM["nu"], LM["lambda_min"], LM["lambda_max"], LM["converged_threshold"],
                      d_proj.data_ptr(), self.state.data_ptr(), None, self.torch.cuda.current_stream().cuda_stream), name)
        kw = (LM["nu"], LM["lambda_min"], LM["lambda_max"], LM["converged_threshold"])
        if self.joint:
            g8.lm8_step(self.want, g8.sym8(tot[:36]), tot[36:44], tot[44], *kw)
        else:
            gn.lm_step(self.want, gn.sym6(tot[:21]), tot[21:27], tot[27], *kw)
        self.close(proj, "step")

    def relevel(self, proj_next, skip=None, lambda_init=None):
        from gsaj import _lib
        lam = LM["lambda_init"] if lambda_init is None else lambda_init
        d_proj = self.t(proj_next)
        _lib.check(self.lib.gsaj_pose_gn_relevel(self.state.data_ptr(), self.state.numel(), d_proj.data_ptr(), lam,
                                                 None if skip is None else skip.data_ptr(), self.torch.cuda.current_stream().cuda_stream),
                   "gsaj_pose_gn_relevel")

    def close(self, proj, tag):
        (g8.assert_lm8_state_close if self.joint else gn.assert_lm_state_close)(self.state.cpu().numpy(), self.want, proj, tag)


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
@pytest.mark.parametrize("history", ["accept+accept", "accept+reject", "nothing accepted"])
def test_relevel_against_the_restatement(history, joint):
    import torch

    s = _Solver(torch, joint, seed=11)
    for loss in dict([("accept+accept", (1.0, 0.5)), ("accept+reject", (1.0, 1.5)), ("nothing accepted", ())])[history]:
        s.step(loss, s.proj)
    before = s.state.cpu().numpy().astype(np.float64)
    if history != "nothing accepted":   # the proposal the relevel discards differs from the accepted pose (and exposure)
        assert np.abs(before[0:16] - before[88:104]).max() > 1e-4 and before[82] == 1.0
        assert (s.want["accepted"], s.want["rejected"]) == ((2, 0) if history == "accept+accept" else (1, 1))
        assert not joint or np.abs(before[33:35] - before[148:150]).max() > 1e-6
    lam = 0.02   # (not the steps' lambda_init: the relevel writes the one it is given)
    s.relevel(s.proj_next, lambda_init=lam)
    pr.relevel(s.want, s.proj, s.proj_next, lam)
    after = s.state.cpu().numpy()
    s.close(s.proj_next, "relevel after %s" % history)
    pr.assert_relevelled(after, history)
    assert after[80] == F(lam) and np.array_equal(after[83:85], before[83:85].astype(F)), "lambda_init written, the counters kept"
    if history != "nothing accepted":
        assert np.array_equal(after[0:16], before[88:104].astype(F)), "back to the accepted pose, bit for bit"
        assert not joint or np.array_equal(after[33:35], before[148:150].astype(F))
    else:
        assert np.array_equal(after[0:16], before[0:16].astype(F)) and np.array_equal(after[33:35], before[33:35].astype(F))
    # the step after it accepts whatever its loss -- also one far above the coarse level's -- and counts on
    counted = (s.want["accepted"], s.want["rejected"])
    s.want["lam"] = LM["lambda_init"]   # (the first step of a level starts from ITS lambda_init argument)
    s.step(100.0, s.proj_next)
    assert (s.want["accepted"], s.want["rejected"]) == (counted[0] + 1, counted[1])
    assert float(s.state[81]) == pytest.approx(100.0, rel=1e-6) and float(s.state[82]) == 1.0


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_relevel_with_a_non_zero_skip_word_changes_nothing(joint):
    import torch

    s = _Solver(torch, joint, seed=12)
    s.step(1.0, s.proj)
    s.step(1.5, s.proj)
    before = s.state.clone()
    s.relevel(s.proj_next, skip=torch.ones(1, dtype=torch.int32, device=s.dev))
    assert torch.equal(s.state, before)
    s.relevel(s.proj_next, skip=torch.zeros(1, dtype=torch.int32, device=s.dev))
    assert not torch.equal(s.state, before)
