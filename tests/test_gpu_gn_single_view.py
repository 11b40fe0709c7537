"""GPU: the single-frame Gauss-Newton entry points are the batched kernels at K = 1 (csrc/pose_jac.hip: k_splat_jac, k_render_jac,
k_gn_step), told apart from the batched entry points by the host alone (csrc/api.hip: pose_jac).  What that host branch can get wrong,
on the small scene of tests/gn_single_view_cases.py, with SH colours and with precomputed colours:

  * the single forms promise to work from any workspace address: every workspace 16 bytes past a 256-byte boundary (the forward's
    too) gives the bits of aligned workspaces; the batched forms refuse such a workspace;
  * the explicit form (seed / curvature images, sums in the Jacobian workspace behind the rows) gives the same bits whichever of H
    and g is asked for, and before and after a K = 2 batched call on other buffers;
  * the step entry points: a set skip word leaves the state alone; otherwise the state is the batched entry's at K = 1, whatever its
    skip stride.
Everything is compared bit for bit: there is no tolerance in this file."""
import pytest

import gn_single_view_cases as cs

pytestmark = pytest.mark.gpu

_WORLDS = {}


def _world(colours):
    """the world and view 1 through the single-frame entry points on aligned workspaces, made once per colour form"""
    if colours not in _WORLDS:
        w = cs.World(colours)
        _WORLDS[colours] = (w, cs.Frame(w, 1))
    return _WORLDS[colours]


@pytest.mark.parametrize("colours", cs.COLOURS)
@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_unaligned_workspaces_give_the_bits_of_aligned_ones_and_the_batched_forms_refuse_them(colours, joint):
    import torch

    w, fr = _world(colours)
    assert fr.ctx.lib.gsaj_pose_jac_partial_rows(cs.W, cs.H) == cs.ROWS
    want = fr.jac_loss(joint)
    rows = want["partials"]
    assert bool(torch.isfinite(rows).all()) and bool((rows != cs.SENTINEL).all()) and bool(rows.any())
    assert not bool(rows[list(cs.PADDING)].any()), "the workgroups without a tile write zero rows"
    un = cs.Frame(w, 1, unaligned=True)
    assert torch.equal(un.ctx.color, fr.ctx.color) and torch.equal(un.ctx.depth, fr.ctx.depth)
    got = un.jac_loss(joint)
    assert torch.equal(got["partials"], rows), "partials differ on unaligned workspaces"
    assert torch.equal(got["jacobian"], want["jacobian"]), "jac_out differs on unaligned workspaces"
    # the batched form at K = 1 on aligned workspaces: the same bits; with any one workspace off the boundary: refused
    win = cs.Window(w, 1)
    c = win.ctx
    bat = win.jac_loss(joint)
    one = cs.Frame(w, 0).jac_loss(joint)
    assert torch.equal(bat["partials"][0], one["partials"]) and torch.equal(bat["jacobian"][0], one["jacobian"])
    for name in ("geom", "img", "binning", "jac_ws"):
        keep = getattr(c, name)
        moved = cs.off_boundary(keep.numel(), w.dev)
        moved.copy_(keep)
        setattr(c, name, moved)
        c._bind()
        with pytest.raises(Exception, match="256-byte aligned"):
            win.jac_loss(joint)
        setattr(c, name, keep)
        c._bind()
    again = win.jac_loss(joint)
    assert torch.equal(again["partials"], bat["partials"])


@pytest.mark.parametrize("colours", cs.COLOURS)
def test_explicit_form_whichever_sums_are_asked_for_and_around_a_batched_call(colours):
    import torch

    w, fr = _world(colours)

    def explicit():
        both = fr.jac(seeds=w.seeds, curvature=w.curv, want_jacobian=True, want_images=True)
        h_only = fr.jac(curvature=w.curv, want_jacobian=True, want_images=True)
        g_only = fr.jac(seeds=w.seeds, want_jacobian=True, want_images=True)
        none = fr.jac(want_jacobian=True, want_images=True)
        assert h_only["g"] is None and g_only["H"] is None and none["H"] is None and none["g"] is None
        assert torch.equal(h_only["H"], both["H"]) and torch.equal(g_only["g"], both["g"])
        for o in (h_only, g_only, none):
            for k in ("jacobian", "color", "depth"):
                assert torch.equal(o[k], both[k]), k
        assert bool(both["H"].any()) and bool(both["g"].any()) and bool(torch.isfinite(both["H"]).all())
        assert torch.equal(both["color"], fr.ctx.color) and torch.equal(both["depth"], fr.ctx.depth), "the forward's bits"
        return both

    before = explicit()
    win = cs.Window(w, 2)
    for joint in (False, True):
        rows = win.jac_loss(joint)["partials"]
        assert bool((rows != cs.SENTINEL).all())
    after = explicit()
    for k in ("H", "g", "jacobian", "color", "depth"):
        assert torch.equal(before[k], after[k]), "%s changed across a batched call on other buffers" % k


@pytest.mark.parametrize("joint", [False, True], ids=["6-form", "joint"])
def test_single_step_skip_word_and_the_batched_step_at_one_view(joint):
    import torch

    w, fr = _world("sh")
    rows = fr.jac_loss(joint)["partials"]
    start = cs.new_states(w, cs.K, joint)[1:2].clone()
    skip = torch.ones(4, dtype=torch.int32, device=w.dev)
    s = start.clone()
    cs.step(w, joint, rows, s[0], skip=skip)
    assert torch.equal(s, start), "a set skip word: the state is untouched"
    skip.zero_()
    cs.step(w, joint, rows, s[0], skip=skip)
    assert not torch.equal(s, start) and bool(torch.isfinite(s).all())
    for stride in (0, 4, 12):
        b = start.clone()
        cs.step_batch(w, joint, rows[None], b, active=None, skip=skip, skip_stride=stride)
        assert torch.equal(b, s), "the batched step at K = 1 with skip stride %d differs from the single step" % stride
    none = start.clone()
    cs.step(w, joint, rows, none[0], skip=None)
    assert torch.equal(none, s), "no skip word at all"
    # and a second step, from the stepped state, through both entries
    b = s.clone()
    cs.step(w, joint, rows, s[0], skip=skip)
    cs.step_batch(w, joint, rows[None], b, skip=skip, skip_stride=8)
    assert torch.equal(b, s)
