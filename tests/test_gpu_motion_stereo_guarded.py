"""GPU: gsaj_motion_stereo under the guarded allocator of tests/guards.py -- the (a)-(d) protocol of tests/test_gpu_memory_contracts.py
(its _contract, used as it is): an unguarded run whose outputs are kept, then for both fills three guarded runs on inputs A, B, A with
every band of the workspace, idx16 and the depth intact, the first run bitwise the unguarded run, no fp32 output still holding the
fill, and the third run bitwise the first.  The workspace's contract is "no initialisation needed" (include/gsaj.h "motion stereo": S is
zeroed on the stream inside the call), so it is poisoned again before every run.  B is a smaller image with fewer hypotheses on an
object of its own: the sizes of a MotionStereo are fixed when it is made.

gsaj_motion_stereo_bytes is not a row of that file's CONTRACTS table (its name does not end in _workspace_bytes); this file is its
guarded run."""
import pytest

import sweep_restated as sw
import test_gpu_memory_contracts as mc

pytestmark = pytest.mark.gpu


def _op_sweep(inp, st):
    import torch
    from gsaj import MotionStereo

    c, D, paths = inp
    cam = c["cam"]
    H, W = c["ref"].shape
    key = ("m", W, H, D)
    if key not in st:
        st[key] = MotionStereo(W, H, mc.DEV, cam["fx"], cam["fy"], cam["cx"], cam["cy"], num_hypotheses=D, block_radius=2, paths=paths)
        st.setdefault("all", []).append(st[key].workspace)
        st["scratch"] = lambda: st["all"]
    m = st[key]
    idx16 = mc.E(H, W, dtype=torch.int16)
    depth = mc.E(H, W)
    m(c["dev"][0], c["dev"][1], c["dev"][2], c["dev"][3], 0.2, 0.7, out_idx16=idx16, out_depth=depth)
    return dict(idx16=idx16, depth=depth, grad=m.gradient_bytes(), pc=m.pixel_costs(), cost=m.cost_volume(), sums=m.sums())


def _inputs(W, H, motion):
    c = dict(sw.case(W, H, motion))
    c["dev"] = [mc._t(c[k]) for k in ("ref", "src", "ref_w2c", "src_w2c")]   # inputs: not a guarded route
    return c


@pytest.mark.parametrize("paths", [4, 8])
def test_motion_stereo(monkeypatch, paths):
    """A: 96 x 40, D = 32; B: 65 x 33, D = 16.  pc, C and S end at the workspace's exact end; S is summed into and must start from the
    call's own zeroes, not from the fill."""
    A, B = _inputs(96, 40, "forward"), _inputs(65, 33, "mixed")
    mc._contract(monkeypatch, _op_sweep, (A, 32, paths), (B, 16, paths), "motion stereo paths=%d" % paths)
