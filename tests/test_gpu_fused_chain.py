"""GPU: the whole-window batched backward forms a (view, Gaussian)'s ten sums INSIDE k_chain_window (the row walk of k_gather_sums on
k_gather_sums' own grid of 64-row groups, no gsum round trip), the split sequence GSAJ_BWD_ONLY_COMPOSITE -> GSAJ_BWD_ONLY_CHAIN
goes through k_gather_sums and gsum as before.  Same additions in the same order: every output of the two must be the SAME BITS
(torch.equal, no tolerance) -- the summed per-Gaussian gradients, the per-view dL/dmean2D and dL/dtau rows, the per-view dL/dtau
sums -- and the sums summed again on demand after the fused call (BatchContext.view_sums) must be the bits the split sequence left
in the workspace.  Cases (tests/fused_chain_cases.py): the bench's cfg2 window; small scenes with K = 3 (partial group of views),
K = 11 (second launch of 8 views, accumulating), Gaussian counts that are not multiples of 32 or 64, a view that sees nothing, both
record formats, every SH storage size; a scene with planted runs that cross the walk's group, half-block and block boundaries."""
import pytest

import fused_chain_cases as cs

pytestmark = pytest.mark.gpu


def _assert_same_bits(K, cams, sc, deg, record_bits, dLc, dLd, bg=cs.BG):
    import torch

    bf, fused, sums_f = cs.window(K, cams, sc, deg, record_bits, dLc, dLd, False, bg)
    bs, split, sums_s = cs.window(K, cams, sc, deg, record_bits, dLc, dLd, True, bg)
    assert torch.equal(bf.radii, bs.radii)
    for n in cs.OUTPUTS:
        assert torch.isfinite(fused[n]).all(), n
        assert torch.equal(fused[n], split[n]), "dL/d%s: fused and split backward differ (max |diff| %.3e of max %.3e)" % (
            n, float((fused[n] - split[n]).abs().max()), float(split[n].abs().max()))
    for v in range(K):
        assert torch.equal(sums_f[v], sums_s[v]), "view %d: the sums summed on demand differ from the ones the split backward stored" % v
    # (not vacuous: something was rendered and back-propagated)
    assert float(fused["mean3D"].abs().max()) > 0.0 and max(float(x.abs().max()) for x in sums_f) > 0.0
    return bf, fused


def _assert_blind(bc, fused, blind):
    assert int(bc.radii[blind].max()) == 0  # nothing visible in that view
    assert float(fused["mean2D"][blind].abs().max()) == 0.0 and float(fused["tau_all"][blind].abs().max()) == 0.0


@pytest.mark.parametrize("K,P,coeffs,bits,blind", cs.SMALL)
def test_fused_backward_equals_split_backward_bit_for_bit(K, P, coeffs, bits, blind):
    bc, fused = _assert_same_bits(*cs.small_case(K, P, coeffs, bits, blind))
    if blind is not None:
        _assert_blind(bc, fused, blind)
    assert int((bc.radii > 0).sum()) > 0


@pytest.mark.parametrize("bits", [32, 16])
def test_fused_backward_equals_split_backward_on_the_bench_window(bits):
    """cfg2, the 8 keyframes and the pixel-gradient seeds bench.py runs (rank 0)."""
    _assert_same_bits(*cs.bench_case(bits), bg=(0.0, 0.0, 0.0))


def test_fused_backward_equals_split_backward_across_group_boundaries():
    """fused_chain_cases.planted_case: runs of more than 128 rows on both sides of the half-block edge and of the block edge, short runs
    beside them, a view without rows, a last chain workgroup that is the first half of its block.  That the scene is what it says
    is checked here, on the device's own tile counts."""
    from gsaj import rasterizer as C

    args = cs.planted_case()
    K, cams, P = args[0], args[1], args[2]["means3D"].shape[0]
    bc, fused = _assert_same_bits(*args)
    _assert_blind(bc, fused, 1)
    blk = lambda buf, stride, k: buf[k * stride:(k + 1) * stride]  # noqa: E731
    for k in (0, 2):
        dbg = C.debug_export(P, bc.capacity, cams[0]["W"], cams[0]["H"], blk(bc.geom, bc.geom_stride, k), blk(bc.binning, bc.bin_stride, k),
                             blk(bc.img, bc.img_stride, k))
        tt = dbg["tiles_touched"].cpu().numpy()
        assert (tt[list(cs.PLANTED)] > 128).all(), (k, tt[list(cs.PLANTED)])
        for h in range(0, P, 32):
            others = [int(tt[i]) for i in range(h, h + 32) if i not in cs.PLANTED]
            assert any(1 <= n <= 63 for n in others), (k, h, others)
