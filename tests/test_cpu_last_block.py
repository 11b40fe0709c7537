"""The comparators of tests/test_gpu_last_block.py, without a device: at every rung of the workgroup-count ladder
(tests/last_block_ladder.py) each one accepts the correct sum and rejects the two sums a broken last-workgroup hand-off
(csrc/last_block.h) would give -- one workgroup's partial left out (the last, and one from the middle), and one workgroup's partial
taken from input B inside the sum for input A (what a stale line in the reading CU's cache holds after the run on B).  The bounds are
the ones the suite already has (tests/loss_restated.py, tests/test_gpu_ssim.py; the bounding box is exact); A and B are chosen so that
both wrong sums stand out at them."""
import numpy as np
import pytest

import last_block_ladder as lb
import loss_restated as lr


def rejected(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


def groups(n, block):
    return -(-n // block)


@pytest.mark.parametrize("W,H", lb.LOSS_SIZES)
def test_loss_scalars(W, H):
    A, B = lb.loss_frames(W, H)
    G = groups(W * H, lr.WG)
    assert G in (1, 2, 256, 257, 513)
    mirror = lr.restate_frame(A, dtype=np.float32)["value"]   # an honest fp32 evaluation in the kernel's order
    lr.assert_loss_close(mirror, A["want"], "%dx%d" % (W, H), outputs=lr.SCALARS)
    for k in lb.wrong_rungs(G):
        for what, got in zip(("dropped", "stale"), lb.loss_wrong_scalars(A, B, k)):
            assert rejected(lambda: lr.assert_loss_close(got, A["want"], "x", outputs=lr.SCALARS)), (W, H, k, what)
            for s in ("loss", "l1_rgb"):   # (not only somewhere: at the loss itself)
                assert rejected(lambda: lr.assert_loss_close(got, A["want"], "x", outputs=(s,))), (W, H, k, what, s)


@pytest.mark.parametrize("P", lb.ISO_P)
def test_isotropic_loss(P):
    A, B = lb.iso_cases(P)
    G = groups(P, lb.ISO_BLOCK)
    assert G in (1, 2, 257)
    want = A["want"]
    grad = want["value"]["dL_dscales"]
    mirror = lr.iso_restate(A["scales"], lr.ISO_WEIGHT, dtype=np.float32)["value"]
    lr.assert_iso_close(mirror["loss"], mirror["dL_dscales"], want, "P %d" % P)
    pa, ka = lb.iso_partials(A)
    assert pa.size == G and abs(ka * pa.sum() - want["value"]["loss"]) <= 1e-12 * want["value"]["loss"]
    for k in lb.wrong_rungs(G):
        for what, loss in zip(("dropped", "stale"), lb.iso_wrong_losses(A, B, k)):
            assert rejected(lambda: lr.assert_iso_close(loss, grad, want, "x")), (P, k, what)


@pytest.mark.parametrize("N,C,W,H", lb.SSIM_CASES)
def test_ssim_means(N, C, W, H):
    A, B = lb.ssim_pairs(N, C, W, H)
    pa, pb = lb.ssim_partials(A), lb.ssim_partials(B)
    G = pa.shape[1]
    assert G in (1, 2, 288, 765)
    S32, _ = lb.sr.ssim_forward(A["x"], A["y"], dtype=np.float32)   # an fp32 evaluation of the map, summed exactly
    lb.assert_ssim_means(np.concatenate([S32.reshape(N, -1).astype(np.float64).mean(axis=1), [S32.astype(np.float64).mean()]]), A, "fp32")
    lb.assert_ssim_means(lb.ssim_out_from_partials(pa, A), A, "partials")
    for n in range(N):
        for k in lb.wrong_rungs(G):
            for what, v in (("dropped", 0.0), ("stale", pb[n, k])):
                bad = pa.copy()
                bad[n, k] = v
                assert rejected(lambda: lb.assert_ssim_means(lb.ssim_out_from_partials(bad, A), A, "x")), (N, C, W, H, n, k, what)


@pytest.mark.parametrize("n", lb.KNN_N)
def test_bounding_box_order(n):
    A, B = lb.knn_points(n)
    pa, pb = lb.knn_box_partials(A), lb.knn_box_partials(B)
    G = pa.shape[0]
    assert G in (1, 2, 256, 257, 513)
    box = lb.knn_box(pa)
    assert np.array_equal(box, np.concatenate([np.minimum(A.min(axis=0), 0), np.maximum(A.max(axis=0), 0)]))
    codes, idx = lb.knn_order(A, box)
    lb.assert_knn_order(codes, idx, A, box, "n %d" % n)
    for k in lb.wrong_rungs(G):
        rest = np.delete(pa, k, axis=0)
        dropped = lb.knn_box(rest) if rest.size else np.zeros(6, np.float32)
        stale = lb.knn_box(np.concatenate([rest, pb[k:k + 1]]))
        for what, wrong in (("dropped", dropped), ("stale", stale)):
            assert not np.array_equal(wrong, box), (n, k, what)
            c, i = lb.knn_order(A, wrong)   # what the device would hand back had it folded this box
            assert rejected(lambda: lb.assert_knn_order(c, i, A, box, "x")), (n, k, what)


@pytest.mark.parametrize("P", lb.BWD_P)
def test_tau_sum(P):
    A, B = lb.tau_rows(P)
    pa, pb = lb.tau_partials(A), lb.tau_partials(B)
    G = pa.shape[0]
    assert G in (1, 2, 256, 257, 513)
    fold = lambda part: part.astype(np.float64).sum(axis=0).astype(np.float32)  # noqa: E731  (fp64 over the workgroups, one rounding)
    lb.assert_tau_sum(fold(pa), A, "P %d" % P)
    for k in lb.wrong_rungs(G):
        for what, v in (("dropped", np.zeros(6, np.float32)), ("stale", pb[k])):
            bad = pa.copy()
            bad[k] = v
            assert rejected(lambda: lb.assert_tau_sum(fold(bad), A, "x")), (P, k, what)
