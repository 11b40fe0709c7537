"""NumPy restatements (float64) for the batched Gauss-Newton path -- csrc/pose_jac.hip: k_splat_jac, k_render_jac and
k_gn_step<6> / k_gn_step<8> launched over K views, k_gn_select -- TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_gn_window.py,
tests/test_gpu_pose_jacobian_batch.py and tests/test_gpu_gn_window.py.

K views of one map are K independent single-view problems, so the per-view restatement is tests/gn_restated.py / gn8_restated.py
applied view by view: nothing new is restated there.  What a batched kernel can get wrong is WHICH view's data it reads, so every
view of the window has its own camera (the scene's, moved by two small left increments), ground truth, mask and exposure, and the
mutants swap exactly those:

  window_cameras     the K = 3 cameras of the 72x40 scene
  ground_truth       view v's ground truth near view v's render (the recipe of tests/test_gpu_pose_jacobian.py, seeded per view)
  view_equations     one view's normal equations (either form) from ITS Jacobian, images, ground truth, mask and exposure
  window_equations   all K of them, with a `mutant=` that hands view v something of view 0's
  window_step        K lm_step / lm8_step calls with `active` and skip words
  select             k_gn_select

Mutants: "gt_of_view_0", "exposure_of_view_0", "mask_of_view_0", "camera_rows_of_view_0" (view v's walk over view 0's derivative
rows), "rows_into_previous_state" (view v's rows stepped into view v - 1's state), "select_ignores_active"."""
import numpy as np

import gn8_restated as g8
import gn_restated as gn
import loss_restated as lr

F = np.float32
K = 3
EXPOSURES = ((0.2, -0.05), (-0.1, 0.03), (0.0, 0.0))
# left increments [rho, theta] of views 1 and 2 against the scene's camera: about a pixel at the scene's depths, so that every view
# bins differently and no two views share a tile list
INCREMENTS = ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.02, -0.012, 0.015, 0.006, -0.004, 0.003), (-0.015, 0.02, -0.01, -0.005, 0.007, -0.004))
EQUATION_MUTANTS = ("gt_of_view_0", "exposure_of_view_0", "mask_of_view_0", "camera_rows_of_view_0")
MUTANTS = EQUATION_MUTANTS + ("rows_into_previous_state", "select_ignores_active")


def window_cameras():
    """-> (cams [K], sc, planted): the scene of gn_restated.jac_scene seen from K poses."""
    cam, sc, planted = gn.jac_scene()
    return [g8.camera_at(cam, gn.se3_exp(tau) @ np.asarray(cam["w2c"], np.float64)) for tau in INCREMENTS], sc, planted


def ground_truth(color, depth, view):
    """(gt [3,H,W], gt_depth [H,W], mask [H,W] uint8) near the given render; every view draws from its own seed."""
    rng = np.random.default_rng(9 + 17 * view)
    H, W = gn.JAC_H, gn.JAC_W
    c, d = np.asarray(color, F).reshape(3, H, W), np.asarray(depth, F).reshape(H, W)
    gt = np.clip(c + rng.normal(scale=0.08, size=c.shape) + 0.05 * np.sin((np.arange(W) + 11 * view) / 7.0)[None, None, :], 0.0, 1.5).astype(F)
    gt[:, 3 + 2 * view:6 + 2 * view, 10:30] = 0.001                # below the rgb boundary threshold
    gd = (d + rng.normal(scale=0.1, size=d.shape)).astype(F)
    gd[rng.uniform(size=d.shape) < 0.1] = 0.0                      # no depth measured
    mask = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint8)
    return gt, gd, mask


def view_equations(J, img, truth, exposure, delta, joint, mono=False, masked=False, alpha=0.9, rgb_thr=0.01):
    """One view: img = dict(image [3,H,W], depth [1,H,W], opacity [1,H,W]) (fp32, the forward's), truth = (gt, gt_depth, mask).
    -> (the normal equations with their bounds: gn.normal_equations / g8.normal_equations8, irls's dict)."""
    flags = lr.TRACKING | (lr.MONOCULAR if mono else 0)
    gt, gd, mask = truth
    a, b = F(exposure[0]), F(exposure[1])
    q = gn.irls(flags, alpha, rgb_thr, img["image"], img["depth"], img["opacity"], gt, None if mono else gd, mask if masked else None, a, b,
                delta=delta)
    if joint:
        return g8.normal_equations8(J, img["image"], a, q["s"], q["h"], q["err_s"], q["err_h"]), q
    return gn.normal_equations(J, q["s"], q["h"], q["err_s"], q["err_h"]), q


def window_equations(views, truths, exposures, delta, joint, mono=False, masked=False, mutant=None):
    """views[v] = dict(J, image, depth, opacity[, st, rows: the oracle's state and derivative rows, for the camera mutant]).
    -> [(equations, irls dict)] per view.  A mutant hands view v > 0 something of view 0's."""
    assert mutant in (None,) + EQUATION_MUTANTS, mutant
    out = []
    for v, view in enumerate(views):
        J = view["J"]
        if mutant == "camera_rows_of_view_0" and v > 0:
            J = gn.jacobian(view["st"], views[0]["rows"], gn.JAC_BG)[0]
        gt, gd, mask = truths[v]
        if mutant == "gt_of_view_0":
            gt, gd = truths[0][0], truths[0][1]
        if mutant == "mask_of_view_0":
            mask = truths[0][2]
        e = exposures[0] if mutant == "exposure_of_view_0" else exposures[v]
        out.append(view_equations(J, view, (gt, gd, mask), e, delta, joint, mono, masked))
    return out


def window_step(states, sums, joint, lm, active=None, skip=None, mutant=None):
    """states[v]: lm_new_state / lm8_new_state; sums[v] = (H, g, loss) of view v's rows.  One batched step: view v is stepped with
    ITS sums unless it is inactive or its skip word is set (then nothing of it changes)."""
    assert mutant in (None, "rows_into_previous_state"), mutant
    n = len(states)
    for v in range(n):
        if (active is not None and not active[v]) or (skip is not None and skip[v]):
            continue
        H, g, loss = sums[min(v + 1, n - 1)] if mutant == "rows_into_previous_state" else sums[v]
        (g8.lm8_step if joint else gn.lm_step)(states[v], H, g, loss, lm["nu"], lm["lambda_min"], lm["lambda_max"], lm["converged_threshold"])
    return states


def select(acc_loss, has, active=None, mutant=None):
    """k_gn_select: the index of the smallest accepted loss among the views that are active, have accepted a pose and have a finite
    loss; ties to the lowest index; (-1, inf) if none.  acc_loss as fp32."""
    assert mutant in (None, "select_ignores_active"), mutant
    best, best_loss = -1, float("inf")
    for v, (l, h) in enumerate(zip(np.asarray(acc_loss, F), has)):
        if active is not None and not active[v] and mutant != "select_ignores_active":
            continue
        if not h or not np.isfinite(l):
            continue
        if best < 0 or float(l) < best_loss:
            best, best_loss = v, float(l)
    return best, best_loss
