"""eval_rendering, eval_ate and save_gaussians under the reference's import path, with its signatures and the files it writes
(utils/eval_utils.py:68-192), restated on top of gsaj.evaluation.

eval_rendering visits the frames the reference visits: every 5th index below len(frames) - 1 that is not a keyframe.  The
reference bounds the walk by `iteration` unless `iteration == "final" or "before_opt"`; a non-empty string is true, so that
condition always holds and `iteration` only names the output directory.  That is kept.  Each visited frame is render() ->
FrameEvaluator.add (three launches, nothing read back); the table is read once after the walk.  The 8-bit pictures the reference
collects per frame are never used there and are not built here (FrameEvaluator.add(u8_out=...) makes them).
LPIPS: the reference scores every frame with torchmetrics' AlexNet LPIPS, whose weights are a download.  Here "mean_lpips" is None
unless the caller hands in lpips_fn(image, gt) -> scalar, called with the clamped image and the ground truth, both [C,H,W] device
tensors; its values are read after the walk too.
eval_ate aligns with gsaj.evaluation.ate (Umeyama's closed form, what evo's align_trajectory computes) and writes
plot/trj_<label>.json and plot/stats_<label>.json.  Neither function plots or logs, and neither needs wandb, cv2 or evo.
"""
import json
import os

import numpy as np

from gaussian_splatting.gaussian_renderer import render
from gsaj.evaluation import FrameEvaluator, ate

FRAME_INTERVAL = 5
ATE_KEYS = ("rmse", "mean", "median", "std", "min", "max", "sse")  # what evo's APE.get_all_statistics returns


def _write_json(directory, name, doc):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, name), "w", encoding="utf-8") as fh:
        json.dump(doc, fh, indent=4)


def _camera_to_world(R, T):
    """The inverse of the world-to-camera pose [R | T] as a 4x4 fp64 matrix, as np.linalg.inv gives it (R may carry a scale)."""
    w2c = np.eye(4)
    w2c[:3, :3] = R.detach().cpu().numpy()
    w2c[:3, 3] = T.detach().cpu().numpy()
    return np.linalg.inv(w2c)


def eval_ate(frames, kf_ids, save_dir, iterations, final=False, monocular=False):
    """Trajectory error over the keyframes kf_ids of frames (each with uid, R, T, R_gt, T_gt) -> the RMSE.  Writes
    plot/trj_<label>.json = {"trj_id", "trj_est", "trj_gt"} (camera-to-world matrices as nested lists) and plot/stats_<label>.json
    (ATE_KEYS); label is "final" or the zero-padded iteration.  The scale is estimated only for monocular runs."""
    keyframes = [frames[k] for k in kf_ids]
    est = [_camera_to_world(f.R, f.T) for f in keyframes]
    gt = [_camera_to_world(f.R_gt, f.T_gt) for f in keyframes]
    label = "final" if final else "%04d" % iterations
    plot_dir = os.path.join(save_dir, "plot")
    _write_json(plot_dir, "trj_%s.json" % label,
                {"trj_id": [f.uid for f in keyframes], "trj_est": [m.tolist() for m in est], "trj_gt": [m.tolist() for m in gt]})
    stats = ate(gt, est, correct_scale=monocular)
    _write_json(plot_dir, "stats_%s.json" % label, {k: stats[k] for k in ATE_KEYS})
    return stats["rmse"]


def eval_rendering(frames, gaussians, dataset, save_dir, pipe, background, kf_indices, iteration="final", lpips_fn=None,
                   per_frame=None):
    """Mean PSNR / SSIM (/ LPIPS) of the map over the evaluated frames -> {"mean_psnr", "mean_ssim", "mean_lpips"}, also written
    to psnr/<iteration>/final_result.json.  per_frame: an optional dict that receives "frame_idx" and the evaluator's per-frame
    "psnr", "ssim", "mse", "count" lists (the return value and the file keep the reference's three keys)."""
    end_idx = len(frames) - 1  # whatever `iteration` is: see the module's docstring
    visited = [i for i in range(0, end_idx, FRAME_INTERVAL) if i not in kf_indices]
    evaluator, lpips = None, []
    for i in visited:
        gt_image = dataset[i][0]
        image = render(frames[i], gaussians, pipe, background)["render"].detach().contiguous()
        if evaluator is None:
            C, H, W = gt_image.shape
            evaluator = FrameEvaluator(W, H, gt_image.device, C=C)
        evaluator.add(image, gt_image)
        if lpips_fn is not None:
            lpips.append(lpips_fn(evaluator.clamped(), gt_image))

    nan = float("nan")
    scores = evaluator.summary() if evaluator is not None else dict(mean_psnr=nan, mean_ssim=nan, psnr=[], ssim=[], mse=[], count=[])
    if per_frame is not None:
        per_frame.update(frame_idx=visited, **{k: scores[k] for k in ("psnr", "ssim", "mse", "count")})
    result = {"mean_psnr": scores["mean_psnr"], "mean_ssim": scores["mean_ssim"],
              "mean_lpips": float(np.mean([float(v) for v in lpips])) if lpips else None}
    _write_json(os.path.join(save_dir, "psnr", str(iteration)), "final_result.json", result)
    return result


def save_gaussians(gaussians, name, iteration, final=False):
    """The map as <name>/point_cloud/final/point_cloud.ply, or .../iteration_<iteration>/...; nothing when name is None."""
    if name is not None:
        gaussians.save_ply(os.path.join(name, "point_cloud", "final" if final else "iteration_%s" % iteration, "point_cloud.ply"))
