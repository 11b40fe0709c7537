"""The front end's keyframe decisions, on the host, from integer counts (gsaj.covisibility.CovisibilityWindow.counts).

Restates FrontEnd.is_keyframe, the `len(window) < window_size` branch and the single_thread rule of FrontEnd.run, and
FrontEnd.add_to_window (utils/slam_frontend.py:198-286, 412-434), outcomes and quirks included.  Nothing here touches a
device tensor: the counts are Python ints, the poses 4 x 4 world-to-camera matrices on the host, median_depth a Python float.

    counts  = (per_kf, n_query) with per_kf = {kf_id: (|query & kf|, |kf|)}, as CovisibilityWindow.counts() returns it
    poses   = {frame index: 4 x 4 world-to-camera matrix} (what getWorld2View2(R, T) gives the reference)
    config  = the "Training" dict of the reference's configuration

Ratios.  The reference divides two int64 count tensors: both are converted to float32, the quotient is float32, and the
comparison with the Python threshold is made in float32.  So 9 / 10 is NOT < 0.9, 3 / 10 IS <= 0.3 and 2 / 5 IS <= 0.4; a
comparison of the float32 quotient with a double decides the first one the other way.  0 / 0 is NaN, and every comparison
with NaN is false.
"""
import numpy as np
import torch

N_DONT_TOUCH = 2  # the first two entries of the new window are never candidates for removal


def ratio(num, den):
    """float32(num) / float32(den) as a numpy.float32; NaN for 0 / 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(num) / np.float32(den)


def _lt(r, thr):
    return bool(r < np.float32(thr))


def _le(r, thr):
    return bool(r <= np.float32(thr))


def _pose(T):
    if torch.is_tensor(T):
        T = T.detach().cpu()
    return torch.as_tensor(np.asarray(T, dtype=np.float32)).reshape(4, 4)


def pose_distance(T_i, T_j):
    """|| (T_i T_j^-1)[0:3, 3] ||, the reference's float32 torch expression on the host (a 0-dim float32 tensor)."""
    return torch.norm((_pose(T_i) @ torch.linalg.inv(_pose(T_j)))[0:3, 3])


def overlap_ratio(counts, kf_id):
    """intersection / union of the query with keyframe kf_id (is_keyframe, run): the union is |a| + |b| - |a & b|."""
    per_kf, n_query = counts
    inter, n_kf = per_kf[kf_id]
    return ratio(inter, n_query + n_kf - inter)


def is_keyframe(cur_idx, last_kf_idx, counts, poses, config, median_depth):
    """FrontEnd.is_keyframe: (overlap < kf_overlap and dist > kf_min_translation * median_depth) or
    dist > kf_translation * median_depth."""
    dist = pose_distance(poses[cur_idx], poses[last_kf_idx])
    md = torch.tensor(float(median_depth), dtype=torch.float32)
    dist_check = bool(dist > config["kf_translation"] * md)
    dist_check2 = bool(dist > config["kf_min_translation"] * md)
    return (_lt(overlap_ratio(counts, last_kf_idx), config["kf_overlap"]) and dist_check2) or dist_check


def wants_keyframe(cur_idx, window, counts, poses, config, median_depth):
    """What FrontEnd.run decides after a tracked frame (:412-434): is_keyframe against the newest keyframe window[0]; while the
    window is shorter than window_size, instead "kf_interval frames have passed and overlap < kf_overlap"; in single_thread
    mode additionally only after kf_interval frames."""
    last = window[0]
    check_time = (cur_idx - last) >= config["kf_interval"]
    create = is_keyframe(cur_idx, last, counts, poses, config, median_depth)
    if len(window) < config["window_size"]:
        create = check_time and _lt(overlap_ratio(counts, last), config["kf_overlap"])
    if config.get("single_thread", False):
        create = check_time and create
    return bool(create)


def add_to_window(cur_idx, counts, poses, window, config, initialized):
    """FrontEnd.add_to_window -> (new window, removed frame or None).  The current frame goes to the front.  Of the entries from
    the third on whose overlap coefficient |query & kf| / min(|query|, |kf|) is at or below the cut-off (kf_cutoff, 0.4 when the
    key is absent and always 0.4 while not initialised) only the LAST one leaves.  If the window is still longer than
    window_size, the entry (again from the third on) with the largest sqrt(dist to current) * sum_j 1 / (dist_ij + 1e-6) leaves
    as well, and `removed` names that one."""
    per_kf, n_query = counts
    window = [cur_idx] + list(window)
    cut_off = config["kf_cutoff"] if "kf_cutoff" in config else 0.4
    if not initialized:
        cut_off = 0.4
    to_remove = []
    for kf in window[N_DONT_TOUCH:]:
        inter, n_kf = per_kf[kf]
        if _le(ratio(inter, min(n_query, n_kf)), cut_off):
            to_remove.append(kf)
    removed = None
    if to_remove:
        window.remove(to_remove[-1])
        removed = to_remove[-1]
    if len(window) > config["window_size"]:
        cand = window[N_DONT_TOUCH:]
        inv_dist = []
        for i in cand:
            inv = [1.0 / (pose_distance(poses[i], poses[j]) + 1e-6).item() for j in cand if j != i]
            k = torch.sqrt(pose_distance(poses[i], poses[cur_idx])).item()
            inv_dist.append(k * sum(inv))
        removed = cand[int(np.argmax(inv_dist))]
        window.remove(removed)
    return window, removed
