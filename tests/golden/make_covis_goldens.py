"""Regenerates tests/golden/covis_prune.npz and tests/golden/kf_decisions.npz from a checkout of the reference:

    python tests/golden/make_covis_goldens.py /path/to/reference

Inputs and recorded outcomes only.  The outcomes come from the reference's own statements, run on CPU tensors:
  * FrontEnd.is_keyframe and FrontEnd.add_to_window (utils/slam_frontend.py): the two FunctionDef nodes are taken from the parsed
    file (the module itself needs the whole SLAM stack to import) and called unbound on a
    SimpleNamespace(config, cameras, median_depth, initialized), with the reference's own getWorld2View2
    (gaussian_splatting/utils/graphics_utils.py, taken the same way);
  * the statements of FrontEnd.run between `last_keyframe_idx = ...` and `if create_kf:` (the window_size override and the
    single_thread rule), taken from the parsed method and executed on a namespace holding what they read;
  * the n_obs / to_prune statements of BackEnd.map (utils/slam_backend.py), taken from the parsed method the same way, in both
    prune modes, initialised and not.
Visibility is stored as uint8, poses as the float32 world-to-camera matrices getWorld2View2 returns.
"""
import ast
import functools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

P_DEC = 40          # Gaussians of a decision case
BASE = dict(kf_translation=0.08, kf_min_translation=0.05, kf_overlap=0.9, kf_cutoff=0.3, window_size=8, kf_interval=5,
            single_thread=False)
MEDIAN_DEPTH = 2.0  # distance thresholds 0.16 and 0.10; the poses below stay at least 0.02 away from both


def _function(path, cls, name):
    tree = ast.parse(open(path).read())
    body = tree.body if cls is None else [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    return [n for n in body if isinstance(n, ast.FunctionDef) and n.name == name][0]


def _compiled(nodes, path, ns):
    exec(compile(ast.Module(body=list(nodes), type_ignores=[]), path, "exec"), ns)
    return ns


def _sibling_run(fn, starts, stops):
    """The consecutive statements of one block inside fn, from the first for which starts(stmt) up to the first for which
    stops(stmt) (excluded)."""
    for node in ast.walk(fn):
        for field in ("body", "orelse"):
            block = getattr(node, field, None)
            if not isinstance(block, list):
                continue
            for a, stmt in enumerate(block):
                if starts(stmt):
                    b = next(i for i in range(a, len(block)) if stops(block[i]))
                    return block[a:b]
    raise RuntimeError("statements not found in %s" % fn.name)


def _assigns(name):
    return lambda s: isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Name) and s.targets[0].id == name


def visibility(cur_n, kfs):
    """cur: ones at [0, cur_n).  kfs: {id: (intersection, count)} -> ones at [0, intersection) and outside cur."""
    cur = np.zeros(P_DEC, np.uint8)
    cur[:cur_n] = 1
    out = {}
    for kf, (inter, n) in kfs.items():
        v = np.zeros(P_DEC, np.uint8)
        v[:inter] = 1
        v[cur_n:cur_n + n - inter] = 1
        assert inter <= cur_n and cur_n + n - inter <= P_DEC and int((v & cur).sum()) == inter and int(v.sum()) == n
        out[kf] = v
    return cur, out


def camera(x, z=0.0, yaw=0.0):
    """A camera with world-to-camera rotation `yaw` about y and translation (x, 0, z)."""
    c, s = np.cos(yaw), np.sin(yaw)
    return SimpleNamespace(R=torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float32),
                           T=torch.tensor([x, 0.0, z], dtype=torch.float32))


def decision_cases():
    """name -> dict(kind, cfg, cur, window, initialized, cur_n, kfs, x = {frame: camera x}).  Frame 20 is the current frame."""
    cfg = lambda **kw: dict(BASE, **kw)  # noqa: E731
    no_cut = {k: v for k, v in BASE.items() if k != "kf_cutoff"}
    near = {20: 0.0, 10: 0.13, 9: 0.5, 8: 1.0, 7: 1.5, 6: 2.1, 5: 2.8, 4: 3.6, 3: 4.5, 2: 5.5}
    C = {}
    # ---- is_keyframe: dist to the last keyframe 10; thresholds 0.16 (alone) and 0.10 (with the overlap) -------------------
    K = dict(kind="is_keyframe", cfg=cfg(), cur=20, window=[10], initialized=True)
    C["kf_far_alone"] = dict(K, cur_n=10, kfs={10: (10, 10)}, x={20: 0.0, 10: 0.5})            # ratio 1, dist 0.5: third clause
    C["kf_overlap_and_min_dist"] = dict(K, cur_n=10, kfs={10: (5, 10)}, x=near)                 # 5/15 < 0.9, 0.10 < 0.13 < 0.16
    C["kf_overlap_but_too_close"] = dict(K, cur_n=10, kfs={10: (5, 10)}, x={20: 0.0, 10: 0.05})  # dist_check2 says no
    C["kf_ratio_exactly_at_overlap"] = dict(K, cur_n=9, kfs={10: (9, 10)}, x=near)              # 9/10 is not < 0.9
    C["kf_ratio_just_below_overlap"] = dict(K, cur_n=9, kfs={10: (8, 9)}, x=near)               # 8/10
    C["kf_empty_union"] = dict(K, cur_n=0, kfs={10: (0, 0)}, x=near)                            # NaN: the overlap clause is false
    C["kf_empty_union_far"] = dict(K, cur_n=0, kfs={10: (0, 0)}, x={20: 0.0, 10: 0.5})
    # ---- run(): the window_size override and the single_thread rule ------------------------------------------------------
    R = dict(kind="wants_keyframe", cur=20, initialized=True)
    C["run_short_window_time_and_overlap"] = dict(R, cfg=cfg(), window=[10, 9], cur_n=10, kfs={10: (5, 10), 9: (1, 3)}, x={20: 0.0, 10: 0.01, 9: 0.5})
    C["run_short_window_too_soon"] = dict(R, cfg=cfg(kf_interval=11), window=[10, 9], cur_n=10, kfs={10: (5, 10), 9: (1, 3)}, x={20: 0.0, 10: 0.5, 9: 1.0})
    C["run_short_window_ratio_at_overlap"] = dict(R, cfg=cfg(), window=[10, 9], cur_n=9, kfs={10: (9, 10), 9: (1, 3)}, x={20: 0.0, 10: 0.5, 9: 1.0})
    C["run_full_window_uses_is_keyframe"] = dict(R, cfg=cfg(window_size=2, kf_interval=11), window=[10, 9], cur_n=10, kfs={10: (10, 10), 9: (1, 3)}, x={20: 0.0, 10: 0.5, 9: 1.0})
    C["run_single_thread_too_soon"] = dict(R, cfg=cfg(window_size=2, kf_interval=11, single_thread=True), window=[10, 9], cur_n=10, kfs={10: (10, 10), 9: (1, 3)}, x={20: 0.0, 10: 0.5, 9: 1.0})
    C["run_single_thread_in_time"] = dict(R, cfg=cfg(window_size=2, single_thread=True), window=[10, 9], cur_n=10, kfs={10: (10, 10), 9: (1, 3)}, x={20: 0.0, 10: 0.5, 9: 1.0})
    # ---- add_to_window --------------------------------------------------------------------------------------------------
    A = dict(kind="add_to_window", cur=20, initialized=True, x=near)
    C["add_ratio_exactly_at_cutoff"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=10, kfs={10: (10, 10), 9: (4, 12), 8: (3, 12)})       # 3/10 <= 0.3
    C["add_ratio_just_above_cutoff"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=10, kfs={10: (10, 10), 9: (4, 12), 8: (4, 12)})
    C["add_not_initialized_forces_0p4"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=5, kfs={10: (5, 5), 9: (3, 12), 8: (2, 12)}, initialized=False)  # 2/5 <= 0.4
    C["add_initialized_same_counts"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=5, kfs={10: (5, 5), 9: (3, 12), 8: (2, 12)})         # 2/5 > 0.3
    C["add_empty_denominator"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=10, kfs={10: (10, 10), 9: (0, 0), 8: (5, 12)})             # NaN: stays
    C["add_empty_query"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=0, kfs={10: (0, 10), 9: (0, 5), 8: (0, 12)})
    C["add_two_below_cutoff_last_leaves"] = dict(A, cfg=cfg(), window=[10, 9, 8, 7], cur_n=10, kfs={10: (0, 10), 9: (1, 12), 8: (6, 12), 7: (2, 12)})  # 10 is protected
    C["add_overflow_argmax_leaves"] = dict(A, cfg=cfg(window_size=5), window=[10, 9, 8, 7, 6], cur_n=10, kfs={k: (8, 12) for k in (10, 9, 8, 7, 6)})
    C["add_cutoff_and_overflow_two_leave"] = dict(A, cfg=cfg(window_size=4), window=[10, 9, 8, 7, 6], cur_n=10, kfs={10: (8, 12), 9: (8, 12), 8: (1, 12), 7: (8, 12), 6: (8, 12)})
    C["add_window_of_one"] = dict(A, cfg=cfg(), window=[10], cur_n=10, kfs={10: (0, 10)})
    C["add_window_empty"] = dict(A, cfg=cfg(), window=[], cur_n=10, kfs={})
    C["add_cutoff_absent_defaults_0p4"] = dict(A, cfg=dict(no_cut), window=[10, 9, 8], cur_n=20, kfs={10: (10, 10), 9: (9, 20), 8: (7, 20)})   # 7/20 <= 0.4, > 0.3
    C["add_cutoff_0p3_same_counts"] = dict(A, cfg=cfg(), window=[10, 9, 8], cur_n=20, kfs={10: (10, 10), 9: (9, 20), 8: (7, 20)})
    return C


def make_decisions(ref):
    fe = os.path.join(ref, "utils", "slam_frontend.py")
    gu = os.path.join(ref, "gaussian_splatting", "utils", "graphics_utils.py")
    ns = _compiled([_function(gu, None, "getWorld2View2")], gu, {"torch": torch, "np": np})
    ns = _compiled([_function(fe, "FrontEnd", "is_keyframe"), _function(fe, "FrontEnd", "add_to_window")], fe, ns)
    run = _sibling_run(_function(fe, "FrontEnd", "run"), _assigns("last_keyframe_idx"),
                       lambda s: isinstance(s, ast.If) and isinstance(s.test, ast.Name) and s.test.id == "create_kf")
    run_code = compile(ast.Module(body=run, type_ignores=[]), fe, "exec")
    out, meta = {}, {}
    for name, c in decision_cases().items():
        cur_v, kf_v = visibility(c["cur_n"], c["kfs"])
        frames = sorted(set([c["cur"]] + list(c["window"])))
        cams = {f: camera(c["x"][f], z=0.01 * (f % 3), yaw=0.02 * (f % 5)) for f in frames}
        me = SimpleNamespace(config={"Training": c["cfg"]}, cameras=cams, median_depth=torch.tensor(MEDIAN_DEPTH),
                             initialized=c["initialized"])
        cur_t = torch.from_numpy(cur_v).long()
        occ = {k: torch.from_numpy(v).long() for k, v in kf_v.items()}
        if c["kind"] == "is_keyframe":
            result = dict(decision=bool(ns["is_keyframe"](me, c["cur"], c["window"][0], cur_t, occ)))
        elif c["kind"] == "wants_keyframe":
            me.current_window, me.occ_aware_visibility = list(c["window"]), occ
            me.kf_interval, me.window_size, me.single_thread = c["cfg"]["kf_interval"], c["cfg"]["window_size"], c["cfg"]["single_thread"]
            me.is_keyframe = functools.partial(ns["is_keyframe"], me)
            env = {"self": me, "torch": torch, "cur_frame_idx": c["cur"], "render_pkg": {"n_touched": torch.from_numpy(cur_v.astype(np.int32) * 7)}}
            exec(run_code, env)
            result = dict(decision=bool(env["create_kf"]))
        else:
            window, removed = ns["add_to_window"](me, c["cur"], cur_t, occ, list(c["window"]))
            result = dict(window_out=[int(w) for w in window], removed=None if removed is None else int(removed))
        meta[name] = dict(kind=c["kind"], config=c["cfg"], cur=c["cur"], window=list(c["window"]), initialized=c["initialized"],
                          median_depth=MEDIAN_DEPTH, frames=frames, kf_ids=list(kf_v.keys()), **result)
        out[name + "/cur"] = cur_v
        out[name + "/kf"] = np.stack([kf_v[k] for k in kf_v]) if kf_v else np.zeros((0, P_DEC), np.uint8)
        out[name + "/w2c"] = np.stack([ns["getWorld2View2"](cams[f].R, cams[f].T).numpy() for f in frames]).astype(np.float32)
        print(name, result)
    out["cases"] = np.array(json.dumps(meta, sort_keys=True))
    np.savez_compressed(os.path.join(HERE, "kf_decisions.npz"), **out)


def make_prune(ref):
    import covis_restated as cr

    be = os.path.join(ref, "utils", "slam_backend.py")
    stmts = _sibling_run(_function(be, "BackEnd", "map"), _assigns("prune_mode"),
                         lambda s: isinstance(s, ast.If) and "monocular" in ast.unparse(s.test))
    code = compile(ast.Module(body=stmts, type_ignores=[]), be, "exec")
    K, P = 8, 1000
    window = [31, 4, 27, 12, 19, 8, 23, 16]  # not sorted: the third-newest is 23
    n_touched = cr.make_case(P, K, 0.35, 5)
    vis = (n_touched > 0).astype(np.uint8)
    ids = np.random.default_rng(6).choice(np.array([0] + window, np.int32), size=P).astype(np.int32)
    out = dict(window=np.asarray(window, np.int32), n_touched=n_touched, visibility=vis, unique_kfIDs=ids)
    for mode in ("odometry", "slam"):
        for initialized in (False, True):
            me = SimpleNamespace(config={"Training": {"prune_mode": mode, "window_size": K}}, initialized=initialized,
                                 gaussians=SimpleNamespace(n_obs=torch.zeros(P).int(), unique_kfIDs=torch.from_numpy(ids.copy())),
                                 occ_aware_visibility={kf: torch.from_numpy(vis[k]).long() for k, kf in enumerate(window)})
            env = {"self": me, "torch": torch, "current_window": list(window)}
            exec(code, env)
            tag = "%s_%d" % (mode, int(initialized))
            out["to_prune_" + tag] = env["to_prune"].numpy().astype(np.uint8)
            out["n_obs_" + tag] = me.gaussians.n_obs.numpy().astype(np.int32)
            print(tag, "pruned", int(out["to_prune_" + tag].sum()), "of", P)
    np.savez_compressed(os.path.join(HERE, "covis_prune.npz"), **out)


if __name__ == "__main__":
    make_decisions(sys.argv[1])
    make_prune(sys.argv[1])
    for f in ("kf_decisions.npz", "covis_prune.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
