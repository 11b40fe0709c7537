#!/usr/bin/env python3
"""Every output of the Gauss-Newton entry points on the scene of tests/gn_single_view_cases.py (200 Gaussians, 40 x 24, SH and
precomputed colours), as SHA-256: the five Jacobian entry points -- explicit (H, g, jac_out, the re-derived images), loss-fused and
joint through the single-frame forms for each of the three views, and through the batched forms at K = 1 and K = 3 (partials, jac_out)
-- and the four step entry points: the state after each of three steps (forward at the state's pose, Jacobian walk, step), single
and batched at K = 1 and K = 3.  Run once per library (GSAJ_LIB_PATH names the one to load), one process each, the same package; the
calls and their arguments are the same, so the two outputs must be equal hash for hash.

    GSAJ_LIB_PATH=<parent's library> python tools/gn_same_bits.py PARENT.json
    python tools/gn_same_bits.py CHANGE.json
    python tools/gn_same_bits.py --compare PARENT.json CHANGE.json OUT.json
"""
import numpy as np

from same_bits import main, sha


def run(torch):
    import gn_single_view_cases as cs
    from gsaj.gauss_newton import GaussNewtonTracker, GaussNewtonWindow

    out = {}
    for colours in cs.COLOURS:
        w = cs.World(colours)
        for v in range(cs.K):
            fr = cs.Frame(w, v)
            o = fr.jac(seeds=w.seeds, curvature=w.curv, want_jacobian=True, want_images=True)
            out["%s/explicit/view%d" % (colours, v)] = {k: sha(o[k]) for k in ("H", "g", "jacobian", "color", "depth")}
            for joint in (False, True):
                o = fr.jac_loss(joint)
                out["%s/%s/single/view%d" % (colours, "loss8" if joint else "loss", v)] = dict(partials=sha(o["partials"]), jac_out=sha(o["jacobian"]))
        for k in (1, cs.K):
            win = cs.Window(w, k)
            for joint in (False, True):
                o = win.jac_loss(joint)
                out["%s/%s/batch/K%d" % (colours, "loss8" if joint else "loss", k)] = dict(partials=sha(o["partials"]), jac_out=sha(o["jacobian"]))
        # three steps of the trackers: every view starts at its neighbour's pose
        head = (cs.P, cs.W, cs.H, 16, w.dev)
        cam = (w.praw.reshape(4, 4), w.tan[0], w.tan[1], w.bg, w.means, w.opac)
        starts = [w.w2cs[(v + 1) % cs.K] for v in range(cs.K)]
        for joint in (False, True):
            form = "gn8" if joint else "gn"
            for v in range(cs.K):
                tr = GaussNewtonTracker(*head, starts[v], *cam, alpha=0.9, irls_delta=0.03, solve_exposure=joint, **w.kw)
                tr.set_frame(w.gt_c[v], w.gt_d[v], grad_mask=w.mask[v].reshape(1, cs.H, cs.W))
                for it in range(3):
                    tr.iterate(1)
                    out["%s/%s/step/view%d/it%d" % (colours, form, v, it)] = dict(state=sha(tr.state))
            for k in (1, cs.K):
                win = GaussNewtonWindow(k, *head[:4], w.dev, np.stack(starts[:k]), *cam, alpha=0.9, irls_delta=0.03, solve_exposure=joint, **w.kw)
                for v in range(k):
                    win.set_view(v, w.gt_c[v], w.gt_d[v], grad_mask=w.mask[v].reshape(1, cs.H, cs.W))
                for it in range(3):
                    win.iterate(1)
                    out["%s/%s/step_batch/K%d/it%d" % (colours, form, k, it)] = dict(state=sha(win.state), best=repr(win.best()))
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    main("gn_same_bits", run, "tools/gn_same_bits.py on the parent's library and on this change's, one process each, the same package: SHA-256 of "
         "every output of the five Jacobian entry points and of the state after each of three steps through the four step entry points")
