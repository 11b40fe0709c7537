"""NumPy restatement of the reference's prune_points + _prune_optimizer (gaussian_splatting/scene/gaussian_model.py:559-597) on the
record tests/golden/make_prune_goldens.py writes: WHICH tensors lose rows (the six parameters, exp_avg and exp_avg_sq of each, the
three bookkeeping tensors, unique_kfIDs and n_obs), that the kept rows keep their order and their bits (none is reset), and that
the optimizer's step is left alone.  Shared by the CPU test and the GPU tests."""
import numpy as np

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
AUX = ("xyz_gradient_accum", "denom", "max_radii2D", "unique_kfIDs", "n_obs")


def case(z, name):
    """The arrays of one case ("aniso" / "iso") of prune_P120.npz without their prefix."""
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def keep_rows(a, mask):
    """a[~mask] spelled out: the stable order of the rows whose mask byte is zero."""
    return np.stack([a[i] for i in range(a.shape[0]) if not mask[i]]) if not mask.all() else a[:0]


def prune(rec):
    """in_* + mask -> the out_* the reference leaves."""
    mask = rec["mask"] != 0
    out = {}
    for n in NAMES:
        for pre in ("", "exp_avg_", "exp_avg_sq_"):
            out["out_%s%s" % (pre, n)] = keep_rows(rec["in_%s%s" % (pre, n)], mask)
        out["out_step_" + n] = rec["in_step_" + n]
    for a in AUX:
        out["out_" + a] = keep_rows(rec["in_" + a], mask)
    return out


def bits(a):
    """The array's bytes as integers, so that a comparison sees NaN payloads and signed zeros."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize % 4 else a.view(np.int32)
