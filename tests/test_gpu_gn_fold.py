"""GPU: the fold of the partial rows (csrc/gn_state.h gn_sum_rows) as gsaj_pose_gn_step and gsaj_pose_gn8_step run it, on synthetic
rows, against tests/gn_restated.fold_rows BIT FOR BIT: float64 addition in a fixed order is reproducible, so there is no tolerance.

The row counts sit on either side of one row group per row (32 / 16), of one full trip of the four-deep load loop (128 / 64 rows) and
of two (257 / 129): the path a real frame takes (640 x 480 has 4800 rows), which the Jacobian and alignment cases, tens of rows each,
do not reach.  The step is the first call on a zeroed state, so it accepts: the accepted H and g and the three loss floats of the state
are the sums."""
import numpy as np
import pytest

import gn_restated as gn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _rows(n, row, seed):
    """Random finite fp32 rows over twelve binades of magnitude and both signs (the order of the additions matters); slot 30 holds
    small integers, as a count does."""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((n, row)) * 10.0 ** rng.integers(-6, 7, (n, row))).astype(F)
    rows[:, 30] = rng.integers(0, 257, n).astype(F)
    assert np.isfinite(rows).all()
    return rows


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


# (entry, floats of the state, floats of a row, row groups, unknowns, where the state keeps the accepted g)
FORMS = {6: ("gsaj_pose_gn_step", 136, 32, 32, 125), 8: ("gsaj_pose_gn8_step", 152, 64, 16, 140)}
CASES = [(6, n) for n in (1, 31, 32, 33, 127, 128, 129, 257)] + [(8, n) for n in (1, 15, 16, 17, 63, 64, 65, 129)]


@pytest.mark.parametrize("nx,n", CASES, ids=["gn%d-%d" % c for c in CASES])
def test_the_accepted_sums_of_a_first_step_are_the_ordered_float64_fold(nx, n):
    import torch

    from gsaj import _lib
    lib = _lib.load()
    name, floats, row, groups, g_at = FORMS[nx]
    nh = nx * (nx + 1) // 2
    rows = _rows(n, row, 100 * nx + n)
    want = gn.fold_rows(rows, groups).astype(F)
    partials = torch.from_numpy(rows).to(DEV)
    state = torch.zeros(floats, dtype=torch.float32, device=DEV)
    proj = torch.eye(4, dtype=torch.float32, device=DEV)
    _lib.check(getattr(lib, name)(partials.data_ptr(), n, 1e-3, 4.0, 1e-7, 1e7, 1e-4, proj.data_ptr(), state.data_ptr(), None,
                                  torch.cuda.current_stream().cuda_stream), name)
    s = state.cpu().numpy()
    assert s[82] == 1.0 and s[83] == 1.0 and s[84] == 0.0, "the first call accepts"
    got = np.concatenate([s[104:104 + nh], s[g_at:g_at + nx], s[85:88]])
    bad = np.nonzero(_bits(got) != _bits(want[:nh + nx + 3]))[0]
    assert bad.size == 0, "slots %s: device %s, ordered fold %s" % (bad.tolist(), got[bad], want[bad])
    assert _bits(s[81:82]) == _bits(want[nh + nx:nh + nx + 1]), "the accepted loss is the loss sum"
