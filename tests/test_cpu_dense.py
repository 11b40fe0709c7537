"""The dense path's fp64 restatement (tests/dense_restated.py) without a device: pinned to the arrays recorded from the reference,
shown to be feasible for a correct fp32 evaluation (oracle/dense_oracle.py passes its bounds on every generated case), and shown to
reject wrong kernels (the `mutant=` switch).

| id | bug                                                              | case                        | rejected at            |
|----|------------------------------------------------------------------|-----------------------------|------------------------|
| D1 | suffix includes the Gaussian's own term                          | stack-129, saturated-129    | front rows             |
| D2 | guard at 0.99 instead of 0.999; naive: suffix / 1 for dropped    | saturated-129, both modes   | rows with 0.99 .. 0.999|
| D3 | Gaussian 128 missing from the pass-1 totals                      | needles-129, offscreen-300  | rows in front of 128   |
| D4 | pixels of the ragged last workgroup skipped                      | saturated-129 (33x17)       | rows under pixels 512..|
| D5 | T not advanced across a chunk boundary                           | needles-129, saturated-300  | rows 128..             |
| D6 | dL/dSigma off-diagonals swapped / symmetrised                    | offscreen-129, cov asymm.   | dL/dSigma[0][1], [1][0]|
| D7 | back-most row off by 5e-4 of the tensor's max (old blind spot)   | stack-300, oracle's output  | old check PASSES it    |
| D8 | suffix as fp64 total - fp64 prefix (k_dense_bwd once did)        | stack-129 .. stack-300      | rows with T < 1e-11    |
"""
import os

import numpy as np
import pytest

import dense_restated as dr
from oracle import dense_oracle as dor

TOL = 5e-4   # tests/test_gpu_dense.py: the tolerance its tensor-wide check uses for the recorded arrays
DENSE = ["dense_N1_64x48.npz", "dense_N15_64x48.npz", "dense_N15_64x48_ortho.npz", "dense_N64_64x48.npz", "dense_N15_640x480.npz"]


def _rel(a, b):
    """The old check of tests/test_gpu_dense.py: max |err| over the tensor's max."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def rejected(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


def case(kind, N, naive=False, variant="pixel"):
    (c,) = [c for c in dr.CASES if c[0] == kind and c[1] == N]
    return dr.make_case(*c, naive=naive, variant=variant)


def f32(a):
    return np.asarray(a, np.float32)


# ---- pinned to the recordings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DENSE)
def test_restatement_reproduces_the_dense_goldens(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    r = dr.restate(g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["opacities"][g["order"], 0], f32(g["seed_color"]), f32(g["seed_depth"]))
    N = int(g["N"])
    for s, want, nm in ((slice(0, 2), g["grad_mu"], "mu"), (slice(2, 6), g["grad_Sigma"], "Sigma"), (slice(6, 7), g["grad_depth"], "depth"),
                        (slice(7, 10), g["grad_color"], "color")):
        assert _rel(r["value"][:, s].reshape(np.asarray(want).shape), want) < TOL, (name, nm)
    assert r["value"].shape == (N, 10) and (r["mass"] >= np.abs(r["value"]) * (1 - 1e-12)).all() and (r["cond"] >= 0).all()


@pytest.mark.parametrize("name", ["dense_normalised_N15_64x48.npz", "dense_normalised_N64_64x48.npz"])
def test_restatement_reproduces_the_normalised_goldens(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    intr = (float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"]))
    r = dr.restate(g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["alpha"], f32(g["seed_color"]), f32(g["seed_depth"]),
                   normalised_intrinsics=intr)
    assert np.abs(r["value"][:, 0:2] - g["grad_mu"]).max() < 2e-5 * np.abs(g["grad_mu"]).max()
    assert np.abs(r["value"][:, 2:6].reshape(-1, 2, 2) - g["grad_Sigma"]).max() < 2e-5 * np.abs(g["grad_Sigma"]).max()


@pytest.mark.parametrize("name,naive", [("naive_N4_12x9.npz", False), ("naive_N4_12x9.npz", True), ("naive_edge_N5_12x9.npz", True)])
def test_restatement_reproduces_the_naive_loop_goldens(golden_dir, name, naive):
    g = np.load(os.path.join(golden_dir, name))
    order = np.argsort(g["depth"], kind="stable")
    r = dr.restate(g["mean_2D"][order], g["cov_2D"][order], g["color"][order], g["depth"][order], g["alpha"][order], f32(g["seed_color"]),
                   f32(g["seed_depth"]), naive_guards=naive)
    inv = np.argsort(order)
    mu, S = r["value"][inv, 0:2], r["value"][inv, 2:6].reshape(-1, 2, 2)
    assert np.abs(mu - g["grad_mu"]).max() < 3e-6 * np.abs(g["grad_mu"]).max()
    assert np.abs(S - g["grad_Sigma"]).max() < 3e-6 * np.abs(g["grad_Sigma"]).max()
    if name.startswith("naive_edge"):
        assert np.all(mu[3] == 0) and np.all(r["mass"][inv][3, :6] == 0)   # the 1e-9-opacity entry is skipped entirely


def test_restatement_reproduces_the_render_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "dense_N15_640x480.npz"))
    rec = np.load(os.path.join(golden_dir, "dense_render_N15_640x480.npz"))
    r = dr.restate(g["mean_2D"], g["cov_2D"], g["color"], g["depth"], g["opacities"][g["order"], 0], f32(g["seed_color"]), f32(g["seed_depth"]))
    img = np.clip(r["render_value"][:, :3].reshape(480, 640, 3), 0.0, 1.0)
    assert np.abs(img[::4, ::4] - rec["image_sub4"]).max() < 3e-6 * max(float(rec["vmax"]), 1.0)
    assert np.abs(img.sum(axis=1) - rec["row_sum"]).max() < 1e-5 * np.abs(rec["row_sum"]).max()
    assert np.abs(img.sum(axis=0) - rec["col_sum"]).max() < 1e-5 * np.abs(rec["col_sum"]).max()


# ---- the bound is not tighter than fp32 allows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", dr.runs(), ids=dr.run_id)
def test_fp32_oracle_is_within_the_bounds_and_margins_hold(run):
    """oracle/dense_oracle.py is a correct fp32 evaluation in another summation order (suffix sums from the back, NumPy's pairwise
    row sums): it must pass, and so must the restatement itself.  make_case asserts the guard margins of the case."""
    c, naive, variant = run
    inp, intr, r = dr.make_case(*c, naive=naive, variant=variant)
    m = r["margins"]
    for k in ("0.999", "clip") + (("1e-8",) if c[0] in dr.NAIVE_KINDS else ()):
        assert m[k] >= dr.MARGIN and m["scaled"][k] >= 1.0, (dr.run_id(run), k, m[k])
    assert max(dr.assert_dense_close(r["value"], r, dr.run_id(run)).values()) == 0.0
    got = dor.dense_backward(*dr.args_of(inp), naive_guards=naive, normalised_intrinsics=intr)
    dr.note("oracle_fp32_cpu", "test_dense_backward_per_gaussian_bounds", dr.assert_dense_close(got, r, dr.run_id(run)))
    if not naive and variant == "pixel":
        img, dep = dor.dense_render(*dr.args_of(inp)[:5], c[3], c[2])
        dr.note("oracle_fp32_cpu", "test_dense_render_per_pixel_bounds", dr.assert_render_close(img, dep, r, dr.run_id(run)))


def test_cases_cover_the_boundaries():
    ns = {c[1] for c in dr.CASES}
    assert ns == {1, 2, 127, 128, 129, 255, 256, 257, 300}
    for n in ns:   # every N at least once on an image that is no multiple of the workgroup
        assert any(c[1] == n and (c[2] * c[3]) % dr.WG for c in dr.CASES), n
    for kind in dr.KINDS:
        assert {129, 300} <= {c[1] for c in dr.CASES if c[0] == kind}, kind
    assert {(c[2], c[3]) for c in dr.CASES} == {(16, 16), (17, 15), (33, 17), (64, 48)}
    assert any(naive for _, naive, _ in dr.runs()) and any(v == "normalised" for _, _, v in dr.runs())


def test_saturated_and_offscreen_cases_reach_their_branches():
    inp, _, r = case("saturated", 129)
    o = inp["opac"]
    assert (o == 1.0).any() and (o == 1.5).any() and ((o > 0.999) & (o < 1.0)).any() and ((o > 0.99) & (o < 0.999)).any()
    inp, _, r = case("offscreen", 300)
    assert (r["mass"].max(axis=1) == 0).any() and (inp["opac"] < 1e-8).any()          # a row no pixel reaches; alphas below 1e-8
    assert ((inp["means2D"][:, 0] < 0) | (inp["means2D"][:, 0] > 32)).sum() > 20
    inp, _, _ = case("needles", 129)
    S = inp["covs2D"].astype(np.float64)
    assert 3e3 < np.linalg.cond(S).max() <= 1.1e4


# ---- canaries ------------------------------------------------------------------------------------------------------------------------
def _mutant_rejected(kind, N, mutant, naive=False):
    inp, intr, r = case(kind, N, naive=naive)
    m = dr.restate(*dr.args_of(inp), naive_guards=naive, normalised_intrinsics=intr, mutant=mutant)
    msg = rejected(lambda: dr.assert_dense_close(m["value"], r, "%s/%s-%d" % (mutant, kind, N)))
    assert msg is not None and "of Gaussian" in msg, (mutant, kind, N, msg)
    return msg


@pytest.mark.parametrize("kind,N", [("stack", 129), ("saturated", 129)])
def test_canary_suffix_includes_own_term(kind, N):
    _mutant_rejected(kind, N, "suffix_with_self")


@pytest.mark.parametrize("naive", [False, True])
def test_canary_guard_threshold_moved(naive):
    _mutant_rejected("saturated", 129, "guard_099", naive=naive)


@pytest.mark.parametrize("kind,N", [("needles", 129), ("offscreen", 300)])
def test_canary_first_gaussian_of_second_chunk_missing_from_totals(kind, N):
    _mutant_rejected(kind, N, "totals_skip_128")


def test_canary_ragged_last_workgroup_skipped():
    _mutant_rejected("saturated", 129, "skip_ragged_block")


@pytest.mark.parametrize("kind,N", [("needles", 129), ("saturated", 300)])
def test_canary_T_not_advanced_across_chunk_boundary(kind, N):
    msg = _mutant_rejected(kind, N, "T_stalls_at_chunk")
    assert int(msg.split("of Gaussian ")[1].split()[0]) >= dr.DCHUNK, msg


@pytest.mark.parametrize("mutant", ["sigma_swapped", "sigma_symmetrised"])
def test_canary_sigma_off_diagonals(mutant):
    inp, _, _ = case("offscreen", 129)
    cov = inp["covs2D"].copy()
    cov[:, 0, 1] *= np.float32(1.01)   # slightly asymmetric: q = Sigma^-1 D and r = D^T Sigma^-1 differ
    args = (inp["means2D"], cov) + dr.args_of(inp)[2:]
    r = dr.restate(*args)
    assert np.abs(r["value"][:, 3] - r["value"][:, 4]).max() > 1e-4 * np.abs(r["value"][:, 3]).max()   # [0][1] = 1/2 w q_0 r_1, [1][0] = 1/2 w q_1 r_0
    msg = rejected(lambda: dr.assert_dense_close(dr.restate(*args, mutant=mutant)["value"], r, mutant))
    assert msg is not None and "dL/dSigma[" in msg and "of Gaussian" in msg, msg


@pytest.mark.parametrize("N", [129, 300])
def test_canary_old_blind_spot_back_row(N):
    """The oracle's own output with the back-most row off by 5e-4 of the tensor's max (less 0.1 %, so that the old check's strict
    `<` holds): the tensor-wide check test_gpu_dense.py had passes it, the per-row comparator rejects it and names the row."""
    inp, _, r = case("stack", N)
    want = dor.dense_backward(*dr.args_of(inp))
    ok = dr.to10(*want)
    bad = ok.copy()
    for nm, s in dr.TENSORS:
        bad[N - 1, s.start] += 0.999 * TOL * np.abs(ok[:, s]).max()
        assert _rel(bad[:, s], ok[:, s]) < TOL                    # the old check: passes
    assert max(dr.assert_dense_close(ok, r, "oracle").values()) < 1.0
    for nm, s in dr.TENSORS:
        one = ok.copy()
        one[N - 1, s.start] = bad[N - 1, s.start]
        msg = rejected(lambda: dr.assert_dense_close(one, r, "blind-spot/" + nm))
        assert msg is not None and "of Gaussian %d " % (N - 1) in msg, (nm, msg)


@pytest.mark.parametrize("N", [129, 255, 300])
def test_canary_suffix_as_total_minus_prefix(N):
    """What k_dense_bwd once did: S_i = fp64 total - fp64 prefix is rounded at 1e-16 of the total, and behind a stack with
    T < 1e-11 that is more than S_i itself.  The old tensor-wide check cannot see it; the per-row bound does."""
    inp, _, r = case("stack", N)
    m = dr.restate(*dr.args_of(inp), mutant="suffix_total_minus_prefix")
    for nm, s in dr.TENSORS:
        assert _rel(m["value"][:, s], r["value"][:, s]) < TOL
    msg = _mutant_rejected("stack", N, "suffix_total_minus_prefix")
    assert "dL/dmu" in msg or "dL/dSigma" in msg
