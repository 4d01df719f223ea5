"""CPU tests of the value fixture tests/distinct_hypers.py (no GPU): the drawn hyper-parameters differ along every axis, K_uu stays
as well conditioned as in the workload they replace (so the project's tolerances still apply), each index mistake the fixture is
for moves the oracle's nll by at least 1000 x the tolerance of the GPU tests that use the case, and the two CPU gradient
references agree on every case the gradient tests use.

Read the mutation test as the argument for tests/test_gpu_distinct_hypers.py: a kernel that reads `loglengthscales[d][p']` with the
wrong p', one lengthscale for every p, `logvariance` or `log_Q` of another latent dim (a missing `d_begin` offset) or the wrong
column of C / d / log_Rchols computes the mutated nll, which is at least 1000 tolerances away from the one the GPU test asks for.
On the workloads of `synthetic.make_workload` every one of these mutations changes the nll by exactly nothing."""
import numpy as np
import pytest

import distinct_hypers as dh
from ffvd_amd import synthetic
from oracle import ffvd_oracle as orc

DRAWN = ("loglengthscales", "logvariance", "log_Q", "CC", "DD", "log_Rchols")


@pytest.mark.parametrize("case", list(dh.CASES))
def test_entries_are_pairwise_distinct_along_every_axis(case):
    params, Y, c, meta = dh.workload(case)
    base = dh.base_workload(case)[0]
    for k in ("X", "Z", "U"):
        np.testing.assert_array_equal(params[k], base[k])              # inputs stay as drawn
    for k in DRAWN:
        a = params[k]
        assert a.shape == base[k].shape and np.all(np.isfinite(a)), k
        if k in ("loglengthscales", "logvariance") and meta["kernel_type"] != "SquaredExponential":
            np.testing.assert_array_equal(a, base[k])                   # LinearK: its variances already differ per d
            if k == "loglengthscales":
                continue
        for axis in range(a.ndim):
            lines = np.moveaxis(a, axis, -1).reshape(-1, a.shape[axis])
            for line in lines:
                assert len(np.unique(line)) == line.size, (k, axis)
    R = params["log_Rchols"]
    if meta["Ydim"] > 1:
        assert not np.any(R[0, 1:] == R[1:, 0])                         # row 0 (the one the likelihood reads) is not column 0
    if meta["kernel_type"] == "SquaredExponential":
        ls, var = np.exp(params["loglengthscales"]), np.exp(params["logvariance"])
        assert np.all((ls >= 0.7) & (ls <= 5.0)) and np.all((var >= 0.05) & (var <= 2.0))
    Q = np.exp(params["log_Q"])
    assert np.all((Q >= 0.02) & (Q <= 0.5))
    assert np.all((np.exp(R) >= 0.2) & (np.exp(R) <= 0.9))


def test_the_fixture_is_a_copy_and_the_workload_draw_is_untouched():
    params, Y, c, meta = synthetic.make_named("tiny")
    keep = {k: np.array(v) for k, v in params.items()}
    a, b = dh.distinct(params, meta, 7), dh.distinct(params, meta, 7)
    for k in params:
        np.testing.assert_array_equal(params[k], keep[k])
        np.testing.assert_array_equal(a[k], b[k])                       # seeded
        assert a[k] is not params[k]
    assert not np.array_equal(dh.distinct(params, meta, 8)["log_Q"], a["log_Q"])


@pytest.mark.parametrize("case", list(dh.CASES))
def test_condition_number_stays_within_four_times_the_base_workload(case):
    """cond(K_uu + 1e-5 I) <= 4 x the unmodified workload's for every (shape, seed) pair the GPU tests use: under that condition the
    project's tolerances -- the predicted 4 eps cond of the Gram route included -- still apply."""
    params, Y, c, meta = dh.workload(case)
    base = dh.base_workload(case)[0]
    kf, kb = dh.kuu_condition(params, meta), dh.kuu_condition(base, meta)
    print(f"{case}: cond(K_uu + jitter I) {kf:.2e}, base workload {kb:.2e}, ratio {kf / kb:.2f}")
    assert kf <= 4.0 * kb


def _mean_nll(params, Y, c, meta, collapse):
    return orc.nll_terms_chains(params, Y, c, U_collapse=collapse, kernel_type=meta["kernel_type"])["nll"]


@pytest.mark.parametrize("case", list(dh.CASES))
def test_each_index_mistake_moves_the_nll_by_1000_tolerances(case):
    params, Y, c, meta = dh.workload(case)
    muts = dh.mutations(meta)
    assert muts
    for collapse in (True, False) if case != "tshard" else (True,):          # (a T-shard handle has no explicit-U form)
        nll = dh.forward_reference(case, collapse)["nll"]
        tol = dh.nll_tolerance(case, collapse, nll)
        for name, fn in muts.items():
            moved = abs(_mean_nll(fn(params), Y, c, meta, collapse) - nll)
            print(f"{case} {'B' if collapse else 'A'} {name}: nll moves by {moved:.2e} = {moved / tol:.1e} x the tolerance {tol:.1e}")
            assert moved >= 1000.0 * tol, (case, collapse, name, moved, tol)


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_the_same_mistakes_are_invisible_on_the_plain_workload(name):
    """What the fixture is for: on `make_workload`'s values the lengthscale and variance mutations change nothing at all."""
    params, Y, c, meta = synthetic.make_named(name)
    nll = _mean_nll(params, Y, c, meta, True)
    for mut in ("roll loglengthscales along p", "broadcast ls[d][0] over p", "roll logvariance along d"):
        assert _mean_nll(dh.MUTATIONS[mut][1](params), Y, c, meta, True) == nll, mut


@pytest.mark.parametrize("case", list(dh.GRAD_CASES) + ["tshard", "lin_y2"])
def test_the_two_gradient_references_agree(case):
    """Closed form (oracle/ffvd_grad_oracle.py) against torch autograd of the independent restatement, per key and in the
    normalisation of the GPU tests (per latent dim for logvariance, log_Q and loglengthscales).  The GPU tests' bounds are never
    below 10 x this disagreement (distinct_hypers.grad_bound), so it has to stay small: 1e-8 or better on every key."""
    if case == "lin_y2":            # (the closed form is SE only: the LinearK gradient tests have autograd as their one reference)
        ref = dh.autograd_reference(case, True)
        assert all(np.all(np.isfinite(v)) for v in ref.values()) and "loglengthscales" not in ref
        return
    for collapse in (True, False) if case != "tshard" else (True,):
        errs = dh.reference_disagreement(case, collapse)
        print(f"{case} {'B' if collapse else 'A'}: " + ", ".join(f"{k}={v:.1e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 1e-8, (k, v)                               # the references pin every key to 1e-8 or better


@pytest.mark.parametrize("d_begin,d_count", [(1, 2), (2, 1)])
def test_index_mistakes_move_the_share_of_a_dim_shard(d_begin, d_count):
    """The shard test of the GPU file compares a shard that starts at d_begin > 0 with `orc.nll_terms_shard` at 1e-9 (1e-10 on the
    one-launch path): a shard that reads the variance, Q or lengthscales of the dims [0, d_count) instead of its own -- the missing
    d_begin offset -- moves that share by at least 1000 x the tolerance.  (On the plain workload the variance is the same for every
    dim and the mistake cancels.)"""
    params, Y, c, meta = dh.workload("ragged")
    D = meta["D"]
    assert d_begin + d_count == D

    def share(p, collapse):
        return np.mean([orc.nll_terms_shard(dict(p, X=p["X"][s]), Y, c, d_begin, d_count, False, U_collapse=collapse)["nll"]
                        for s in range(meta["S"])])

    for collapse in (True, False):
        nll = share(params, collapse)
        tol = 1e-9 * abs(nll)
        for key in ("logvariance", "log_Q", "loglengthscales"):
            moved = abs(share(dict(params, **{key: np.roll(params[key], d_begin, axis=0)}), collapse) - nll)     # dims [0, d_count) land on the shard's
            print(f"shard [{d_begin}, {d_begin + d_count}) {'B' if collapse else 'A'} {key} without the offset: share moves by {moved:.2e} "
                  f"= {moved / tol:.1e} x the tolerance {tol:.1e}")
            assert moved >= 1000.0 * tol, (key, moved, tol)
