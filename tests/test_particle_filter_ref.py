"""The NumPy reference of the particle filter (tests/particle_filter_ref.py) pinned on its own, without a GPU: against the exact
Kalman filter on a linear-Gaussian model, the properties of systematic resampling, unobserved rows, and the measure of the margin
condition that tests/test_gpu_filter_particle.py rests on when it asks the device for identical ancestors."""
import numpy as np
import pytest

import filter_ref as fr
import particle_filter_ref as pf


# ---- a linear-Gaussian model: the exact answer is the Kalman filter ------------------------------------------------------------------
def _linear_model():
    rng = np.random.default_rng(11)
    D, J, n = 3, 2, 12
    F = 0.15 * rng.standard_normal((D, D)) - 0.1 * np.eye(D)
    b = 0.1 * rng.standard_normal(D)
    v, Q = np.array([0.02, 0.05, 0.03]), np.array([0.04, 0.02, 0.05])
    CC, DD, sd = rng.standard_normal((D, J)), 0.2 * rng.standard_normal(J), np.array([0.3, 0.5])
    x0, A0 = rng.standard_normal(D), rng.standard_normal((D, D))
    S0 = 0.2 * (A0 @ A0.T / D + 0.1 * np.eye(D))
    S0 = np.triu(S0) + np.triu(S0, 1).T
    x, Y = x0 + np.linalg.cholesky(S0) @ rng.standard_normal(D), np.empty((n, J))
    for i in range(n):
        x = x + F @ x + b + np.sqrt(v + Q) * rng.standard_normal(D)
        Y[i] = x @ CC + DD + sd * rng.standard_normal(J)
    Y[4, 1] = np.nan
    Y[7] = np.nan
    return dict(F=F, b=b, v=v, Q=Q, CC=CC, DD=DD, sd=sd, x0=x0, S0=S0, Y=Y, D=D, n=n)


def _run_linear(m, N, seed):
    rng = np.random.default_rng(seed)
    cond = lambda i, X: (X @ m["F"].T + m["b"][None, :], np.broadcast_to(m["v"], X.shape))
    return pf.run(cond, m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["Q"], rng.standard_normal((m["n"], N, m["D"])),
                  rng.random(m["n"]), rng.standard_normal((N, m["D"])))


def test_on_a_linear_gaussian_model_the_filter_approaches_the_kalman_filter():
    """Affine conditional mean F x + b, constant variance, N = 4096: m_filt within 6 sqrt(diag(S_filt^KF) / ess) of the exact filter at
    every one of the 12 rows; log_evidence within 6 of its Monte-Carlo standard errors, estimated from 20 further seeds."""
    m = _linear_model()
    D = m["D"]
    kf = fr.filter(m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["v"] + m["Q"], fr.linear_transition(np.eye(D) + m["F"], m["b"]))
    out = _run_linear(m, 4096, 100)
    for i in range(m["n"]):
        tol = 6.0 * np.sqrt(np.diagonal(kf["S_filt"][i]) / out["ess"][i])
        err = np.abs(out["m_filt"][i] - kf["m_filt"][i])
        print(f"row {i}: ess {out['ess'][i]:.1f}, |m_filt - KF| {np.round(err, 5).tolist()}, 6 se {np.round(tol, 5).tolist()}")
        assert np.all(err <= tol), i
    exact = float(np.nansum(kf["lpd_joint"]))
    se = float(np.std([_run_linear(m, 4096, 200 + s)["log_evidence"] for s in range(20)], ddof=1))
    print(f"log_evidence {out['log_evidence']:.5f}, Kalman {exact:.5f}, Monte-Carlo standard error {se:.5f}")
    assert abs(out["log_evidence"] - exact) <= 6.0 * se
    assert np.isnan(out["lpd_joint"][7]) and np.all(np.isnan(out["lpd"][7])) and np.isnan(out["lpd"][4, 1]) and np.isfinite(out["lpd"][4, 0])
    np.testing.assert_array_equal(out["S_pred"], np.swapaxes(out["S_pred"], -1, -2))
    np.testing.assert_array_equal(out["S_filt"], np.swapaxes(out["S_filt"], -1, -2))


# ---- systematic resampling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_systematic_ancestors_are_sorted_and_offspring_counts_are_within_one(seed):
    rng = np.random.default_rng(seed)
    N = 257
    W = np.exp(2.0 * rng.standard_normal(N))
    a, cdf, tot = pf.ancestors(W, rng.random())
    assert a.shape == (N,) and a.min() >= 0 and a.max() <= N - 1
    assert np.all(np.diff(a) >= 0)
    counts = np.bincount(a, minlength=N)
    assert np.all(np.abs(counts - N * W / W.sum()) < 1.0 + 1e-9)


def test_equal_weights_give_the_identity_for_every_uniform():
    """unif -> 1 from below is taken to 1 - 1e-12: far enough from 1 that unif + i is still resolved in fp64 for i < 2048 (spacing
    2.3e-13 at 2047; at 1 - 2^-53 the sum itself rounds to i + 1), close enough that any threshold convention off by one would show."""
    for N in (48, 2048):
        for u in (1e-12, 0.3, 1.0 - 1e-12):
            a, _, _ = pf.ancestors(np.ones(N), u)
            np.testing.assert_array_equal(a, np.arange(N))
    a, _, _ = pf.ancestors(np.ones(48, dtype=np.longdouble), np.nextafter(1.0, 0.0))
    np.testing.assert_array_equal(a, np.arange(48))


# ---- unobserved rows -----------------------------------------------------------------------------------------------------------------
def test_a_row_with_nothing_observed_changes_nothing_but_the_propagation():
    m = _linear_model()
    out = _run_linear(m, 64, 5)
    N = 64
    np.testing.assert_array_equal(out["ancestors"][7], np.arange(N))
    np.testing.assert_array_equal(out["m_filt"][7], out["m_pred"][7])
    np.testing.assert_array_equal(out["S_filt"][7], out["S_pred"][7])
    assert out["ess"][7] == N and np.isnan(out["lpd_joint"][7])
    # the particles of row 8 are those of row 7 pushed through the transition: no resampling in between
    rng = np.random.default_rng(5)
    eps = rng.standard_normal((m["n"], N, m["D"]))
    X = out["particles"][7]
    want = X + (X @ m["F"].T + m["b"][None, :]) + eps[8] * np.sqrt(m["v"] + m["Q"])[None, :]
    np.testing.assert_array_equal(out["particles"][8], want)
    assert out["log_evidence"] == np.nansum(out["lpd_joint"])


# ---- the margin condition of the device tests ------------------------------------------------------------------------------------------
def test_the_margin_of_a_track_is_measured_against_every_cdf_entry():
    """`margin` on the linear model: fp64 against np.longdouble draw identical ancestors and the smallest distance of a threshold
    (unif + i) / N to a cdf_k / tot exceeds max(1e-8, 1000 x the cdf drift between the precisions) -- the condition
    tests/test_gpu_filter_particle.py asserts for every one of its fixtures (they are built on the device's posterior path, so that
    check is marked gpu); a threshold moved onto a cdf entry is seen."""
    m = _linear_model()
    N, rng = 48, np.random.default_rng(9)
    eps, unif, xi0 = rng.standard_normal((m["n"], N, m["D"])), rng.random(m["n"]), rng.standard_normal((N, m["D"]))
    res = {}
    for t in (np.float64, np.longdouble):
        cond = lambda i, X, t=t: (X @ np.asarray(m["F"], dtype=t).T + np.asarray(m["b"], dtype=t)[None, :],
                                  np.broadcast_to(np.asarray(m["v"], dtype=t), X.shape))
        f = pf.run(cond, m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["Q"], eps, unif, xi0, dtype=t)
        res[t] = {k: np.asarray(v)[None, None] for k, v in f.items()}
    gap, drift, same = pf.margin(res[np.float64], unif, res[np.longdouble])
    print(f"smallest gap {gap:.3e}, cdf drift {drift:.3e}, identical ancestors {same}")
    assert same and gap >= max(1e-8, 1000.0 * drift) and gap < 1.0 / N
    moved = np.array(unif)
    moved[3] = (res[np.float64]["cdf"][0, 0, 3, 10] * N) % 1.0    # a threshold of row 3 on cdf entry 10
    assert pf.margin(res[np.float64], moved)[0] < 1e-12
