"""The NumPy reference of the particle filter with adaptive resampling (tests/particle_adaptive_ref.py) pinned on its own, without a
GPU: against the bootstrap reference where it must equal it, against the product of the row likelihoods where it never resamples,
against the exact Kalman filter on the linear-Gaussian model of tests/test_particle_filter_ref.py, and on unobserved rows."""
import numpy as np
import pytest

import filter_ref as fr
import particle_adaptive_ref as pe
import particle_filter_ref as pf
from test_particle_filter_ref import _linear_model


def _draws(m, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m["n"], N, m["D"])), rng.random(m["n"]), rng.standard_normal((N, m["D"]))


def _cond(m):
    return lambda i, X: (X @ m["F"].T + m["b"][None, :], np.broadcast_to(m["v"], X.shape))


def _run(m, N, seed, thr, dtype=np.float64, run=pe.run):
    eps, unif, xi0 = _draws(m, N, seed)
    kw = {} if run is pf.run else dict(ess_threshold=thr)
    return run(_cond(m), m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["Q"], eps, unif, xi0, dtype=dtype, **kw)


def _kalman(m):
    return fr.filter(m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["v"] + m["Q"], fr.linear_transition(np.eye(m["D"]) + m["F"], m["b"]))


# ---- threshold 2: the bootstrap filter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["float64", "longdouble"])
@pytest.mark.parametrize("N", [48, 300])
def test_with_threshold_two_it_is_the_bootstrap_reference(dtype, N):
    """a = 0 on every row: exp(0) = 1, 0 + l = l, 1 x = x, A = N -- every key the two share with array_equal, in both dtypes"""
    m = _linear_model()
    a, b = _run(m, N, 3, 2.0, dtype), _run(m, N, 3, None, dtype, run=pf.run)
    for k in b:
        assert a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    seen = ~np.isnan(b["lpd_joint"])
    np.testing.assert_array_equal(a["resampled"], seen.astype(np.int64))
    np.testing.assert_array_equal(a["logw"], np.zeros_like(a["logw"]))
    W = a["weights"][seen]
    assert float(np.max(np.abs(W.sum(axis=1) - 1.0))) <= 1e-12


# ---- threshold 0: sequential importance sampling ------------------------------------------------------------------------------------------
def test_with_threshold_zero_the_weights_are_the_product_of_the_row_likelihoods_along_each_path():
    m = _linear_model()
    N = 64
    out = _run(m, N, 4, 0.0)
    np.testing.assert_array_equal(out["ancestors"], np.broadcast_to(np.arange(N), out["ancestors"].shape))
    np.testing.assert_array_equal(out["resampled"], np.zeros(m["n"], dtype=np.int64))
    # particle i keeps slot i: its path is particles[:, i]; log of the product of its row likelihoods over the observed entries
    X, Y, sd = out["particles"], m["Y"], m["sd"]
    r = Y[:, None, :] - (X @ m["CC"] + m["DD"][None, None, :])
    l = -0.5 * (np.log(2.0 * np.pi) + np.log(sd * sd))[None, None, :] - 0.5 * r * r / (sd * sd)[None, None, :]
    path = np.nansum(l, axis=2).sum(axis=0)                                        # (N,)
    w = np.exp(path - path.max())
    w /= w.sum()
    err = float(np.max(np.abs(out["weights"][-1] - w)))
    print(f"final weights against the normalised path likelihoods: max error {err:.3e}; ess {out['ess'][-1]:.2f} of {N}")
    assert err <= 1e-12
    # and the evidence estimate is the plain importance-sampling one: the mean of the path likelihoods
    want = path.max() + np.log(np.mean(np.exp(path - path.max())))
    assert abs(out["log_evidence"] - want) <= 1e-9 * (1.0 + abs(want))
    assert out["logw"][-1].max() == 0.0


# ---- the linear-Gaussian model: the exact answer is the Kalman filter --------------------------------------------------------------------
def test_on_a_linear_gaussian_model_the_filtered_mean_approaches_the_kalman_filter_s_as_n_grows():
    """thr = 0.5.  The root-mean-square error of m_filt over rows, dims and 8 seeds at N = 64, 512 and 4096: each step of 8 x in N
    must shrink it (a Monte-Carlo error shrinks by sqrt(8) = 2.8; asked: by 1.8), and at N = 4096 every entry lies within
    6 sqrt(diag(S_filt^KF) / ess) of the exact filter."""
    m, kf = _linear_model(), _kalman(_linear_model())
    rms = {}
    for N in (64, 512, 4096):
        errs = [_run(m, N, 300 + s, 0.5)["m_filt"] - kf["m_filt"] for s in range(8)]
        rms[N] = float(np.sqrt(np.mean(np.square(errs))))
    print("rms error of m_filt against the Kalman filter: " + ", ".join(f"N = {N}: {e:.5f}" for N, e in rms.items()))
    assert rms[512] <= rms[64] / 1.8 and rms[4096] <= rms[512] / 1.8
    out = _run(m, 4096, 100, 0.5)
    assert 0 < out["resampled"].sum() < np.sum(~np.isnan(out["lpd_joint"]))       # (rows of both kinds)
    for i in range(m["n"]):
        tol = 6.0 * np.sqrt(np.diagonal(kf["S_filt"][i]) / out["ess"][i])
        assert np.all(np.abs(out["m_filt"][i] - kf["m_filt"][i]) <= tol), i
    np.testing.assert_array_equal(out["S_pred"], np.swapaxes(out["S_pred"], -1, -2))
    np.testing.assert_array_equal(out["S_filt"], np.swapaxes(out["S_filt"], -1, -2))


@pytest.mark.parametrize("thr", [0.0, 0.5, 2.0])
def test_the_evidence_estimate_is_unbiased_whether_or_not_a_row_resamples(thr):
    """mean over 400 seeds of exp(log_evidence - the Kalman log-likelihood) at N = 256 is within 4 of its own sample standard errors
    of 1.  (The estimate itself is unbiased, not its logarithm.)"""
    m = _linear_model()
    exact = float(np.nansum(_kalman(m)["lpd_joint"]))
    ratio = np.exp(np.array([_run(m, 256, 1000 + s, thr)["log_evidence"] for s in range(400)]) - exact)
    mean, se = float(ratio.mean()), float(ratio.std(ddof=1) / np.sqrt(ratio.size))
    print(f"thr {thr}: mean ratio {mean:.4f}, standard error {se:.4f}, sd of log_evidence {float(np.std(np.log(ratio), ddof=1)):.4f}")
    assert abs(mean - 1.0) <= 4.0 * se


# ---- unobserved rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, 0.5])
def test_a_row_with_nothing_observed_changes_nothing_but_the_propagation(thr):
    """Row 7 of the model: identity ancestors, m_filt / S_filt = m_pred / S_pred bit for bit, a kept, weights = e / A, ess =
    A^2 / sum e^2, no decision; the particles of row 8 are those of row 7 pushed through the transition."""
    m = _linear_model()
    N = 64
    out = _run(m, N, 5, thr)
    np.testing.assert_array_equal(out["ancestors"][7], np.arange(N))
    np.testing.assert_array_equal(out["m_filt"][7], out["m_pred"][7])
    np.testing.assert_array_equal(out["S_filt"][7], out["S_pred"][7])
    assert np.isnan(out["lpd_joint"][7]) and np.all(np.isnan(out["lpd"][7])) and out["resampled"][7] == 0
    np.testing.assert_array_equal(out["logw"][7], out["logw"][6])
    e = np.exp(out["logw"][6])
    np.testing.assert_array_equal(out["weights"][7], e / e.sum())
    assert out["ess"][7] == e.sum() * e.sum() / (e * e).sum()
    if out["resampled"][6] == 0:                                                     # carried: the weights of row 6, up to the rounding of exp
        assert float(np.max(np.abs(out["weights"][7] - out["weights"][6]))) <= 1e-15
    eps = _draws(m, N, 5)[0]
    X = out["particles"][7]
    want = X + (X @ m["F"].T + m["b"][None, :]) + eps[8] * np.sqrt(m["v"] + m["Q"])[None, :]
    np.testing.assert_array_equal(out["particles"][8], want)
    assert out["log_evidence"] == np.nansum(out["lpd_joint"])


def test_the_margin_measures_the_distance_of_ess_to_the_threshold():
    """`margin` on one track shaped as `tracks` shapes it: ess_gap is the smallest |ess / N - thr| over the observed rows, and a
    threshold moved onto a row's ess / N closes it."""
    m = _linear_model()
    out = _run(m, 48, 6, 0.5)
    ref = {k: np.asarray(v)[None, None] for k, v in out.items() if k != "log_evidence"}
    unif = _draws(m, 48, 6)[1]
    got = pe.margin(ref, unif, 0.5)
    seen = ~np.isnan(out["lpd_joint"])
    assert got["ess_gap"] == float(np.min(np.abs(out["ess_frac"][seen] - 0.5))) and got["same"] and got["same_decisions"]
    row = int(np.flatnonzero(seen)[2])
    assert pe.margin(ref, unif, float(out["ess_frac"][row]))["ess_gap"] == 0.0
