"""The NumPy reference of the fully adapted particle filter (tests/particle_adapted_ref.py) pinned on its own, without a GPU: against
the exact Kalman filter where the transition does not depend on x (every weight is 1: the filter is exact at any N), its scalar updates
against the batch update, against the Kalman filter on the linear-Gaussian model of tests/test_particle_filter_ref.py, against the
bootstrap reference on a record with sharp observations (the point of the method), unobserved rows, and the two precisions."""
import numpy as np

import cubature_filter_ref as cf
import filter_ref as fr
import particle_adapted_ref as pa
import particle_filter_ref as pf
from test_particle_filter_ref import _linear_model


def _cond(m, t=np.float64):
    F, b, v = np.asarray(m["F"], dtype=t), np.asarray(m["b"], dtype=t), np.asarray(m["v"], dtype=t)
    return lambda i, X: (X @ F.T + b[None, :], np.broadcast_to(v, X.shape))


def _draws(m, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m["n"], N, m["D"])), rng.random(m["n"]), rng.standard_normal((N, m["D"]))


def _run(mod, m, N, seed, dtype=np.float64):
    eps, unif, xi0 = _draws(m, N, seed)
    return mod.run(_cond(m, dtype), m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["Q"], eps, unif, xi0, dtype=dtype)


def _kalman(m):
    D = m["D"]
    return fr.filter(m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["v"] + m["Q"], fr.linear_transition(np.eye(D) + m["F"], m["b"]))


def _sharp_model():
    """The linear model with ten times sharper observations, sd = (0.03, 0.05): the record regenerated from the same model with
    default_rng(77), Y[4, 1] = Y[7] = NaN as before."""
    m = dict(_linear_model())
    rng = np.random.default_rng(77)
    D, n = m["D"], m["n"]
    m["sd"] = np.array([0.03, 0.05])
    x, Y = m["x0"] + np.linalg.cholesky(m["S0"]) @ rng.standard_normal(D), np.empty((n, 2))
    for i in range(n):
        x = x + m["F"] @ x + m["b"] + np.sqrt(m["v"] + m["Q"]) * rng.standard_normal(D)
        Y[i] = x @ m["CC"] + m["DD"] + m["sd"] * rng.standard_normal(2)
    Y[4, 1] = np.nan
    Y[7] = np.nan
    m["Y"] = Y
    return m


# ---- a transition that does not depend on x: every weight is 1 ---------------------------------------------------------------------------
def test_with_an_x_independent_transition_every_weight_is_one_and_the_filter_is_the_kalman_filter():
    """F = -I (and b = 0, so that X + (-X) is exactly 0 in floating point and every parent has the same mu bit for bit): x_{t+1} ~
    N(0, v + Q) whatever x_t is.  Every parent then predicts y_t equally well: ess == N exactly at every row, and lpd_joint, m_filt and
    S_filt are the Kalman filter's at any N (here 16) to 1e-12 -- no Monte-Carlo error is left in them."""
    m = dict(_linear_model())
    D = m["D"]
    m["F"], m["b"] = -np.eye(D), np.zeros(D)
    out, kf = _run(pa, m, 16, 3), _kalman(m)
    assert np.all(out["ess"] == 16.0)
    for k in ("lpd_joint", "m_filt", "S_filt"):
        ok = ~np.isnan(kf[k])
        np.testing.assert_array_equal(np.isnan(out[k]), ~ok, err_msg=k)
        err = float(np.max(np.abs(out[k][ok] - kf[k][ok])))
        print(f"x-independent transition: {k}: max error against the Kalman filter {err:.3e}")
        assert err <= 1e-12, k
    assert abs(out["log_evidence"] - np.nansum(kf["lpd_joint"])) <= 1e-12 * m["n"]


# ---- the scalar updates ----------------------------------------------------------------------------------------------------------------
def test_the_ascending_scalar_updates_equal_the_batch_update():
    """(mt, P, L) of `update` against the batch form through np.linalg.solve, J = 4 with one output unobserved, D = 3, 7 particles with
    different (mu, s): 1e-12.  P stays exactly symmetric."""
    rng = np.random.default_rng(5)
    N, D, J = 7, 3, 4
    mu, s = rng.standard_normal((N, D)), 0.05 + rng.random((N, D))
    CC, DD, sd = rng.standard_normal((D, J)), rng.standard_normal(J), 0.1 + rng.random(J)
    y, seen = rng.standard_normal(J), np.array([True, False, True, True])
    mt, P, L = pa.update(mu, s, y, seen, CC, DD, sd)
    np.testing.assert_array_equal(P, np.swapaxes(P, 1, 2))
    H = CC[:, seen].T
    for i in range(N):
        S0 = np.diag(s[i])
        S = H @ S0 @ H.T + np.diag(sd[seen] ** 2)
        r = y[seen] - (H @ mu[i] + DD[seen])
        K = np.linalg.solve(S, H @ S0).T
        want_m, want_P = mu[i] + K @ r, S0 - K @ H @ S0
        want_L = -0.5 * (seen.sum() * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + r @ np.linalg.solve(S, r))
        assert np.max(np.abs(mt[i] - want_m)) <= 1e-12 and np.max(np.abs(P[i] - want_P)) <= 1e-12 and abs(L[i] - want_L) <= 1e-12, i


def test_the_batched_factor_is_cubature_filter_ref_factor():
    """`factors` against cubature_filter_ref.factor matrix by matrix: positive definite, singular (a zero column) and indefinite
    inputs give the same zero columns, and entries within 1e-13 max|P| (the two sum the same <= 3 products per entry in different
    orders: a few units of 2^-53 of entries of size <= max|P|, divided by pivots >= 0.1 here)."""
    rng = np.random.default_rng(8)
    A = rng.standard_normal((6, 4, 4))
    P = A @ np.swapaxes(A, 1, 2)
    P[1, 2, :] = P[1, :, 2] = 0.0                                                   # a zero pivot
    P[2] = P[2] - 3.0 * np.eye(4)                                                   # indefinite
    P[3, 0, 0] = -1.0
    Lf, zeroed = pa.factors(P)
    for i in range(6):
        want = cf.factor(P[i])
        np.testing.assert_array_equal(Lf[i] == 0.0, want == 0.0, err_msg=str(i))
        assert np.max(np.abs(Lf[i] - want)) <= 1e-13 * np.max(np.abs(P[i])), i
        np.testing.assert_array_equal(zeroed[i], np.diagonal(Lf[i]) == 0.0)
    assert zeroed[1, 2] and zeroed[3, 0] and zeroed[2].any() and not zeroed[0].any()


# ---- against the Kalman filter ----------------------------------------------------------------------------------------------------------
def test_on_a_linear_gaussian_model_the_filter_approaches_the_kalman_filter():
    """The test of the bootstrap reference with the same bounds: N = 4096, m_filt within 6 sqrt(diag(S_filt^KF) / ess) of the exact
    filter at every one of the 12 rows; log_evidence within 6 of its Monte-Carlo standard errors, estimated from 20 further seeds."""
    m = _linear_model()
    kf, out = _kalman(m), _run(pa, m, 4096, 100)
    for i in range(m["n"]):
        tol = 6.0 * np.sqrt(np.diagonal(kf["S_filt"][i]) / out["ess"][i])
        err = np.abs(out["m_filt"][i] - kf["m_filt"][i])
        print(f"row {i}: ess {out['ess'][i]:.1f}, |m_filt - KF| {np.round(err, 5).tolist()}, 6 se {np.round(tol, 5).tolist()}")
        assert np.all(err <= tol), i
    exact = float(np.nansum(kf["lpd_joint"]))
    se = float(np.std([_run(pa, m, 4096, 200 + s)["log_evidence"] for s in range(20)], ddof=1))
    print(f"log_evidence {out['log_evidence']:.5f}, Kalman {exact:.5f}, Monte-Carlo standard error {se:.5f}")
    assert abs(out["log_evidence"] - exact) <= 6.0 * se
    assert np.isnan(out["lpd_joint"][7]) and np.all(np.isnan(out["lpd"][7])) and np.isnan(out["lpd"][4, 1]) and np.isfinite(out["lpd"][4, 0])
    np.testing.assert_array_equal(out["S_pred"], np.swapaxes(out["S_pred"], -1, -2))
    np.testing.assert_array_equal(out["S_filt"], np.swapaxes(out["S_filt"], -1, -2))


# ---- sharp observations: where the bootstrap filter collapses ---------------------------------------------------------------------------
def test_on_a_sharp_record_the_evidence_estimate_is_far_less_noisy_than_the_bootstrap_filter():
    """sd = (0.03, 0.05), 40 seeds, N = 64, the same draws for both filters: the standard deviation of log_evidence of the adapted
    filter is at most a third of the bootstrap filter's, and the adapted mean lies within 6 sd / sqrt(40) of the exact log evidence."""
    m = _sharp_model()
    exact = float(np.nansum(_kalman(m)["lpd_joint"]))
    le = {name: np.array([_run(mod, m, 64, 1000 + s)["log_evidence"] for s in range(40)]) for name, mod in (("adapted", pa), ("bootstrap", pf))}
    sd = {k: float(np.std(v, ddof=1)) for k, v in le.items()}
    mean = {k: float(np.mean(v)) for k, v in le.items()}
    print(f"sharp record: exact {exact:.4f}; adapted mean {mean['adapted']:.4f} sd {sd['adapted']:.4f}; bootstrap mean "
          f"{mean['bootstrap']:.4f} sd {sd['bootstrap']:.4f}; ratio {sd['bootstrap'] / sd['adapted']:.1f}")
    assert sd["adapted"] <= sd["bootstrap"] / 3.0
    assert abs(mean["adapted"] - exact) <= 6.0 * sd["adapted"] / np.sqrt(40.0)


# ---- unobserved rows and ordering -------------------------------------------------------------------------------------------------------
def test_unobserved_rows_keep_the_set_and_an_unobserved_record_is_the_bootstrap_rollout():
    m = _linear_model()
    N = 64
    out = _run(pa, m, N, 5)
    np.testing.assert_array_equal(out["ancestors"][7], np.arange(N))
    np.testing.assert_array_equal(out["m_filt"][7], out["m_pred"][7])
    np.testing.assert_array_equal(out["S_filt"][7], out["S_pred"][7])
    assert out["ess"][7] == N and np.isnan(out["lpd_joint"][7])
    assert np.all(np.diff(out["ancestors"], axis=1) >= 0) and out["ancestors"].min() >= 0 and out["ancestors"].max() <= N - 1
    assert out["log_evidence"] == np.nansum(out["lpd_joint"])
    # the set after the unobserved row 7 is the set after row 6 pushed through the transition with eps[7]
    eps = _draws(m, N, 5)[0]
    X = out["particles"][6]
    want = X + (X @ m["F"].T + m["b"][None, :]) + eps[7] * np.sqrt(m["v"] + m["Q"])[None, :]
    np.testing.assert_array_equal(out["particles"][7], want)
    blind = dict(m, Y=np.full_like(m["Y"], np.nan))
    a, b = _run(pa, blind, N, 5), _run(pf, blind, N, 5)
    np.testing.assert_array_equal(a["particles"], b["particles"])
    np.testing.assert_array_equal(a["ancestors"], np.broadcast_to(np.arange(N), a["ancestors"].shape))
    assert np.all(a["ess"] == N) and a["log_evidence"] == 0.0


# ---- the two precisions -----------------------------------------------------------------------------------------------------------------
def test_fp64_and_longdouble_draw_identical_ancestors():
    """The linear model and the sharp one, N = 48: identical ancestors in the two precisions, and the margin of
    tests/test_gpu_filter_adapted.py's condition (the thresholds stay away from the cdf entries)."""
    for name, m in (("linear", _linear_model()), ("sharp", _sharp_model())):
        unif = _draws(m, 48, 9)[1]
        res = {t: {k: np.asarray(v)[None, None] for k, v in _run(pa, m, 48, 9, dtype=t).items()} for t in (np.float64, np.longdouble)}
        gap, drift, same = pa.margin(res[np.float64], unif, res[np.longdouble])
        print(f"{name}: smallest gap {gap:.3e}, cdf drift {drift:.3e}, identical ancestors {same}")
        assert same and gap >= max(1e-8, 1000.0 * drift)
        np.testing.assert_array_equal(res[np.float64]["zeroed"], res[np.longdouble]["zeroed"])
