"""The NumPy reference of the particle forecast fan (tests/forecast_particle_ref.py) pinned on its own, without a GPU: against the
exact Kalman predictor on the linear-Gaussian model of tests/test_particle_filter_ref.py, a track from an all-NaN origin, and the
NaN pattern of lpd_fc."""
import numpy as np
import pytest

import filter_ref as fr
import forecast_particle_ref as fpr
import particle_filter_ref as pf
from test_particle_filter_ref import _linear_model

H, N = 3, 4096


def _draws(m, n, seed):
    rng = np.random.default_rng(seed)
    return dict(eps=rng.standard_normal((m["n"], n, m["D"])), unif=rng.random(m["n"]), xi0=rng.standard_normal((n, m["D"])),
                eps_fc=rng.standard_normal((m["n"], H, n, m["D"])))


def _cond(m):
    return lambda i, X: (X @ m["F"].T + m["b"][None, :], np.broadcast_to(m["v"], X.shape))


def _track(m, d, o, dtype=np.float64):
    return fpr.track(_cond(m), m["x0"], m["S0"], m["Y"], o, H, m["CC"], m["DD"], m["sd"], m["Q"], d["eps"], d["unif"], d["eps_fc"][o], d["xi0"],
                     dtype=dtype)


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_on_a_linear_gaussian_model_the_tracks_approach_the_kalman_predictor(seed):
    """Affine conditional mean, constant variance, N = 4096, h = 3, every origin 0 .. 8: |m_fc - Kalman predictor| within
    6 sqrt(diag(S_fc^KF) / min_{i <= o} ess_i) at every horizon."""
    m = _linear_model()
    D = m["D"]
    A, Qt = np.eye(D) + m["F"], np.diag(m["v"] + m["Q"])
    kf = fr.filter(m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["v"] + m["Q"], fr.linear_transition(A, m["b"]))
    d, worst = _draws(m, N, seed), 0.0
    for o in range(m["n"] - H):
        f = _track(m, d, o)
        mk, Sk, ess = kf["m_filt"][o], kf["S_filt"][o], float(np.min(f["filter"]["ess"][:o + 1]))
        for k in range(H):
            mk, Sk = A @ mk + m["b"], A @ Sk @ A.T + Qt
            tol = 6.0 * np.sqrt(np.diagonal(Sk) / ess)
            err = np.abs(f["m_fc"][k] - mk)
            worst = max(worst, float(np.max(err / tol)))
            assert np.all(err <= tol), (o, k)
        np.testing.assert_array_equal(f["S_fc"], np.swapaxes(f["S_fc"], -1, -2))
    print(f"seed {seed}: the worst ratio of |m_fc - Kalman predictor| to its bound is {worst:.3f}")


def test_a_track_from_an_all_nan_origin_continues_that_rows_particles_unresampled():
    m = _linear_model()
    n = 64
    d = _draws(m, n, 5)
    full = pf.run(_cond(m), m["x0"], m["S0"], m["Y"], m["CC"], m["DD"], m["sd"], m["Q"], d["eps"], d["unif"], d["xi0"])
    assert np.all(np.isnan(m["Y"][7]))
    f = _track(m, d, 7)
    X = full["particles"][7]
    np.testing.assert_array_equal(f["filter"]["particles"][7], X)
    for k in range(H):
        X = X + (X @ m["F"].T + m["b"][None, :]) + d["eps_fc"][7][k] * np.sqrt(m["v"] + m["Q"])[None, :]
        np.testing.assert_array_equal(f["fc_particles"][k], X)
        np.testing.assert_array_equal(f["m_fc"][k], X.sum(axis=0) / n)
    # an observed origin: the start is that row's particles through that row's ancestors
    g = _track(m, d, 5)
    X = full["particles"][5][full["ancestors"][5]]
    np.testing.assert_array_equal(g["fc_particles"][0], X + (X @ m["F"].T + m["b"][None, :]) + d["eps_fc"][5][0] * np.sqrt(m["v"] + m["Q"])[None, :])


def test_lpd_fc_is_nan_exactly_where_the_target_is():
    m = _linear_model()
    d = _draws(m, 64, 6)
    for o in range(m["n"] - H):
        f = _track(m, d, o)
        np.testing.assert_array_equal(np.isnan(f["lpd_fc"]), np.isnan(m["Y"][o + 1: o + 1 + H]))
    f = _track(m, d, 4)                                           # rows 5, 6, 7: row 7 is all NaN
    assert np.all(np.isnan(f["lpd_fc"][2])) and np.all(np.isfinite(f["lpd_fc"][:2]))
    wide = _track(m, d, 4, dtype=np.longdouble)
    assert wide["lpd_fc"].dtype == np.longdouble and np.allclose(np.asarray(wide["lpd_fc"][:2], dtype=np.float64), f["lpd_fc"][:2], atol=1e-9)
