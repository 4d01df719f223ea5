"""The NumPy reference of the adapted particle forecast fan (tests/forecast_adapted_ref.py) pinned on its own, without a GPU: a track
is the adapted records reference over the truncated record continued by NaN rows; on a scalar linear-Gaussian model its rows approach
the exact Kalman k-step prediction; S_fc is exactly symmetric and lpd_fc is NaN exactly where the target is."""
import numpy as np

import forecast_adapted_ref as far
import particle_adapted_ref as pa
from test_particle_adapted_ref import _cond
from test_particle_filter_ref import _linear_model

H = 3
ORIGINS = (0, 3, 4, 6, 8)                                          # (3: the row before a partly observed one; 6: before an unobserved one; 8: the last admissible)


def _draws(m, N, B, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((m["n"], N, m["D"])), rng.random(m["n"]), rng.standard_normal((N, m["D"])),
            rng.standard_normal((B, h, N, m["D"])))


def _fan(m, N, origins, h, seed, dtype=np.float64):
    eps, unif, xi0, eps_fc = _draws(m, N, len(origins), h, seed)
    return far.run(_cond(m, dtype), m["x0"], m["S0"], m["Y"], origins, h, m["CC"], m["DD"], m["sd"], m["Q"], eps, unif, lambda b: eps_fc[b],
                   xi0, dtype=dtype)


# ---- (a) a track is the records reference over the truncated record ----------------------------------------------------------------------
def test_a_track_is_the_adapted_filter_over_the_cut_record_continued_by_nan_rows():
    """D = 3, J = 2, N = 48, h = 3, five origins: m_fc, S_fc and fc_particles against m_pred, S_pred and particles at rows
    o + 1 .. o + h of particle_adapted_ref.run over Y[:o + 1] followed by h all-NaN rows with the draws concatenated: 1e-12."""
    m, N = _linear_model(), 48
    eps, unif, xi0, eps_fc = _draws(m, N, len(ORIGINS), H, 21)
    out = _fan(m, N, ORIGINS, H, 21)
    J = m["Y"].shape[1]
    for b, o in enumerate(ORIGINS):
        Yc = np.concatenate((m["Y"][:o + 1], np.full((H, J), np.nan)))
        f = pa.run(_cond(m), m["x0"], m["S0"], Yc, m["CC"], m["DD"], m["sd"], m["Q"], np.concatenate((eps[:o + 1], eps_fc[b])),
                   np.concatenate((unif[:o + 1], np.zeros(H))), xi0)
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("fc_particles", "particles")):
            err = float(np.max(np.abs(out[mine][b] - f[theirs][o + 1:])))
            print(f"origin {o}: {mine} against {theirs} of the cut record: {err:.3e}")
            assert err <= 1e-12, (mine, o)
        # and the start is the filter's own stored set: the filter over the whole record agrees with the cut one up to row o
        np.testing.assert_array_equal(out["filter"]["particles"][o], f["particles"][o])


def test_the_first_row_of_a_track_is_the_filters_prediction_of_the_next_row():
    """m_fc, S_fc, lpd_fc at k = 1 from origin o against m_pred, S_pred, lpd of row o + 1 of the same filter: 1e-12 (the same
    expressions on the same set); lpd of an unobserved row is NaN in both."""
    m = _linear_model()
    origins = list(range(m["n"] - H))
    out = _fan(m, 48, origins, H, 22)
    f = out["filter"]
    for b, o in enumerate(origins):
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("lpd_fc", "lpd")):
            a, w = out[mine][b, 0], f[theirs][o + 1]
            np.testing.assert_array_equal(np.isnan(a), np.isnan(w), err_msg=f"{mine}, origin {o}")
            ok = ~np.isnan(w)
            assert not ok.any() or float(np.max(np.abs(a[ok] - w[ok]))) <= 1e-12, (mine, o)


# ---- (b) against the exact k-step prediction of a scalar linear-Gaussian model -----------------------------------------------------------
def _scalar_model():
    rng = np.random.default_rng(31)
    n = 12
    m = dict(F=np.array([[-0.15]]), b=np.array([0.08]), v=np.array([0.03]), Q=np.array([0.04]), CC=np.array([[1.3]]), DD=np.array([-0.2]),
             sd=np.array([0.3]), x0=np.array([0.5]), S0=np.array([[0.2]]), D=1, n=n)
    x, Y = m["x0"] + np.sqrt(0.2) * rng.standard_normal(1), np.empty((n, 1))
    for i in range(n):
        x = x + m["F"] @ x + m["b"] + np.sqrt(m["v"] + m["Q"]) * rng.standard_normal(1)
        Y[i] = x @ m["CC"] + m["DD"] + m["sd"] * rng.standard_normal(1)
    m["Y"] = Y
    return m


def _kalman_fan(m, origins, h):
    """the exact filter of the scalar model, then from every origin the exact k-step predictive mean, variance and log density of
    Y[o + k]"""
    a, b, q = 1.0 + m["F"][0, 0], m["b"][0], m["v"][0] + m["Q"][0]
    c, d, r = m["CC"][0, 0], m["DD"][0], m["sd"][0] ** 2
    mf, Pf = np.empty(m["n"]), np.empty(m["n"])
    mu, P = m["x0"][0], m["S0"][0, 0]
    for i in range(m["n"]):
        mu, P = a * mu + b, a * a * P + q
        s = c * c * P + r
        k = P * c / s
        mu, P = mu + k * (m["Y"][i, 0] - (c * mu + d)), P - k * c * P
        mf[i], Pf[i] = mu, P
    out = dict(m_fc=np.empty((len(origins), h)), S_fc=np.empty((len(origins), h)), lpd_fc=np.empty((len(origins), h)))
    for bi, o in enumerate(origins):
        mu, P = mf[o], Pf[o]
        for k in range(h):
            mu, P = a * mu + b, a * a * P + q
            s, e = c * c * P + r, m["Y"][o + 1 + k, 0] - (c * mu + d)
            out["m_fc"][bi, k], out["S_fc"][bi, k], out["lpd_fc"][bi, k] = mu, P, -0.5 * (np.log(2 * np.pi) + np.log(s) + e * e / s)
    return out


def test_on_a_scalar_linear_gaussian_model_the_rows_approach_the_exact_k_step_prediction():
    """N = 4096, origins (0, 3, 7), k = 1 .. 4: m_fc, S_fc and lpd_fc within 5 Monte-Carlo standard errors of the Kalman k-step
    predictive mean, variance and log density; the standard error of each entry is the standard deviation of the reference over 20
    further seeds."""
    m, origins, h, N = _scalar_model(), (0, 3, 7), 4, 4096
    exact = _kalman_fan(m, origins, h)
    flat = lambda o: dict(m_fc=o["m_fc"][..., 0], S_fc=o["S_fc"][..., 0, 0], lpd_fc=o["lpd_fc"][..., 0])
    out = flat(_fan(m, N, origins, h, 300))
    seeds = [flat(_fan(m, N, origins, h, 400 + s)) for s in range(20)]
    for k in ("m_fc", "S_fc", "lpd_fc"):
        se = np.std(np.stack([s[k] for s in seeds]), axis=0, ddof=1)
        err = np.abs(out[k] - exact[k])
        print(f"{k}: largest |reference - Kalman| / se {float(np.max(err / se)):.2f}; se between {float(se.min()):.2e} and {float(se.max()):.2e}")
        assert np.all(se > 0.0)
        assert np.all(err <= 5.0 * se), k


# ---- (c) symmetry and NaN -----------------------------------------------------------------------------------------------------------------
def test_s_fc_is_exactly_symmetric_and_lpd_fc_is_nan_exactly_where_the_target_is():
    m = _linear_model()
    origins = list(range(m["n"] - H))
    for t in (np.float64, np.longdouble):
        out = _fan(m, 48, origins, H, 23, dtype=t)
        np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
        Yt = m["Y"][np.asarray(origins)[:, None] + 1 + np.arange(H)[None, :]]
        np.testing.assert_array_equal(np.isnan(out["lpd_fc"]), np.isnan(Yt))
        assert np.isnan(Yt).any() and not np.isnan(Yt).all()
        assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"])) and np.all(np.isfinite(out["fc_particles"]))
        assert out["m_fc"].dtype == t and out["lpd_fc"].dtype == t


def test_the_two_precisions_agree_where_the_ancestors_do():
    """fp64 against np.longdouble on the linear model, N = 48: identical ancestors in the filter stage, and the forecast rows within
    1e-10 of one another (no resampling happens in a track: nothing discontinuous is left)."""
    m = _linear_model()
    a, w = _fan(m, 48, ORIGINS, H, 9), _fan(m, 48, ORIGINS, H, 9, dtype=np.longdouble)
    np.testing.assert_array_equal(a["filter"]["ancestors"], w["filter"]["ancestors"])
    for k in far.ARRAYS:
        ok = ~np.isnan(a[k])
        assert float(np.max(np.abs(a[k][ok] - w[k][ok]))) <= 1e-10, k
