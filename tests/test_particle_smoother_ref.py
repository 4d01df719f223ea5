"""tests/particle_smoother_ref.py pinned without a GPU: against the exact RTS smoother of a scalar linear-Gaussian model, and the exact
properties the device tests rely on.

The model: x' = 0.9 x + N(0, 0.3), y = x + N(0, 0.2) (variances), x0 = 0.5, 12 rows, row 4 missing; N = 4096 particles, 20 seeds of
draws on one simulated record.  The bounds are statistical with the margins DESIGN.md section 9, "Particle smoothing" records:
|m_smooth - m_RTS| <= 6 sqrt(P_s / ess_smooth) (the 6 is the filter test's own; 4.2 was measured), |S_smooth / P_s - 1| <=
6 sqrt(2 / min ess_smooth) (0.17 measured against 0.60), and the RMS standardised error of the smoother below the genealogy
estimate's below the filtered mean's (0.026 / 0.063 / 0.63 measured)."""
import functools

import numpy as np

import particle_filter_ref as pf
import particle_smoother_ref as ps

A, Q, RV, X0, ROWS, MISSING, N, SEEDS = 0.9, 0.3, 0.2, 0.5, 12, 4, 4096, 20
CC, DD, SD = np.ones((1, 1)), np.zeros(1), np.array([np.sqrt(RV)])


def linear_cond(i, X):
    return (A - 1.0) * X, np.zeros_like(X)


def record(missing=(MISSING,)):
    rng = np.random.default_rng(2024)
    x, Y = X0, np.zeros((ROWS, 1))
    for i in range(ROWS):
        x = A * x + np.sqrt(Q) * rng.standard_normal()
        Y[i, 0] = x + np.sqrt(RV) * rng.standard_normal()
    Y[list(missing)] = np.nan
    return Y


def rts(Y):
    """the Kalman filter and the RTS smoother of the model: (m_filt, P_filt, m_s, P_s), each (rows,)"""
    n = Y.shape[0]
    mp, Pp, mf, Pf = (np.zeros(n) for _ in range(4))
    m, P = X0, 0.0
    for i in range(n):
        mp[i], Pp[i] = A * m, A * A * P + Q
        if np.isnan(Y[i, 0]):
            m, P = mp[i], Pp[i]
        else:
            k = Pp[i] / (Pp[i] + RV)
            m, P = mp[i] + k * (Y[i, 0] - mp[i]), (1.0 - k) * Pp[i]
        mf[i], Pf[i] = m, P
    ms, Ps = mf.copy(), Pf.copy()
    for i in range(n - 2, -1, -1):
        g = Pf[i] * A / Pp[i + 1]
        ms[i] = mf[i] + g * (ms[i + 1] - mp[i + 1])
        Ps[i] = Pf[i] + g * g * (Ps[i + 1] - Pp[i + 1])
    return mf, Pf, ms, Ps


def smoothed(seed, Y, n=N, cond=linear_cond, q=Q):
    rng = np.random.default_rng(seed)
    eps, unif = rng.standard_normal((Y.shape[0], n, 1)), rng.random(Y.shape[0])
    return ps.run(cond, np.array([X0]), None, Y, CC, DD, SD, np.array([q]), eps, unif)


@functools.lru_cache(maxsize=None)
def runs():
    """the 20 seeds, computed once and never modified"""
    Y = record()
    return Y, [smoothed(100 + s, Y) for s in range(SEEDS)]


def test_against_the_kalman_smoother():
    Y, outs = runs()
    mf, Pf, ms, Ps = rts(Y)
    z_s, z_g, z_f, worst, ratio, least, norm = [], [], [], 0.0, [], np.inf, 0.0
    for f in outs:
        g = ps.genealogy(f["particles"], f["ancestors"], f["weights"])
        err = f["m_smooth"][:, 0] - ms
        worst = max(worst, float(np.max(np.abs(err) / np.sqrt(Ps / f["ess_smooth"]))))
        z_s.append(err / np.sqrt(Ps))
        z_g.append((g["m_smooth"][:, 0] - ms) / np.sqrt(Ps))
        z_f.append((f["m_filt"][:, 0] - ms) / np.sqrt(Ps))
        ratio.append(f["S_smooth"][:, 0, 0] / Ps)
        least = min(least, float(np.min(f["ess_smooth"])))
        norm = max(norm, float(np.max(np.abs(f["w_smooth"].sum(axis=1) - 1.0))))
        # the last row is the W-weighted filtered mean
        assert abs(f["m_smooth"][-1, 0] - f["m_filt"][-1, 0]) <= 1e-12
        # exactly 0 where a particle has no offspring
        for t in range(ROWS - 1):
            childless = np.ones(N, dtype=bool)
            childless[f["ancestors"][t]] = False
            assert childless.any() == (t != MISSING)              # (the unobserved row keeps its particles)
            assert np.all(f["w_smooth"][t][childless] == 0.0) and np.all(f["w_smooth"][t] >= 0.0)
    rms = [float(np.sqrt(np.mean(np.square(z)))) for z in (z_s, z_g, z_f)]
    ratio = np.array(ratio)
    print(f"largest |m_smooth - m_RTS| sqrt(ess_smooth / P_s) {worst:.3f}; RMS standardised error: smoother {rms[0]:.4f}, genealogy "
          f"{rms[1]:.4f}, filtered mean {rms[2]:.4f}; largest |z| {float(np.max(np.abs(z_s))):.4f}; smallest ess_smooth {least:.1f}; "
          f"S_smooth / P_s in [{ratio.min():.3f}, {ratio.max():.3f}]; largest |sum w - 1| {norm:.2e}")
    assert worst <= 6.0
    assert float(np.max(np.abs(ratio - 1.0))) <= 6.0 * np.sqrt(2.0 / least)
    assert rms[0] < rms[1] < rms[2]
    assert norm <= 1e-12


def test_in_extended_precision_the_recursion_gives_the_same_smoother():
    """the fp64 recursion against np.longdouble on one seed's stacks at N = 256: the reference's own error is rounding"""
    Y = record()
    f = smoothed(7, Y, n=256)
    wide = ps.recursion(f["particles"], f["ancestors"], f["trans_mean"], f["trans_var"], f["weights"], dtype=np.longdouble)
    for k in ps.SMOOTHED:
        err = float(np.max(np.abs(f[k] - wide[k]) / (256.0 if k == "ess_smooth" else 1.0)))
        print(f"{k}: fp64 against longdouble {err:.2e}")
        assert wide[k].dtype == np.longdouble and err <= 1e-12, k


def test_a_near_deterministic_transition_is_the_genealogy():
    """Variance 0 and Q = 1e-12 (a transition deviation of 1e-6) with transition means at least 1e-3 apart: every off-diagonal
    density underflows to exactly 0, c_j = log f_jj, every exponent on the diagonal is exactly 0 and the recursion folds the weights
    through the ancestors as the genealogy does: array_equal.  The means are kept apart by an offset per particle index (the copies
    of a resampled particle would otherwise share their mean, and the density between two copies is not small)."""
    def cond(i, X):
        return (A - 1.0) * X + 1e-3 * np.arange(X.shape[0])[:, None], np.zeros_like(X)
    for missing in ((MISSING,), (MISSING, ROWS - 1)):
        f = smoothed(5, record(missing), n=64, cond=cond, q=1e-12)
        g = ps.genealogy(f["particles"], f["ancestors"], f["weights"])
        assert len(np.unique(f["ancestors"][0])) < 64              # resampling happened
        for k in ps.SMOOTHED:
            np.testing.assert_array_equal(f[k], g[k], err_msg=k)


def test_with_the_last_row_unobserved_the_last_weights_are_uniform():
    f = smoothed(3, record((MISSING, ROWS - 1)), n=48)
    np.testing.assert_array_equal(f["w_smooth"][-1], np.full(48, 1.0 / 48))
    np.testing.assert_array_equal(f["weights"][-1], np.ones(48))
    np.testing.assert_array_equal(f["ancestors"][-1], np.arange(48))
    assert abs(f["w_smooth"][0].sum() - 1.0) <= 1e-12


def test_one_row_is_the_filtered_row():
    f = smoothed(3, record()[:1], n=48)
    m, S, e = ps.moments(f["particles"][0], f["weights"][0] / f["weights"][0].sum())
    np.testing.assert_array_equal(f["m_smooth"][0], m)
    assert abs(f["m_smooth"][0, 0] - f["m_filt"][0, 0]) <= 1e-14 and abs(f["ess_smooth"][0] - f["ess"][0]) <= 1e-9


def test_the_kept_terms_compose_the_particles_and_the_weights_are_the_filters():
    """X^- = trans_mean + eps sqrt(trans_var) bit for bit in the reference, and weights_of reproduces the filter's ess"""
    Y = record()
    rng = np.random.default_rng(11)
    eps, unif = rng.standard_normal((ROWS, 64, 1)), rng.random(ROWS)
    f = ps.run(linear_cond, np.array([X0]), None, Y, CC, DD, SD, np.array([Q]), eps, unif)
    np.testing.assert_array_equal(f["particles"], f["trans_mean"] + eps * np.sqrt(f["trans_var"]))
    W = f["weights"]
    np.testing.assert_allclose(W.sum(axis=1) ** 2 / (W * W).sum(axis=1), f["ess"], rtol=1e-12)
    np.testing.assert_array_equal(W[MISSING], np.ones(64))
