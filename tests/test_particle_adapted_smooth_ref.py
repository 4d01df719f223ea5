"""tests/particle_adapted_smooth_ref.py pinned without a GPU: against the exact RTS smoother of the scalar linear-Gaussian model of
tests/test_particle_smoother_ref.py (its model, record and 20 seeds of draws, N = 4096, computed once), in extended precision, and the
backward simulation against the marginal smoother.

The bounds are that test's own: |m_smooth - m_RTS| <= 6 sqrt(P_s / ess_smooth) (4.00 measured), |S_smooth / P_s - 1| <=
6 sqrt(2 / min ess_smooth) (0.089 measured against 0.192), |sum w - 1| <= 1e-12 (4.4e-16 measured), and the RMS standardised error
of the smoother below the adapted filtered mean's (0.021 against 0.50 measured).  The smallest ess_smooth is reported beside the
bootstrap smoother's on the same draws (1947 against 438 measured) and not asserted."""
import functools

import numpy as np

import particle_adapted_smooth_ref as pas
import test_particle_smoother_ref as boot
from test_particle_smoother_ref import CC, DD, MISSING, N, Q, ROWS, SD, SEEDS, X0, linear_cond, record, rts


def smoothed(seed, Y, n=N, unif_bs=None, b=None, dtype=np.float64, smoother=True):
    """the draws of test_particle_smoother_ref.smoothed (eps, then unif), then the uniforms of the backward simulation"""
    rng = np.random.default_rng(seed)
    eps, unif = rng.standard_normal((Y.shape[0], n, 1)), rng.random(Y.shape[0])
    if b is not None:
        unif_bs = rng.random((Y.shape[0], b))
    f = pas.run(linear_cond, np.array([X0]), None, Y, CC, DD, SD, np.array([Q]), eps, unif, None, unif_bs, dtype=dtype, smoother=smoother)
    f["unif_bs"] = unif_bs
    return f


@functools.lru_cache(maxsize=None)
def runs():
    """the 20 seeds, computed once and never modified"""
    Y = record()
    return Y, [smoothed(100 + s, Y) for s in range(SEEDS)]


def test_against_the_kalman_smoother():
    Y, outs = runs()
    mf, Pf, ms, Ps = rts(Y)
    z_s, z_f, worst, ratio, least, norm = [], [], 0.0, [], np.inf, 0.0
    for f in outs:
        err = f["m_smooth"][:, 0] - ms
        worst = max(worst, float(np.max(np.abs(err) / np.sqrt(Ps / f["ess_smooth"]))))
        z_s.append(err / np.sqrt(Ps))
        z_f.append((f["m_filt"][:, 0] - ms) / np.sqrt(Ps))
        ratio.append(f["S_smooth"][:, 0, 0] / Ps)
        least = min(least, float(np.min(f["ess_smooth"])))
        norm = max(norm, float(np.max(np.abs(f["w_smooth"].sum(axis=1) - 1.0))))
        np.testing.assert_array_equal(f["w_smooth"][ROWS - 1], np.full(N, 1.0 / N))
        assert np.all(f["w_smooth"] >= 0.0)
    rms = [float(np.sqrt(np.mean(np.square(z)))) for z in (z_s, z_f)]
    ratio = np.array(ratio)
    least_boot = min(float(np.min(f["ess_smooth"])) for f in boot.runs()[1])
    print(f"largest |m_smooth - m_RTS| sqrt(ess_smooth / P_s) {worst:.3f}; RMS standardised error: smoother {rms[0]:.4f}, adapted filtered "
          f"mean {rms[1]:.4f}; smallest ess_smooth {least:.1f} (bootstrap smoother on the same draws: {least_boot:.1f}); largest "
          f"|S_smooth / P_s - 1| {float(np.max(np.abs(ratio - 1.0))):.3f} (bound {6.0 * np.sqrt(2.0 / least):.3f}); largest |sum w - 1| "
          f"{norm:.2e}")
    assert worst <= 6.0
    assert float(np.max(np.abs(ratio - 1.0))) <= 6.0 * np.sqrt(2.0 / least)
    assert norm <= 1e-12
    assert rms[0] < rms[1]


def test_the_draws_are_the_bootstrap_tests_own():
    """the same seed gives the bootstrap run's eps and unif: on an all-NaN record the two filters, the two kept stacks and the two
    smoothers coincide (identity ancestors, unit weights)"""
    Y = np.full((ROWS, 1), np.nan)
    a, b = smoothed(100, Y, n=64), boot.smoothed(100, Y, n=64)
    for k in ("particles", "trans_mean", "trans_var") + pas.SMOOTHED:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_in_extended_precision_the_recursion_and_the_backward_simulation_agree():
    """fp64 against np.longdouble at N = 256, B = 64: SMOOTHED and the trajectory moments to 1e-12, identical indices (the margin says
    why)"""
    Y = record()
    f = smoothed(7, Y, n=256, b=64)
    wide = pas.recursion(f["particles"], f["trans_mean"], f["trans_var"], dtype=np.longdouble)
    for k in pas.SMOOTHED:
        err = float(np.max(np.abs(f[k] - wide[k]) / (256.0 if k == "ess_smooth" else 1.0)))
        print(f"{k}: fp64 against longdouble {err:.2e}")
        assert wide[k].dtype == np.longdouble and err <= 1e-12, k
    w = smoothed(7, Y, n=256, unif_bs=f["unif_bs"], dtype=np.longdouble, smoother=False)
    np.testing.assert_array_equal(f["ancestors"], w["ancestors"])
    gap, drift, same = pas.margin(f, None, w)
    print(f"gap {gap:.3e}, drift {drift:.3e}")
    assert same and gap >= max(1e-8, 1000.0 * drift)
    np.testing.assert_array_equal(f["traj_index"], w["traj_index"])
    for k in pas.MOMENTS:
        ok = ~np.isnan(f[k])
        np.testing.assert_array_equal(ok, ~np.isnan(w[k]))
        err = float(np.max(np.abs(f[k][ok] - w[k][ok])))
        print(f"{k}: fp64 against longdouble {err:.2e}")
        assert w[k].dtype == np.longdouble and err <= 1e-12, k


def test_the_backward_simulation_agrees_with_the_marginal_smoother():
    """B = 4096 trajectories on one seed's stacks at N = 256: conditional on the filter's run k_t has the law w_smooth[t], so m_traj is
    the mean of B draws of variance S_smooth"""
    b = 4096
    f = smoothed(21, record(), n=256, b=b)
    dev = np.abs(f["m_traj"] - f["m_smooth"])
    lim = 6.0 * np.sqrt(np.diagonal(f["S_smooth"], axis1=1, axis2=2) / b)
    print(f"largest |m_traj - m_smooth| / sqrt(diag S_smooth / B) {float(np.max(dev / (lim / 6.0))):.3f}")
    assert np.all(dev <= lim)
    for t in range(ROWS):                                         # the gather; no ancestor indirection
        np.testing.assert_array_equal(f["trajectories"][:, t], f["particles"][t][f["traj_index"][t]])
    np.testing.assert_array_equal(f["traj_index"][-1], np.minimum(np.floor(f["unif_bs"][-1] * 256).astype(np.int64), 255))
    assert np.isnan(f["lag_cov"][-1, 0, 0]) and not np.isnan(f["lag_cov"][:-1]).any()


def test_one_row_is_the_plain_mean_of_the_filtered_set():
    """n = 1: the unweighted particle estimate, not the Rao-Blackwellised m_filt"""
    f = smoothed(3, record()[:1], n=48)
    X = f["particles"][0]
    np.testing.assert_array_equal(f["w_smooth"][0], np.full(48, 1.0 / 48))
    assert abs(f["m_smooth"][0, 0] - X.mean()) <= 1e-15 and abs(f["S_smooth"][0, 0, 0] - X.var()) <= 1e-15
    assert abs(f["ess_smooth"][0] - 48.0) <= 1e-12 and f["m_smooth"][0, 0] != f["m_filt"][0, 0]


def test_the_unobserved_row_keeps_the_recursion_unchanged():
    """row MISSING takes the bootstrap propagation; the kept moments are still those of the set carried into the row"""
    f = runs()[1][0]
    np.testing.assert_array_equal(f["ancestors"][MISSING], np.arange(N))
    X = f["particles"][MISSING]
    np.testing.assert_array_equal(f["trans_mean"][MISSING + 1], X + (boot.A - 1.0) * X)
    assert abs(f["w_smooth"][MISSING].sum() - 1.0) <= 1e-12
