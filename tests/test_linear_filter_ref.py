"""The mathematics of the linearised (extended Kalman) filter, pinned without a device: tests/linear_filter_ref.py, the transition the
GPU tests hand to filter_ref.filter.

1. From S = 0 one step gives m_pred = x0 + mean and S_pred = diag(var + Q) of the ORACLE's conditional at [x0, c_0], in both q_modes,
   within the floors tests/test_transition_grad_ref.py uses against the oracle (1e-11 + 1e-9 max|ref| on the mean, 1e-11 + 1e-8
   max|ref| on the variance, max over the oracle's values at the rows of that test's Xnew, three of which start the filter here;
   1.5e-10 on m130's variance as there); the off-diagonal of S_pred is an exact zero.
2. On a linear-Gaussian model the linearisation IS the model: filter_ref.linear_transition and a hand-built linearised transition
   that returns the same A give identical filters and smoothers (array_equal).
3. Against moment matching (filter_ref.gp_transition) in np.longdouble, with Q fixed and S0 = s S_bar, the one-step difference in
   m_pred is first order in s: moment matching adds tr(Hessian S) / 2 + O(s^2) to the mean, the linearisation nothing.  So
   d(s) / d(s / 2) = 2 (1 + O(s)).  Measured in np.longdouble on every shape: the relative deviation of the ratio from 2 is 3e-2 at
   s = 2^-5 and falls with s, below 1e-3 (ratio within 2 +- 2e-3) for s <= 2^-10, while d itself (1e-5 .. 1e-7 there) stays
   thirteen orders above longdouble's rounding.  The test uses s = 2^-10 .. 2^-13 and the band [1.99, 2.01], five times that
   deviation; the ratios are printed.  Skipped where np.longdouble is no wider than fp64 (WIDE), as the sibling tests are."""
import numpy as np
import pytest

import filter_ref as fr
import linear_filter_ref as lf
import moment_ref as mr
from oracle import ffvd_oracle as orc
from test_transition_grad_ref import MODES, SHAPES, WIDE, case, floor, needs_longdouble

ROWS = (0, 3, 10)                                # rows of the shared Xnew: two near the data, one far from it


def _start(cs, n):
    D = cs["D"]
    return cs["Xnew"][n, :D], cs["Xnew"][n:n + 1, D:]


def _unobserved(D):
    return np.full((1, 1), np.nan), np.ones((D, 1)), np.zeros(1), np.ones(1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_step_from_a_point_is_the_oracle_conditional(shape, mode):
    cs = case(shape)
    U, H = cs["post"][0]
    D = cs["D"]
    beta, Gam = mr.posterior_terms(cs["L"], U, H, mode)
    Q = np.linspace(0.01, 0.03, D)
    fn = orc.conditional_after_kernel_precalculation
    if mode == "reference":                                      # the oracle on all rows of Xnew, as test_values_match_the_oracle
        om, ov = fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=H, white=True)
    else:
        outs = [fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=H[d:d + 1], white=True) for d in range(D)]
        om, ov = outs[0][0], np.stack([outs[d][1][:, d] for d in range(D)], axis=1)
    for n in ROWS:
        x0, c = _start(cs, n)
        f = fr.filter(x0, np.zeros((D, D)), *_unobserved(D), Q, lf.ekf_transition(c, cs["Z"], cs["kern"], beta, Gam))
        em = float(np.max(np.abs(f["m_pred"][0] - x0 - om[n])))
        ev = float(np.max(np.abs(np.diag(f["S_pred"][0]) - Q - ov[n])))
        print(f"{shape} {mode} row {n}: mean {em:.3e} (floor {floor('mean', om):.3e}), var {ev:.3e} (floor {floor('var', ov):.3e})")
        assert em <= floor("mean", om) and ev <= floor("var", ov)
        off = f["S_pred"][0] - np.diag(np.diag(f["S_pred"][0]))
        np.testing.assert_array_equal(off, np.zeros((D, D)))
        np.testing.assert_array_equal(f["cross"][0], np.zeros((D, D)))
        np.testing.assert_array_equal(f["m_filt"], f["m_pred"])


def test_on_a_linear_gaussian_model_the_linearisation_is_the_model():
    rng = np.random.default_rng(41)
    D, J, n = 3, 2, 9
    A, b = np.eye(D) + 0.3 * rng.standard_normal((D, D)), rng.standard_normal(D)
    CC, DD, sd, Q = rng.standard_normal((D, J)), rng.standard_normal(J), np.asarray((0.3, 0.7)), np.asarray((0.05, 0.1, 0.2))
    Y = rng.standard_normal((n, J))
    Y[2, :] = np.nan
    Y[5, 0] = np.nan
    x0, S0 = rng.standard_normal(D), 0.4 * np.eye(D)
    Jac = A - np.eye(D)

    def hand(i, mu, S):                                           # (m, J S J^T + diag(v), S J^T) with v = 0: what ekf_transition returns
        return Jac @ mu + b, Jac @ S @ Jac.T + np.diag(np.zeros(D)), S @ Jac.T

    lin, ekf = (fr.filter(x0, S0, Y, CC, DD, sd, Q, tr) for tr in (fr.linear_transition(A, b), hand))
    for k in lin:
        np.testing.assert_array_equal(lin[k], ekf[k], err_msg=k)
    for u, v in zip(fr.smooth(lin), fr.smooth(ekf)):
        np.testing.assert_array_equal(u, v)
    # and A S A^T + diag(Q), S A^T are what comes out
    np.testing.assert_allclose(lin["S_pred"][0], A @ S0 @ A.T + np.diag(Q), rtol=0, atol=1e-14)
    np.testing.assert_allclose(lin["cross"][0], S0 @ A.T, rtol=0, atol=1e-14)


@needs_longdouble
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_difference_from_moment_matching_is_first_order_in_the_start_covariance(shape):
    assert WIDE
    t = np.longdouble
    cs = case(shape)
    U, H = cs["post"][0]
    D = cs["D"]
    beta, Gam = mr.posterior_terms(cs["L"], U, H, "intent", dtype=t)
    R = np.random.default_rng(11).standard_normal((D, D))
    Sbar = (R @ R.T / D + 0.1 * np.eye(D)).astype(t)
    Q = np.full(D, 0.01)
    for n in ROWS[:2]:
        x0, c = _start(cs, n)
        d = []
        for k in (10, 11, 12, 13):
            S0 = t(2) ** -k * Sbar
            a = fr.filter(x0, S0, *_unobserved(D), Q, fr.gp_transition(c, cs["Z"], cs["kern"], beta, Gam, dtype=t), dtype=t)
            b = fr.filter(x0, S0, *_unobserved(D), Q, lf.ekf_transition(c, cs["Z"], cs["kern"], beta, Gam, dtype=t), dtype=t)
            d.append(float(np.max(np.abs(a["m_pred"] - b["m_pred"]))))
        ratios = [d[i] / d[i + 1] for i in range(len(d) - 1)]
        print(f"{shape} row {n}: |m_pred(moment) - m_pred(linearised)| at s = 2^-10 .. 2^-13: {d}, ratios {ratios}")
        assert all(x > 1e-12 for x in d), d
        for r in ratios:
            assert 1.99 <= r <= 2.01, (d, ratios)
