"""The mathematics of the cubature (sigma-point) filter, pinned without a device: tests/cubature_filter_ref.py, the transition the GPU
tests hand to filter_ref.filter.

1. From S = 0 all 2D points coincide: one step gives m_pred = x0 + mean and diag(S_pred) = var + Q of the ORACLE's conditional at
   [x0, c_0], in both q_modes, within the floors of tests/test_transition_grad_ref.py; `cross` is exact zeros; the off-diagonals of
   S_pred (w sum_i of products of rounding residues of the mean) are below the variance floor.
2. The rule is exact for affine maps: on the linear-Gaussian model of tests/test_linear_filter_ref.py every filter and smoother array
   is within 1e-12 of filter_ref.linear_transition (1.8e-14 measured; it sums differently, hence not array_equal).
3. Against moment matching (filter_ref.gp_transition) in np.longdouble, with Q fixed and S0 = 2^-k S_bar, the one-step difference in
   m_pred, S_pred and cross is SECOND order in the start covariance: d(k) / d(k + 1) -> 4, where the linearised rule's ratio is 2
   (tests/test_linear_filter_ref.py).  k = 8 .. 11, band [3.9, 4.1] (3.978 .. 4.001 measured: five times the largest deviation); every
   difference is >= 3e-12, far above longdouble rounding.  At k = 8 the linearised rule's m_pred is at least 100 times farther from
   moment matching than the cubature one (at least 512 measured).
4. A rank-deficient start covariance (one zero row and column) and S0 = 0 run without NaN over 12 observed rows; every S_pred is
   symmetric and positive definite (the factorisation gives a zero column for a pivot <= 0)."""
import numpy as np
import pytest

import cubature_filter_ref as cf
import filter_ref as fr
import linear_filter_ref as lf
import moment_ref as mr
from oracle import ffvd_oracle as orc
from test_linear_filter_ref import ROWS, _start, _unobserved
from test_transition_grad_ref import MODES, SHAPES, WIDE, case, floor, needs_longdouble


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_step_from_a_point_is_the_oracle_conditional(shape, mode):
    cs = case(shape)
    U, H = cs["post"][0]
    D = cs["D"]
    beta, Gam = mr.posterior_terms(cs["L"], U, H, mode)
    Q = np.linspace(0.01, 0.03, D)
    fn = orc.conditional_after_kernel_precalculation
    if mode == "reference":
        om, ov = fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=H, white=True)
    else:
        outs = [fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=H[d:d + 1], white=True) for d in range(D)]
        om, ov = outs[0][0], np.stack([outs[d][1][:, d] for d in range(D)], axis=1)
    for n in ROWS:
        x0, c = _start(cs, n)
        f = fr.filter(x0, np.zeros((D, D)), *_unobserved(D), Q, cf.ckf_transition(c, cs["Z"], cs["kern"], beta, Gam))
        em = float(np.max(np.abs(f["m_pred"][0] - x0 - om[n])))
        ev = float(np.max(np.abs(np.diag(f["S_pred"][0]) - Q - ov[n])))
        off = float(np.max(np.abs(f["S_pred"][0] - np.diag(np.diag(f["S_pred"][0])))))
        print(f"{shape} {mode} row {n}: mean {em:.3e} (floor {floor('mean', om):.3e}), var {ev:.3e}, off-diagonal {off:.3e} "
              f"(floor {floor('var', ov):.3e})")
        assert em <= floor("mean", om) and ev <= floor("var", ov) and off <= floor("var", ov)
        np.testing.assert_array_equal(f["cross"][0], np.zeros((D, D)))
        np.testing.assert_array_equal(f["m_filt"], f["m_pred"])


def test_on_a_linear_gaussian_model_the_rule_is_exact():
    rng = np.random.default_rng(41)                               # the model of test_linear_filter_ref.py
    D, J, n = 3, 2, 9
    A, b = np.eye(D) + 0.3 * rng.standard_normal((D, D)), rng.standard_normal(D)
    CC, DD, sd, Q = rng.standard_normal((D, J)), rng.standard_normal(J), np.asarray((0.3, 0.7)), np.asarray((0.05, 0.1, 0.2))
    Y = rng.standard_normal((n, J))
    Y[2, :] = np.nan
    Y[5, 0] = np.nan
    x0, S0 = rng.standard_normal(D), 0.4 * np.eye(D)
    F = A - np.eye(D)
    cond = lambda i, X: (X @ F.T + b[None, :], np.zeros_like(X))
    lin, ckf = (fr.filter(x0, S0, Y, CC, DD, sd, Q, tr) for tr in (fr.linear_transition(A, b), cf.cubature_transition(cond)))
    worst = 0.0
    for k in lin:
        ok = ~np.isnan(lin[k])
        np.testing.assert_array_equal(np.isnan(ckf[k]), ~ok, err_msg=k)
        worst = max(worst, float(np.max(np.abs(lin[k][ok] - ckf[k][ok]))))
    for u, v in zip(fr.smooth(lin), fr.smooth(ckf)):
        worst = max(worst, float(np.max(np.abs(u - v))))
    print(f"linear-Gaussian model: largest difference from linear_transition {worst:.3e}")
    assert worst <= 1e-12


@needs_longdouble
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_difference_from_moment_matching_is_second_order_in_the_start_covariance(shape):
    assert WIDE
    t = np.longdouble
    cs = case(shape)
    U, H = cs["post"][0]
    D = cs["D"]
    beta, Gam = mr.posterior_terms(cs["L"], U, H, "intent", dtype=t)
    R = np.random.default_rng(11).standard_normal((D, D))
    Sbar = (R @ R.T / D + 0.1 * np.eye(D)).astype(t)
    Q = np.full(D, 0.01)
    keys = ("m_pred", "S_pred", "cross")
    for n in ROWS[:2]:
        x0, c = _start(cs, n)
        model = (c, cs["Z"], cs["kern"], beta, Gam)
        d, ekf = {k: [] for k in keys}, None
        for k in (8, 9, 10, 11):
            S0 = t(2) ** -k * Sbar
            a = fr.filter(x0, S0, *_unobserved(D), Q, fr.gp_transition(*model, dtype=t), dtype=t)
            b = fr.filter(x0, S0, *_unobserved(D), Q, cf.ckf_transition(*model, dtype=t), dtype=t)
            for key in keys:
                d[key].append(float(np.max(np.abs(a[key] - b[key]))))
            if k == 8:
                e = fr.filter(x0, S0, *_unobserved(D), Q, lf.ekf_transition(*model, dtype=t), dtype=t)
                ekf = float(np.max(np.abs(a["m_pred"] - e["m_pred"])))
        for key in keys:
            ratios = [d[key][i] / d[key][i + 1] for i in range(3)]
            print(f"{shape} row {n}: |{key}(moment) - {key}(cubature)| at s = 2^-8 .. 2^-11: {d[key]}, ratios {ratios}")
            assert all(x >= 3e-12 for x in d[key]), (key, d[key])
            for r in ratios:
                assert 3.9 <= r <= 4.1, (key, d[key], ratios)
        print(f"{shape} row {n}: at s = 2^-8 the linearised m_pred differs by {ekf:.3e}, {ekf / d['m_pred'][0]:.1f} times the cubature one")
        assert ekf >= 100.0 * d["m_pred"][0]


@pytest.mark.parametrize("start", ["rank-deficient", "zero"])
@pytest.mark.parametrize("shape", ["tiny", "small"])
def test_a_semi_definite_start_runs_and_stays_positive_definite(shape, start):
    cs = case(shape)
    U, H = cs["post"][0]
    D, n = cs["D"], 12
    beta, Gam = mr.posterior_terms(cs["L"], U, H, "reference")
    rng = np.random.default_rng(17)
    S0 = np.zeros((D, D))
    if start == "rank-deficient":
        R = rng.standard_normal((D, D))
        S0 = 0.05 * (R @ R.T / D + 0.1 * np.eye(D))
        S0[D // 2, :] = 0.0                                       # one zero row and column: a zero pivot in the middle
        S0[:, D // 2] = 0.0
        L = cf.factor(S0)
        assert np.all(L[:, D // 2] == 0.0) and np.allclose(L @ L.T, S0, rtol=0, atol=1e-15)
    x0, ctrl = cs["Xnew"][0, :D], cs["Xnew"][:n, D:]
    CC, DD, sd, Q = np.eye(D)[:, :1], np.zeros(1), np.asarray((0.3,)), np.full(D, 0.01)
    Y = x0[0] + 0.3 * rng.standard_normal((n, 1))
    f = fr.filter(x0, S0, Y, CC, DD, sd, Q, cf.ckf_transition(ctrl, cs["Z"], cs["kern"], beta, Gam))
    f["m_smooth"], f["S_smooth"] = fr.smooth(f)
    assert all(np.all(np.isfinite(v)) for v in f.values())
    np.testing.assert_array_equal(f["S_pred"], np.swapaxes(f["S_pred"], -1, -2))
    low = float(np.min(np.linalg.eigvalsh(f["S_pred"])))
    print(f"{shape}, {start} start: smallest eigenvalue of S_pred over {n} rows {low:.3e}")
    assert low > 0.0
