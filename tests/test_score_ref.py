"""CPU: tests/score_ref.py, the reference of the device scores, pinned five ways: against mpmath at 30 digits on small mixtures,
against the closed form of one Gaussian, against quadrature of int (F - 1{x >= y})^2 dx, against the identity F(q_p) = p, and
against a permutation of the components.  The bounds are rounding-level: a few units of fp64 roundoff of sums of K (or K^2)
terms of size max|term|, and for a quantile the displacement 1 / f(q) of a root by such an error in F."""
import mpmath as mp
import numpy as np
import pytest
from scipy.integrate import quad

import score_ref as sr

EPS = sr.EPS


def _mixture(seed, K, bimodal=False):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal(K) * 0.8 + (np.where(np.arange(K) % 2 == 0, -2.5, 2.5) if bimodal else 0.3)
    var = 0.2 + rng.random(K)
    return mu, var, float(rng.standard_normal() * 1.5)


def _mp_A(d, v):
    return d * mp.erf(d / mp.sqrt(2 * v)) + mp.sqrt(2 * v / mp.pi) * mp.exp(-d * d / (2 * v))


def _mp_cdf(mu, var, x):
    return sum(mp.erfc((m - x) / mp.sqrt(2 * v)) / 2 for m, v in zip(mu, var)) / len(mu)


def _mp_crps(mu, var, y):
    K = len(mu)
    first = sum(_mp_A(y - m, v) for m, v in zip(mu, var)) / K
    pair = sum(_mp_A(mu[k] - mu[l], var[k] + var[l]) for k in range(K) for l in range(K))
    return first - pair / (2 * K * K)


@pytest.mark.parametrize("K,bimodal", [(1, False), (2, True), (3, False), (7, True), (8, False)])
def test_against_mpmath_at_30_digits(K, bimodal):
    mp.mp.dps = 30
    worst = dict(crps=0.0, pit=0.0, quantile=0.0)
    for seed in range(4):
        mu, var, y = _mixture(100 * K + seed, K, bimodal)
        mmu, mvar, my = [mp.mpf(float(m)) for m in mu], [mp.mpf(float(v)) for v in var], mp.mpf(y)
        scale = float(np.max(np.abs(mu)) + abs(y) + np.sqrt(np.max(var)))
        e_crps = abs(float(mp.mpf(float(sr.crps(mu, var, np.float64(y)))) - _mp_crps(mmu, mvar, my)))
        e_pit = abs(float(mp.mpf(float(sr.cdf(mu, var, np.float64(y)))) - _mp_cdf(mmu, mvar, my)))
        assert e_crps <= 16.0 * EPS * scale, (K, seed, e_crps)
        assert e_pit <= 8.0 * EPS, (K, seed, e_pit)
        worst["crps"], worst["pit"] = max(worst["crps"], e_crps / scale), max(worst["pit"], e_pit)
        for p in (0.05, 0.5, 0.95):
            q = sr.quantile(mu, var, p)
            exact = mp.findroot(lambda x: _mp_cdf(mmu, mvar, x) - p, mp.mpf(q))
            f = float(sr.pdf(mu, var, np.float64(q)))
            e_q = abs(float(mp.mpf(q) - exact))
            assert e_q <= 8.0 * EPS / f + 8.0 * EPS * max(1.0, abs(q)), (K, seed, p, e_q)
            worst["quantile"] = max(worst["quantile"], e_q)
    print(f"K = {K}{' bimodal' if bimodal else ''}: distance to mpmath: crps {worst['crps']:.2e} (relative to the scale), "
          f"pit {worst['pit']:.2e}, quantile {worst['quantile']:.2e}")


def test_one_gaussian_is_the_closed_form():
    rng = np.random.default_rng(3)
    for _ in range(50):
        mu, sigma, y = rng.standard_normal() * 3.0, 0.1 + rng.random() * 2.0, rng.standard_normal() * 4.0
        got = float(sr.crps(np.array([mu]), np.array([sigma ** 2]), np.float64(y)))
        assert abs(got - sr.crps_gaussian(mu, sigma, y)) <= 16.0 * EPS * (abs(y - mu) + sigma)
    # the K components equal: the mixture is that Gaussian
    got = float(sr.crps(np.full(5, 0.7), np.full(5, 0.49), np.float64(-0.2)))
    assert abs(got - sr.crps_gaussian(0.7, 0.7, -0.2)) <= 16.0 * EPS


@pytest.mark.parametrize("K,bimodal", [(1, False), (4, True), (7, False)])
def test_against_quadrature_of_the_definition(K, bimodal):
    mu, var, y = _mixture(40 + K, K, bimodal)
    lo, hi = sr.bracket(mu, var)
    lo, hi = min(float(lo), y - 1.0), max(float(hi), y + 1.0)
    F = lambda x: float(sr.cdf(mu, var, np.float64(x)))
    left, e1 = quad(lambda x: F(x) ** 2, lo, y, epsabs=1e-13, epsrel=1e-13, limit=400)
    right, e2 = quad(lambda x: (F(x) - 1.0) ** 2, y, hi, epsabs=1e-13, epsrel=1e-13, limit=400)
    got = float(sr.crps(mu, var, np.float64(y)))
    assert abs(got - (left + right)) <= 1e-12 + e1 + e2            # (the tails beyond 8.5 sigma hold less than 1e-30)


@pytest.mark.parametrize("K,bimodal", [(1, False), (2, True), (16, True), (33, False)])
def test_the_quantile_inverts_the_distribution_function(K, bimodal):
    mu, var, _ = _mixture(70 + K, K, bimodal)
    for p in (1e-9, 0.01, 0.05, 0.3, 0.5, 0.8, 0.95, 1.0 - 1e-9):
        q = sr.quantile(mu, var, p)
        f = float(sr.pdf(mu, var, np.float64(q)))
        # F is good to a few roundoffs of a K-term mean; the root is bracketed to 4 eps |q|, which moves F by f times that
        assert abs(float(sr.cdf(mu, var, np.float64(q))) - p) <= 8.0 * EPS + 8.0 * EPS * max(1.0, abs(q)) * f, (K, p)
    lv = np.array([0.1, 0.5, 0.9])
    many = sr.quantiles(np.stack([mu, mu + 1.0]), np.stack([var, var]), lv)
    assert many.shape == (2, 3) and np.all(np.diff(many, axis=1) > 0.0)
    np.testing.assert_allclose(many[1], many[0] + 1.0, rtol=0.0, atol=64.0 * EPS * (1.0 + np.max(np.abs(many))) +
                               64.0 * EPS / float(np.min(sr.pdf(mu, var, many[0]))))


def test_a_permutation_of_the_components_changes_roundoff_only():
    mu, var, y = _mixture(11, 40, True)
    perm = np.random.default_rng(1).permutation(40)
    scale = float(np.max(np.abs(mu)) + abs(y) + 1.0)
    assert abs(float(sr.crps(mu, var, np.float64(y))) - float(sr.crps(mu[perm], var[perm], np.float64(y)))) <= 64.0 * EPS * scale
    assert abs(float(sr.cdf(mu, var, np.float64(y))) - float(sr.cdf(mu[perm], var[perm], np.float64(y)))) <= 8.0 * EPS
    for p in (0.05, 0.5, 0.95):
        q = sr.quantile(mu, var, p)
        f = float(sr.pdf(mu, var, np.float64(q)))
        assert abs(q - sr.quantile(mu[perm], var[perm], p)) <= 16.0 * EPS / f + 16.0 * EPS * max(1.0, abs(q))


def test_the_stacks_give_the_components_of_the_summaries():
    """points: mu = x CC + DD with the output's noise variance; moments: CC^T m + DD and CC^T S CC + sd^2; S = 0 is the points form;
    NaN targets give NaN crps and pit and leave the quantiles alone"""
    rng = np.random.default_rng(5)
    K, steps, D, J = 6, 3, 4, 2
    x, CC, DD, sd = rng.standard_normal((K, steps, D)), rng.standard_normal((D, J)), rng.standard_normal(J), np.array([0.3, 0.6])
    mu, var = sr.components_points(x, CC, DD, sd)
    assert mu.shape == var.shape == (steps, J, K)
    np.testing.assert_allclose(mu, np.transpose(x @ CC + DD, (1, 2, 0)), rtol=0.0, atol=1e-14)
    assert np.all(var == (sd ** 2)[None, :, None])
    L = rng.standard_normal((K, steps, D, D)) * 0.3
    S = L @ np.swapaxes(L, -1, -2)
    mu2, var2 = sr.components_moments(x, S, CC, DD, sd)
    np.testing.assert_allclose(mu2, mu, rtol=0.0, atol=1e-14)
    assert np.all(var2 > var)
    mu3, var3 = sr.components_moments(x, np.zeros_like(S), CC, DD, sd)
    np.testing.assert_allclose(var3, var, rtol=0.0, atol=1e-16)
    Y = rng.standard_normal((2, J))
    Y[1, 0] = np.nan
    lv = np.array([0.25, 0.75])
    r, clean = sr.score(mu2, var2, Y, lv), sr.score(mu2, var2, np.nan_to_num(Y), lv)
    assert r["crps"].shape == r["pit"].shape == (2, J) and r["quantiles"].shape == (steps, J, 2)
    assert np.isnan(r["crps"][1, 0]) and np.isnan(r["pit"][1, 0]) and np.sum(np.isnan(r["crps"])) == 1 == np.sum(np.isnan(r["pit"]))
    np.testing.assert_array_equal(r["quantiles"], clean["quantiles"])
    np.testing.assert_array_equal(r["crps"][0], clean["crps"][0])
    assert np.all((r["pit"][0] > 0.0) & (r["pit"][0] < 1.0)) and np.all(r["crps"][0] > 0.0)
