"""The fp64 NumPy / scipy restatement of the scores of ffvd_amd/csrc/predict_score.h: CRPS, PIT and quantiles of an equal-weight
mixture of K Gaussians N(mu_k, v_k) per target (row t, output j), and the components themselves from a stack of points or of
Gaussian states.  tests/test_score_ref.py pins it (mpmath, the single-Gaussian closed form, quadrature, F(q_p) = p, permutations);
tests/test_gpu_score.py holds the device to it.

  A(d, v)    = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v))                      (= E|N(d, v)|)
  crps       = (1/K) sum_k A(y - mu_k, v_k) - (1/(2 K^2)) sum_k sum_l A(mu_k - mu_l, v_k + v_l)      (Grimit et al. 2006)
  pit        = F(y),  F(x) = (1/K) sum_k Phi((x - mu_k) / sqrt v_k)
  quantile_p = the x with F(x) = p: scipy.optimize.brentq inside [min mu - 8.5 max sigma, max mu + 8.5 max sigma]
"""
import numpy as np
from scipy.optimize import brentq
from scipy.special import erf, erfc

EPS = float(np.finfo(np.float64).eps)
BRACKET = 8.5


def components_points(x, CC, DD, sd):
    """x (K, steps, D) -> mu, var (steps, J, K): mu = sum_d x CC (d ascending) + DD_j, var = sd_j^2"""
    x, CC = np.asarray(x, dtype=np.float64), np.asarray(CC, dtype=np.float64)
    K, steps, D = x.shape
    acc = np.zeros((K, steps, CC.shape[1]))
    for d in range(D):
        acc = acc + x[:, :, d, None] * CC[d][None, None, :]
    mu = np.transpose(acc + np.asarray(DD)[None, None, :], (1, 2, 0))
    return np.ascontiguousarray(mu), np.ascontiguousarray(np.broadcast_to((np.asarray(sd) ** 2)[None, :, None], mu.shape))


def components_moments(m, S, CC, DD, sd):
    """m (G, steps, D), S (G, steps, D, D) -> mu, var (steps, J, G): mu = CC_j^T m + DD_j, var = CC_j^T S CC_j + sd_j^2"""
    m, S, CC = np.asarray(m, dtype=np.float64), np.asarray(S, dtype=np.float64), np.asarray(CC, dtype=np.float64)
    mu = np.einsum("gtd,dj->tjg", m, CC) + np.asarray(DD)[None, :, None]
    var = np.einsum("aj,gtab,bj->tjg", CC, S, CC) + (np.asarray(sd) ** 2)[None, :, None]
    return np.ascontiguousarray(mu), np.ascontiguousarray(var)


def abs_moment(d, v):
    """A(d, v) = E|N(d, v)|"""
    return d * erf(d / np.sqrt(2.0 * v)) + np.sqrt(2.0 * v / np.pi) * np.exp(-d * d / (2.0 * v))


def crps(mu, var, y):
    """mu, var (..., K), y (...) -> crps (...); NaN where y is NaN"""
    mu, var, y = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K = mu.shape[-1]
    out = np.empty(y.shape)
    for i in np.ndindex(*y.shape):
        m, v = mu[i], var[i]
        first = np.sum(abs_moment(y[i] - m, v)) / K
        pair = np.sum(abs_moment(m[:, None] - m[None, :], v[:, None] + v[None, :]))
        out[i] = first - pair / (2.0 * K * K)
    return out


def cdf(mu, var, x):
    """F(x) of the mixtures mu, var (..., K) at x (...)"""
    x = np.asarray(x, dtype=np.float64)
    return np.mean(0.5 * erfc((mu - x[..., None]) / np.sqrt(2.0 * var)), axis=-1)


def pdf(mu, var, x):
    x = np.asarray(x, dtype=np.float64)
    return np.mean(np.exp(-(x[..., None] - mu) ** 2 / (2.0 * var)) / np.sqrt(2.0 * np.pi * var), axis=-1)


def bracket(mu, var):
    w = BRACKET * np.sqrt(np.max(var, axis=-1))
    return np.min(mu, axis=-1) - w, np.max(mu, axis=-1) + w


def quantile(mu, var, p):
    """the x with F(x) = p of ONE mixture (mu, var (K,)): brentq to rounding level"""
    lo, hi = bracket(mu, var)
    return brentq(lambda x: float(cdf(mu, var, np.float64(x))) - p, float(lo), float(hi), xtol=4.0 * EPS, rtol=4.0 * EPS, maxiter=500)


def quantiles(mu, var, levels):
    """mu, var (..., K), levels (Q,) -> (..., Q)"""
    out = np.empty(mu.shape[:-1] + (len(levels),))
    for i in np.ndindex(*mu.shape[:-1]):
        for q, p in enumerate(levels):
            out[i + (q,)] = quantile(mu[i], var[i], float(p))
    return out


def score(mu, var, Y, levels):
    """What the device calls return for the mixtures mu, var (steps, J, K): crps, pit (n_test, J) (None without Y), quantiles
    (steps, J, Q)."""
    res = dict(crps=None, pit=None, quantiles=quantiles(mu, var, levels))
    if Y is not None:
        Y = np.asarray(Y, dtype=np.float64)
        n = Y.shape[0]
        res["crps"], res["pit"] = crps(mu[:n], var[:n], Y), np.where(np.isnan(Y), np.nan, cdf(mu[:n], var[:n], np.nan_to_num(Y)))
    return res


def crps_gaussian(mu, sigma, y):
    """the closed form for one Gaussian: sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)], z = (y - mu) / sigma"""
    z = (y - mu) / sigma
    Phi, phi = 0.5 * erfc(-z / np.sqrt(2.0)), np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    return sigma * (z * (2.0 * Phi - 1.0) + 2.0 * phi - 1.0 / np.sqrt(np.pi))
