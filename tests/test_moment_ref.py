"""The mathematics of moment-matched prediction, pinned without a device: the one-step mean, Cov(f), input-output covariance V and
Sigma' of tests/moment_ref.py (the NumPy restatement the GPU tests compare with) against tensor Gauss-Hermite quadrature -- 80 nodes
per axis -- of the oracle's conditional_after_kernel_precalculation at x ~ N(mu, Sigma), for D = 1 and D = 2 with one control column and
no q_sqrt / an upper-triangular q_sqrt / a dense q_sqrt.  The integrands are Gaussians times smooth SE kernels with lengthscales >= 0.8
against a state spread <= 0.45: 80 nodes integrate them to rounding (about 3e-15 was seen); 1e-11 is asserted, far below any wrong
term (the terms are 1e-3 and more)."""
import numpy as np
import pytest
from numpy.polynomial.hermite_e import hermegauss

import moment_ref as mr
from oracle import ffvd_oracle as orc

M, C, NODES, TOL = 7, 1, 80, 1e-11


def _case(D, qkind, seed):
    rng = np.random.default_rng(seed)
    P = D + C
    kern = [orc.SquaredExponential(np.log(0.5 + rng.random()), np.log(0.8 + rng.random(P))) for _ in range(D)]
    Z = rng.standard_normal((M, P))
    W = [np.triu(0.3 * rng.standard_normal((M, M))) + np.eye(M) for _ in range(D)]
    U = rng.standard_normal((M, D))
    q = None
    if qkind != "none":
        q = 0.25 * rng.standard_normal((D, M, M))
        if qkind == "upper":
            q = np.triu(q)
    A = rng.standard_normal((D, D))
    S = 0.05 * (A @ A.T) / D + 0.02 * np.eye(D)
    mu, c, Q = 0.3 * rng.standard_normal(D), rng.standard_normal(C), 0.01 + 0.02 * rng.random(D)
    return kern, Z, W, U, q, mu, S, c, Q


def _quadrature(kern, Z, W, U, q, mu, S, c):
    D = mu.shape[0]
    x1, w1 = hermegauss(NODES)
    w1 = w1 / np.sqrt(2 * np.pi)
    grids = np.meshgrid(*([x1] * D), indexing="ij")
    xi = np.stack([g.reshape(-1) for g in grids], axis=1)
    w = np.prod(np.stack([wg.reshape(-1) for wg in np.meshgrid(*([w1] * D), indexing="ij")], axis=1), axis=1)
    L = np.linalg.cholesky(S)
    dx = xi @ L.T
    X = np.concatenate((mu[None, :] + dx, np.repeat(c[None, :], xi.shape[0], axis=0)), axis=1)
    fm, fv = orc.conditional_after_kernel_precalculation(W, X, Z, kern, U, q_sqrt=q, white=True)
    Ef = w @ fm
    Cf = (fm * w[:, None]).T @ fm - np.outer(Ef, Ef) + np.diag(w @ fv)
    V = (dx * w[:, None]).T @ fm
    return Ef, Cf, V


@pytest.mark.parametrize("qkind", ["none", "upper", "dense"])
@pytest.mark.parametrize("D", [1, 2])
def test_one_step_against_gauss_hermite_quadrature(D, qkind):
    kern, Z, W, U, q, mu, S, c, Q = _case(D, qkind, 100 * D + ("none", "upper", "dense").index(qkind))
    beta, Gam = mr.posterior_terms(W, U, q, "reference")
    Ef, Cf, V = mr.step_parts(mu, S, c, Z, kern, beta, Gam)
    rEf, rCf, rV = _quadrature(kern, Z, W, U, q, mu, S, c)
    m1, S1 = mr.propagate(mu, S, c[None, :], Z, kern, beta, Gam, Q, 1)
    rS1 = S + rCf + rV + rV.T + np.diag(Q)
    errs = dict(mean=np.max(np.abs(Ef - rEf)), cov_f=np.max(np.abs(Cf - rCf)), V=np.max(np.abs(V - rV)),
                mean_next=np.max(np.abs(m1[0] - (mu + rEf))), S_next=np.max(np.abs(S1[0] - rS1)))
    print(f"D={D} q_sqrt={qkind}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert min(np.max(np.abs(rEf)), np.max(np.abs(rCf)), np.max(np.abs(rV))) > 1e-4          # nothing here is trivially zero
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    np.testing.assert_array_equal(S1[0], S1[0].T)


def test_the_intent_mode_uses_slice_a():
    """q_mode "intent": dim a's variance takes slice a -- equal to "reference" on dim 0, different on dim 1."""
    kern, Z, W, U, q, mu, S, c, Q = _case(2, "dense", 5)
    (b0, G0), (b1, G1) = mr.posterior_terms(W, U, q, "reference"), mr.posterior_terms(W, U, q, "intent")
    np.testing.assert_array_equal(b0, b1)
    np.testing.assert_array_equal(G0[0], G1[0])
    assert np.max(np.abs(G0[1] - G1[1])) > 1e-3
    fm, fv = orc.conditional_after_kernel_precalculation(W, np.concatenate((mu, c))[None, :], Z, kern, U, q_sqrt=q[1:2], white=True)
    _, Cf, _ = mr.step_parts(mu, np.zeros((2, 2)), c, Z, kern, b1, G1)
    assert abs(Cf[1, 1] - fv[0, 1]) <= 1e-12 and abs(Cf[0, 1]) <= 1e-14


def test_the_extended_precision_restatement_agrees():
    """np.longdouble runs through the same code (the hand-written elimination): the fp64 restatement is within 1e-12 of it"""
    kern, Z, W, U, q, mu, S, c, Q = _case(2, "upper", 9)
    W, U = [0.3 * w for w in W], 0.1 * U               # a gentle transition function: three steps stay in the data's range
    ld = np.longdouble
    b64, G64 = mr.posterior_terms(W, U, q, "reference")
    bl, Gl = mr.posterior_terms(W, U, q, "reference", dtype=ld)
    ctrl = np.repeat(c[None, :], 3, axis=0)
    m64, S64 = mr.propagate(mu, S, ctrl, Z, kern, b64, G64, Q, 3)
    ml, Sl = mr.propagate(mu, S, ctrl, Z, kern, bl, Gl, Q, 3, dtype=ld)
    assert ml.dtype == ld and Sl.dtype == ld and np.all(np.isfinite(m64)) and np.all(np.isfinite(S64))
    assert np.max(np.abs(m64 - ml)) <= 1e-12 and np.max(np.abs(S64 - Sl)) <= 1e-12
