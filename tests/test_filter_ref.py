"""The mathematics of tests/filter_ref.py (the NumPy restatement the GPU filter tests compare with), pinned without a device:

1. with a LINEAR transition x' = A x + b + N(0, Q), for which assumed-density filtering is exact, the filtered and smoothed moments and
   the sum of lpd_joint equal the exact conditioning of the stacked joint Gaussian of all states and observations (a brute-force
   n D system through np.linalg), with whole-row, single-entry and trailing gaps;
2. the sequence of scalar updates (what the device runs) equals the joint update (what the reference runs);
3. with no observation at all the filter IS moment_ref.propagate, bit for bit.

Bound 1e-11 (the systems are of order one and conditioned below 1e4: rounding is near 1e-14); the measured value is printed."""
import numpy as np
import pytest

import filter_ref as fr
import moment_ref as mr
from oracle import ffvd_oracle as orc

TOL, STEPS = 1e-11, 6
NAN = np.nan


def _linear_case(D, J, seed):
    rng = np.random.default_rng(seed)
    A = 0.8 * np.eye(D) + 0.2 * rng.standard_normal((D, D))
    b, Q = 0.3 * rng.standard_normal(D), 0.02 + 0.05 * rng.random(D)
    R = rng.standard_normal((D, D))
    S0, mu0 = 0.1 * (R @ R.T) / D + 0.05 * np.eye(D), rng.standard_normal(D)
    CC, DD, sd = rng.standard_normal((D, J)), rng.standard_normal(J), (0.4, 0.05, 1.3)[:J] if J == 3 else (0.3,)
    Y = rng.standard_normal((STEPS, J))
    Y[1, :] = NAN                                                               # a whole row
    if J > 1:
        Y[2, 1] = NAN                                                           # one entry missing
        Y[3, :2] = NAN                                                          # one entry present
    return A, b, Q, mu0, S0, CC, DD, np.asarray(sd), Y


def _brute_force(A, b, Q, mu0, S0, CC, DD, sd, Y, upto):
    """Posterior mean / covariance of z = [x_1 .. x_n] (x_i: the state after step i - 1, which emits row i - 1) given the observed
    entries of rows < upto, and the log marginal likelihood of those entries."""
    n, D = Y.shape[0], mu0.shape[0]
    mz, Sz = np.zeros(n * D), np.zeros((n * D, n * D))
    m, S, blocks = mu0, S0, []
    for i in range(n):
        m, S = A @ m + b, A @ S @ A.T + np.diag(Q)
        mz[i * D:(i + 1) * D], blocks = m, blocks + [S]
    for i in range(n):
        Cij = blocks[i]
        for j in range(i, n):
            Sz[i * D:(i + 1) * D, j * D:(j + 1) * D] = Cij
            Sz[j * D:(j + 1) * D, i * D:(i + 1) * D] = Cij.T
            Cij = Cij @ A.T
    rows, ys, ds, rs = [], [], [], []
    for i in range(upto):
        for j in range(Y.shape[1]):
            if not np.isnan(Y[i, j]):
                h = np.zeros(n * D)
                h[i * D:(i + 1) * D] = CC[:, j]
                rows.append(h), ys.append(Y[i, j]), ds.append(DD[j]), rs.append(sd[j] ** 2)
    if not rows:
        return mz, Sz, 0.0
    H, y = np.stack(rows), np.asarray(ys)
    Sy = H @ Sz @ H.T + np.diag(rs)
    e = y - (H @ mz + np.asarray(ds))
    K = np.linalg.solve(Sy, H @ Sz).T
    ll = -0.5 * (len(y) * np.log(2 * np.pi) + np.linalg.slogdet(Sy)[1] + e @ np.linalg.solve(Sy, e))
    return mz + K @ e, Sz - K @ H @ Sz, ll


@pytest.mark.parametrize("trailing", [False, True], ids=["", "trailing gap"])
@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("D", [2, 3])
def test_linear_transition_against_the_stacked_joint_gaussian(D, J, trailing):
    A, b, Q, mu0, S0, CC, DD, sd, Y = _linear_case(D, J, 10 * D + J)
    if trailing:
        Y[-2:] = NAN
    f = fr.filter(mu0, S0, Y, CC, DD, sd, Q, fr.linear_transition(A, b))
    ms, Ss = fr.smooth(f)
    err = 0.0
    for i in range(STEPS):
        sl = slice(i * D, (i + 1) * D)
        mz, Sz, _ = _brute_force(A, b, Q, mu0, S0, CC, DD, sd, Y, i)            # given rows < i: the predicted state of index i
        err = max(err, np.max(np.abs(f["m_pred"][i] - mz[sl])), np.max(np.abs(f["S_pred"][i] - Sz[sl, sl])))
        if i > 0:
            pl = slice((i - 1) * D, i * D)
            err = max(err, np.max(np.abs(f["cross"][i] - Sz[pl, sl])))
        mz, Sz, _ = _brute_force(A, b, Q, mu0, S0, CC, DD, sd, Y, i + 1)        # given rows <= i: the filtered state
        err = max(err, np.max(np.abs(f["m_filt"][i] - mz[sl])), np.max(np.abs(f["S_filt"][i] - Sz[sl, sl])))
    mz, Sz, ll = _brute_force(A, b, Q, mu0, S0, CC, DD, sd, Y, STEPS)           # given everything: the smoothed states
    for i in range(STEPS):
        sl = slice(i * D, (i + 1) * D)
        err = max(err, np.max(np.abs(ms[i] - mz[sl])), np.max(np.abs(Ss[i] - Sz[sl, sl])))
    e_ll = abs(np.nansum(f["lpd_joint"]) - ll)
    print(f"D={D} J={J} trailing={trailing}: moments {err:.3e}, sum of lpd_joint {e_ll:.3e} (log likelihood {ll:.6f})")
    assert err <= TOL and e_ll <= TOL
    seen = ~np.isnan(Y)
    assert np.array_equal(np.isnan(f["lpd"]), ~seen) and np.array_equal(np.isnan(f["lpd_joint"]), ~seen.any(axis=1))
    np.testing.assert_array_equal(ms[-1], f["m_filt"][-1])
    np.testing.assert_array_equal(Ss[-1], f["S_filt"][-1])
    for i in np.flatnonzero(~seen.any(axis=1)):                                  # a row without an observation changes nothing
        np.testing.assert_array_equal(f["m_filt"][i], f["m_pred"][i])
        np.testing.assert_array_equal(f["S_filt"][i], f["S_pred"][i])
    # one observed entry in a row: the joint density of the row is that entry's marginal
    one = np.flatnonzero(seen.sum(axis=1) == 1)
    assert np.max(np.abs(f["lpd_joint"][one] - np.nansum(f["lpd"][one], axis=1))) <= TOL


def _gp_case(D, J, seed, M=7, C=1):
    """A proper sparse-GP posterior (W = L^-T of K_uu, |q| < 1: variances stay positive over the steps) with a contracting mean."""
    rng = np.random.default_rng(seed)
    P = D + C
    kern = [orc.SquaredExponential(np.log(0.5 + rng.random()), np.log(0.8 + rng.random(P))) for _ in range(D)]
    Z = rng.standard_normal((M, P))
    W = []
    for k in kern:
        d = (Z[:, None, :] - Z[None, :, :]) / np.exp(k.loglengthscales)[None, None, :]
        K = np.exp(k.logvariance) * np.exp(-0.5 * np.sum(d * d, axis=2)) + 1e-6 * np.eye(M)
        W.append(np.linalg.inv(np.linalg.cholesky(K)).T)
    U = 0.3 * rng.standard_normal((M, D))
    q = np.triu(rng.standard_normal((D, M, M)))
    q = 0.7 * q / np.linalg.norm(q, ord=2, axis=(1, 2))[:, None, None]
    beta, Gam = mr.posterior_terms(W, U, q, "reference")
    R = rng.standard_normal((D, D))
    mu, S, Q = 0.3 * rng.standard_normal(D), 0.05 * (R @ R.T) / D + 0.02 * np.eye(D), 0.01 + 0.02 * rng.random(D)
    ctrl = rng.standard_normal((STEPS, C))
    CC, DD, sd = rng.standard_normal((D, J)), rng.standard_normal(J), np.asarray((0.4, 0.05, 1.3)[:J])
    return kern, Z, beta, Gam, mu, S, ctrl, Q, CC, DD, sd


@pytest.mark.parametrize("D,J", [(1, 1), (2, 1), (2, 3)])
def test_sequential_update_against_the_joint_update(D, J):
    kern, Z, beta, Gam, mu, S, ctrl, Q, CC, DD, sd = _gp_case(D, J, 7 * D + J)
    trans = fr.gp_transition(ctrl, Z, kern, beta, Gam)
    free = fr.filter(mu, S, np.full((STEPS, J), NAN), CC, DD, sd, Q, trans)
    rng = np.random.default_rng(3)
    Y = free["m_pred"] @ CC + DD + 0.5 * rng.standard_normal((STEPS, J))
    Y[2, :] = NAN
    if J > 1:
        Y[3, 0] = NAN
    a, b = fr.filter(mu, S, Y, CC, DD, sd, Q, trans), fr.filter(mu, S, Y, CC, DD, sd, Q, trans, update="sequential")
    sa, sb = fr.smooth(a), fr.smooth(b)
    err = max(float(np.nanmax(np.abs(a[k] - b[k]))) for k in a)
    err = max(err, float(np.max(np.abs(sa[0] - sb[0]))), float(np.max(np.abs(sa[1] - sb[1]))))
    print(f"D={D} J={J}: sequential against joint {err:.3e}")
    assert err <= TOL
    for k in a:
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k


@pytest.mark.parametrize("D", [1, 2])
def test_without_observations_the_filter_is_the_propagation(D):
    kern, Z, beta, Gam, mu, S, ctrl, Q, CC, DD, sd = _gp_case(D, 2, 40 + D)
    f = fr.filter(mu, S, np.full((STEPS, 2), NAN), CC, DD, sd, Q, fr.gp_transition(ctrl, Z, kern, beta, Gam))
    m_x, S_x = mr.propagate(mu, S, ctrl, Z, kern, beta, Gam, Q, STEPS)
    for k, ref in (("m_pred", m_x), ("m_filt", m_x), ("S_pred", S_x), ("S_filt", S_x)):
        np.testing.assert_array_equal(f[k], ref, err_msg=k)
    assert np.all(np.isnan(f["lpd"])) and np.all(np.isnan(f["lpd_joint"]))
    ms, Ss = fr.smooth(f)                                                        # nothing was learnt: smoothing changes nothing but rounding
    assert np.max(np.abs(ms - m_x)) <= TOL and np.max(np.abs(Ss - S_x)) <= TOL
