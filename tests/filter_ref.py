"""NumPy restatement of Gaussian filtering and RTS smoothing by moment matching ("Filtering and smoothing";
Deisenroth et al. 2012): test infrastructure, no product path imports it.  Built on moment_ref.step_parts / ge_solve, in a
floating-point type of the caller's choice (np.float64: the reference; np.longdouble: that reference's own error).

The transition is a callable  trans(i, mu, S) -> (E[f], Cov(f), V)  with f = x_i - x_{i-1} WITHOUT the process noise and column a of
V = Cov(x_{i-1}, f_a): `gp_transition` wraps moment_ref.step_parts, `linear_transition` is x' = A x + b, for which the filter is
exact.  The measurement update is written in the JOINT form (gain K = S H (H^T S H + R)^-1, log-determinant from ge_solve's
determinant), which makes it independent of the sequence of scalar updates the device runs; `update="sequential"` is that sequence,
kept here to pin the two against each other.  The timing convention is the project's: the state after step i emits row i of Y."""
import numpy as np

import moment_ref as mr


def gp_transition(ctrl, Z, kern, beta, Gam, dtype=np.float64):
    """ctrl (>= steps, C) or None"""
    def trans(i, mu, S):
        c = np.zeros(0, dtype=dtype) if ctrl is None else ctrl[i]
        return mr.step_parts(mu, S, c, Z, kern, beta, Gam, dtype=dtype)
    return trans


def linear_transition(A, b, dtype=np.float64):
    A, b = np.asarray(A, dtype=dtype), np.asarray(b, dtype=dtype)
    F = A - np.eye(A.shape[0], dtype=dtype)

    def trans(i, mu, S):
        return F @ mu + b, F @ S @ F.T, S @ F.T
    return trans


def _mirror(S):
    return np.triu(S) + np.triu(S, 1).T


def _log2pi(t):
    return np.log(t(2) * t(np.pi))


def update_joint(mu, S, y, CC, DD, sd, t):
    """(mu, S, joint log density) after conditioning on the observed (non-NaN) entries of y at once; nothing observed: unchanged, NaN"""
    idx = np.flatnonzero(~np.isnan(np.asarray(y, dtype=np.float64)))
    if idx.size == 0:
        return mu, S, t(np.nan)
    H = CC[:, idx]                                                               # (D, k)
    PH = S @ H
    Sy = H.T @ PH + np.diag(sd[idx] ** 2)
    e = np.asarray(y, dtype=t)[idx] - (H.T @ mu + DD[idx])
    sol, det = mr.ge_solve(Sy, np.concatenate((PH.T, e[:, None]), axis=1))       # Sy^-1 [H^T S | e]
    mu = mu + PH @ sol[:, -1]
    S = _mirror(S - PH @ sol[:, :-1])
    return mu, S, -0.5 * (idx.size * _log2pi(t) + np.log(det) + e @ sol[:, -1])


def update_sequential(mu, S, y, CC, DD, sd, t):
    """the same conditioning as scalar updates in ascending j (exact: the noise is diagonal)"""
    lj, seen = t(0), False
    for j in range(len(y)):
        if np.isnan(np.float64(y[j])):
            continue
        h = CC[:, j]
        Sh = S @ h
        s = h @ Sh + sd[j] ** 2
        e = t(y[j]) - h @ mu - DD[j]
        mu = mu + Sh * e / s
        S = _mirror(S - np.outer(Sh, Sh) / s)
        lj, seen = lj - 0.5 * (_log2pi(t) + np.log(s)) - 0.5 * e * e / s, True
    return mu, S, (lj if seen else t(np.nan))


def filter(mu0, S0, Y, CC, DD, sd, Q, trans, dtype=np.float64, update="joint"):
    """Y (steps, J), NaN = unobserved.  Returns a dict: m_pred, S_pred, m_filt, S_filt, cross (steps, ...), lpd (steps, J; the
    marginal of every observed entry under the predicted state), lpd_joint (steps,)."""
    t = dtype
    upd = update_joint if update == "joint" else update_sequential
    mu, S = np.asarray(mu0, dtype=t), np.asarray(S0, dtype=t)
    CC, DD, sd = np.asarray(CC, dtype=t), np.asarray(DD, dtype=t), np.asarray(sd, dtype=t)
    Y = np.asarray(Y)
    n, J, D = Y.shape[0], CC.shape[1], mu.shape[0]
    Qd = np.diag(np.asarray(Q, dtype=t))
    out = dict(m_pred=np.zeros((n, D), dtype=t), S_pred=np.zeros((n, D, D), dtype=t), m_filt=np.zeros((n, D), dtype=t),
               S_filt=np.zeros((n, D, D), dtype=t), cross=np.zeros((n, D, D), dtype=t), lpd=np.full((n, J), np.nan, dtype=t),
               lpd_joint=np.full(n, np.nan, dtype=t))
    for i in range(n):
        Ef, Cf, V = trans(i, mu, S)
        X = S + V
        mu = mu + Ef
        S = S + Cf + V + V.T + Qd                                                # (moment_ref.propagate's expression, in its order)
        S = _mirror(S)
        out["m_pred"][i], out["S_pred"][i], out["cross"][i] = mu, S, X
        ym, yv = CC.T @ mu + DD, np.einsum("kj,kl,lj->j", CC, S, CC) + sd ** 2
        seen = ~np.isnan(np.asarray(Y[i], dtype=np.float64))
        r = np.where(seen, np.asarray(Y[i], dtype=t), ym) - ym
        out["lpd"][i] = np.where(seen, -0.5 * (_log2pi(t) + np.log(yv)) - 0.5 * r * r / yv, t(np.nan))
        mu, S, out["lpd_joint"][i] = upd(mu, S, Y[i], CC, DD, sd, t)
        out["m_filt"][i], out["S_filt"][i] = mu, S
    return out


def smooth(f, dtype=np.float64):
    """RTS pass over the dict of `filter`: m_smooth (steps, D), S_smooth (steps, D, D); the last row is the filtered one."""
    t = dtype
    n = f["m_filt"].shape[0]
    ms, Ss = np.array(f["m_filt"], dtype=t), np.array(f["S_filt"], dtype=t)
    for i in range(n - 2, -1, -1):
        Sp, X = np.asarray(f["S_pred"][i + 1], dtype=t), np.asarray(f["cross"][i + 1], dtype=t)
        JT, _ = mr.ge_solve(Sp, X.T)                                             # J^T = (S^-)^-1 X^T
        Jm = JT.T
        ms[i] = f["m_filt"][i] + Jm @ (ms[i + 1] - f["m_pred"][i + 1])
        Ss[i] = _mirror(f["S_filt"][i] + Jm @ (Ss[i + 1] - Sp) @ Jm.T)
    return ms, Ss
