"""NumPy restatement of the linearised (extended Kalman) transition of the filter ("Linearised filtering"): test
infrastructure, no product path imports it.  `ekf_transition` is a transition callable of filter_ref.filter, built on
transition_grad_ref.linearize evaluated at the single row [mu, ctrl[i]], in a floating-point type of the caller's choice (np.float64:
the reference; np.longdouble: that reference's own error).

With m, v the mean and variance of the conditional at that row and J the Jacobian of m with respect to the D state columns, it
returns  E[f] = m,  Cov(f) = J S J^T + diag(v),  V = S J^T,  so that filter_ref.filter forms  m^- = mu + m,
S^- = S + Cov(f) + V + V^T + Q = A S A^T + diag(v + Q)  and  cross = S + V = S A^T  with A = I + J."""
import numpy as np

import transition_grad_ref as tg


def ekf_transition(ctrl, Z, kern, beta, Gam, dtype=np.float64):
    """ctrl (>= steps, C) or None"""
    t = dtype

    def trans(i, mu, S):
        mu, S = np.asarray(mu, dtype=t), np.asarray(S, dtype=t)
        c = np.zeros(0, dtype=t) if ctrl is None else np.asarray(ctrl[i], dtype=t)
        x = np.concatenate((mu, c))[None, :]
        mean, var, dmean, _ = tg.linearize(x, Z, kern, beta, Gam, dtype=t)
        J = dmean[0][:, :mu.shape[0]]                                            # (D, D): row = dim of f, column = state component
        return mean[0], J @ S @ J.T + np.diag(var[0]), S @ J.T
    return trans
