"""NumPy restatement of the cubature (sigma-point) transition of the filter ("Cubature filtering"; Arasaratnam &
Haykin 2009, the third-degree spherical rule): test infrastructure, no product path imports it.  `ckf_transition` is a transition
callable of filter_ref.filter, built on transition_grad_ref.linearize evaluated at the 2D points of a step, in a floating-point type
of the caller's choice (np.float64: the reference; np.longdouble: that reference's own error).

With L the lower Cholesky factor of S without pivoting (a pivot <= 0 gives a zero column: S = 0 and rank-deficient S are allowed),
dx_i = +sqrt(D) (column i of L), dx_{i+D} = -dx_i, the points x_i = [mu + dx_i, ctrl[i]] and w = 1 / (2D), it returns
  E[f] = w sum_i m(x_i),  Cov(f) = w sum_i (m(x_i) - E[f]) (m(x_i) - E[f])^T + diag(w sum_i v(x_i)),  V = w sum_i dx_i (m(x_i) - E[f])^T
with m, v the mean and variance of the conditional, so that filter_ref.filter forms m^- = mu + E[f],
S^- = S + Cov(f) + V + V^T + Q and cross = S + V.

`cubature_transition` is the rule for any conditional (an affine map, for which it is exact, among them).  `tracks` and `reference`
are records_ref's compositions with this transition: one filter_ref.filter per (group, record)."""
import numpy as np

import filter_ref as fr
import moment_ref as mr
import records_ref as rr
import transition_grad_ref as tg

MOMENTS, DENSITIES = rr.MOMENTS, rr.DENSITIES


def factor(S, dtype=np.float64):
    """Lower Cholesky factor without pivoting; a pivot <= 0 (or NaN) leaves its column zero."""
    t = dtype
    S = np.asarray(S, dtype=t)
    D = S.shape[0]
    L = np.zeros((D, D), dtype=t)
    for j in range(D):
        p = S[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0:
            continue
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, D):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def offsets(S, dtype=np.float64):
    """(2D, D): row i is dx_i"""
    t = dtype
    D = np.shape(S)[0]
    half = (np.sqrt(t(D)) * factor(S, dtype=t)).T
    return np.concatenate((half, -half))


def cubature_transition(cond, dtype=np.float64):
    """The rule for any conditional: cond(i, X) -> (mean, var), each (2D, D), at the state rows X (2D, D) of step i."""
    t = dtype

    def trans(i, mu, S):
        mu, S = np.asarray(mu, dtype=t), np.asarray(S, dtype=t)
        D = mu.shape[0]
        dx = offsets(S, dtype=t)
        mean, var = cond(i, mu[None, :] + dx)
        w = t(1) / t(2 * D)
        Ef = w * mean.sum(axis=0)
        dm = mean - Ef[None, :]
        return Ef, w * (dm.T @ dm) + np.diag(w * var.sum(axis=0)), w * (dx.T @ dm)
    return trans


def ckf_transition(ctrl, Z, kern, beta, Gam, dtype=np.float64):
    """The rule on the GP conditional of one group; ctrl (>= steps, C) or None"""
    t = dtype

    def cond(i, X):
        c = np.zeros(0, dtype=t) if ctrl is None else np.asarray(ctrl[i], dtype=t)
        rows = np.concatenate((X, np.broadcast_to(c, (X.shape[0], c.shape[0]))), axis=1)
        return tg.linearize(rows, Z, kern, beta, Gam, dtype=t)[:2]
    return cubature_transition(cond, dtype=t)


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, lengths=None, dtype=np.float64):
    """records_ref.tracks with the cubature transition: arrays (G, R, steps, ...) in `dtype`, NaN at and beyond a record's length."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    tail = dict(m_pred=(D,), S_pred=(D, D), m_filt=(D,), S_filt=(D, D), cross=(D, D), m_smooth=(D,), S_smooth=(D, D), lpd=(J,), lpd_joint=())
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=dtype) for k, s in tail.items()}
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            trans = ckf_transition(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = fr.filter(x0[g][r], S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], trans, dtype=dtype)
            f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=dtype)
            for k in tail:
                out[k][g, r, :n] = f[k]
    return out


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide):
    """records_ref.reference with the cubature transition: `tracks` in fp64 (`ref`) and its largest error per array against the same
    composition in np.longdouble (`e_ref`; zeros when `wide` is false)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, lengths, dtype=t)
    ref = res[np.float64]
    e_ref = {}
    for k in MOMENTS + DENSITIES:
        ok = ~np.isnan(ref[k])
        e_ref[k] = float(np.max(np.abs(ref[k][ok] - res[np.longdouble][k][ok]))) if wide and ok.any() else 0.0
    return ref, e_ref
