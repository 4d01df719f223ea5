"""NumPy restatement of the fully adapted particle filter over many records ("Adapted particle filtering"): test
infrastructure, no product path imports it.  In a floating-point type of the caller's choice (np.float64: the reference;
np.longdouble: that reference's own error).

Per track with N particles and the draws of tests/particle_filter_ref.py (eps (steps, N, D), unif (steps,), xi0 (N, D)); X_t is the
equally weighted set carried into row t, X_0 the bootstrap reference's start by the same expression:
  parents    (mean, var) = cond(t, X_t):  mu = X_t + mean,  s = var + Q
  moments    m_pred = sum_i mu_i / N,  S_pred = sum_i (mu_i - m_pred)(mu_i - m_pred)^T / N + diag(sum_i s_i / N)  (mirrored)
  densities  lpd[t, j] = log mean_i N(y_tj; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + sd_j^2), the largest exponent subtracted,
             NaN where y_tj is NaN
  update     per particle from (m, P) = (mu_i, diag s_i), L_i = 0, over the observed j in ascending order:
             h = P c_j, sig2 = c_j . h + sd_j^2, r = y_tj - (c_j . m + DD_j), L_i += -1/2 (log 2 pi + log sig2 + r^2 / sig2),
             m += h (r / sig2), P -= h h^T / sig2                                                      -> mt_i, P_i
  filtered   lpd_joint[t] = log mean_i exp L_i;  W_i = exp(L_i - max L);  ess = (sum W)^2 / sum W^2;
             m_filt = sum W mt / sum W,  S_filt = sum W (P_i + (mt_i - m_filt)(mt_i - m_filt)^T) / sum W  (mirrored)
  resample   particle_filter_ref.ancestors(W, unif[t]) -> a
  draw       X_{t+1,i} = mt_{a_i} + factor(P_{a_i}) eps[t, i]   (cubature_filter_ref.factor's convention: unpivoted, a pivot <= 0
             leaves its column zero)
  a row with nothing observed: X_{t+1} = X_t + mean + eps[t] sqrt(var + Q) (the bootstrap reference's expression), a_i = i, W = 1,
             ess = N, m_filt = m_pred, S_filt = S_pred, lpd_joint NaN
particles[t] is X_{t+1}, the filtered set after row t; ancestors[t, i] indexes the set carried into row t.  log_evidence is the sum of
lpd_joint over the rows that have an observation.

`run`, `tracks` and `reference` are shaped like particle_filter_ref's, whose `ancestors`, `gp_cond`, `draws_of` and `margin` are
reused.  `update` and `factors` are the two per-particle pieces, vectorised over the particles."""
import numpy as np

import cubature_filter_ref as cf
import moment_ref as mr
import particle_filter_ref as pf
from particle_filter_ref import DENSITIES, EXTRA, MOMENTS, ancestors, draws_of, gp_cond, margin   # noqa: F401  (reused by the tests)


def update(mu, s, y, seen, CC, DD, sd, dtype=np.float64):
    """The exact scalar updates of every particle over the observed outputs in ascending j.  mu, s (N, D); y (J,) with any value where
    `seen` is False.  Returns mt (N, D), P (N, D, D) and L (N,)."""
    t = dtype
    N, D = mu.shape
    m = np.array(mu, dtype=t)
    P = np.zeros((N, D, D), dtype=t)
    P[:, np.arange(D), np.arange(D)] = s
    L = np.zeros(N, dtype=t)
    for j in np.flatnonzero(seen):
        c = CC[:, j]
        h = P @ c                                                                   # (N, D)
        sig2 = h @ c + sd[j] * sd[j]
        r = y[j] - (m @ c + DD[j])
        L = L + t(-0.5) * (pf._log2pi(t) + np.log(sig2) + r * r / sig2)
        m = m + h * (r / sig2)[:, None]
        P = P - h[:, :, None] * h[:, None, :] / sig2[:, None, None]
    return m, P, L


def factors(P, dtype=np.float64):
    """cubature_filter_ref.factor of every P[i] (N, D, D): lower Cholesky factors without pivoting, a pivot <= 0 (or NaN) leaves its
    column zero.  Returns the factors (N, D, D) and which columns were zeroed (N, D)."""
    t = dtype
    P = np.asarray(P, dtype=t)
    N, D = P.shape[:2]
    Lf, zeroed = np.zeros((N, D, D), dtype=t), np.zeros((N, D), dtype=bool)
    for j in range(D):
        p = P[:, j, j] - np.einsum("nk,nk->n", Lf[:, j, :j], Lf[:, j, :j])
        ok = p > 0
        zeroed[:, j] = ~ok
        q = np.sqrt(np.where(ok, p, t(1)))
        Lf[:, j, j] = np.where(ok, q, t(0))
        for i in range(j + 1, D):
            v = (P[:, i, j] - np.einsum("nk,nk->n", Lf[:, i, :j], Lf[:, j, :j])) / q
            Lf[:, i, j] = np.where(ok, v, t(0))
    return Lf, zeroed


def run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0=None, dtype=np.float64):
    """One track.  cond(i, X) -> (mean, var), each (N, D), at the state rows X (N, D) of step i.  Y (steps, J), NaN = unobserved.
    Returns a dict: MOMENTS, lpd (steps, J), lpd_joint, ess (steps,), particles (steps, N, D: the filtered sets X_{t+1}), ancestors
    (steps, N) int, cdf (steps, N: cdf / tot, ones where nothing is observed), zeroed (steps, N, D: the columns of the factor of the
    drawn particle's parent that a pivot <= 0 left zero), log_evidence."""
    t = dtype
    eps, unif = np.asarray(eps, dtype=t), np.asarray(unif, dtype=t)
    CC, DD, sd, Q = np.asarray(CC, dtype=t), np.asarray(DD, dtype=t), np.asarray(sd, dtype=t), np.asarray(Q, dtype=t)
    Y = np.asarray(Y)
    (n, J), (N, D) = Y.shape, eps.shape[1:]
    X = np.broadcast_to(np.asarray(x0, dtype=t), (N, D)).copy()
    if S0 is not None:
        X = X + np.asarray(xi0, dtype=t) @ cf.factor(S0, dtype=t).T
    out = dict(m_pred=np.zeros((n, D), dtype=t), S_pred=np.zeros((n, D, D), dtype=t), m_filt=np.zeros((n, D), dtype=t),
               S_filt=np.zeros((n, D, D), dtype=t), lpd=np.full((n, J), np.nan, dtype=t), lpd_joint=np.full(n, np.nan, dtype=t),
               ess=np.zeros(n, dtype=t), particles=np.zeros((n, N, D), dtype=t), ancestors=np.zeros((n, N), dtype=np.int64),
               cdf=np.ones((n, N), dtype=t), zeroed=np.zeros((n, N, D), dtype=bool))
    for i in range(n):
        mean, var = cond(i, X)
        mu, s = X + mean, var + Q[None, :]
        mp = mu.sum(axis=0) / t(N)
        dx = mu - mp[None, :]
        Sp = pf._mirror(dx.T @ dx / t(N) + np.diag(s.sum(axis=0) / t(N)))
        out["m_pred"][i], out["S_pred"][i] = mp, Sp
        seen = ~np.isnan(np.asarray(Y[i], dtype=np.float64))
        y = np.where(seen, np.asarray(Y[i], dtype=t), t(0))
        if not seen.any():
            X = X + mean + eps[i] * np.sqrt(var + Q[None, :])
            out["particles"][i], out["ancestors"][i] = X, np.arange(N)
            out["m_filt"][i], out["S_filt"][i], out["ess"][i] = mp, Sp, t(N)
            continue
        s2 = s @ (CC * CC) + (sd * sd)[None, :]                                     # (N, J)
        r = y[None, :] - (mu @ CC + DD[None, :])
        l = t(-0.5) * (pf._log2pi(t) + np.log(s2) + r * r / s2)
        out["lpd"][i] = np.where(seen, pf._logmeanexp(l, t), t(np.nan))
        mt, P, L = update(mu, s, y, seen, CC, DD, sd, dtype=t)
        W = np.exp(L - L.max())
        sw = W.sum()
        mf = (W[:, None] * mt).sum(axis=0) / sw
        df = mt - mf[None, :]
        out["m_filt"][i] = mf
        out["S_filt"][i] = pf._mirror((W[:, None, None] * (P + df[:, :, None] * df[:, None, :])).sum(axis=0) / sw)
        out["ess"][i] = sw * sw / (W * W).sum()
        out["lpd_joint"][i] = pf._logmeanexp(L, t)
        a, cdf, tot = pf.ancestors(W, unif[i])
        out["ancestors"][i], out["cdf"][i] = a, cdf / tot
        Lf, zeroed = factors(P, dtype=t)
        X = mt[a] + np.einsum("nij,nj->ni", Lf[a], eps[i])
        out["particles"][i], out["zeroed"][i] = X, zeroed[a]
    out["log_evidence"] = np.nansum(out["lpd_joint"])
    return out


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0=None, lengths=None, dtype=np.float64):
    """particle_filter_ref.tracks with `run` above: arrays (G, R, steps, ...) in `dtype`, NaN (ancestors -1, zeroed False) at and
    beyond a record's length; log_evidence (G, R)."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    N = np.shape(eps)[-2]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    tail = dict(m_pred=(D,), S_pred=(D, D), m_filt=(D,), S_filt=(D, D), lpd=(J,), lpd_joint=(), ess=(), particles=(N, D), cdf=(N,))
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=dtype) for k, s in tail.items()}
    out["ancestors"] = np.full((G, R, steps, N), -1, dtype=np.int64)
    out["zeroed"] = np.zeros((G, R, steps, N, D), dtype=bool)
    out["log_evidence"] = np.zeros((G, R), dtype=dtype)
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            cond = gp_cond(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = run(cond, x0[g][r], None if S0 is None else S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], draws_of(eps, g, r, 3)[:n],
                    draws_of(unif, g, r, 1)[:n], None if xi0 is None else draws_of(xi0, g, r, 2), dtype=dtype)
            for k in list(tail) + ["ancestors", "zeroed"]:
                out[k][g, r, :n] = f[k]
            out["log_evidence"][g, r] = f["log_evidence"]
    return out


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide, eps, unif, xi0=None):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`), its largest error per array against the same
    composition in np.longdouble (`e_ref`; zeros when `wide` is false), and the longdouble composition itself (`wide_ref`, None when
    `wide` is false)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0, lengths, dtype=t)
    ref = res[np.float64]
    e_ref = {}
    for k in MOMENTS + DENSITIES + EXTRA:
        ok = ~np.isnan(ref[k])
        e_ref[k] = float(np.max(np.abs(ref[k][ok] - res[np.longdouble][k][ok]))) if wide and ok.any() else 0.0
    return ref, e_ref, res.get(np.longdouble) if wide else None
