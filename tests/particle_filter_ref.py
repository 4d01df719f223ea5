"""NumPy restatement of the bootstrap particle filter over many records ("Particle filtering"): test
infrastructure, no product path imports it.  In a floating-point type of the caller's choice (np.float64: the reference;
np.longdouble: that reference's own error).

Per track with N particles, eps (steps, N, D) standard normal, unif (steps,) in [0, 1), xi0 (N, D) standard normal:
  start      X_0 = x0 + xi0 L0^T, L0 = cubature_filter_ref.factor(S0) (unpivoted, a pivot <= 0 gives a zero column); S0 None: all at x0
  propagate  (m, v) = cond(t, X_t):  X^- = X_t + m + eps[t] sqrt(v + Q)
  moments    m_pred = sum_i X^-_i / N,  S_pred = sum_i (X^-_i - m_pred)(X^-_i - m_pred)^T / N  (centred, mirrored)
  densities  l_ij = log N(y_tj; CC[:, j] . X^-_i + DD_j, sd_j^2);  lpd[t, j] = max_i l_ij + log(sum_i exp(l_ij - max) / N), NaN where
             y_tj is NaN;  L_i = sum over the observed j of l_ij;  lpd_joint[t] the same expression on L, NaN with nothing observed
  filtered   W_i = exp(L_i - max L);  m_filt, S_filt the W-weighted mean and centred covariance;  ess = (sum W)^2 / sum W^2;
             nothing observed: W = 1
  resample   systematic, only with an observed entry: cdf = np.cumsum(W) (sequential), tot = cdf[-1],
             a_i = min(#{k: cdf_k <= (unif[t] + i) / N tot}, N - 1) (oracle/ffvd_pg_oracle.categorical_from_uniform's convention, sorted
             thresholds);  X_{t+1} = X^-[a];  otherwise a_i = i
log_evidence is the sum of lpd_joint over the rows that have an observation.

`run` is the method for any conditional cond(i, X) -> (mean, var); `gp_cond` is the GP conditional of one group through
transition_grad_ref.linearize(...)[:2]; `tracks` and `reference` are shaped like cubature_filter_ref's.  `margin` measures the
condition the device tests rest on: how far every threshold is from every cdf entry."""
import numpy as np

import cubature_filter_ref as cf
import moment_ref as mr
import transition_grad_ref as tg

MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt")
DENSITIES = ("lpd", "lpd_joint")
EXTRA = ("ess", "particles")


def _log2pi(t):
    return np.log(t(2) * t(np.pi))


def _mirror(S):
    return np.triu(S) + np.triu(S, 1).T


def _logmeanexp(L, t):
    mx = L.max(axis=0)
    return mx + np.log(np.exp(L - mx).sum(axis=0) / t(L.shape[0]))


def ancestors(W, u):
    """Systematic resampling: W (N,) non-negative weights, u in [0, 1).  Returns the ancestors (N,), the cdf and its total."""
    t = W.dtype.type
    N = W.shape[0]
    cdf = np.cumsum(W)                                            # sequential, index order
    tot = cdf[-1]
    thr = (t(u) + np.arange(N, dtype=W.dtype)) / t(N) * tot
    return np.minimum(np.searchsorted(cdf, thr, side="right"), N - 1), cdf, tot


def run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0=None, dtype=np.float64):
    """One track.  cond(i, X) -> (mean, var), each (N, D), at the state rows X (N, D) of step i.  Y (steps, J), NaN = unobserved.
    Returns a dict: MOMENTS, lpd (steps, J), lpd_joint, ess (steps,), particles (steps, N, D: the X^-), ancestors (steps, N) int,
    cdf (steps, N: cdf / tot, ones where nothing is observed), log_evidence."""
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
               cdf=np.ones((n, N), dtype=t))
    lc = -0.5 * (_log2pi(t) + np.log(sd * sd))
    for i in range(n):
        mean, var = cond(i, X)
        X = X + mean + eps[i] * np.sqrt(var + Q[None, :])
        mp = X.sum(axis=0) / t(N)
        dx = X - mp[None, :]
        out["particles"][i], out["m_pred"][i], out["S_pred"][i] = X, mp, _mirror(dx.T @ dx / t(N))
        seen = ~np.isnan(np.asarray(Y[i], dtype=np.float64))
        y = np.where(seen, np.asarray(Y[i], dtype=t), t(0))
        r = y[None, :] - (X @ CC + DD[None, :])
        l = lc[None, :] - 0.5 * r * r / (sd * sd)[None, :]                          # (N, J)
        out["lpd"][i] = np.where(seen, _logmeanexp(l, t), t(np.nan))
        L = (l * seen[None, :]).sum(axis=1) if seen.any() else np.zeros(N, dtype=t)
        W = np.exp(L - L.max())
        sw = W.sum()
        mf = (W[:, None] * X).sum(axis=0) / sw
        df = X - mf[None, :]
        out["m_filt"][i], out["S_filt"][i] = mf, _mirror((W[:, None] * df).T @ df / sw)
        out["ess"][i] = sw * sw / (W * W).sum()
        if seen.any():
            out["lpd_joint"][i] = _logmeanexp(L, t)
            a, cdf, tot = ancestors(W, unif[i])
            out["ancestors"][i], out["cdf"][i] = a, cdf / tot
            X = X[a]
        else:
            out["ancestors"][i] = np.arange(N)
    out["log_evidence"] = np.nansum(out["lpd_joint"])
    return out


def gp_cond(ctrl, Z, kern, beta, Gam, dtype=np.float64):
    """The GP conditional of one group at [X, ctrl[i]]; ctrl (>= steps, C) or None"""
    t = dtype

    def cond(i, X):
        c = np.zeros(0, dtype=t) if ctrl is None else np.asarray(ctrl[i], dtype=t)
        rows = np.concatenate((X, np.broadcast_to(c, (X.shape[0], c.shape[0]))), axis=1)
        return tg.linearize(rows, Z, kern, beta, Gam, dtype=t)[:2]
    return cond


def draws_of(x, g, r, base):
    """the slice of a draw array for track (g, r): `base` trailing dimensions; shared, per record or per (group, record)"""
    x = np.asarray(x)
    return x if x.ndim == base else x[r] if x.ndim == base + 1 else x[g, r]


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0=None, lengths=None, dtype=np.float64):
    """terms: per group (beta, Gamma) in `dtype`; gs: per group a dict with Z, okern, Q; ctrl (R, steps, C) or None; Y (R, steps, J);
    x0 (G, R, D); S0 (G, R, D, D) or None; eps / unif / xi0 in any of their three layouts.  Returns a dict of arrays (G, R, steps, ...)
    in `dtype`, NaN (ancestors -1) at and beyond a record's length; cdf is cdf / tot (ones where nothing is resampled); log_evidence
    (G, R)."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    N = np.shape(eps)[-2]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    tail = dict(m_pred=(D,), S_pred=(D, D), m_filt=(D,), S_filt=(D, D), lpd=(J,), lpd_joint=(), ess=(), particles=(N, D), cdf=(N,))
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=dtype) for k, s in tail.items()}
    out["ancestors"] = np.full((G, R, steps, N), -1, dtype=np.int64)
    out["log_evidence"] = np.zeros((G, R), dtype=dtype)
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            cond = gp_cond(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = run(cond, x0[g][r], None if S0 is None else S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], draws_of(eps, g, r, 3)[:n],
                    draws_of(unif, g, r, 1)[:n], None if xi0 is None else draws_of(xi0, g, r, 2), dtype=dtype)
            for k in list(tail) + ["ancestors"]:
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


def margin(ref, unif, wide_ref=None):
    """The condition the device tests rest on.  Returns (gap, drift, same): the smallest distance of any threshold (unif + i) / N to
    any cdf_k / tot over the resampled rows of `ref` (a dict of `tracks`), the largest |cdf / tot| difference between `ref` and
    `wide_ref`, and whether the two drew identical ancestors (drift 0 and True without `wide_ref`)."""
    cdf, anc = ref["cdf"], ref["ancestors"]
    G, R, steps, N = cdf.shape
    gap = np.inf
    for g in range(G):
        for r in range(R):
            u = draws_of(unif, g, r, 1)
            for i in range(steps):
                c = np.asarray(cdf[g, r, i], dtype=np.float64)
                if np.isnan(c[0]) or np.all(c == 1.0):            # beyond the record's length; nothing observed: no resampling
                    continue
                thr = (float(u[i]) + np.arange(N)) / N
                gap = min(gap, float(np.min(np.abs(thr[:, None] - c[None, :]))))
    if wide_ref is None:
        return gap, 0.0, True
    ok = ~np.isnan(cdf)
    drift = float(np.max(np.abs(cdf[ok] - np.asarray(wide_ref["cdf"], dtype=np.float64)[ok])))
    return gap, drift, bool(np.array_equal(anc, wide_ref["ancestors"]))
