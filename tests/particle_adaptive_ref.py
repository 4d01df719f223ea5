"""NumPy restatement of the particle filter with adaptive (ESS-triggered) resampling over many records (DESIGN.md section 9,
"Adaptive resampling"): test infrastructure, no product path imports it.  In a floating-point type of the caller's choice (np.float64:
the reference; np.longdouble: that reference's own error).

The bootstrap filter of tests/particle_filter_ref.py carrying a WEIGHTED set: per track the particles X and the log-weights a, whose
largest entry is exactly 0 (a = 0 at the start).  The draws and their indexing are that filter's; unif[t] is not read on a row that
does not resample.  Row t, with e = exp(a) and A = sum e:
  propagate  X^- = X + m + eps[t] sqrt(v + Q)
  moments    m_pred = sum_i e_i X^-_i / A,  S_pred = sum_i e_i (X^-_i - m_pred)(X^-_i - m_pred)^T / A  (centred, mirrored)
  densities  l_ij as the bootstrap filter;  lpd[t, j] = max_i (a_i + l_ij) + log(sum_i exp(a_i + l_ij - max) / A), NaN where y_tj is
             NaN;  b_i = a_i + sum over the observed j of l_ij;  lpd_joint[t] = max b + log(sum_i exp(b_i - max b) / A)
  filtered   W_i = exp(b_i - max b);  m_filt, S_filt the W-weighted mean and centred covariance;  ess = (sum W)^2 / sum W^2;
             weights[t] = W / sum W
  decide     (a row with an observed entry)  ess < ess_threshold N: particle_filter_ref.ancestors(W, unif[t]), X <- X^-[anc], a <- 0,
             resampled[t] = 1;  otherwise anc_i = i, X <- X^-, a <- b - max b (the difference itself), resampled[t] = 0
  a row with nothing observed: the propagation alone; m_filt = m_pred, S_filt = S_pred, lpd and lpd_joint NaN, ess = A^2 / sum e^2,
             weights[t] = e / A, anc_i = i, a kept, resampled[t] = 0
log_evidence is the sum of lpd_joint over the rows that have an observation: the unbiased SMC estimate whether or not a row resamples.
With a = 0 every expression is the bootstrap filter's (e = 1, A = N exactly): with ess_threshold > 1, `run` equals
particle_filter_ref.run in every key the two share, with np.array_equal.

`run`, `tracks`, `reference` and `margin` are shaped like particle_filter_ref's; `margin` adds the condition the decision rests on:
how far ess / N is from the threshold on every observed row."""
import numpy as np

import cubature_filter_ref as cf
import moment_ref as mr
import particle_filter_ref as pf
from particle_filter_ref import MOMENTS, DENSITIES, draws_of, gp_cond   # noqa: F401  (shared with the tests)

EXTRA = ("ess", "particles", "weights")


def run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0=None, ess_threshold=0.5, dtype=np.float64):
    """One track.  The arguments of particle_filter_ref.run plus ess_threshold.  Returns its dict plus weights (steps, N), resampled
    (steps,) int, logw (steps, N: a after the row) and ess_frac (steps,: ess / N); cdf is ones on the rows that do not resample."""
    t = dtype
    eps, unif = np.asarray(eps, dtype=t), np.asarray(unif, dtype=t)
    CC, DD, sd, Q = np.asarray(CC, dtype=t), np.asarray(DD, dtype=t), np.asarray(sd, dtype=t), np.asarray(Q, dtype=t)
    Y = np.asarray(Y)
    (n, J), (N, D) = Y.shape, eps.shape[1:]
    X = np.broadcast_to(np.asarray(x0, dtype=t), (N, D)).copy()
    if S0 is not None:
        X = X + np.asarray(xi0, dtype=t) @ cf.factor(S0, dtype=t).T
    a = np.zeros(N, dtype=t)
    out = dict(m_pred=np.zeros((n, D), dtype=t), S_pred=np.zeros((n, D, D), dtype=t), m_filt=np.zeros((n, D), dtype=t),
               S_filt=np.zeros((n, D, D), dtype=t), lpd=np.full((n, J), np.nan, dtype=t), lpd_joint=np.full(n, np.nan, dtype=t),
               ess=np.zeros(n, dtype=t), particles=np.zeros((n, N, D), dtype=t), ancestors=np.zeros((n, N), dtype=np.int64),
               cdf=np.ones((n, N), dtype=t), weights=np.zeros((n, N), dtype=t), resampled=np.zeros(n, dtype=np.int64),
               logw=np.zeros((n, N), dtype=t))
    lc = -0.5 * (pf._log2pi(t) + np.log(sd * sd))
    for i in range(n):
        mean, var = cond(i, X)
        X = X + mean + eps[i] * np.sqrt(var + Q[None, :])
        e = np.exp(a)
        A = e.sum()
        mp = (e[:, None] * X).sum(axis=0) / A
        dx = X - mp[None, :]
        out["particles"][i], out["m_pred"][i], out["S_pred"][i] = X, mp, pf._mirror((e[:, None] * dx).T @ dx / A)
        seen = ~np.isnan(np.asarray(Y[i], dtype=np.float64))
        out["ancestors"][i] = np.arange(N)
        if not seen.any():
            out["m_filt"][i], out["S_filt"][i] = out["m_pred"][i], out["S_pred"][i]
            out["ess"][i] = A * A / (e * e).sum()
            out["weights"][i], out["logw"][i] = e / A, a
            continue
        y = np.where(seen, np.asarray(Y[i], dtype=t), t(0))
        r = y[None, :] - (X @ CC + DD[None, :])
        l = lc[None, :] - 0.5 * r * r / (sd * sd)[None, :]                          # (N, J)
        al = a[:, None] + l
        mx = al.max(axis=0)
        out["lpd"][i] = np.where(seen, mx + np.log(np.exp(al - mx).sum(axis=0) / A), t(np.nan))
        b = a + (l * seen[None, :]).sum(axis=1)
        na = b - b.max()
        W = np.exp(na)
        sw = W.sum()
        out["lpd_joint"][i] = b.max() + np.log(sw / A)
        mf = (W[:, None] * X).sum(axis=0) / sw
        df = X - mf[None, :]
        out["m_filt"][i], out["S_filt"][i] = mf, pf._mirror((W[:, None] * df).T @ df / sw)
        out["ess"][i] = sw * sw / (W * W).sum()
        out["weights"][i] = W / sw
        if out["ess"][i] < t(ess_threshold) * t(N):
            anc, cdf, tot = pf.ancestors(W, unif[i])
            out["ancestors"][i], out["cdf"][i], out["resampled"][i] = anc, cdf / tot, 1
            X, a = X[anc], np.zeros(N, dtype=t)
        else:
            a = na
        out["logw"][i] = a
    out["log_evidence"] = np.nansum(out["lpd_joint"])
    out["ess_frac"] = out["ess"] / t(N)
    return out


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0=None, lengths=None, ess_threshold=0.5, dtype=np.float64):
    """particle_filter_ref.tracks with `run` above: arrays (G, R, steps, ...) in `dtype`, NaN (ancestors, resampled -1) at and beyond a
    record's length; log_evidence (G, R)."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    N = np.shape(eps)[-2]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    tail = dict(m_pred=(D,), S_pred=(D, D), m_filt=(D,), S_filt=(D, D), lpd=(J,), lpd_joint=(), ess=(), ess_frac=(), particles=(N, D),
                cdf=(N,), weights=(N,), logw=(N,))
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=dtype) for k, s in tail.items()}
    out["ancestors"] = np.full((G, R, steps, N), -1, dtype=np.int64)
    out["resampled"] = np.full((G, R, steps), -1, dtype=np.int64)
    out["log_evidence"] = np.zeros((G, R), dtype=dtype)
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            cond = gp_cond(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = run(cond, x0[g][r], None if S0 is None else S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], draws_of(eps, g, r, 3)[:n],
                    draws_of(unif, g, r, 1)[:n], None if xi0 is None else draws_of(xi0, g, r, 2), ess_threshold, dtype=dtype)
            for k in list(tail) + ["ancestors", "resampled"]:
                out[k][g, r, :n] = f[k]
            out["log_evidence"][g, r] = f["log_evidence"]
    return out


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide, eps, unif, xi0=None, ess_threshold=0.5):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`), its largest error per array against the same
    composition in np.longdouble (`e_ref`; zeros when `wide` is false), and the longdouble composition itself (`wide_ref`, None when
    `wide` is false).  e_ref means what it says only where the two precisions decide and draw alike (`margin`)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0, lengths, ess_threshold, dtype=t)
    ref = res[np.float64]
    e_ref = {}
    for k in MOMENTS + DENSITIES + EXTRA:
        ok = ~np.isnan(ref[k])
        e_ref[k] = float(np.max(np.abs(ref[k][ok] - res[np.longdouble][k][ok]))) if wide and ok.any() else 0.0
    return ref, e_ref, res.get(np.longdouble) if wide else None


def margin(ref, unif, ess_threshold, wide_ref=None):
    """The conditions the device tests rest on.  Returns a dict: gap, drift, same (particle_filter_ref.margin over the rows that
    resample: the smallest threshold-to-cdf distance, the cdf drift, identical ancestors), same_decisions (fp64 and longdouble resample
    the same rows), ess_gap (the smallest |ess / N - ess_threshold| over the observed rows) and ess_drift (the largest difference of
    ess / N between the two precisions there)."""
    gap, drift, same = pf.margin(ref, unif, wide_ref)
    seen = ~np.isnan(ref["lpd_joint"])
    frac = np.asarray(ref["ess_frac"], dtype=np.float64)
    ess_gap = float(np.min(np.abs(frac[seen] - ess_threshold))) if seen.any() else np.inf
    out = dict(gap=gap, drift=drift, same=same, same_decisions=True, ess_gap=ess_gap, ess_drift=0.0)
    if wide_ref is not None:
        out["same_decisions"] = bool(np.array_equal(ref["resampled"], wide_ref["resampled"]))
        if seen.any():
            out["ess_drift"] = float(np.max(np.abs(frac[seen] - np.asarray(wide_ref["ess_frac"], dtype=np.float64)[seen])))
    return out
