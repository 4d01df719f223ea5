"""NumPy restatement of the adapted particle forecast fan ("Adapted particle forecasts"): test infrastructure, no
product path imports it.  In a floating-point type of the caller's choice (np.float64: the reference; np.longdouble: that reference's
own error).

The filter stage is tests/particle_adapted_ref.py's `run` over the one record.  The track of origin o starts from particles[o], the
equally weighted filtered set after row o (a copy: no ancestor is read), and for k = 1 .. h, with (mean, var) = cond(o + k, X):
  mu = X + mean,  s = var + Q
  m_fc[k - 1] = sum_i mu_i / N
  S_fc[k - 1] = sum_i (mu_i - m_fc)(mu_i - m_fc)^T / N + diag(sum_i s_i / N)                       (mirrored; no draw enters)
  lpd_fc[k - 1, j] = log mean_i N(Y[o + k, j]; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + sd_j^2), the largest exponent subtracted,
                     NaN where Y[o + k, j] is NaN
  X <- mu + eps_fc[k - 1] sqrt(s);  fc_particles[k - 1] = X
Every sum runs over the particles in index order (NumPy's own reduction); the device's order differs and is not mimicked."""
import numpy as np

import moment_ref as mr
import particle_adapted_ref as pa
import particle_filter_ref as pf
from forecast_particle_ref import fc_draws_of, group_draws_of

ARRAYS = ("m_fc", "S_fc", "lpd_fc", "fc_particles")
FILTER = ("m_pred", "S_pred", "m_filt", "S_filt", "lpd", "lpd_joint", "ess", "particles")


def step(mean, var, X, y, CC, DD, sd, Q, eps, dtype=np.float64):
    """One forecast row from the set X (N, D) with its conditional (mean, var) against the target y (J,): m, S, lpd and the next set"""
    t = dtype
    N = X.shape[0]
    mu, s = X + mean, var + Q[None, :]
    m = mu.sum(axis=0) / t(N)
    dx = mu - m[None, :]
    S = pf._mirror(dx.T @ dx / t(N) + np.diag(s.sum(axis=0) / t(N)))
    seen = ~np.isnan(np.asarray(y, dtype=np.float64))
    yy = np.where(seen, np.asarray(y, dtype=t), t(0))
    s2 = s @ (CC * CC) + (sd * sd)[None, :]
    r = yy[None, :] - (mu @ CC + DD[None, :])
    l = t(-0.5) * (pf._log2pi(t) + np.log(s2) + r * r / s2)
    lpd = np.where(seen, pf._logmeanexp(l, t), t(np.nan))
    return m, S, lpd, mu + eps * np.sqrt(s)


def track(cond, start, Y, o, h, CC, DD, sd, Q, eps_fc, dtype=np.float64):
    """One track from the set `start` (N, D) = particles[o] of the filter: cond(i, X) is the conditional at row i of the record (rows
    o + 1 .. o + h among them); eps_fc (h, N, D).  Returns the dict of ARRAYS."""
    t = dtype
    CC, DD, sd, Q = np.asarray(CC, dtype=t), np.asarray(DD, dtype=t), np.asarray(sd, dtype=t), np.asarray(Q, dtype=t)
    eps_fc = np.asarray(eps_fc, dtype=t)
    Y = np.asarray(Y)
    X = np.array(start, dtype=t)
    N, D = X.shape
    out = dict(m_fc=np.zeros((h, D), dtype=t), S_fc=np.zeros((h, D, D), dtype=t), lpd_fc=np.zeros((h, Y.shape[1]), dtype=t),
               fc_particles=np.zeros((h, N, D), dtype=t))
    for k in range(h):
        mean, var = cond(o + 1 + k, X)
        out["m_fc"][k], out["S_fc"][k], out["lpd_fc"][k], X = step(mean, var, X, Y[o + 1 + k], CC, DD, sd, Q, eps_fc[k], dtype=t)
        out["fc_particles"][k] = X
    return out


def run(cond, x0, S0, Y, origins, h, CC, DD, sd, Q, eps, unif, eps_fc_of, xi0=None, dtype=np.float64):
    """The filter over the record and every track of one group.  eps_fc_of(b): the forecast draws (h, N, D) of origin b.  Returns the
    ARRAYS as (B, h, ...) and `filter`, the dict of particle_adapted_ref.run."""
    f = pa.run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0, dtype=dtype)
    per = [track(cond, f["particles"][int(o)], Y, int(o), h, CC, DD, sd, Q, eps_fc_of(b), dtype=dtype) for b, o in enumerate(origins)]
    out = {k: np.stack([p[k] for p in per]) for k in ARRAYS}
    out["filter"] = f
    return out


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, origins, h, eps, unif, eps_fc, xi0=None, dtype=np.float64):
    """terms: per group (beta, Gamma) in `dtype`; gs: per group a dict with Z, okern, Q; ctrl (steps, C) or None; Y (steps, J); x0
    (G, D); S0 (G, D, D) or None; eps / unif / xi0 shared or per group, eps_fc in any of its three layouts.  Returns the ARRAYS as
    (G, B, h, ...) and the filter's arrays (FILTER, ancestors, cdf, log_evidence) as (G, 1, steps, ...): the layout of
    particle_adapted_ref.tracks with one record, which `margin` takes."""
    per = []
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        cond = pf.gp_cond(ctrl, grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
        per.append(run(cond, x0[g], None if S0 is None else S0[g], Y, origins, h, CC, DD, sd, grp["Q"], group_draws_of(eps, g, 3),
                       group_draws_of(unif, g, 1), lambda b, g=g: fc_draws_of(eps_fc, g, b),
                       None if xi0 is None else group_draws_of(xi0, g, 2), dtype=dtype))
    out = {k: np.stack([p[k] for p in per]) for k in ARRAYS}
    flt = {k: np.stack([np.asarray(p["filter"][k])[None] for p in per]) for k in FILTER + ("ancestors", "cdf", "log_evidence")}
    return out, flt


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, origins, h, wide, eps, unif, eps_fc, xi0=None):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`, the filter's arrays under ref["filter"]), its
    largest error per array against the same composition in np.longdouble (`e_ref`, the filter's keys among them; zeros when `wide` is
    false), and the longdouble filter arrays (None when `wide` is false)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, origins, h, eps, unif, eps_fc, xi0, dtype=t)
    (ref, flt), e_ref = res[np.float64], {}
    for k in ARRAYS + FILTER:
        a = ref[k] if k in ARRAYS else flt[k]
        ok = ~np.isnan(a)
        if wide and ok.any():
            w = res[np.longdouble][0][k] if k in ARRAYS else res[np.longdouble][1][k]
            e_ref[k] = float(np.max(np.abs(a[ok] - w[ok])))
        else:
            e_ref[k] = 0.0
    return dict(ref, filter=flt), e_ref, res[np.longdouble][1] if wide else None
