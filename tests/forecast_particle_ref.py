"""NumPy restatement of the particle forecast fan ("Particle forecasts"): test infrastructure, no product path
imports it.  The reference is DEFINED by particle_filter_ref.run: the track of origin o is `run` over rows 0 .. o of the record
followed by h all-NaN rows, with the filter's draws of rows 0 .. o and the forecast draws concatenated (the uniforms of the NaN rows
are never read: zeros).  m_fc, S_fc and fc_particles are its m_pred, S_pred and particles at rows o + 1 .. o + h; lpd_fc is taken
from those particles against the true targets Y[o + 1 .. o + h]:
  lpd_fc[k - 1, j] = max_i l_ij + log(sum_i exp(l_ij - max) / N),  l_ij = log N(Y[o + k, j]; CC[:, j] . X_i + DD_j, sd_j^2),
NaN where the target is NaN.  In a floating-point type of the caller's choice (np.float64: the reference; np.longdouble: that
reference's own error)."""
import numpy as np

import particle_filter_ref as pf
import moment_ref as mr

ARRAYS = ("m_fc", "S_fc", "lpd_fc", "fc_particles")


def lpd_of(X, y, CC, DD, sd, dtype=np.float64):
    """log mean_i N(y_j; CC[:, j] . X_i + DD_j, sd_j^2) per output j; X (N, D), y (J,), NaN = unobserved -> NaN"""
    t = dtype
    CC, DD, sd = np.asarray(CC, dtype=t), np.asarray(DD, dtype=t), np.asarray(sd, dtype=t)
    seen = ~np.isnan(np.asarray(y, dtype=np.float64))
    yy = np.where(seen, np.asarray(y, dtype=t), t(0))
    lc = -0.5 * (np.log(t(2) * t(np.pi)) + np.log(sd * sd))
    r = yy[None, :] - (np.asarray(X, dtype=t) @ CC + DD[None, :])
    l = lc[None, :] - 0.5 * r * r / (sd * sd)[None, :]
    mx = l.max(axis=0)
    return np.where(seen, mx + np.log(np.exp(l - mx).sum(axis=0) / t(l.shape[0])), t(np.nan))


def track(cond, x0, S0, Y, o, h, CC, DD, sd, Q, eps, unif, eps_fc, xi0=None, dtype=np.float64):
    """One track: cond(i, X) is the conditional at row i of the record (rows o + 1 .. o + h among them); eps (steps, N, D), unif
    (steps,), eps_fc (h, N, D).  Returns the dict of ARRAYS and `filter`, the whole dict of `run` over the o + 1 + h rows."""
    Y = np.asarray(Y)
    J = Y.shape[1]
    Yc = np.concatenate((Y[:o + 1], np.full((h, J), np.nan)))
    ec = np.concatenate((np.asarray(eps)[:o + 1], np.asarray(eps_fc)))
    uc = np.concatenate((np.asarray(unif)[:o + 1], np.zeros(h)))
    f = pf.run(cond, x0, S0, Yc, CC, DD, sd, Q, ec, uc, xi0, dtype=dtype)
    P = f["particles"][o + 1:]
    lpd = np.stack([lpd_of(P[k], Y[o + 1 + k], CC, DD, sd, dtype) for k in range(h)])
    return dict(m_fc=f["m_pred"][o + 1:], S_fc=f["S_pred"][o + 1:], lpd_fc=lpd, fc_particles=P, filter=f)


def fc_draws_of(x, g, b):
    """the slice of eps_fc for track (g, b): (h, N, D), (B, h, N, D) or (G, B, h, N, D)"""
    x = np.asarray(x)
    return x if x.ndim == 3 else x[b] if x.ndim == 4 else x[g, b]


def group_draws_of(x, g, base):
    x = np.asarray(x)
    return x if x.ndim == base else x[g]


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, origins, h, eps, unif, eps_fc, xi0=None, dtype=np.float64):
    """terms: per group (beta, Gamma) in `dtype`; gs: per group a dict with Z, okern, Q; ctrl (steps, C) or None; Y (steps, J); x0
    (G, D); S0 (G, D, D) or None; eps / unif / xi0 shared or per group, eps_fc in any of its three layouts.  Returns the ARRAYS as
    (G, B, h, ...) in `dtype`."""
    Y = np.asarray(Y)
    G, B, J, D, N = len(gs), len(origins), Y.shape[1], np.shape(x0)[-1], np.shape(eps)[-2]
    tail = dict(m_fc=(D,), S_fc=(D, D), lpd_fc=(J,), fc_particles=(N, D))
    out = {k: np.zeros((G, B, h) + s, dtype=dtype) for k, s in tail.items()}
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        cond = pf.gp_cond(ctrl, grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
        for b, o in enumerate(origins):
            f = track(cond, x0[g], None if S0 is None else S0[g], Y, int(o), h, CC, DD, sd, grp["Q"], group_draws_of(eps, g, 3),
                      group_draws_of(unif, g, 1), fc_draws_of(eps_fc, g, b), None if xi0 is None else group_draws_of(xi0, g, 2), dtype=dtype)
            for k in tail:
                out[k][g, b] = f[k]
    return out


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, origins, h, wide, eps, unif, eps_fc, xi0=None):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`) and its largest error per array against the
    same composition in np.longdouble (`e_ref`; zeros when `wide` is false)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, origins, h, eps, unif, eps_fc, xi0, dtype=t)
    ref, e_ref = res[np.float64], {}
    for k in ARRAYS:
        ok = ~np.isnan(ref[k])
        e_ref[k] = float(np.max(np.abs(ref[k][ok] - res[np.longdouble][k][ok]))) if wide and ok.any() else 0.0
    return ref, e_ref
