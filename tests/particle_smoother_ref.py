"""NumPy restatement of the marginal particle smoother on the carried sets ("Particle smoothing"): test
infrastructure, no product path imports it.  In a floating-point type of the caller's choice (np.float64: the reference;
np.longdouble: that reference's own error), on top of particle_filter_ref.run with a recording `cond`.

Per track of n rows, with X_t the set the filter carries into row t, mu_t = X_t + m(X_t) (`trans_mean`), s_t = v(X_t) + Q
(`trans_var`), X^-_t = mu_t + eps[t] sqrt(s_t) (`particles`), W_t (`weights`) and a_t (`ancestors`):
  w_smooth[n-1] = W_{n-1} / sum W_{n-1};  for t = n-2 .. 0, with x_j = X^-_{t+1,j}, mu_i = mu_{t+1,i}, s_i = s_{t+1,i}:
  log f_ij = -1/2 sum_d ((x_jd - mu_id)^2 / s_id + log s_id)
  c_j = max_i log f_ij + log sum_i exp(log f_ij - max);  omega_i = sum_j w_smooth[t+1, j] exp(log f_ij - c_j)
  w_smooth[t, k] = sum_{i: a_t[i] = k} omega_i  (ascending i; exactly 0 without offspring; nothing is renormalised)
  m_smooth = sum_k w_k X^-_tk / sum_k w_k,  S_smooth the w-weighted centred covariance (mirrored),  ess_smooth = (sum w)^2 / sum w^2.

`weights_of` forms W_t from the stored X^- and Y by the filter's expressions; `recursion` is the smoother on given stacks (the device's
own, or the reference's); `genealogy` is the estimate a user can build from `particles` and `ancestors` alone, as the same fold of
the last row's weights without the transition densities; `run` is filter + smoother for any cond(i, X) -> (mean, var); `tracks`
and `reference` are shaped like particle_filter_ref's."""
import numpy as np

import moment_ref as mr
import particle_filter_ref as pf

SMOOTHED = ("m_smooth", "S_smooth", "ess_smooth", "w_smooth")
KEPT = ("weights", "trans_mean", "trans_var")
BLOCK = 256


def recording(cond, Q, dtype=np.float64):
    """cond with the transition mean X + m and the transition variance v + Q of every call kept in the returned dict of lists"""
    Q = np.asarray(Q, dtype=dtype)
    rec = dict(trans_mean=[], trans_var=[])

    def wrapped(i, X):
        mean, var = cond(i, X)
        rec["trans_mean"].append(X + mean)
        rec["trans_var"].append(var + Q[None, :])
        return mean, var
    return wrapped, rec


def weights_of(particles, Y, CC, DD, sd, dtype=np.float64):
    """W (n, N) of the filter from the stored X^- (n, N, D) and Y (n, J): exp(L_i - max L), L_i the sum of l_ij over the observed j in
    ascending j; ones for a row with nothing observed."""
    t = dtype
    X, CC, DD, sd = (np.asarray(a, dtype=t) for a in (particles, CC, DD, sd))
    Y = np.asarray(Y)
    n, N = X.shape[:2]
    W = np.ones((n, N), dtype=t)
    lc = -0.5 * (pf._log2pi(t) + np.log(sd * sd))
    for i in range(n):
        seen = ~np.isnan(np.asarray(Y[i], dtype=np.float64))
        if not seen.any():
            continue
        L = np.zeros(N, dtype=t)
        for j in np.flatnonzero(seen):
            e = (t(Y[i, j]) - X[i] @ CC[:, j]) - DD[j]
            L = L + (lc[j] - 0.5 * e * e / (sd[j] * sd[j]))
        W[i] = np.exp(L - L.max())
    return W


def fold(omega, a):
    """sum of omega_i over the i with a_i = k, in ascending i; exactly 0 without offspring"""
    w = np.zeros_like(omega)
    np.add.at(w, np.asarray(a, dtype=np.int64), omega)
    return w


def moments(X, w):
    sw = w.sum()
    m = (w[:, None] * X).sum(axis=0) / sw
    dx = X - m[None, :]
    return m, pf._mirror((w[:, None] * dx).T @ dx / sw), sw * sw / (w * w).sum()


def _finish(X, w):
    n, N, D = X.shape
    out = dict(w_smooth=w, m_smooth=np.zeros((n, D), dtype=X.dtype), S_smooth=np.zeros((n, D, D), dtype=X.dtype),
               ess_smooth=np.zeros(n, dtype=X.dtype))
    for r in range(n):
        out["m_smooth"][r], out["S_smooth"][r], out["ess_smooth"][r] = moments(X[r], w[r])
    return out


def recursion(particles, ancestors, trans_mean, trans_var, weights, dtype=np.float64):
    """The smoother on the stacks of one track: particles, trans_mean, trans_var (n, N, D), ancestors, weights (n, N).  Returns a dict of
    SMOOTHED in `dtype`."""
    t = dtype
    X, tm, tv, W = (np.asarray(a, dtype=t) for a in (particles, trans_mean, trans_var, weights))
    n, N, D = X.shape
    w = np.zeros((n, N), dtype=t)
    w[n - 1] = W[n - 1] / W[n - 1].sum()
    for r in range(n - 2, -1, -1):
        x, mu, s = X[r + 1], tm[r + 1], tv[r + 1]
        ls, omega = np.log(s).sum(axis=1), np.zeros(N, dtype=t)
        for j0 in range(0, N, BLOCK):                             # columns j in blocks (the tables of a block stay in cache)
            xb = x[j0:j0 + BLOCK]
            q = np.zeros((N, xb.shape[0]), dtype=t)               # [i, j]
            for d in range(D):
                u = xb[None, :, d] - mu[:, None, d]
                q += u * u / s[:, None, d]
            lf = -0.5 * (q + ls[:, None])
            mx = lf.max(axis=0)
            c = mx + np.log(np.exp(lf - mx[None, :]).sum(axis=0))
            omega += (np.exp(lf - c[None, :]) * w[r + 1][None, j0:j0 + BLOCK]).sum(axis=1)
        w[r] = fold(omega, ancestors[r])
    return _finish(X, w)


def genealogy(particles, ancestors, weights, dtype=np.float64):
    """The estimate from `particles` and `ancestors` alone: X^-_tk weighted by the last row's weight of its surviving descendants (the
    fold of `recursion` with omega = w_smooth[t+1]).  Returns a dict of SMOOTHED."""
    t = dtype
    X, W = np.asarray(particles, dtype=t), np.asarray(weights, dtype=t)
    n, N = W.shape
    w = np.zeros((n, N), dtype=t)
    w[n - 1] = W[n - 1] / W[n - 1].sum()
    for r in range(n - 2, -1, -1):
        w[r] = fold(w[r + 1], ancestors[r])
    return _finish(X, w)


def run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0=None, dtype=np.float64):
    """particle_filter_ref.run with a recording cond, then the smoother.  Returns the filter's dict plus KEPT and SMOOTHED."""
    wrapped, rec = recording(cond, Q, dtype)
    f = pf.run(wrapped, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0, dtype=dtype)
    f["trans_mean"], f["trans_var"] = np.stack(rec["trans_mean"]), np.stack(rec["trans_var"])
    f["weights"] = weights_of(f["particles"], Y, CC, DD, sd, dtype)
    f.update(recursion(f["particles"], f["ancestors"], f["trans_mean"], f["trans_var"], f["weights"], dtype))
    return f


TAILS = dict(m_smooth=lambda N, D: (D,), S_smooth=lambda N, D: (D, D), ess_smooth=lambda N, D: (), w_smooth=lambda N, D: (N,),
             weights=lambda N, D: (N,), trans_mean=lambda N, D: (N, D), trans_var=lambda N, D: (N, D))


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0=None, lengths=None, dtype=np.float64):
    """particle_filter_ref.tracks with the smoother: a dict of arrays (G, R, steps, ...) of KEPT, SMOOTHED, particles and ancestors in
    `dtype`, NaN (ancestors -1) at and beyond a record's length."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    N = np.shape(eps)[-2]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    out = {k: np.full((G, R, steps) + s(N, D), np.nan, dtype=dtype) for k, s in TAILS.items()}
    out["particles"] = np.full((G, R, steps, N, D), np.nan, dtype=dtype)
    out["ancestors"] = np.full((G, R, steps, N), -1, dtype=np.int64)
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            cond = pf.gp_cond(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = run(cond, x0[g][r], None if S0 is None else S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], pf.draws_of(eps, g, r, 3)[:n],
                    pf.draws_of(unif, g, r, 1)[:n], None if xi0 is None else pf.draws_of(xi0, g, r, 2), dtype=dtype)
            for k in out:
                out[k][g, r, :n] = f[k]
    return out


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide, eps, unif, xi0=None):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`) and its largest error per array against the same
    composition in np.longdouble (`e_ref`; zeros when `wide` is false; ess_smooth as ess_smooth / N)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0, lengths, dtype=t)
    ref = res[np.float64]
    return ref, errors(ref, res[np.longdouble]) if wide else {k: 0.0 for k in TAILS}


def errors(ref, wide):
    """largest |ref - wide| per array of TAILS over the rows ref has (ess_smooth divided by N)"""
    N = ref["w_smooth"].shape[-1]
    e = {}
    for k in TAILS:
        ok = ~np.isnan(ref[k])
        e[k] = float(np.max(np.abs(ref[k][ok] - wide[k][ok]))) / (N if k == "ess_smooth" else 1) if ok.any() else 0.0
    return e


def on_stacks(out, lengths, dtype=np.float64):
    """`recursion` on the stacks of a device call `out` (particles, ancestors, trans_mean, trans_var, weights: (G, R, steps, ...)),
    track by track over the record's rows: a dict of SMOOTHED (G, R, steps, ...) in `dtype`, NaN at and beyond a record's length."""
    G, R, steps, N, D = out["particles"].shape
    res = {k: np.full((G, R, steps) + TAILS[k](N, D), np.nan, dtype=dtype) for k in SMOOTHED}
    for g in range(G):
        for r in range(R):
            n = int(lengths[r])
            f = recursion(*(out[k][g, r, :n] for k in ("particles", "ancestors", "trans_mean", "trans_var", "weights")), dtype=dtype)
            for k in SMOOTHED:
                res[k][g, r, :n] = f[k]
    return res
