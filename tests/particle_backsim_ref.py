"""NumPy restatement of the particle backward simulation on the carried sets ("Particle backward simulation"):
test infrastructure, no product path imports it.  In a floating-point type of the caller's choice (np.float64: the reference;
np.longdouble: that reference's own error), on the stacks particle_smoother_ref.run keeps.

Per track of n rows, with mu_t = `trans_mean`[t], s_t = `trans_var`[t], X^-_t = `particles`[t], W_t = `weights`[t], a_t = `ancestors`[t]
and the caller's uniforms u = unif_bs[t, b] in [0, 1), trajectory b is a sequence of indices k_t into X^-_t:
  row n-1:       cdf = np.cumsum(W_{n-1}) (sequential), tot = cdf[-1];  k_{n-1} = min(searchsorted(cdf, u tot, side="right"), N - 1)
  t = n-2 .. 0:  with x = X^-_{t+1, k_{t+1}}:  log f_i = -1/2 sum_d ((x_d - mu_{t+1,id})^2 / s_{t+1,id} + log s_{t+1,id}),
                 p_i = exp(log f_i - max_i log f_i),  cdf = np.cumsum(p),  tot = cdf[-1] >= 1,
                 i* = min(searchsorted(cdf, u tot, side="right"), N - 1),  k_t = a_t[i*]
  traj_index[t, b] = k_t;  trajectories[b, t] = X^-_{t, k_t};  m_traj[t] the mean over b;  S_traj[t] the centred covariance with divisor
  B (mirrored);  lag_cov[t] = (1 / B) sum_b (x_t^b - m_traj[t]) (x_{t+1}^b - m_traj[t+1])^T, NaN at t = n - 1.
Conditional on the filter's run P(k_t = k) = w_smooth[t, k] of particle_smoother_ref.recursion (by induction: P(i* = i) is omega_i and
k_t is its fold through a_t).

`backsim` is the method on the stacks of one track; `moments` the three moments of given trajectories; `run` is filter + kept terms +
backward simulation for any cond(i, X) -> (mean, var); `tracks`, `reference` and `on_stacks` are shaped like particle_smoother_ref's.
`margin` extends particle_filter_ref.margin to the backward thresholds: how far every u tot is from every cdf entry, and how far the
cdf moves between the two precisions."""
import numpy as np

import moment_ref as mr
import particle_filter_ref as pf
import particle_smoother_ref as ps

STACKS = ("particles", "ancestors", "trans_mean", "trans_var", "weights")
DRAWN = ("traj_index", "trajectories")
MOMENTS = ("m_traj", "S_traj", "lag_cov")


def _pick(cdf, thr, N):
    """min(#{k: cdf_k <= thr_b}, N - 1) per trajectory; cdf (N,) shared or (B, N)"""
    if cdf.ndim == 1:
        return np.minimum(np.searchsorted(cdf, thr, side="right"), N - 1)
    return np.minimum(np.array([np.searchsorted(cdf[b], thr[b], side="right") for b in range(thr.shape[0])], dtype=np.int64), N - 1)


def moments(traj, dtype=np.float64):
    """traj (B, n, D) -> m_traj (n, D), S_traj (n, D, D) mirrored, lag_cov (n, D, D) with NaN in its last row, in `dtype`"""
    t = dtype
    X = np.asarray(traj, dtype=t)
    B, n, D = X.shape
    m = X.sum(axis=0) / t(B)
    dx = X - m[None]
    S = np.stack([pf._mirror(dx[:, r].T @ dx[:, r] / t(B)) for r in range(n)])
    lag = np.full((n, D, D), np.nan, dtype=t)
    for r in range(n - 1):
        lag[r] = dx[:, r].T @ dx[:, r + 1] / t(B)
    return m, S, lag


def backsim(stacks, unif_bs, dtype=np.float64, keep_cdf=True):
    """stacks: the five arrays of STACKS of one track, (n, N, D) and (n, N); unif_bs (n, B).  Returns a dict: traj_index (n, B) int64,
    trajectories (B, n, D), MOMENTS, `gap` -- the smallest |u tot - cdf_k| / tot over all rows and trajectories -- and with keep_cdf
    `cdf` (n, B, N) = cdf / tot as float64."""
    t = dtype
    X, anc, tm, tv, W = stacks
    X, tm, tv, W = (np.asarray(a, dtype=t) for a in (X, tm, tv, W))
    anc, U = np.asarray(anc, dtype=np.int64), np.asarray(unif_bs, dtype=t)
    n, N, D = X.shape
    B = U.shape[1]
    assert U.shape[0] == n
    idx = np.zeros((n, B), dtype=np.int64)
    cdfs = np.zeros((n, B, N)) if keep_cdf else None
    gap = np.inf
    for r in range(n - 1, -1, -1):
        if r == n - 1:
            cdf = np.cumsum(W[r])                                 # sequential, index order
            tot = cdf[-1]
            thr = U[r] * tot
            k = _pick(cdf, thr, N)
            gap = min(gap, float(np.min(np.abs(thr[:, None] - cdf[None, :])) / tot))
            if keep_cdf:
                cdfs[r] = np.asarray(cdf / tot, dtype=np.float64)[None, :]
        else:
            x, mu, s = X[r + 1][idx[r + 1]], tm[r + 1], tv[r + 1]   # (B, D), (N, D), (N, D)
            q = np.zeros((B, N), dtype=t)
            for d in range(D):
                u = x[:, None, d] - mu[None, :, d]
                q += u * u / s[None, :, d]
            lf = -0.5 * (q + np.log(s).sum(axis=1)[None, :])
            p = np.exp(lf - lf.max(axis=1)[:, None])
            cdf = np.cumsum(p, axis=1)                            # sequential along the particles
            tot = cdf[:, -1]
            thr = U[r] * tot
            k = anc[r][_pick(cdf, thr, N)]
            gap = min(gap, float(np.min(np.abs(thr[:, None] - cdf) / tot[:, None])))
            if keep_cdf:
                cdfs[r] = np.asarray(cdf / tot[:, None], dtype=np.float64)
        idx[r] = k
    traj = np.stack([X[r][idx[r]] for r in range(n)], axis=1)     # (B, n, D)
    m, S, lag = moments(traj, t)
    out = dict(traj_index=idx, trajectories=traj, m_traj=m, S_traj=S, lag_cov=lag, gap=gap)
    if keep_cdf:
        out["cdf"] = cdfs
    return out


def run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, unif_bs, xi0=None, dtype=np.float64, keep_cdf=True, smoother=True):
    """particle_filter_ref.run with a recording cond and the weights (the stacks the device keeps), with `smoother` the marginal
    smoother of particle_smoother_ref (N^2 per row) too, then `backsim` on the stacks.  Returns the filter's dict plus the kept terms,
    DRAWN, MOMENTS, gap_bs and (keep_cdf) cdf_bs."""
    wrapped, rec = ps.recording(cond, Q, dtype)
    f = pf.run(wrapped, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0, dtype=dtype)
    f["trans_mean"], f["trans_var"] = np.stack(rec["trans_mean"]), np.stack(rec["trans_var"])
    f["weights"] = ps.weights_of(f["particles"], Y, CC, DD, sd, dtype)
    if smoother:
        f.update(ps.recursion(f["particles"], f["ancestors"], f["trans_mean"], f["trans_var"], f["weights"], dtype))
    b = backsim([f[k] for k in STACKS], unif_bs, dtype, keep_cdf)
    for k in DRAWN + MOMENTS:
        f[k] = b[k]
    f["gap_bs"] = b["gap"]
    if keep_cdf:
        f["cdf_bs"] = b["cdf"]
    return f


def tails(N, D, B):
    return dict(m_traj=(D,), S_traj=(D, D), lag_cov=(D, D), weights=(N,), trans_mean=(N, D), trans_var=(N, D), particles=(N, D), cdf=(N,),
                cdf_bs=(B, N))


def _empty(G, R, steps, N, D, B, dtype):
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=np.float64 if k.startswith("cdf") else dtype) for k, s in tails(N, D, B).items()}
    out["ancestors"] = np.full((G, R, steps, N), -1, dtype=np.int64)
    out["traj_index"] = np.full((G, R, steps, B), -1, dtype=np.int64)
    out["trajectories"] = np.full((G, R, B, steps, D), np.nan, dtype=dtype)
    out["gap_bs"] = np.inf
    return out


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, unif_bs, xi0=None, lengths=None, dtype=np.float64):
    """particle_smoother_ref.tracks with the backward simulation: a dict of arrays (G, R, steps, ...) in `dtype` (trajectories
    (G, R, B, steps, D)), NaN (indices -1) at and beyond a record's length; cdf is the filter's cdf / tot, cdf_bs the backward one;
    gap_bs the smallest backward gap of the call.  unif_bs in any of its three layouts."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    N, B = np.shape(eps)[-2], np.shape(unif_bs)[-1]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    out = _empty(G, R, steps, N, D, B, dtype)
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            cond = pf.gp_cond(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = run(cond, x0[g][r], None if S0 is None else S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], pf.draws_of(eps, g, r, 3)[:n],
                    pf.draws_of(unif, g, r, 1)[:n], pf.draws_of(unif_bs, g, r, 2)[:n], None if xi0 is None else pf.draws_of(xi0, g, r, 2),
                    dtype=dtype, smoother=False)
            for k in out:
                if k == "trajectories":
                    out[k][g, r, :, :n] = f[k]
                elif k == "gap_bs":
                    out[k] = min(out[k], f[k])
                else:
                    out[k][g, r, :n] = f[k]
    return out


def errors(ref, wide):
    """largest |ref - wide| per array of MOMENTS over the entries ref has"""
    e = {}
    for k in MOMENTS:
        ok = ~np.isnan(ref[k])
        e[k] = float(np.max(np.abs(ref[k][ok] - wide[k][ok]))) if ok.any() else 0.0
    return e


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide, eps, unif, unif_bs, xi0=None):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`), its largest error per array of MOMENTS
    against the same composition in np.longdouble (`e_ref`; zeros when `wide` is false), and the longdouble composition itself
    (`wide_ref`, None when `wide` is false)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, unif_bs, xi0, lengths, dtype=t)
    ref = res[np.float64]
    return ref, errors(ref, res[np.longdouble]) if wide else {k: 0.0 for k in MOMENTS}, res.get(np.longdouble) if wide else None


def on_stacks(out, lengths, unif_bs, dtype=np.float64):
    """`backsim` on the stacks of a device call `out` (STACKS: (G, R, steps, ...)), track by track over the record's rows: a dict of
    DRAWN, MOMENTS and cdf_bs shaped like `tracks`', and gap_bs."""
    G, R, steps, N, D = out["particles"].shape
    B = np.shape(unif_bs)[-1]
    res = {k: v for k, v in _empty(G, R, steps, N, D, B, dtype).items() if k in DRAWN + MOMENTS + ("cdf_bs", "gap_bs")}
    for g in range(G):
        for r in range(R):
            n = int(lengths[r])
            f = backsim([out[k][g, r, :n] for k in STACKS], pf.draws_of(unif_bs, g, r, 2)[:n], dtype)
            for k in DRAWN + MOMENTS:
                if k == "trajectories":
                    res[k][g, r, :, :n] = f[k]
                else:
                    res[k][g, r, :n] = f[k]
            res["cdf_bs"][g, r, :n] = f["cdf"]
            res["gap_bs"] = min(res["gap_bs"], f["gap"])
    return res


def margin(ref, unif=None, wide_ref=None):
    """The condition the device tests rest on.  Returns (gap, drift, same).  gap: the smallest |u tot - cdf_k| / tot over all rows and
    trajectories of `ref` (a dict of `tracks` or of `on_stacks`) and, when `ref` has the filter's cdf and `unif` is given, the gap of
    particle_filter_ref.margin too; drift: the largest |cdf / tot| difference between `ref` and `wide_ref` (backward, and the
    filter's when present); same: whether the two drew identical indices (and ancestors).  Drift 0 and True without `wide_ref`."""
    gap, drift, same = float(ref["gap_bs"]), 0.0, True
    filt = unif is not None and "cdf" in ref
    if filt:
        g, d, s = pf.margin(ref, unif, wide_ref)
        gap, drift, same = min(gap, g), d, s
    if wide_ref is not None:
        same = same and bool(np.array_equal(ref["traj_index"], wide_ref["traj_index"]))
        ok = ~np.isnan(ref["cdf_bs"])
        if ok.any():
            drift = max(drift, float(np.max(np.abs(ref["cdf_bs"][ok] - wide_ref["cdf_bs"][ok]))))
    return gap, drift, same
