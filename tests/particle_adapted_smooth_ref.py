"""NumPy restatement of particle smoothing and backward simulation on the ADAPTED filter's sets ("Adapted particle
smoothing"): test infrastructure, no product path imports it.  A thin composition of the existing references, in a floating-point type
of the caller's choice (np.float64: the reference; np.longdouble: that reference's own error):
  particle_adapted_ref.run with particle_smoother_ref.recording(cond, Q): the filter, with trans_mean[t] = X_t + m(X_t) and trans_var[t] =
    v(X_t) + Q of the set X_t carried into row t -- for t >= 1 the moments of particles[t - 1], particle by particle;
  particle_smoother_ref.recursion(particles, identity ancestors, trans_mean, trans_var, unit weights): particles[t] is equally weighted,
    so the last row is 1 / N, and particle i of row t is carried particle i of row t + 1, so the fold is the identity;
  particle_backsim_ref.backsim on the same stacks with identity ancestors and unit weights: the last row's cdf is 1 .. N and
    k_t is the searched index itself.
`run`, `tracks`, `reference` and `on_stacks` are shaped like the siblings'; `margin` is particle_backsim_ref's (the last row included:
u N must stay clear of the integers)."""
import numpy as np

import moment_ref as mr
import particle_adapted_ref as pa
import particle_backsim_ref as pb
import particle_filter_ref as pf
import particle_smoother_ref as ps
from particle_backsim_ref import DRAWN, MOMENTS, margin                                 # noqa: F401  (reused by the tests)

SMOOTHED = ps.SMOOTHED
KEPT = ("trans_mean", "trans_var")
FILTER = tuple(pf.MOMENTS + pf.DENSITIES + pf.EXTRA)
TAILS = {k: v for k, v in ps.TAILS.items() if k != "weights"}


def stacks_of(particles, trans_mean, trans_var, dtype=np.float64):
    """The five stacks the bootstrap references take, for the adapted sets: identity ancestors and unit weights"""
    n, N = np.shape(particles)[:2]
    return [particles, np.broadcast_to(np.arange(N), (n, N)), trans_mean, trans_var, np.ones((n, N), dtype=dtype)]


def recursion(particles, trans_mean, trans_var, dtype=np.float64):
    """The marginal smoother on the stacks of one track: a dict of SMOOTHED in `dtype`"""
    return ps.recursion(*stacks_of(particles, trans_mean, trans_var, dtype), dtype=dtype)


def backsim(particles, trans_mean, trans_var, unif_bs, dtype=np.float64, keep_cdf=True):
    """The backward simulation on the stacks of one track: particle_backsim_ref.backsim's dict"""
    return pb.backsim(stacks_of(particles, trans_mean, trans_var, dtype), unif_bs, dtype, keep_cdf)


def run(cond, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0=None, unif_bs=None, dtype=np.float64, smoother=True, keep_cdf=True):
    """One track: the adapted filter's dict plus KEPT, with `smoother` SMOOTHED, with unif_bs (n, B) DRAWN, MOMENTS, gap_bs and
    (keep_cdf) cdf_bs."""
    wrapped, rec = ps.recording(cond, Q, dtype)
    f = pa.run(wrapped, x0, S0, Y, CC, DD, sd, Q, eps, unif, xi0, dtype=dtype)
    f["trans_mean"], f["trans_var"] = np.stack(rec["trans_mean"]), np.stack(rec["trans_var"])
    if smoother:
        f.update(recursion(f["particles"], f["trans_mean"], f["trans_var"], dtype))
    if unif_bs is not None:
        b = backsim(f["particles"], f["trans_mean"], f["trans_var"], unif_bs, dtype, keep_cdf)
        for k in DRAWN + MOMENTS:
            f[k] = b[k]
        f["gap_bs"] = b["gap"]
        if keep_cdf:
            f["cdf_bs"] = b["cdf"]
    return f


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0=None, lengths=None, unif_bs=None, dtype=np.float64, smoother=True):
    """particle_adapted_ref.tracks with the smoother and (unif_bs in any of its three layouts) the backward simulation: a dict of
    arrays (G, R, steps, ...) in `dtype` (trajectories (G, R, B, steps, D)), NaN (indices -1) at and beyond a record's length; cdf is
    the filter's cdf / tot, cdf_bs the backward one, gap_bs the smallest backward gap of the call."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    N = np.shape(eps)[-2]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    tail = dict(m_pred=(D,), S_pred=(D, D), m_filt=(D,), S_filt=(D, D), lpd=(J,), lpd_joint=(), ess=(), particles=(N, D), cdf=(N,),
                trans_mean=(N, D), trans_var=(N, D))
    if smoother:
        tail.update({k: TAILS[k](N, D) for k in SMOOTHED})
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=dtype) for k, s in tail.items()}
    out["ancestors"] = np.full((G, R, steps, N), -1, dtype=np.int64)
    out["log_evidence"] = np.zeros((G, R), dtype=dtype)
    if unif_bs is not None:
        B = np.shape(unif_bs)[-1]
        out.update({k: v for k, v in pb._empty(G, R, steps, N, D, B, dtype).items() if k in DRAWN + MOMENTS + ("cdf_bs", "gap_bs")})
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            cond = pf.gp_cond(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = run(cond, x0[g][r], None if S0 is None else S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], pf.draws_of(eps, g, r, 3)[:n],
                    pf.draws_of(unif, g, r, 1)[:n], None if xi0 is None else pf.draws_of(xi0, g, r, 2),
                    None if unif_bs is None else pf.draws_of(unif_bs, g, r, 2)[:n], dtype=dtype, smoother=smoother)
            for k in out:
                if k == "trajectories":
                    out[k][g, r, :, :n] = f[k]
                elif k == "gap_bs":
                    out[k] = min(out[k], f[k])
                elif k == "log_evidence":
                    out[k][g, r] = f[k]
                else:
                    out[k][g, r, :n] = f[k]
    return out


def errors(ref, wide):
    """largest |ref - wide| per float array both have, over the entries ref has (ess_smooth divided by N)"""
    N = ref["particles"].shape[-2]
    e = {}
    for k in ref:
        if k in ("gap_bs", "ancestors", "traj_index") or k.startswith("cdf"):
            continue
        ok = ~np.isnan(ref[k])
        e[k] = float(np.max(np.abs(ref[k][ok] - wide[k][ok]))) / (N if k == "ess_smooth" else 1) if ok.any() else 0.0
    return e


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide, eps, unif, xi0=None, unif_bs=None, smoother=True):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`), its largest error per array against the same
    composition in np.longdouble (`e_ref`; zeros when `wide` is false; ess_smooth as ess_smooth / N), and the longdouble composition
    itself (`wide_ref`, None when `wide` is false)."""
    res = {}
    for t in (np.float64, np.longdouble) if wide else (np.float64,):
        terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t) for i, g in enumerate(gs)]
        res[t] = tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, eps, unif, xi0, lengths, unif_bs, dtype=t, smoother=smoother)
    ref = res[np.float64]
    e_ref = errors(ref, res[np.longdouble]) if wide else {k: 0.0 for k in errors(ref, ref)}
    return ref, e_ref, res.get(np.longdouble) if wide else None


def on_stacks(out, lengths, unif_bs=None, dtype=np.float64):
    """The recursion (unif_bs None) or the backward simulation on the stacks of a device call `out` (particles, trans_mean, trans_var:
    (G, R, steps, ...)), track by track over the record's rows: a dict of SMOOTHED, or of DRAWN, MOMENTS, cdf_bs and gap_bs, shaped
    like `tracks`'."""
    G, R, steps, N, D = out["particles"].shape
    if unif_bs is None:
        res = {k: np.full((G, R, steps) + TAILS[k](N, D), np.nan, dtype=dtype) for k in SMOOTHED}
    else:
        B = np.shape(unif_bs)[-1]
        res = {k: v for k, v in pb._empty(G, R, steps, N, D, B, dtype).items() if k in DRAWN + MOMENTS + ("cdf_bs", "gap_bs")}
    for g in range(G):
        for r in range(R):
            n = int(lengths[r])
            st = [out[k][g, r, :n] for k in ("particles", "trans_mean", "trans_var")]
            if unif_bs is None:
                f = recursion(*st, dtype=dtype)
                for k in SMOOTHED:
                    res[k][g, r, :n] = f[k]
                continue
            f = backsim(*st, pf.draws_of(unif_bs, g, r, 2)[:n], dtype)
            for k in DRAWN + MOMENTS:
                if k == "trajectories":
                    res[k][g, r, :, :n] = f[k]
                else:
                    res[k][g, r, :n] = f[k]
            res["cdf_bs"][g, r, :n] = f["cdf"]
            res["gap_bs"] = min(res["gap_bs"], f["gap"])
    return res
