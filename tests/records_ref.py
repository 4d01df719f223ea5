"""NumPy reference of the linearised filter over many records ("Filtering many records"): test infrastructure,
no product path imports it.

Definition: a track (group g, record r) is filter_ref.filter with linear_filter_ref.ekf_transition on the posterior of group g, run
ONCE PER (group, record) over the first lengths[r] rows of Y[r] with the control rows ctrl[r] and the start N(x0[g, r], S0[g, r]),
then filter_ref.smooth over those rows.  Rows at and beyond a record's length are NaN in every array.  In a floating-point type of
the caller's choice (np.float64: the reference; np.longdouble: that reference's own error e_ref).  The pooled one-step arrays and the
per-record scalars are formed in NumPy from stacks (the reference's or a device's) by `pooled` and `scalars`."""
import numpy as np

import filter_ref as fr
import linear_filter_ref as lf
import moment_ref as mr

MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "m_smooth", "S_smooth")
DENSITIES = ("lpd", "lpd_joint")


def tracks(terms, gs, ctrl, Y, CC, DD, sd, x0, S0, lengths=None, dtype=np.float64):
    """terms: per group (beta, Gamma) in `dtype`; gs: per group a dict with Z, okern, Q; ctrl (R, steps, C) or None; Y (R, steps, J);
    x0 (G, R, D); S0 (G, R, D, D); lengths (R,) or None.  Returns a dict of arrays (G, R, steps, ...) in `dtype`: MOMENTS, lpd,
    lpd_joint; NaN at and beyond a record's length."""
    Y = np.asarray(Y)
    G, (R, steps, J), D = len(gs), Y.shape, np.shape(x0)[-1]
    ln = np.full(R, steps) if lengths is None else np.asarray(lengths)
    tail = dict(m_pred=(D,), S_pred=(D, D), m_filt=(D,), S_filt=(D, D), cross=(D, D), m_smooth=(D,), S_smooth=(D, D), lpd=(J,), lpd_joint=())
    out = {k: np.full((G, R, steps) + s, np.nan, dtype=dtype) for k, s in tail.items()}
    for g, grp in enumerate(gs):
        beta, Gam = terms[g]
        for r in range(R):
            n = int(ln[r])
            trans = lf.ekf_transition(None if ctrl is None else ctrl[r][:n], grp["Z"], grp["okern"], beta, Gam, dtype=dtype)
            f = fr.filter(x0[g][r], S0[g][r], Y[r][:n], CC, DD, sd, grp["Q"], trans, dtype=dtype)
            f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=dtype)
            for k in tail:
                out[k][g, r, :n] = f[k]
    return out


def reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, mode, lengths, wide):
    """On the oracle's posterior of every group (gs[g]["orc"]): `tracks` in fp64 (`ref`) and, per array of MOMENTS and DENSITIES, its
    largest error against the same composition in np.longdouble over the entries that are not NaN (`e_ref`; zeros when `wide` is
    false)."""
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


def pooled(m_pred, S_pred, CC, DD, sd, Y):
    """The one-step summary over the groups (equal weights) per record and row, (R, steps, J) each, from stacks (G, R, steps, ...):
    moment_ref.summary record by record."""
    R = np.shape(Y)[0]
    per = [mr.summary(m_pred[:, r], S_pred[:, r], CC, DD, sd, np.asarray(Y)[r]) for r in range(R)]
    return dict(predict_y=np.stack([p["y_mean"] for p in per]), predict_y_var_total=np.stack([p["y_var_total"] for p in per]),
                lpd_mix=np.stack([p["lpd"] for p in per]), lpd_gauss=np.stack([p["lpd_gauss"] for p in per]))


def scalars(Y, lpd_mix, lpd_joint, predict_y, Y_train_std=1.0):
    """Per record, arrays (R,): ll (mean of lpd_mix over the observed entries), ll_joint (mean over the rows with an observed entry of
    log mean_g exp(lpd_joint[g, r, i])), ll_original_units (ll - log Y_train_std), RMSE (observed entries of the first 30 rows, times
    Y_train_std); ll_all: the mean of lpd_mix over every observed entry of every record."""
    Y = np.asarray(Y)
    R = Y.shape[0]
    out = dict(ll=np.full(R, np.nan), ll_joint=np.full(R, np.nan), RMSE=np.full(R, np.nan))
    for r in range(R):
        seen = ~np.isnan(Y[r])
        if seen.any():
            out["ll"][r] = np.mean(lpd_mix[r][seen])
            rows = seen.any(axis=1)
            lj = lpd_joint[:, r][:, rows]
            out["ll_joint"][r] = np.mean(np.log(np.mean(np.exp(lj - lj.max(axis=0)), axis=0)) + lj.max(axis=0))
        s30 = seen[:30]
        if s30.any():
            out["RMSE"][r] = np.sqrt(np.mean((Y[r][:30][s30] - predict_y[r][:30][s30]) ** 2)) * Y_train_std
    out["ll_original_units"] = out["ll"] - np.log(Y_train_std)
    seen = ~np.isnan(Y)
    out["ll_all"] = float(np.mean(lpd_mix[seen])) if seen.any() else float("nan")
    return out
