"""NumPy reference of the rolling-origin forecasts under the third-degree spherical cubature rule ("Cubature
forecasts"): test infrastructure, no product path imports it.

Definition (`naive`): for an origin o, filter_ref.filter with cubature_filter_ref.ckf_transition over Y[:o + 1] followed by h all-NaN
rows; the track is rows o + 1 .. o + h of m_pred / S_pred.  `tracks` is the same thing cheaper: the filter is causal, so its filtered
state at row o over the whole record is the one over Y[:o + 1], and an unobserved row leaves the state as predicted; the track is
therefore h unobserved rows continued from (m_filt[o], S_filt[o]) with the control rows moved by o + 1.  The two are pinned against
each other bit for bit in tests/test_forecast_cubature_ref.py.  tests/forecast_linear_ref.py is the same file with the extended Kalman
transition; its fixtures (`start_cov`, `long_record`) are used from there."""
import numpy as np

import cubature_filter_ref as cf
import filter_ref as fr
import moment_ref as mr


def tracks(f, origins, h, J, CC, DD, sd, Q, ctrl, Z, kern, beta, Gam, dtype=np.float64, transition=cf.ckf_transition):
    """f: the dict of filter_ref.filter over the record; ctrl: the control rows the filter read (or None).  (B, h, D), (B, h, D, D).
    transition: the factory of the rule, called as cubature_filter_ref.ckf_transition (a test hands the rule on another conditional)."""
    nan = np.full((h, J), np.nan)
    ms, Ss = [], []
    for o in origins:
        c = None if ctrl is None else ctrl[o + 1:]
        t = fr.filter(f["m_filt"][o], f["S_filt"][o], nan, CC, DD, sd, Q, transition(c, Z, kern, beta, Gam, dtype=dtype), dtype=dtype)
        ms.append(t["m_pred"])
        Ss.append(t["S_pred"])
    return np.stack(ms), np.stack(Ss)


def naive(x0, S0, Y, origins, h, CC, DD, sd, Q, ctrl, Z, kern, beta, Gam, dtype=np.float64, transition=cf.ckf_transition):
    """the definition: one filter per origin over the truncated record and h all-NaN rows"""
    J = Y.shape[1]
    ms, Ss = [], []
    for o in origins:
        Yo = np.concatenate((Y[:o + 1], np.full((h, J), np.nan)), axis=0)
        f = fr.filter(x0, S0, Yo, CC, DD, sd, Q, transition(ctrl, Z, kern, beta, Gam, dtype=dtype), dtype=dtype)
        ms.append(f["m_pred"][o + 1: o + 1 + h])
        Ss.append(f["S_pred"][o + 1: o + 1 + h])
    return np.stack(ms), np.stack(Ss)


def reference(gs, ctrl, Y, CC, DD, sd, qs, S0, mode, origins, h, wide):
    """Per group the filter and its tracks on the oracle's posterior in fp64, stacked (G, B, h, ...): (`ref`, keys m, S), and the
    largest error of that against the same composition in np.longdouble (`e_ref`; zeros when `wide` is false)."""
    ref, e_ref = dict(m=[], S=[]), dict(m=0.0, S=0.0)
    J = Y.shape[1]
    for i, g in enumerate(gs):
        res = {}
        for t in (np.float64, np.longdouble) if wide else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
            f = fr.filter(g["X"][-1], S0[i], Y, CC, DD, sd, g["Q"], cf.ckf_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t), dtype=t)
            res[t] = tracks(f, origins, h, J, CC, DD, sd, g["Q"], ctrl, g["Z"], g["okern"], beta, Gam, dtype=t)
        ref["m"].append(res[np.float64][0])
        ref["S"].append(res[np.float64][1])
        if wide:
            e_ref["m"] = max(e_ref["m"], float(np.max(np.abs(res[np.float64][0] - res[np.longdouble][0]))))
            e_ref["S"] = max(e_ref["S"], float(np.max(np.abs(res[np.float64][1] - res[np.longdouble][1]))))
    return {k: np.stack(v) for k, v in ref.items()}, e_ref
