"""NumPy reference of the rolling-origin forecasts under the linearised (extended Kalman) rule ("Linearised
forecasts"): test infrastructure, no product path imports it.

Definition (`naive`): for an origin o, filter_ref.filter with linear_filter_ref.ekf_transition over Y[:o + 1] followed by h all-NaN
rows; the track is rows o + 1 .. o + h of m_pred / S_pred.  `tracks` is the same thing cheaper: the filter is causal, so its filtered
state at row o over the whole record is the one over Y[:o + 1], and an unobserved row leaves the state as predicted; the track is
therefore h unobserved rows continued from (m_filt[o], S_filt[o]) with the control rows moved by o + 1.  The two are pinned against
each other bit for bit in tests/test_forecast_linear_ref.py.

`long_record` is the fixture that crosses a row-tile boundary of the device's product kernel (138 origins per unit), built without a
device so that the reference can be checked on the CPU."""
import functools

import numpy as np

import filter_ref as fr
import linear_filter_ref as lf
import moment_ref as mr
from ffvd_amd import synthetic
from oracle import ffvd_oracle as orc


def tracks(f, origins, h, J, CC, DD, sd, Q, ctrl, Z, kern, beta, Gam, dtype=np.float64):
    """f: the dict of filter_ref.filter over the record; ctrl: the control rows the filter read (or None).  (B, h, D), (B, h, D, D)"""
    nan = np.full((h, J), np.nan)
    ms, Ss = [], []
    for o in origins:
        c = None if ctrl is None else ctrl[o + 1:]
        t = fr.filter(f["m_filt"][o], f["S_filt"][o], nan, CC, DD, sd, Q, lf.ekf_transition(c, Z, kern, beta, Gam, dtype=dtype), dtype=dtype)
        ms.append(t["m_pred"])
        Ss.append(t["S_pred"])
    return np.stack(ms), np.stack(Ss)


def naive(x0, S0, Y, origins, h, CC, DD, sd, Q, ctrl, Z, kern, beta, Gam, dtype=np.float64):
    """the definition: one filter per origin over the truncated record and h all-NaN rows"""
    J = Y.shape[1]
    ms, Ss = [], []
    for o in origins:
        Yo = np.concatenate((Y[:o + 1], np.full((h, J), np.nan)), axis=0)
        f = fr.filter(x0, S0, Yo, CC, DD, sd, Q, lf.ekf_transition(ctrl, Z, kern, beta, Gam, dtype=dtype), dtype=dtype)
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
            f = fr.filter(g["X"][-1], S0[i], Y, CC, DD, sd, g["Q"], lf.ekf_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t), dtype=t)
            res[t] = tracks(f, origins, h, J, CC, DD, sd, g["Q"], ctrl, g["Z"], g["okern"], beta, Gam, dtype=t)
        ref["m"].append(res[np.float64][0])
        ref["S"].append(res[np.float64][1])
        if wide:
            e_ref["m"] = max(e_ref["m"], float(np.max(np.abs(res[np.float64][0] - res[np.longdouble][0]))))
            e_ref["S"] = max(e_ref["S"], float(np.max(np.abs(res[np.float64][1] - res[np.longdouble][1]))))
    return {k: np.stack(v) for k, v in ref.items()}, e_ref


def start_cov(G, D, seed=5):
    """tests/test_gpu_moment_grouped.py's start covariances (restated, so that the CPU test of this reference imports no GPU test module)"""
    rng = np.random.default_rng(seed)
    out = np.empty((G, D, D))
    for g in range(G):
        A = rng.standard_normal((D, D))
        S = (0.05 + 0.45 * rng.random()) * (A @ A.T / D + 0.1 * np.eye(D))
        out[g] = np.triu(S) + np.triu(S, 1).T
    return out


LONG_N, LONG_H = 140, 2


@functools.lru_cache(maxsize=None)
def long_record():
    """synthetic "tiny" with T = 160 and two chains (M = 24, D = 2, C = 1), a 140-row record built like the one of
    tests/test_gpu_filter_linear.py::test_a_second_column_stride (default_rng(3) controls, default_rng(31) noise of 0.3 around the
    emission of the chains' last states), row 7 unobserved, q slices, q_mode "intent", a start covariance, h = 2: 138 origins.
    The oracle's posterior per chain, no device.  Shared, never modified."""
    params, _, c, meta = synthetic.make_named("tiny", T=160, S=2)
    T, D, n = meta["T"], meta["D"], LONG_N
    okern, Q = orc.make_kernels(params, kernel_type=meta["kernel_type"]), np.exp(params["log_Q"])
    Lo = orc.kernel_pre_cal(params["Z"], okern)
    gs = []
    for s in range(2):
        X = params["X"][s]
        Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, np.concatenate((X[:T], c[:T]), axis=1), X, params["Z"], okern, Q)
        gs.append(dict(Z=params["Z"], okern=okern, X=X, Q=Q, orc=dict(L=list(Lo), U=Uo, H=np.asarray(Ho))))
    call = np.concatenate((c, np.random.default_rng(3).standard_normal((n, meta["C"]))), axis=0)
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    Y = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(31).standard_normal((n, CC.shape[1]))
    Y[7] = np.nan
    return dict(params=params, c=c, meta=meta, gs=gs, call=call, ctrl=call[T: T + n], Y=Y, CC=CC, DD=DD, lr=lr, sd=np.exp(np.asarray(lr)[0]),
                S0=start_cov(2, D), qs=[g["orc"]["H"] for g in gs], mode="intent", origins=list(range(n - LONG_H)), h=LONG_H)
