"""Posterior rollouts / prediction: the loop of BaseModel.collect_samples_formal
(vfegpssm/base_model.py:197-350) with the R posterior rollouts advanced side by side on the GPU.

The reference builds `num` rollouts one after another, each `test_len` sequential calls of
conditional_after_kernel_precalculation at ONE point; with the collapsed U (case 4) they differ only by their
noise draws, so here every step is one batched call at the R current states: `ffvd_op_rollout` enqueues
steps x (projection, q_sqrt inflation, conditional, update) on one stream without host round trips.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .conditionals_multi_output import JITTER, Q_MODES, check_conditional_query, pack_posterior_groups
from .kernels import stack_hypers


def rollout(Lm_inverse_seq, Z, kern, U_val, q_sqrt, x_last, control_inputs, ctrl_offset, steps, Q, eps):
    """predict_x, predict_x_var (R, steps, D) of base_model.py:288-314.

    q_sqrt: None or the (D, M, M) stack U_variance_cholesky -- slice d = 0 is used for every dim;
    x_last: (D,) = layers[-1].X[-1]; control_inputs: (n, C), row ctrl_offset + t feeds step t;
    eps: (steps, R, D) standard-normal draws (tf.random.normal at :306, injected)."""
    kind, _, logvar, loglen = stack_hypers(kern)
    D = len(kern)
    Z = _lib.as_f64(Z)
    M, P = Z.shape
    eps = _lib.as_f64(eps)
    if eps.ndim != 3 or eps.shape[2] != D or eps.shape[0] != steps:
        raise ValueError(f"eps: expected ({steps}, R, {D}), got {eps.shape}")
    R = eps.shape[1]
    C = P - D
    ctrl = None
    if C > 0:
        ci = _lib.as_f64(control_inputs)
        if ci.ndim != 2 or ci.shape[1] != C or ci.shape[0] < ctrl_offset + steps:
            raise ValueError(f"control_inputs: need at least {ctrl_offset + steps} rows of {C} columns")
        ctrl = np.ascontiguousarray(ci[ctrl_offset: ctrl_offset + steps])
    W = _lib.as_f64(np.stack([np.asarray(w) for w in Lm_inverse_seq]), (D, M, M), "Lm_inverse_seq")
    f = _lib.as_f64(U_val, (M, D), "U_val")
    qs = None
    if q_sqrt is not None:
        q = np.asarray(q_sqrt, dtype=np.float64)
        if q.ndim != 3 or q.shape[1:] != (M, M):
            raise ValueError("Bad dimension for q_sqrt: expected (D, M, M)")
        qs = np.ascontiguousarray(q[0])
    x_last = _lib.as_f64(x_last, (D,), "x_last")
    log_Q = np.log(_lib.as_f64(Q, (D,), "Q"))
    px, pv = np.empty((R, steps, D)), np.empty((R, steps, D))
    rc = _lib.load().ffvd_op_rollout(kind, _lib.dptr(W), _lib.dptr(Z), M, P, D, _lib.dptr(logvar),
                                     None if loglen is None else _lib.dptr(loglen), _lib.dptr(f),
                                     None if qs is None else _lib.dptr(qs), _lib.dptr(x_last), R,
                                     None if ctrl is None else _lib.dptr(ctrl), C, steps, _lib.dptr(log_Q), _lib.dptr(eps),
                                     _lib.dptr(px), _lib.dptr(pv))
    _lib.check(rc, None, "ffvd_op_rollout")
    return px, pv


def _pack_rollout_groups(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, eps):
    """Shape checks and packing of `rollout_grouped`'s arguments (before the library is loaded): the leading arguments of
    `ffvd_op_rollout_grouped` up to eps, and the shapes."""
    G = len(kerns)
    if G < 1:
        raise ValueError("rollout_grouped: at least one group is needed")
    for name, seq in (("Lm_inverse_seqs", Lm_inverse_seqs), ("Zs", Zs), ("U_vals", U_vals), ("x_lasts", x_lasts), ("Qs", Qs)):
        if len(seq) != G:
            raise ValueError(f"{name}: expected {G} groups, got {len(seq)}")
    if q_sqrts is not None and len(q_sqrts) != G:
        raise ValueError(f"q_sqrts: expected None or {G} groups, got {len(q_sqrts)}")
    hy = [stack_hypers(k) for k in kerns]
    kind, D = hy[0][0], len(kerns[0])
    Z0 = np.asarray(Zs[0])
    if Z0.ndim != 2:
        raise ValueError(f"Zs[0]: expected (M, P), got {Z0.shape}")
    M, P = Z0.shape
    for g in range(G):
        if hy[g][0] != kind:
            raise ValueError(f"kerns[{g}]: every group must use the same kernel type")
        if len(kerns[g]) != D:
            raise ValueError(f"kerns[{g}]: expected {D} kernels (one per latent dim), got {len(kerns[g])}")
    eps = _lib.as_f64(eps)
    if eps.ndim != 4 or eps.shape[0] != steps or eps.shape[1] != G or eps.shape[2] < 1 or eps.shape[3] != D:
        raise ValueError(f"eps: expected ({steps}, {G}, R >= 1, {D}), got {eps.shape}")
    R = eps.shape[2]
    C = P - D
    ctrl = None
    if C > 0:
        ci = _lib.as_f64(control_inputs)
        if ci.ndim != 2 or ci.shape[1] != C or ci.shape[0] < ctrl_offset + steps:
            raise ValueError(f"control_inputs: need at least {ctrl_offset + steps} rows of {C} columns")
        ctrl = np.ascontiguousarray(ci[ctrl_offset: ctrl_offset + steps])
    # the small arrays are packed (one upload per kind); the M x M matrices are NOT copied on the host: the library gets a table of
    # pointers and sends every matrix from where it lies into its slot of the padded device stack
    Z = np.empty((G, M, P))
    Wm, qm = [], []                                  # (keeps the matrices alive until the call returns)
    f = np.empty((G, M, D))
    xl, log_Q, logvar = np.empty((G, D)), np.empty((G, D)), np.empty((G, D))
    loglen = None if hy[0][3] is None else np.empty((G, D, P))
    for g in range(G):
        Z[g] = _lib.as_f64(Zs[g], (M, P), f"Zs[{g}]")
        if len(Lm_inverse_seqs[g]) != D:
            raise ValueError(f"Lm_inverse_seqs[{g}]: expected {D} matrices, got {len(Lm_inverse_seqs[g])}")
        for d in range(D):
            Wm.append(_lib.as_f64(Lm_inverse_seqs[g][d], (M, M), f"Lm_inverse_seqs[{g}][{d}]"))
        f[g] = _lib.as_f64(U_vals[g], (M, D), f"U_vals[{g}]")
        xl[g] = _lib.as_f64(x_lasts[g], (D,), f"x_lasts[{g}]")
        log_Q[g] = np.log(_lib.as_f64(Qs[g], (D,), f"Qs[{g}]"))
        logvar[g] = _lib.as_f64(hy[g][2], (D,), f"kerns[{g}] logvariance")
        if loglen is not None:
            loglen[g] = _lib.as_f64(hy[g][3], (D, P), f"kerns[{g}] loglengthscales")
        if q_sqrts is not None:
            q = np.asarray(q_sqrts[g], dtype=np.float64)
            if q.ndim != 3 or q.shape[1:] != (M, M) or q.shape[0] < 1:
                raise ValueError(f"Bad dimension for q_sqrts[{g}]: expected (D, M, M)")
            qm.append(np.ascontiguousarray(q[0]))
    import ctypes
    Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
    qt = (ctypes.c_void_p * len(qm))(*[q.ctypes.data for q in qm]) if q_sqrts is not None else None
    args = (kind, G, Wt, _lib.dptr(Z), M, P, D, _lib.dptr(logvar), None if loglen is None else _lib.dptr(loglen), _lib.dptr(f), qt,
            _lib.dptr(xl), R, None if ctrl is None else _lib.dptr(ctrl), C, steps, _lib.dptr(log_Q), _lib.dptr(eps))
    return dict(args=args, G=G, R=R, D=D, steps=steps, keep=(Wm, qm, Z, logvar, loglen, f, xl, ctrl, log_Q, eps))


def rollout_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, eps):
    """G independent posteriors rolled forward by one call (`ffvd_op_rollout_grouped`): one launch per step for all groups.

    Every argument but control_inputs / ctrl_offset / steps / eps is a length-G sequence of the matching argument of `rollout`
    (one posterior per SG-HMC sample, or per chain); q_sqrts: None or G stacks (D, M, M), slice 0 of each is used;
    eps: (steps, G, R, D).  Kernel kind, M, P and D are common to the groups.  Returns predict_x, predict_x_var (G, R, steps, D);
    group g's slab is bit-identical to what a G = 1 call on that group alone returns."""
    a = _pack_rollout_groups(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, eps)
    G, R, D = a["G"], a["R"], a["D"]
    px, pv = np.empty((G, R, steps, D)), np.empty((G, R, steps, D))
    rc = _lib.load().ffvd_op_rollout_grouped(*a["args"], _lib.dptr(px), _lib.dptr(pv))
    _lib.check(rc, None, "ffvd_op_rollout_grouped")
    return px, pv


def _pack_posterior_rollout(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, eps, jitter, groups_per_pass):
    """Shape checks and packing of `posterior_rollout_grouped`'s arguments (before the library is loaded): the leading arguments
    of `ffvd_op_posterior_rollout_grouped` up to eps, and the shapes."""
    a = pack_posterior_groups(Zs, kerns, Xs, control_inputs, Qs, who)
    G, nm, M, D, C = a["G"], a["n_models"], a["M"], a["D"], a["C"]
    steps = int(steps)
    if steps < 0 or int(ctrl_offset) < 0 or int(groups_per_pass) < 0:
        raise ValueError(f"{who}: steps, ctrl_offset and groups_per_pass must not be negative")
    eps = _lib.as_f64(eps)
    if eps.ndim != 4 or eps.shape[0] != steps or eps.shape[1] != G or eps.shape[2] < 1 or eps.shape[3] != D:
        raise ValueError(f"eps: expected ({steps}, {G}, R >= 1, {D}), got {eps.shape}")
    R = eps.shape[2]
    ctrl = None
    if C > 0:
        ci = _lib.as_f64(control_inputs)
        if ci.shape[0] < ctrl_offset + steps:
            raise ValueError(f"control_inputs: need at least {ctrl_offset + steps} rows of {C} columns")
        ctrl = np.ascontiguousarray(ci[ctrl_offset: ctrl_offset + steps])
    dp = _lib.dptr
    args = (a["kind"], G, nm, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]), None if a["loglen"] is None else dp(a["loglen"]), dp(a["X"]),
            None if a["ctrl"] is None else dp(a["ctrl"]), C, a["T"], dp(a["log_Q"]), float(jitter), int(groups_per_pass), R,
            None if ctrl is None else dp(ctrl), steps, dp(eps))
    return dict(args=args, G=G, R=R, M=M, D=D, steps=steps, keep=(a, ctrl, eps))


def posterior_rollout_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, eps, *, jitter=JITTER, groups_per_pass=0,
                              return_U=False):
    """The collapsed posterior of G groups and their rollouts in ONE call (`ffvd_op_posterior_rollout_grouped`): what
    `conditionals_multi_output.collapse_u_mean_grouped` followed by `rollout_grouped` computes, without the posteriors leaving the
    device.  `Zs` / `kerns`: one model (shared by the groups: one per chain) or length-G sequences (one per SG-HMC sample); Xs: G
    trajectories (T+1, D), the rollouts of group g start at Xs[g][-1]; Qs: G vectors (D,) or one; rows [0, T) of control_inputs feed
    the posterior, rows [ctrl_offset, ctrl_offset + steps) the rollouts; eps: (steps, G, R, D).
    Returns predict_x, predict_x_var (G, R, steps, D) and, with return_U, U_means (G, M, D)."""
    who = "posterior_rollout_grouped"
    a = _pack_posterior_rollout(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, eps, jitter, groups_per_pass)
    G, R, M, D, steps = a["G"], a["R"], a["M"], a["D"], a["steps"]
    px, pv = np.empty((G, R, steps, D)), np.empty((G, R, steps, D))
    U = np.empty((G, M, D)) if return_U else None
    dp = _lib.dptr
    rc = _lib.load().ffvd_op_posterior_rollout_grouped(*a["args"], dp(px), dp(pv), None if U is None else dp(U))
    _lib.check(rc, None, who)
    return (px, pv, U) if return_U else (px, pv)


def posterior_conditional_grouped(Zs, kerns, Xs, Qs, control_inputs, Xnew, *, q_mode="reference", jitter=JITTER, groups_per_pass=0,
                                  rows_per_pass=0, per_group=True, summary=True, return_U=False):
    """The collapsed posterior of G groups and its transition function f(x, c) at Xnew (N, P) in ONE call
    (`ffvd_op_posterior_conditional_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `conditional_grouped` computes, without the posteriors leaving the device.  `Zs` / `kerns` / `Xs` / `Qs` / `control_inputs`: as
    `posterior_rollout_grouped`; q_mode, per_group, summary, rows_per_pass: as `conditional_grouped`.
    Returns (means, vars, mix_mean, mix_var) and, with return_U, U_means (G, M, D)."""
    who = "posterior_conditional_grouped"
    a = pack_posterior_groups(Zs, kerns, Xs, control_inputs, Qs, who)
    G, nm, M, D = a["G"], a["n_models"], a["M"], a["D"]
    if int(groups_per_pass) < 0:
        raise ValueError(f"{who}: groups_per_pass must be 0 (automatic) or positive")
    Xnew, qm = check_conditional_query(who, Xnew, a["P"], q_mode, rows_per_pass, per_group, summary)
    N = Xnew.shape[0]
    means, vars_ = (np.empty((G, N, D)), np.empty((G, N, D))) if per_group else (None, None)
    mm, mv = (np.empty((N, D)), np.empty((N, D))) if summary else (None, None)
    U = np.empty((G, M, D)) if return_U else None
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = _lib.load().ffvd_op_posterior_conditional_grouped(a["kind"], G, nm, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]), opt(a["loglen"]),
                                                           dp(a["X"]), opt(a["ctrl"]), a["C"], a["T"], dp(a["log_Q"]), float(jitter),
                                                           int(groups_per_pass), qm, dp(Xnew), N, int(rows_per_pass), opt(means),
                                                           opt(vars_), opt(mm), opt(mv), opt(U))
    _lib.check(rc, None, who)
    return (means, vars_, mm, mv, U) if return_U else (means, vars_, mm, mv)


def posterior_conditional_grad_grouped(Zs, kerns, Xs, Qs, control_inputs, Xnew, *, q_mode="reference", jitter=JITTER, groups_per_pass=0,
                                       rows_per_pass=0, per_group=True, summary=True, variance=True, return_U=False):
    """The collapsed posterior of G groups and the linearisation of its transition function f(x, c) at Xnew (N, P) in ONE call
    (`ffvd_op_posterior_conditional_grad_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `conditional_grad_grouped` computes, without the posteriors leaving the device.  SE-ARD kernels only.  `Zs` / `kerns` / `Xs` / `Qs` /
    `control_inputs`: as `posterior_rollout_grouped`; the other arguments and the returned dict: as `conditional_grad_grouped`, plus
    `U_means` (G, M, D) with return_U."""
    from .conditionals_multi_output import GRAD_KEYS, check_se_only, grad_outputs
    who = "posterior_conditional_grad_grouped"
    a = pack_posterior_groups(Zs, kerns, Xs, control_inputs, Qs, who)
    check_se_only(who, a["kind"])
    G, nm, M, D, P = a["G"], a["n_models"], a["M"], a["D"], a["P"]
    if int(groups_per_pass) < 0:
        raise ValueError(f"{who}: groups_per_pass must be 0 (automatic) or positive")
    Xnew, qm = check_conditional_query(who, Xnew, P, q_mode, rows_per_pass, per_group, summary)
    N = Xnew.shape[0]
    out = grad_outputs(G, N, D, P, per_group, summary, variance)
    U = np.empty((G, M, D)) if return_U else None
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = _lib.load().ffvd_op_posterior_conditional_grad_grouped(a["kind"], G, nm, dp(a["Z"]), M, P, D, dp(a["logvar"]), opt(a["loglen"]),
                                                                dp(a["X"]), opt(a["ctrl"]), a["C"], a["T"], dp(a["log_Q"]), float(jitter),
                                                                int(groups_per_pass), qm, dp(Xnew), N, int(rows_per_pass),
                                                                *[opt(out[k]) for k in GRAD_KEYS], opt(U))
    _lib.check(rc, None, who)
    if return_U:
        out["U_means"] = U
    return out


def predict_y_summary(predict_x, predict_x_var, CC, DD, log_Rchols, Y_test=None, Y_train_std=1.0):
    """base_model.py:330-348 (host-side: a (num, test_len, D) x (D, Ydim) contraction and three means)."""
    CC, DD = np.asarray(CC, dtype=np.float64), np.asarray(DD, dtype=np.float64)
    predict_y = (np.mean(np.einsum("ijk,kl->ijl", predict_x, CC), axis=0) + DD[None, :]).reshape(-1)
    predict_y_var = (np.mean(np.einsum("ijk,kl->ijl", predict_x_var, CC ** 2), axis=0).reshape(-1)
                     + np.exp(2 * np.asarray(log_Rchols, dtype=np.float64))).reshape(-1)
    out = {"predict_y": predict_y, "predict_y_var": predict_y_var}
    if Y_test is not None:
        y30, p30 = np.asarray(Y_test, dtype=np.float64)[:30].reshape(-1), predict_y[:30]
        out["RMSE"] = float(np.sqrt(np.mean((y30 - p30) ** 2)) * Y_train_std)
    return out


SUMMARY_MAX_OUTPUTS = 8       # J <= 8, as the particle-Gibbs step


def _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test):
    """Shape checks of the emission and the held-out data (before the library is loaded).  The noise standard deviation of output
    j is exp(log_Rchols[0, j]): row 0, the row the likelihood of the nll uses (dgp_model.py:250); a vector of J entries (or a scalar
    for J = 1) is taken as that row."""
    CC = _lib.as_f64(CC)
    if CC.ndim != 2 or CC.shape[0] != D or not 1 <= CC.shape[1] <= SUMMARY_MAX_OUTPUTS:
        raise ValueError(f"{who}: CC: expected ({D}, J) with 1 <= J <= {SUMMARY_MAX_OUTPUTS}, got {CC.shape}")
    J = CC.shape[1]
    DD = _lib.as_f64(np.asarray(DD, dtype=np.float64).reshape(-1), (J,), "DD")
    lr = np.asarray(log_Rchols, dtype=np.float64)
    if lr.ndim == 2 and lr.shape == (J, J):
        lr = lr[0]
    elif lr.size == J and lr.ndim <= 1:
        lr = lr.reshape(J)
    else:
        raise ValueError(f"{who}: log_Rchols: expected ({J}, {J}) or ({J},), got {lr.shape}")
    sd = np.ascontiguousarray(np.exp(lr))
    if not np.all(np.isfinite(sd)) or not np.all(sd > 0.0):
        raise ValueError(f"{who}: exp(log_Rchols[0, :]) must be finite and positive")
    Y = None
    if Y_test is not None:
        Y = np.asarray(Y_test, dtype=np.float64)
        if Y.ndim == 1 and J == 1:
            Y = Y[:, None]
        if Y.ndim != 2 or Y.shape[1] != J or Y.shape[0] > steps:
            raise ValueError(f"{who}: Y_test: expected (n_test <= {steps}, {J}), got {Y.shape}")
        Y = np.ascontiguousarray(Y)
    return dict(CC=CC, DD=DD, sd=sd, Y=Y, J=J, n_test=0 if Y is None else Y.shape[0])


def _summary_call(m, steps):
    """Output arrays and the trailing arguments of the three summary entry points."""
    J, nt, dp = m["J"], m["n_test"], _lib.dptr
    out = dict(y_mean=np.empty((steps, J)), y_var=np.empty((steps, J)), y_var_total=np.empty((steps, J)))
    if m["Y"] is not None:
        out.update(lpd=np.empty((nt, J)), lpd_gauss=np.empty((nt, J)))
    opt = lambda k: dp(out[k]) if k in out and out[k].size else None            # (no held-out rows: no density is asked for)
    args = (dp(m["CC"]), dp(m["DD"]), dp(m["sd"]), J, dp(m["Y"]) if nt else None, nt, opt("y_mean"), opt("y_var"),
            opt("y_var_total"), opt("lpd"), opt("lpd_gauss"))
    return out, args


def _summary_dict(m, out, Y_train_std):
    """The dict the summary functions return: predict_y / predict_y_var flattened as `predict_y_summary` does, the total variance,
    and with Y_test the densities, their mean `ll` (and in the data's units: minus log Y_train_std) and the RMSE over the first
    30 test points (base_model.py:346-348: `predict_y_summary`'s expression on y_mean)."""
    res = {"predict_y": out["y_mean"].reshape(-1), "predict_y_var": out["y_var"].reshape(-1),
           "predict_y_var_total": out["y_var_total"].reshape(-1)}
    if m["Y"] is not None:
        n30 = min(30, m["n_test"])
        y30, p30 = m["Y"][:n30].reshape(-1), out["y_mean"][:n30].reshape(-1)
        res["RMSE"] = float(np.sqrt(np.mean((y30 - p30) ** 2)) * Y_train_std) if n30 else float("nan")
        ll = float(np.mean(out["lpd"])) if out["lpd"].size else float("nan")
        res.update(lpd=out["lpd"], lpd_gauss=out["lpd_gauss"], ll=ll, ll_original_units=ll - float(np.log(Y_train_std)))
    return res


def rollout_summary(predict_x, predict_x_var, CC, DD, log_Rchols, Y_test=None, Y_train_std=1.0):
    """The held-out predictive summary of base_model.py:330-348 on the GPU (`ffvd_op_rollout_summary`): `predict_y_summary`'s
    predict_y / predict_y_var, and what it lacks -- predict_y_var_total (noise plus the spread of the rollouts: the law of total
    variance) and, with Y_test (n_test <= steps, J), lpd (n_test, J): the log of the Monte-Carlo predictive density of each held-out
    point, lpd_gauss: its moment-matched Gaussian counterpart, ll = mean(lpd), ll_original_units and RMSE.
    predict_x, predict_x_var: (N, steps, D) or (G, R, steps, D); CC (D, J <= 8); DD (J,); log_Rchols (J, J) (row 0 is used) or (J,)."""
    who = "rollout_summary"
    px, pv = _lib.as_f64(predict_x), _lib.as_f64(predict_x_var)
    if px.ndim not in (3, 4) or px.shape != pv.shape:
        raise ValueError(f"{who}: predict_x and predict_x_var: expected equal shapes (N, steps, D) or (G, R, steps, D), got "
                         f"{px.shape} and {pv.shape}")
    steps, D = px.shape[-2:]
    N = int(np.prod(px.shape[:-2]))
    if N < 1 or steps < 1 or D < 1:
        raise ValueError(f"{who}: at least one rollout, one step and one latent dim are needed, got {px.shape}")
    m = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    out, args = _summary_call(m, steps)
    rc = _lib.load().ffvd_op_rollout_summary(_lib.dptr(px), _lib.dptr(pv), N, steps, D, *args)
    _lib.check(rc, None, who)
    return _summary_dict(m, out, Y_train_std)


def rollout_grouped_summary(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, eps, CC, DD,
                            log_Rchols, Y_test=None, Y_train_std=1.0, *, return_rollouts=False):
    """`rollout_grouped` and `rollout_summary` over all G * R rollouts in ONE call (`ffvd_op_rollout_grouped_summary`): the summary
    is formed on the device; the (G, R, steps, D) stacks come down only with return_rollouts (keys predict_x, predict_x_var)."""
    who = "rollout_grouped_summary"
    a = _pack_rollout_groups(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, eps)
    G, R, D = a["G"], a["R"], a["D"]
    m = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    out, args = _summary_call(m, steps)
    px, pv = (np.empty((G, R, steps, D)), np.empty((G, R, steps, D))) if return_rollouts else (None, None)
    opt = lambda x: None if x is None else _lib.dptr(x)
    rc = _lib.load().ffvd_op_rollout_grouped_summary(*a["args"], opt(px), opt(pv), *args)
    _lib.check(rc, None, who)
    res = _summary_dict(m, out, Y_train_std)
    if return_rollouts:
        res.update(predict_x=px, predict_x_var=pv)
    return res


def posterior_rollout_grouped_summary(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, eps, CC, DD, log_Rchols, Y_test=None,
                                      Y_train_std=1.0, *, jitter=JITTER, groups_per_pass=0, return_rollouts=False, return_U=False):
    """`posterior_rollout_grouped` and `rollout_summary` over all G * R rollouts in ONE call
    (`ffvd_op_posterior_rollout_grouped_summary`): posteriors, rollouts and summary stay on the device; the (G, R, steps, D) stacks
    come down only with return_rollouts (keys predict_x, predict_x_var), U_means (G, M, D) only with return_U."""
    who = "posterior_rollout_grouped_summary"
    a = _pack_posterior_rollout(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, eps, jitter, groups_per_pass)
    G, R, M, D, steps = a["G"], a["R"], a["M"], a["D"], a["steps"]
    m = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    out, args = _summary_call(m, steps)
    px, pv = (np.empty((G, R, steps, D)), np.empty((G, R, steps, D))) if return_rollouts else (None, None)
    U = np.empty((G, M, D)) if return_U else None
    opt = lambda x: None if x is None else _lib.dptr(x)
    rc = _lib.load().ffvd_op_posterior_rollout_grouped_summary(*a["args"], opt(px), opt(pv), opt(U), *args)
    _lib.check(rc, None, who)
    res = _summary_dict(m, out, Y_train_std)
    if return_rollouts:
        res.update(predict_x=px, predict_x_var=pv)
    if return_U:
        res["U_means"] = U
    return res


MOMENT_MAX_D, MOMENT_MAX_P, MOMENT_MAX_M = 8, 32, 2048


def _moment_limits(who, kind, M, P, D):
    """The limits of the moment-matched prediction that depend on the model alone (before the library is loaded)."""
    if kind != 0:
        raise ValueError(f"{who}: moment matching is closed-form for the SquaredExponential kernel only (LinearK is rejected)")
    if not 1 <= D <= MOMENT_MAX_D or not D <= P <= MOMENT_MAX_P or not 1 <= M <= MOMENT_MAX_M:
        raise ValueError(f"{who}: expected D <= {MOMENT_MAX_D}, D <= P <= {MOMENT_MAX_P}, M <= {MOMENT_MAX_M}, got D = {D}, P = {P}, M = {M}")


def _moment_run_args(who, G, D, C, control_inputs, ctrl_offset, steps, S0s, q_mode):
    """q_mode code, start covariances (G, D, D) or None, and the control rows of the propagation, checked."""
    if q_mode not in Q_MODES:
        raise ValueError(f"{who}: q_mode: expected one of {sorted(Q_MODES)}, got {q_mode!r}")
    steps, ctrl_offset = int(steps), int(ctrl_offset)
    if steps < 0 or ctrl_offset < 0:
        raise ValueError(f"{who}: steps and ctrl_offset must not be negative")
    S0 = None
    if S0s is not None:
        S0 = _lib.as_f64(S0s, (G, D, D), "S0s")
        if not np.all(np.isfinite(S0)) or not np.array_equal(S0, np.swapaxes(S0, 1, 2)):
            raise ValueError(f"{who}: S0s: every start covariance must be finite and exactly symmetric")
    ctrl = None
    if C > 0:
        ci = _lib.as_f64(control_inputs)
        if ci.ndim != 2 or ci.shape[1] != C or ci.shape[0] < ctrl_offset + steps:
            raise ValueError(f"{who}: control_inputs: need at least {ctrl_offset + steps} rows of {C} columns")
        ctrl = np.ascontiguousarray(ci[ctrl_offset: ctrl_offset + steps])
    return Q_MODES[q_mode], S0, ctrl, steps


def _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode):
    """Shape checks and packing of `moment_grouped`'s arguments (before the library is loaded): the arguments of
    `ffvd_op_moment_grouped` up to log_Qs, and the shapes."""
    G = len(U_vals)
    if G < 1:
        raise ValueError(f"{who}: at least one group is needed")
    one_model = len(kerns) > 0 and not isinstance(kerns[0], (list, tuple))
    if one_model:
        if np.ndim(Zs) != 2:
            raise ValueError(f"{who}: Zs: one list of kernels goes with one (M, P) array, got an array of {np.ndim(Zs)} dimensions")
        Zl, kl, Wl = [Zs], [kerns], [Lm_inverse_seqs]
    else:
        Zl, kl, Wl = list(Zs), list(kerns), list(Lm_inverse_seqs)
        if len(Zl) != len(kl) or len(Wl) != len(kl):
            raise ValueError(f"{who}: expected {len(kl)} models (one per kernel list), got {len(Zl)} Zs and {len(Wl)} Lm_inverse_seqs")
    nm = len(kl)
    if nm not in (1, G):
        raise ValueError(f"{who}: n_models: expected 1 or {G} (one per group of U_vals), got {nm}")
    hy = [stack_hypers(k) for k in kl]
    kind, D = hy[0][0], len(kl[0])
    Z0 = np.asarray(Zl[0])
    if Z0.ndim != 2:
        raise ValueError(f"{who}: Zs[0]: expected (M, P), got {Z0.shape}")
    M, P = Z0.shape
    if any(h[0] != kind for h in hy):
        raise ValueError(f"{who}: every group must use the same kernel type")
    _moment_limits(who, kind, M, P, D)
    C = P - D
    qm, S0, ctrl, steps = _moment_run_args(who, G, D, C, control_inputs, ctrl_offset, steps, S0s, q_mode)
    if len(x_lasts) != G:
        raise ValueError(f"{who}: x_lasts: expected {G} groups, got {len(x_lasts)}")
    Z, logvar, loglen = np.empty((nm, M, P)), np.empty((nm, D)), np.empty((nm, D, P))
    Wm, qmats = [], []                                   # (keeps the matrices alive until the call returns)
    for m in range(nm):
        if len(kl[m]) != D:
            raise ValueError(f"{who}: kerns[{m}]: expected {D} kernels (one per latent dim), got {len(kl[m])}")
        Z[m] = _lib.as_f64(Zl[m], (M, P), f"Zs[{m}]")
        logvar[m] = _lib.as_f64(hy[m][2], (D,), f"kerns[{m}] logvariance")
        loglen[m] = _lib.as_f64(hy[m][3], (D, P), f"kerns[{m}] loglengthscales")
        if len(Wl[m]) != D:
            raise ValueError(f"{who}: Lm_inverse_seqs[{m}]: expected {D} matrices, got {len(Wl[m])}")
        for d in range(D):
            Wm.append(_lib.as_f64(Wl[m][d], (M, M), f"Lm_inverse_seqs[{m}][{d}]"))
    f, xl = np.empty((G, M, D)), np.empty((G, D))
    for g in range(G):
        f[g] = _lib.as_f64(U_vals[g], (M, D), f"U_vals[{g}]")
        xl[g] = _lib.as_f64(x_lasts[g], (D,), f"x_lasts[{g}]")
    Qa = np.asarray(Qs, dtype=np.float64)
    if Qa.shape == (D,):
        Qa = np.broadcast_to(Qa, (G, D))
    if Qa.shape != (G, D):
        raise ValueError(f"{who}: Qs: expected {G} groups of ({D},), got {Qa.shape}")
    log_Q = np.ascontiguousarray(np.log(Qa))
    if q_sqrts is not None:
        if len(q_sqrts) != G:
            raise ValueError(f"{who}: q_sqrts: expected None or {G} groups, got {len(q_sqrts)}")
        for g in range(G):
            q = np.asarray(q_sqrts[g], dtype=np.float64)
            if q.shape != (D, M, M):
                raise ValueError(f"{who}: q_sqrts[{g}]: expected ({D}, {M}, {M}), got {q.shape}")
            qmats.extend(np.ascontiguousarray(q[d]) for d in (range(D) if qm else (0,)))
    import ctypes
    Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
    qt = (ctypes.c_void_p * len(qmats))(*[q.ctypes.data for q in qmats]) if q_sqrts is not None else None
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    args = (kind, G, nm, Wt, dp(Z), M, P, D, dp(logvar), dp(loglen), dp(f), qt, qm, dp(xl), opt(S0), opt(ctrl), C, steps, dp(log_Q))
    return dict(args=args, G=G, M=M, D=D, steps=steps, keep=(Wm, qmats, Z, logvar, loglen, f, xl, S0, ctrl, log_Q))


_NO_SUMMARY = (None, None, None, 0, None, 0, None, None, None, None, None)


def moment_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, *, S0s=None,
                   q_mode="reference"):
    """Moment-matched prediction of G posteriors in one call (`ffvd_op_moment_grouped`): the Gaussian state N(x_last, S0) of every
    group is pushed `steps` times through x' = x + f(x, c_t) + N(0, Q) in closed form and re-approximated as a Gaussian (Girard et
    al. 2003); nothing is sampled, one launch per step serves all groups.  SquaredExponential kernels only.

    `Zs` / `kerns` / `Lm_inverse_seqs`: one model (an (M, P) array, a list of D kernels, D upper-triangular matrices L^-T: shared by
    the groups) or length-G sequences of them; U_vals: G arrays (M, D), the whitened inducing outputs; q_sqrts: None (explicit U) or
    G stacks (D, M, M); q_mode "reference": slice 0 of a group's stack enters every dim's variance (what the rollouts
    do), "intent": slice d enters dim d; x_lasts: G start means (D,); S0s: None (zeros) or (G, D, D) symmetric start covariances;
    rows [ctrl_offset, ctrl_offset + steps) of control_inputs feed the steps; Qs: G vectors (D,) or one.
    Returns m_x (G, steps, D) and S_x (G, steps, D, D): mean and covariance of the state after each step, S_x exactly symmetric;
    group g's slabs are bit-identical to what a G = 1 call on that group alone returns."""
    who = "moment_grouped"
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode)
    G, D, steps = a["G"], a["D"], a["steps"]
    m_x, S_x = np.empty((G, steps, D)), np.empty((G, steps, D, D))
    rc = _lib.load().ffvd_op_moment_grouped(*a["args"], _lib.dptr(m_x), _lib.dptr(S_x), *_NO_SUMMARY)
    _lib.check(rc, None, who)
    return m_x, S_x


def _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass):
    """Shape checks and packing of `posterior_moment_grouped`'s arguments (before the library is loaded): the arguments of
    `ffvd_op_posterior_moment_grouped` up to steps, and the shapes."""
    a = pack_posterior_groups(Zs, kerns, Xs, control_inputs, Qs, who)
    G, nm, M, D, C = a["G"], a["n_models"], a["M"], a["D"], a["C"]
    _moment_limits(who, a["kind"], M, a["P"], D)
    if int(groups_per_pass) < 0:
        raise ValueError(f"{who}: groups_per_pass must be 0 (automatic) or positive")
    qm, S0, ctrl, steps = _moment_run_args(who, G, D, C, control_inputs, ctrl_offset, steps, S0s, q_mode)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    args = (a["kind"], G, nm, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]), dp(a["loglen"]), dp(a["X"]), opt(a["ctrl"]), C, a["T"],
            dp(a["log_Q"]), float(jitter), int(groups_per_pass), qm, opt(S0), opt(ctrl), steps)
    return dict(args=args, G=G, M=M, D=D, steps=steps, keep=(a, S0, ctrl))


def posterior_moment_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, *, S0s=None, q_mode="reference", jitter=JITTER,
                             groups_per_pass=0, return_U=False):
    """The collapsed posterior of G groups and its moment-matched prediction in ONE call (`ffvd_op_posterior_moment_grouped`): what
    `conditionals_multi_output.collapse_u_mean_grouped` followed by `moment_grouped` computes (q_sqrts = L_H^-T, x_lasts = Xs[g][-1]),
    without the posteriors leaving the device.  `Zs` / `kerns` / `Xs` / `Qs` / `control_inputs`: as `posterior_rollout_grouped`.
    Returns m_x (G, steps, D), S_x (G, steps, D, D) and, with return_U, U_means (G, M, D)."""
    who = "posterior_moment_grouped"
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass)
    G, M, D, steps = a["G"], a["M"], a["D"], a["steps"]
    m_x, S_x = np.empty((G, steps, D)), np.empty((G, steps, D, D))
    U = np.empty((G, M, D)) if return_U else None
    dp = _lib.dptr
    rc = _lib.load().ffvd_op_posterior_moment_grouped(*a["args"], dp(m_x), dp(S_x), None if U is None else dp(U), *_NO_SUMMARY)
    _lib.check(rc, None, who)
    return (m_x, S_x, U) if return_U else (m_x, S_x)


def moment_summary(m_x, S_x, CC, DD, log_Rchols, Y_test=None, Y_train_std=1.0):
    """The held-out predictive summary of a moment-matched prediction on the GPU (`ffvd_op_moment_summary`): the dict of
    `rollout_summary`, from Gaussian states instead of rollouts.  m_x (G, steps, D), S_x (G, steps, D, D); per output j and group g,
    m_gj = CC_j^T mu_g + DD_j and s2_gj = CC_j^T Sigma_g CC_j + exp(2 log_Rchols[0, j]); the groups are pooled with equal weights:
    predict_y = mean_g m, predict_y_var_total = mean_g (s2 + m^2) - predict_y^2, lpd = log mean_g N(y; m_g, s2_g) (a mixture of G
    Gaussians), lpd_gauss = log N(y; predict_y, predict_y_var_total).  predict_y_var and predict_y_var_total are BOTH the total
    variance: this method has no separate "reference variance" (the mean of one-step variances of `rollout_summary`)."""
    who = "moment_summary"
    m, S = _lib.as_f64(m_x), _lib.as_f64(S_x)
    if m.ndim != 3 or S.shape != m.shape + (m.shape[2],):
        raise ValueError(f"{who}: expected m_x (G, steps, D) and S_x (G, steps, D, D), got {m.shape} and {S.shape}")
    G, steps, D = m.shape
    if G < 1 or steps < 1 or not 1 <= D <= MOMENT_MAX_D:
        raise ValueError(f"{who}: at least one group, one step and 1 <= D <= {MOMENT_MAX_D} are needed, got {m.shape}")
    s = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    out, args = _summary_call(s, steps)
    rc = _lib.load().ffvd_op_moment_summary(_lib.dptr(m), _lib.dptr(S), G, steps, D, *args)
    _lib.check(rc, None, who)
    return _summary_dict(s, out, Y_train_std)


def moment_grouped_summary(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, CC, DD,
                           log_Rchols, Y_test=None, Y_train_std=1.0, *, S0s=None, q_mode="reference", return_moments=False):
    """`moment_grouped` and `moment_summary` in ONE call: the summary is formed on the device; m_x / S_x come down only with
    return_moments (keys m_x, S_x)."""
    who = "moment_grouped_summary"
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x_lasts, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode)
    G, D, steps = a["G"], a["D"], a["steps"]
    if steps < 1:
        raise ValueError(f"{who}: at least one step is needed")
    s = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    out, args = _summary_call(s, steps)
    m_x, S_x = (np.empty((G, steps, D)), np.empty((G, steps, D, D))) if return_moments else (None, None)
    opt = lambda x: None if x is None else _lib.dptr(x)
    rc = _lib.load().ffvd_op_moment_grouped(*a["args"], opt(m_x), opt(S_x), *args)
    _lib.check(rc, None, who)
    res = _summary_dict(s, out, Y_train_std)
    if return_moments:
        res.update(m_x=m_x, S_x=S_x)
    return res


def posterior_moment_grouped_summary(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, CC, DD, log_Rchols, Y_test=None,
                                     Y_train_std=1.0, *, S0s=None, q_mode="reference", jitter=JITTER, groups_per_pass=0,
                                     return_moments=False, return_U=False):
    """`posterior_moment_grouped` and `moment_summary` in ONE call: posteriors, propagation and summary stay on the device; m_x / S_x
    come down only with return_moments (keys m_x, S_x), U_means (G, M, D) only with return_U."""
    who = "posterior_moment_grouped_summary"
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass)
    G, M, D, steps = a["G"], a["M"], a["D"], a["steps"]
    if steps < 1:
        raise ValueError(f"{who}: at least one step is needed")
    s = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    out, args = _summary_call(s, steps)
    m_x, S_x = (np.empty((G, steps, D)), np.empty((G, steps, D, D))) if return_moments else (None, None)
    U = np.empty((G, M, D)) if return_U else None
    opt = lambda x: None if x is None else _lib.dptr(x)
    rc = _lib.load().ffvd_op_posterior_moment_grouped(*a["args"], opt(m_x), opt(S_x), opt(U), *args)
    _lib.check(rc, None, who)
    res = _summary_dict(s, out, Y_train_std)
    if return_moments:
        res.update(m_x=m_x, S_x=S_x)
    if return_U:
        res["U_means"] = U
    return res


def _filter_steps(who, Y_obs):
    """steps = len(Y_obs)"""
    shape = np.shape(Y_obs)
    if len(shape) not in (1, 2):
        raise ValueError(f"{who}: Y_obs: expected (steps, J), got {shape}")
    return shape[0]


def _pack_filter(who, D, Y_obs, CC, DD, log_Rchols):
    """Shape checks of the observations and the emission of the filter (before the library is loaded): `_pack_summary` with
    steps = len(Y_obs); NaN marks an unobserved entry, an infinity is rejected."""
    m = _pack_summary(who, D, _filter_steps(who, Y_obs), CC, DD, log_Rchols, Y_obs)
    if np.any(np.isinf(m["Y"])):
        raise ValueError(f"{who}: Y_obs: an infinite observation (NaN marks an unobserved entry)")
    return m


FILTER_METHODS = ("moment", "linearised")


def _filter_method(who, method, forecast=False):
    """The propagation rule of the filter family, checked in the packing stage (before the library is loaded): "moment" (moment
    matching, the default) or "linearised" (the extended Kalman rule, `filter_grouped`).  The forecast functions that take `method` accept "moment" only; the
    linearised forecasts are `forecast_linear_grouped` / `posterior_forecast_linear_grouped`."""
    if not isinstance(method, str) or method not in FILTER_METHODS:
        raise ValueError(f"{who}: method: expected one of {list(FILTER_METHODS)}, got {method!r}")
    if forecast and method != "moment":
        raise ValueError(f"{who}: method: the forecast fan is built for \"moment\" only (accepted by the filters: "
                         f"{list(FILTER_METHODS)}), got {method!r}")
    return method


def _filter_call(m, G, D, steps, smooth):
    """Output arrays and the trailing arguments (CC .. lpd_gauss) of the two filter entry points."""
    J, dp = m["J"], _lib.dptr
    out = dict(m_pred=np.empty((G, steps, D)), S_pred=np.empty((G, steps, D, D)), m_filt=np.empty((G, steps, D)),
               S_filt=np.empty((G, steps, D, D)), cross=np.empty((G, steps, D, D)), lpd=np.empty((G, steps, J)),
               lpd_joint=np.empty((G, steps)))
    if smooth:
        out.update(m_smooth=np.empty((G, steps, D)), S_smooth=np.empty((G, steps, D, D)))
    out.update(predict_y=np.empty((steps, J)), predict_y_var_total=np.empty((steps, J)), lpd_mix=np.empty((steps, J)),
               lpd_gauss=np.empty((steps, J)))
    names = ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "lpd", "lpd_joint", "m_smooth", "S_smooth", "predict_y",
             "predict_y_var_total", "lpd_mix", "lpd_gauss")
    args = (dp(m["CC"]), dp(m["DD"]), dp(m["sd"]), J, dp(m["Y"])) + tuple(dp(out[k]) if k in out else None for k in names)
    return out, args


def _filter_dict(m, out, Y_train_std):
    """The dict the filter functions return: the arrays of `_filter_call` and the scalars ll (mean of lpd_mix over the observed
    entries), ll_joint (mean over the rows with an observed entry of log mean_g exp(lpd_joint[g, i]), largest exponent subtracted),
    ll_original_units (ll - log Y_train_std) and RMSE (one-step-ahead, observed entries of the first 30 rows, times Y_train_std)."""
    res = dict(out)
    res.update(_filter_scalars(m["Y"], out["lpd_mix"], out["lpd_joint"], out["predict_y"], Y_train_std))
    return res


def _filter_scalars(Y, lpd_mix, lpd_joint, predict_y, Y_train_std):
    """The scalars of `_filter_dict` for one record: Y, lpd_mix, predict_y (steps, J), lpd_joint (G, steps)."""
    nan = float("nan")
    seen = ~np.isnan(Y)
    ll = float(np.mean(lpd_mix[seen])) if np.any(seen) else nan
    rows = np.any(seen, axis=1)
    ll_joint = nan
    if np.any(rows):
        lj = lpd_joint[:, rows]
        mx = np.max(lj, axis=0)
        ll_joint = float(np.mean(mx + np.log(np.mean(np.exp(lj - mx[None, :]), axis=0))))
    s30 = seen[:30]
    rmse = float(np.sqrt(np.mean((Y[:30][s30] - predict_y[:30][s30]) ** 2)) * Y_train_std) if np.any(s30) else nan
    return dict(ll=ll, ll_joint=ll_joint, ll_original_units=ll - float(np.log(Y_train_std)), RMSE=rmse)


def filter_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols, *,
                   S0s=None, q_mode="reference", smooth=False, Y_train_std=1.0, method="moment"):
    """Gaussian filtering (and, with `smooth`, RTS smoothing) of an observed sequence through G posteriors in one call
    (`ffvd_op_filter_grouped`): `moment_grouped`'s step with a measurement update after every step -- assumed-density filtering by
    moment matching (Deisenroth et al. 2012).  The state after step i emits row i of Y_obs (steps, J): y = CC^T x + DD + noise of
    standard deviation exp(log_Rchols[0, :]); a NaN entry is unobserved (an all-NaN row is a prediction step; trailing all-NaN rows
    forecast from the filtered state).  Every group starts from N(x0s[g], S0s[g]) (S0s None: zeros); the other arguments are
    `moment_grouped`'s, rows [ctrl_offset, ctrl_offset + steps) of control_inputs feed the steps.
    Returns a dict.  Per group: m_pred (G, steps, D), S_pred (G, steps, D, D): the state before row i is seen; m_filt, S_filt:
    after; cross (G, steps, D, D): Cov(x_{i-1}, x_i | y_{0:i-1}), row = component of x_{i-1}; lpd (G, steps, J):
    log p(y_ij | y_{0:i-1}) per entry (marginal), lpd_joint (G, steps): of the observed entries of row i jointly (NaN where
    unobserved); with smooth: m_smooth, S_smooth (the start state is not smoothed).  Pooled over the groups with EQUAL weights (the
    chains are not re-weighted by their likelihoods), one step ahead, (steps, J): predict_y, predict_y_var_total, lpd_mix,
    lpd_gauss.  Scalars: ll, ll_joint, ll_original_units, RMSE (`_filter_dict`).  Every covariance is exactly symmetric; group g's
    arrays are bit-identical to a G = 1 call on that group.
    method "linearised" (`ffvd_op_filter_linear_grouped`): the extended Kalman rule in place of moment matching -- the transition
    is linearised at the filtered mean mu: with m, v the mean and variance of the GP conditional at [mu, c_i] and J the Jacobian of
    m with respect to the state, A = I + J: m_pred = mu + m, S_pred = A S A^T + diag(v + Q), cross = S A^T.  Same update, densities,
    smoother, pooled arrays and guarantees; much cheaper per step, and first order in S where moment matching is exact for the
    Gaussian ("Linearised filtering")."""
    who = "filter_grouped"
    method = _filter_method(who, method)
    steps = _filter_steps(who, Y_obs)
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode)
    m = _pack_filter(who, a["D"], Y_obs, CC, DD, log_Rchols)
    out, args = _filter_call(m, a["G"], a["D"], steps, smooth)
    lib = _lib.load()
    rc = (lib.ffvd_op_filter_linear_grouped if method == "linearised" else lib.ffvd_op_filter_grouped)(*a["args"], *args)
    _lib.check(rc, None, who)
    return _filter_dict(m, out, Y_train_std)


def posterior_filter_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, *, x0s=None, S0s=None,
                             q_mode="reference", smooth=False, Y_train_std=1.0, jitter=JITTER, groups_per_pass=0, method="moment"):
    """The collapsed posterior of G groups and the filter of `filter_grouped` in ONE call (`ffvd_op_posterior_filter_grouped`): what
    `conditionals_multi_output.collapse_u_mean_grouped` followed by `filter_grouped` computes, without the posteriors leaving the
    device.  x0s None: the start means are Xs[g][-1] (the record continues the training sequence), else (G, D).  `Zs` / `kerns` /
    `Xs` / `Qs` / `control_inputs`: as `posterior_moment_grouped`.  method: as `filter_grouped` ("linearised":
    `ffvd_op_posterior_filter_linear_grouped`).  Returns the dict of `filter_grouped`."""
    who = "posterior_filter_grouped"
    method = _filter_method(who, method)
    steps = _filter_steps(who, Y_obs)
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass)
    m = _pack_filter(who, a["D"], Y_obs, CC, DD, log_Rchols)
    x0 = None if x0s is None else _lib.as_f64(x0s, (a["G"], a["D"]), "x0s")
    out, args = _filter_call(m, a["G"], a["D"], steps, smooth)
    pre = a["args"][:17] + (None if x0 is None else _lib.dptr(x0),) + a["args"][17:]
    lib = _lib.load()
    rc = (lib.ffvd_op_posterior_filter_linear_grouped if method == "linearised" else lib.ffvd_op_posterior_filter_grouped)(*pre, *args, None)
    _lib.check(rc, None, who)
    return _filter_dict(m, out, Y_train_std)


def _pack_records(who, G, D, C, x0s, control_records, Y_records, lengths, S0s, records_per_pass):
    """Shape checks and packing of the record arguments of `filter_records_grouped` (before the library is loaded).  Returns a dict:
    R, steps, J, Y (R, steps, J), ctrl (R, steps, C) or None, x0 (G, R, D) or None (x0s None), S0 (G, R, D, D) or None, lengths (R,),
    live (R, steps) bool (row < lengths[r]), rpp.  The control rows beyond a record's length are zeros in ctrl."""
    Y = np.asarray(Y_records, dtype=np.float64)
    if Y.ndim != 3 or Y.shape[0] < 1 or Y.shape[1] < 1:
        raise ValueError(f"{who}: Y_records: expected (R, steps, J) with at least one record and one row, got {Y.shape}")
    R, steps, J = Y.shape
    Y = np.ascontiguousarray(Y)
    if np.any(np.isinf(Y)):
        raise ValueError(f"{who}: Y_records: an infinite observation (NaN marks an unobserved entry)")
    if isinstance(records_per_pass, bool) or int(records_per_pass) != records_per_pass or int(records_per_pass) < 0:
        raise ValueError(f"{who}: records_per_pass must be 0 (automatic) or a positive integer, got {records_per_pass!r}")
    if lengths is None:
        ln = np.full(R, steps, dtype=np.int64)
    else:
        la = np.asarray(lengths)
        if la.shape != (R,) or not (np.issubdtype(la.dtype, np.integer) or np.array_equal(la, np.floor(la))):
            raise ValueError(f"{who}: lengths: expected {R} integers (one per record), got {lengths!r}")
        ln = la.astype(np.int64)
        if np.any(ln < 1) or np.any(ln > steps):
            raise ValueError(f"{who}: lengths: every record needs between 1 and {steps} rows, got {ln.tolist()}")
    live = np.arange(steps)[None, :] < ln[:, None]
    if not np.all(np.isnan(Y[~live])):
        raise ValueError(f"{who}: Y_records: the rows of a record at and beyond its length must be all NaN")
    ctrl = None
    if C > 0:
        if control_records is None:
            raise ValueError(f"{who}: control_records: the model has {C} control columns, expected ({R}, {steps}, {C})")
        ctrl = np.array(_lib.as_f64(control_records, (R, steps, C), "control_records"))
        ctrl[~live] = 0.0
        if not np.all(np.isfinite(ctrl)):
            raise ValueError(f"{who}: control_records: every control row inside a record's length must be finite")
    elif control_records is not None and np.size(control_records) != 0:
        raise ValueError(f"{who}: control_records: the model has no control columns, expected None")
    x0 = None
    if x0s is not None:
        x = np.asarray(x0s, dtype=np.float64)
        if x.shape == (R, D):
            x = np.broadcast_to(x, (G, R, D))
        if x.shape != (G, R, D):
            raise ValueError(f"{who}: x0s: expected ({R}, {D}) or ({G}, {R}, {D}), got {x.shape}")
        x0 = np.ascontiguousarray(x)
    S0 = None
    if S0s is not None:
        s = np.asarray(S0s, dtype=np.float64)
        if s.shape == (R, D, D):
            s = np.broadcast_to(s, (G, R, D, D))
        if s.shape != (G, R, D, D):
            raise ValueError(f"{who}: S0s: expected None, ({R}, {D}, {D}) or ({G}, {R}, {D}, {D}), got {s.shape}")
        if not np.all(np.isfinite(s)) or not np.array_equal(s, np.swapaxes(s, -1, -2)):
            raise ValueError(f"{who}: S0s: every start covariance must be finite and exactly symmetric")
        S0 = np.ascontiguousarray(s)
    return dict(R=R, steps=steps, J=J, Y=Y, ctrl=ctrl, x0=x0, S0=S0, lengths=ln, live=live, rpp=int(records_per_pass))


def _records_placeholders(G, Zs, kerns, steps):
    """Start means (G, D) and control rows (steps, C) of zeros for `_pack_moment_groups`, whose x_lasts / control_inputs slots the
    records replace.  A malformed model gives empty ones: `_pack_moment_groups`' own checks raise."""
    try:
        one = not isinstance(kerns[0], (list, tuple))
        D = len(kerns) if one else len(kerns[0])
        P = np.shape(Zs if one else Zs[0])[1]
    except (IndexError, TypeError):
        D, P = 0, 0
    return np.zeros((G, D)), np.zeros((steps, max(P - D, 0)))


def _records_dict(r, G, out, Y_train_std):
    """The dict `filter_records_grouped` returns, from the arrays of `_filter_call` over R * steps rows: per track (G, R, steps, ...),
    pooled (R, steps, J), NaN in the rows at and beyond a record's length; per record, as arrays (R,): the scalars of `_filter_dict`;
    ll_all: the mean of lpd_mix over every observed entry of every record."""
    R, steps, J, live = r["R"], r["steps"], r["J"], r["live"]
    res, dead = {}, ~live
    for k, v in out.items():
        if k in FORECAST_POOLED:
            res[k] = v.reshape(R, steps, J)
            res[k][dead] = np.nan
        else:
            res[k] = v.reshape((G, R, steps) + v.shape[2:])
            res[k][:, dead] = np.nan
    Y = r["Y"]
    per = [_filter_scalars(Y[i], res["lpd_mix"][i], res["lpd_joint"][:, i], res["predict_y"][i], Y_train_std) for i in range(R)]
    for k in ("ll", "ll_joint", "ll_original_units", "RMSE"):
        res[k] = np.array([p[k] for p in per])
    seen = ~np.isnan(Y)
    res["ll_all"] = float(np.mean(res["lpd_mix"][seen])) if np.any(seen) else float("nan")
    return res


def filter_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols, *,
                           lengths=None, S0s=None, q_mode="reference", smooth=False, Y_train_std=1.0, records_per_pass=0):
    """Linearised (extended Kalman) filtering and, with `smooth`, RTS smoothing of R observed records -- trials, held-out segments,
    cross-validation folds -- through G posteriors in ONE call (`ffvd_op_filter_records_grouped`).  A track (group g, record r) is an
    independent filter of `filter_grouped(method="linearised")`: it runs on the posterior of group g and reads the observations
    Y_records[r] (Y_records (R, steps, J), NaN = unobserved), the control rows control_records[r] (control_records (R, steps, C),
    None when the model has no controls) and starts from N(x0s[g, r], S0s[g, r]).  x0s: (R, D), shared by the groups, or (G, R, D);
    S0s: None (zeros), (R, D, D) or (G, R, D, D).  lengths: None, or (R,) integers in [1, steps] for records of different length:
    rows >= lengths[r] of record r must be all NaN in Y_records; their control rows are not read (zeros are sent), every returned
    array is NaN there and they take no part in any scalar.  The other arguments are `filter_grouped`'s; the posteriors are prepared
    once, the tracks of a pass advance in one launch pair per step (records_per_pass 0: automatic, otherwise at most that many
    records together), and the quadratic forms of all tracks that share a Gamma are one product on the fp64 matrix cores.
    Returns a dict.  Per track, (G, R, steps, ...): m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, with smooth m_smooth,
    S_smooth (as `filter_grouped`, the leading (G, steps) replaced by (G, R, steps)).  Pooled over the groups with EQUAL weights,
    (R, steps, J): predict_y, predict_y_var_total, lpd_mix, lpd_gauss.  Per record, arrays (R,): ll, ll_joint, ll_original_units,
    RMSE (`_filter_dict`'s definitions on that record); ll_all: the mean of lpd_mix over the observed entries of all records.
    A track's arrays are bit-identical whatever the other groups, the other records, their order and records_per_pass are; every
    covariance is exactly symmetric; against `filter_grouped(method="linearised")` on the same record the arrays agree to rounding,
    not bit for bit ("Filtering many records").  SquaredExponential kernels only; moment matching over records
    is not built."""
    return _filter_records_given("filter_records_grouped", "ffvd_op_filter_records_grouped", Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s,
                                 control_records, Y_records, Qs, CC, DD, log_Rchols, lengths, S0s, q_mode, smooth, Y_train_std, records_per_pass)


def _filter_records_given(who, entry, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                          lengths, S0s, q_mode, smooth, Y_train_std, records_per_pass):
    """The body of `filter_records_grouped` and `filter_cubature_records_grouped`: `entry` is the symbol of the library."""
    shape = np.shape(Y_records)
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: Y_records: expected (R, steps, J) with at least one record and one row, got {shape}")
    G = len(U_vals)
    if x0s is None:
        raise ValueError(f"{who}: x0s: the start means are needed, ({shape[0]}, D) or ({G}, {shape[0]}, D)")
    # the model arguments through `_pack_moment_groups`, with placeholders in the three slots the records replace (x_lasts, S0s, ctrl)
    xl, ci = _records_placeholders(G, Zs, kerns, shape[1])
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, xl, ci, 0, shape[1], Qs, None, q_mode)
    D, args = a["D"], a["args"]
    r = _pack_records(who, G, D, args[16], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, fargs = _filter_call(m, G, D, R * steps, smooth)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = getattr(_lib.load(), entry)(*args[:13], R, dp(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), *args[16:], *fargs[:5], r["rpp"], *fargs[5:])
    _lib.check(rc, None, who)
    return _records_dict(r, G, out, Y_train_std)


def posterior_filter_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, *, lengths=None,
                                     x0s=None, S0s=None, q_mode="reference", smooth=False, Y_train_std=1.0, jitter=JITTER,
                                     groups_per_pass=0, records_per_pass=0):
    """The collapsed posterior of G groups and the filter of `filter_records_grouped` in ONE call
    (`ffvd_op_posterior_filter_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `filter_records_grouped` computes, without the posteriors leaving the device.  `Zs` / `kerns` / `Xs` / `Qs` / `control_inputs`
    (the training controls the posteriors are formed with) / jitter / groups_per_pass: as `posterior_filter_grouped`; control_records,
    Y_records, lengths, S0s, records_per_pass: as `filter_records_grouped`; x0s None: every record of group g starts at Xs[g][-1],
    else (R, D) or (G, R, D).  Returns the dict of `filter_records_grouped`."""
    return _filter_records_posterior("posterior_filter_records_grouped", "ffvd_op_posterior_filter_records_grouped", Zs, kerns, Xs, Qs,
                                     control_inputs, control_records, Y_records, CC, DD, log_Rchols, lengths, x0s, S0s, q_mode, smooth, Y_train_std,
                                     jitter, groups_per_pass, records_per_pass)


def _filter_records_posterior(who, entry, Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, lengths, x0s, S0s,
                              q_mode, smooth, Y_train_std, jitter, groups_per_pass, records_per_pass):
    """The body of `posterior_filter_records_grouped` and `posterior_filter_cubature_records_grouped`: `entry` is the symbol of the library."""
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, 0, 0, None, q_mode, jitter, groups_per_pass)
    G, D, args = a["G"], a["D"], a["args"]
    r = _pack_records(who, G, D, args[11], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, fargs = _filter_call(m, G, D, R * steps, smooth)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = getattr(_lib.load(), entry)(*args[:17], R, opt(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), steps, *fargs[:5], r["rpp"], *fargs[5:], None)
    _lib.check(rc, None, who)
    return _records_dict(r, G, out, Y_train_std)


def filter_cubature_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols, *,
                                    lengths=None, S0s=None, q_mode="reference", smooth=False, Y_train_std=1.0, records_per_pass=0):
    """Cubature (sigma-point) filtering and, with `smooth`, RTS smoothing of R observed records through G posteriors in ONE call
    (`ffvd_op_filter_cubature_records_grouped`): `filter_records_grouped` -- its tracks, timing, emission, measurement update,
    densities, smoother, pooled arrays, per-record scalars, parameters, checks, defaults and returned dict -- with the third-degree
    spherical cubature rule (Arasaratnam & Haykin 2009) as the propagation.  Per step, with (mu, S) the filtered state, c the
    record's control row and w = 1 / (2D): L is the lower Cholesky factor of S without pivoting (a pivot <= 0 gives a zero column, so
    S = 0 and a rank-deficient S are allowed); the 2D points are x_i = [mu + dx_i, c] with dx_i = +sqrt(D) (column i of L) and
    dx_{i+D} = -dx_i (the control columns are not spread); with m(x_i), v(x_i) the mean and variance of the GP conditional there,
    mbar = w sum_i m(x_i), Cov(f) = w sum_i (m(x_i) - mbar)(m(x_i) - mbar)^T + diag(w sum_i v(x_i)), V = w sum_i dx_i (m(x_i) - mbar)^T:
    m_pred = mu + mbar, S_pred = S + Cov(f) + V + V^T + diag(Q), cross = S + V.  Its one-step difference from moment matching is
    second order in S where the linearised rule's is first order, so its latent states follow moment matching's far more closely,
    at 2D kernel rows per (track, dim) in the same product on the fp64 matrix cores ("Cubature filtering").
    The guarantees of `filter_records_grouped` hold: pooled with EQUAL weights; a track's arrays are bit-identical whatever the other
    groups, the other records, their order and records_per_pass are; every covariance is exactly symmetric.  From S = 0 a step is the
    conditional at [mu, c] and its `cross` is exact zeros.  SquaredExponential kernels only; R = 1 is a valid single-record call."""
    return _filter_records_given("filter_cubature_records_grouped", "ffvd_op_filter_cubature_records_grouped", Lm_inverse_seqs, Zs, kerns, U_vals,
                                 q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols, lengths, S0s, q_mode, smooth, Y_train_std,
                                 records_per_pass)


def posterior_filter_cubature_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, *, lengths=None,
                                              x0s=None, S0s=None, q_mode="reference", smooth=False, Y_train_std=1.0, jitter=JITTER,
                                              groups_per_pass=0, records_per_pass=0):
    """The collapsed posterior of G groups and the filter of `filter_cubature_records_grouped` in ONE call
    (`ffvd_op_posterior_filter_cubature_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `filter_cubature_records_grouped` computes, without the posteriors leaving the device.  The arguments are
    `posterior_filter_records_grouped`'s; returns the dict of `filter_records_grouped`."""
    return _filter_records_posterior("posterior_filter_cubature_records_grouped", "ffvd_op_posterior_filter_cubature_records_grouped", Zs, kerns,
                                     Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, lengths, x0s, S0s, q_mode, smooth,
                                     Y_train_std, jitter, groups_per_pass, records_per_pass)


PARTICLE_MIN_N, PARTICLE_MAX_N = 2, 2048
PARTICLE_KEYS = ("m_pred", "S_pred", "m_filt", "S_filt", "lpd", "lpd_joint", "predict_y", "predict_y_var_total", "lpd_mix", "lpd_gauss", "ess")


def _particle_layout(who, name, x, tail, G, R):
    """One of the three layouts of a draw array: tail (shared by groups and records), (R,) + tail (shared by the groups) or
    (G, R) + tail.  Returns the contiguous array and its (group, record) strides in doubles (0 = shared)."""
    a = np.asarray(x, dtype=np.float64)
    inner = int(np.prod(tail, dtype=np.int64))
    if a.shape == tuple(tail):
        sg, sr = 0, 0
    elif a.shape == (R,) + tuple(tail):
        sg, sr = 0, inner
    elif a.shape == (G, R) + tuple(tail):
        sg, sr = R * inner, inner
    else:
        raise ValueError(f"{who}: {name}: expected {tuple(tail)}, {(R,) + tuple(tail)} or {(G, R) + tuple(tail)}, got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: {name}: every draw must be finite")
    return np.ascontiguousarray(a), sg, sr


def _pack_particles(who, G, R, steps, D, eps, unif, xi0, with_S0, return_particles):
    """Shape and value checks of the draws of `filter_particle_records_grouped` (before the library is loaded): N from eps, the three
    layouts of eps / unif / xi0, unif in [0, 1), xi0 exactly when S0s is given.  Returns N and the arguments N .. xi0_stride_r."""
    e = np.asarray(eps, dtype=np.float64)
    if e.ndim not in (3, 4, 5) or e.shape[-1] != D:
        raise ValueError(f"{who}: eps: expected ({steps}, N, {D}), ({R}, {steps}, N, {D}) or ({G}, {R}, {steps}, N, {D}), got {e.shape}")
    N = e.shape[-2]
    if not PARTICLE_MIN_N <= N <= PARTICLE_MAX_N:
        raise ValueError(f"{who}: eps: the number of particles N must lie in [{PARTICLE_MIN_N}, {PARTICLE_MAX_N}], got {N}")
    e, eg, er = _particle_layout(who, "eps", e, (steps, N, D), G, R)
    u, ug, ur = _particle_layout(who, "unif", unif, (steps,), G, R)
    if np.any(u < 0.0) or np.any(u >= 1.0):
        raise ValueError(f"{who}: unif: every uniform must lie in [0, 1)")
    if with_S0 != (xi0 is not None):
        raise ValueError(f"{who}: xi0: the start draws ({N}, {D}) are needed exactly when S0s is given (S0s "
                         f"{'given' if with_S0 else 'None'}, xi0 {'None' if xi0 is None else 'given'})")
    x, xg, xr = (None, 0, 0) if xi0 is None else _particle_layout(who, "xi0", xi0, (N, D), G, R)
    if not isinstance(return_particles, (bool, np.bool_)):
        raise ValueError(f"{who}: return_particles: expected a bool, got {return_particles!r}")
    if G * R * steps * N * D >= 2 ** 31:
        raise ValueError(f"{who}: G * R * steps * N * D = {G * R * steps * N * D} must stay below 2^31")
    dp = _lib.dptr
    return N, (N, dp(e), eg, er, dp(u), ug, ur, None if x is None else dp(x), xg, xr), (e, u, x)


def _particle_call(m, G, R, steps, D, N, return_particles):
    """Output arrays and the trailing arguments (m_pred .. ancestors) of the two particle entry points."""
    J, V, dp = m["J"], G * R * steps, _lib.dptr
    out = dict(m_pred=np.empty((G, R * steps, D)), S_pred=np.empty((G, R * steps, D, D)), m_filt=np.empty((G, R * steps, D)),
               S_filt=np.empty((G, R * steps, D, D)), lpd=np.empty((G, R * steps, J)), lpd_joint=np.empty((G, R * steps)),
               predict_y=np.empty((R * steps, J)), predict_y_var_total=np.empty((R * steps, J)), lpd_mix=np.empty((R * steps, J)),
               lpd_gauss=np.empty((R * steps, J)), ess=np.empty((G, R * steps)))
    extra = dict(log_evidence=np.empty((G, R)))
    if return_particles:
        extra.update(particles=np.empty((G, R, steps, N, D)), ancestors=np.empty((G, R, steps, N), dtype=np.int32))
    import ctypes
    anc = extra["ancestors"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if return_particles else None
    args = tuple(dp(out[k]) for k in PARTICLE_KEYS) + (dp(extra["log_evidence"]), dp(extra["particles"]) if return_particles else None, anc)
    return out, extra, args


def _particle_dict(r, G, out, extra, Y_train_std):
    """`_records_dict` plus log_evidence (G, R) and, when asked for, particles / ancestors: NaN (ancestors -1) at and beyond a
    record's length."""
    res = _records_dict(r, G, out, Y_train_std)
    res["log_evidence"] = extra["log_evidence"]
    dead = ~r["live"]
    if "particles" in extra:
        extra["particles"][:, dead] = np.nan
        extra["ancestors"][:, dead] = -1
        res.update(particles=extra["particles"], ancestors=extra["ancestors"])
    return res


def filter_particle_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                    eps, unif, *, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0,
                                    return_particles=False):
    """Bootstrap particle filtering of R observed records through G posteriors in ONE call (`ffvd_op_filter_particle_records_grouped`):
    the fourth records filter, and the only one that does not project the predictive state onto a Gaussian -- it is exact as N grows,
    keeps a non-Gaussian (multi-modal) filtered state and gives the unbiased SMC estimate of the held-out evidence per chain and
    record.  Tracks (group g, record r), passes, `lengths`, NaN = unobserved, timing (the state after step i emits row i), emission,
    staging and q_mode are `filter_records_grouped`'s.  Every random draw is the caller's: eps (steps, N, D), (R, steps, N, D) or
    (G, R, steps, N, D) standard normal (the first two are common random numbers across groups, or across groups and records: each
    track's estimator stays unbiased), unif (steps,), (R, steps) or (G, R, steps) in [0, 1), xi0 (N, D), (R, N, D) or (G, R, N, D)
    standard normal, needed exactly when S0s is given.  N = eps.shape[-2], 2 <= N <= 2048.
    Per track: X_0i = x0 + L0 xi0_i (L0 the unpivoted lower Cholesky factor of S0, a pivot <= 0 gives a zero column; S0s None: all at
    x0).  Step t: with (m_i, v_i) the GP conditional of the group at [X_ti, c_t], X^-_i = X_ti + m_i + eps[t, i] sqrt(v_i + Q);
    m_pred, S_pred: mean and centred covariance of the X^-; l_ij = log N(y_tj; CC[:, j] . X^-_i + DD_j, sd_j^2), lpd[t, j] =
    log mean_i exp l_ij (NaN where unobserved), L_i the sum of l_ij over the observed j, lpd_joint[t] = log mean_i exp L_i (NaN for a
    row with nothing observed); W_i = exp(L_i - max L), m_filt / S_filt the W-weighted mean and centred covariance, ess =
    (sum W)^2 / sum W^2; systematic resampling with unif[t], a_i = min(#{k: cdf_k <= (unif[t] + i) / N cdf_{N-1}}, N - 1), only for
    a row with an observed entry (otherwise the particles are kept, m_filt = m_pred and S_filt = S_pred bit for bit, ess = N).  No
    adaptive resampling in this call: `filter_adaptive_records_grouped` resamples only where the ESS falls below a threshold and
    equals this call bit for bit with a threshold above 1.  There is no smoothing (no `smooth` parameter, no `cross`): particle smoothing is not built into
    this call, `smooth_particle_records_grouped` has it.
    Returns the dict of `filter_records_grouped` without cross, m_smooth and S_smooth, plus ess (G, R, steps) and log_evidence (G, R),
    the sum of lpd_joint over the rows with an observation: the SMC estimate of log p(y) of that record under that chain.  Pooled
    with EQUAL weights, (R, steps, J): predict_y, predict_y_var_total and lpd_gauss from (m_pred, S_pred) as the siblings; lpd_mix =
    log mean_g exp(lpd[g]), the density of the mixture of all G N particles' emissions.  With return_particles also particles
    (G, R, steps, N, D), the X^-, and ancestors (G, R, steps, N) int32.  Every array is NaN (ancestors -1) at and beyond a record's
    length.  A track's arrays are bit-identical whatever the other groups, the other records, their order and records_per_pass are
    (draws permuted with them); every covariance is exactly symmetric ("Particle filtering").  SquaredExponential
    kernels only; R = 1 is a valid single-record call."""
    return _particle_records_given("filter_particle_records_grouped", False, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass,
                                   return_particles)


def _particle_records_given(who, smooth, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                            eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass, return_particles, unif_bs=None,
                            adapted=False):
    """The body of `filter_particle_records_grouped`, with `smooth` of `smooth_particle_records_grouped`, with `smooth` and
    `unif_bs` of `backsim_particle_records_grouped`, and with `adapted` of `filter_adapted_records_grouped`."""
    shape = np.shape(Y_records)
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: Y_records: expected (R, steps, J) with at least one record and one row, got {shape}")
    G = len(U_vals)
    if x0s is None:
        raise ValueError(f"{who}: x0s: the start means are needed, ({shape[0]}, D) or ({G}, {shape[0]}, D)")
    xl, ci = _records_placeholders(G, Zs, kerns, shape[1])
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, xl, ci, 0, shape[1], Qs, None, q_mode)
    D, args = a["D"], a["args"]
    r = _pack_records(who, G, D, args[16], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    N, pargs, keep = _pack_particles(who, G, R, steps, D, eps, unif, xi0, r["S0"] is not None, return_particles)
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, extra, oargs = _particle_call(m, G, R, steps, D, N, bool(return_particles))
    sm, sargs = _smooth_or_backsim_call(who, r, G, D, N, bool(return_particles), smooth, unif_bs, adapted)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rule = "particle_adapted" if adapted else "particle"
    entry = f"ffvd_{rule}_{'smooth' if unif_bs is None else 'backsim'}_records_grouped" if smooth else \
        "ffvd_particle_adapted_records_grouped" if adapted else "ffvd_op_filter_particle_records_grouped"
    rc = getattr(_lib.load(), entry)(*args[:13], R, dp(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), *args[16:], dp(m["CC"]), dp(m["DD"]), dp(m["sd"]),
                                     m["J"], dp(m["Y"]), r["rpp"], *pargs, *oargs, *sargs)
    _lib.check(rc, None, who)
    return _smooth_dict(_particle_dict(r, G, out, extra, Y_train_std), r, sm)


def posterior_filter_particle_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, *,
                                              xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0, jitter=JITTER,
                                              groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and the filter of `filter_particle_records_grouped` in ONE call
    (`ffvd_op_posterior_filter_particle_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `filter_particle_records_grouped` computes, without the posteriors leaving the device.  The model and start arguments are
    `posterior_filter_records_grouped`'s (x0s None: every record of group g starts at Xs[g][-1]); eps, unif, xi0, return_particles and
    the returned dict are `filter_particle_records_grouped`'s."""
    return _particle_records_posterior("posterior_filter_particle_records_grouped", False, Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles)


def _particle_records_posterior(who, smooth, Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, xi0,
                                lengths, x0s, S0s, q_mode, Y_train_std, jitter, groups_per_pass, records_per_pass, return_particles,
                                unif_bs=None, adapted=False):
    """The body of `posterior_filter_particle_records_grouped`, with `smooth` of `posterior_smooth_particle_records_grouped`, with
    `smooth` and `unif_bs` of `posterior_backsim_particle_records_grouped`, and with `adapted` of
    `posterior_filter_adapted_records_grouped`."""
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, 0, 0, None, q_mode, jitter, groups_per_pass)
    G, D, args = a["G"], a["D"], a["args"]
    r = _pack_records(who, G, D, args[11], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    N, pargs, keep = _pack_particles(who, G, R, steps, D, eps, unif, xi0, r["S0"] is not None, return_particles)
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, extra, oargs = _particle_call(m, G, R, steps, D, N, bool(return_particles))
    sm, sargs = _smooth_or_backsim_call(who, r, G, D, N, bool(return_particles), smooth, unif_bs, adapted)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rule = "particle_adapted" if adapted else "particle"
    entry = f"ffvd_posterior_{rule}_{'smooth' if unif_bs is None else 'backsim'}_records_grouped" \
        if smooth else "ffvd_posterior_particle_adapted_records_grouped" if adapted else "ffvd_op_posterior_filter_particle_records_grouped"
    rc = getattr(_lib.load(), entry)(*args[:17], R, opt(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), steps, dp(m["CC"]), dp(m["DD"]), dp(m["sd"]),
                                     m["J"], dp(m["Y"]), r["rpp"], *pargs, *oargs, *sargs, None)
    _lib.check(rc, None, who)
    return _smooth_dict(_particle_dict(r, G, out, extra, Y_train_std), r, sm)


def filter_adapted_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                   eps, unif, *, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0,
                                   return_particles=False):
    """Fully adapted particle filtering of R observed records through G posteriors in ONE call
    (`ffvd_particle_adapted_records_grouped`): `filter_particle_records_grouped` with the optimal proposal in place of the bootstrap
    one (the fully adapted auxiliary particle filter of Pitt & Shephard 1999).  Given the parent particle the transition is Gaussian
    with a diagonal covariance and the emission is linear-Gaussian, so p(y_t | parent) and p(x_t | parent, y_t) are closed forms: the
    parents are weighted by how well they predict y_t BEFORE anything is drawn, resampled, and the children are drawn from the
    optimal proposal; the new set is equally weighted.  Where the observations are informative the bootstrap filter collapses onto a
    few particles and this one does not.  The parameters, the checks, the draws (the same arrays in the same layouts) and the dict
    are `filter_particle_records_grouped`'s.
    Per track, with X_t the equally weighted set carried into row t (X_0: the bootstrap call's start, bit for bit) and (mean_i, v_i)
    the GP conditional at [X_ti, c_t]: mu_i = X_ti + mean_i, s_i = v_i + Q; m_pred = mean of the mu_i, S_pred = their centred
    covariance (divisor N) + diag(mean of the s_i) -- the moments of the mixture (1/N) sum_i N(mu_i, diag s_i), no draw enters;
    lpd[t, j] = log mean_i N(y_tj; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + sd_j^2); per particle, from (mu_i, diag s_i), exact
    scalar Kalman updates over the observed j in ascending order give (mt_i, P_i) and L_i = log p(y_t | parent i); lpd_joint[t] =
    log mean_i exp L_i; W_i = exp(L_i - max L), ess = (sum W)^2 / sum W^2; m_filt, S_filt: the moments of the mixture
    sum W_i N(mt_i, P_i) / sum W; systematic resampling of the parents with unif[t] (the bootstrap call's rule) gives a_i;
    X_{t+1,i} = mt_{a_i} + chol(P_{a_i}) eps[t, i] (unpivoted lower factor, a pivot <= 0 gives a zero column).  A row with nothing
    observed takes the bootstrap call's propagation X_ti + mean_i + eps[t, i] sqrt(v_i + Q) with a_i = i, ess = N and m_filt / S_filt
    = m_pred / S_pred bit for bit: a record that is all NaN returns `filter_particle_records_grouped`'s particles bit for bit.
    log_evidence stays the unbiased SMC estimate.
    Two of the returned arrays differ in meaning from the bootstrap call's: particles[t] (G, R, steps, N, D) is X_{t+1}, the equally
    weighted FILTERED set after row t (not X^-), and ancestors[t, i] indexes the set carried INTO row t.  Smoothing and backward
    simulation on the adapted sets are `smooth_adapted_records_grouped` and `backsim_adapted_records_grouped`; there is no forecast on
    them ("Adapted particle filtering")."""
    return _particle_records_given("filter_adapted_records_grouped", False, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass,
                                   return_particles, adapted=True)


def posterior_filter_adapted_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, *,
                                             xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0, jitter=JITTER,
                                             groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and the filter of `filter_adapted_records_grouped` in ONE call
    (`ffvd_posterior_particle_adapted_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `filter_adapted_records_grouped` computes, without the posteriors leaving the device.  The parameters are
    `posterior_filter_particle_records_grouped`'s, the returned dict is `filter_adapted_records_grouped`'s (particles[t] is the
    filtered set X_{t+1}; ancestors[t, i] indexes the set carried into row t)."""
    return _particle_records_posterior("posterior_filter_adapted_records_grouped", False, Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles, adapted=True)


def _ess_threshold(who, ess_threshold):
    """The check of an ESS threshold: a finite real number >= 0 (not a bool)."""
    t = ess_threshold
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) or not np.isfinite(t) or t < 0:
        raise ValueError(f"{who}: ess_threshold: expected a finite number >= 0 (0 never resamples, above 1 always), got {t!r}")
    return float(t)


def _adaptive_call(G, R, steps, N, return_particles):
    """Output arrays and the trailing arguments (weights, resampled) of the four adaptive entry points."""
    import ctypes
    ad = dict(resampled=np.empty((G, R, steps), dtype=np.int32))
    if return_particles:
        ad["weights"] = np.empty((G, R, steps, N))
    return ad, (_lib.dptr(ad["weights"]) if return_particles else None, ad["resampled"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)))


def _adaptive_dict(res, r, ad):
    """`_particle_dict` plus resampled (-1 at and beyond a record's length) and, when asked for, weights (NaN there)."""
    dead = ~r["live"]
    ad["resampled"][:, dead] = -1
    if "weights" in ad:
        ad["weights"][:, dead] = np.nan
    res.update(ad)
    return res


def _adaptive_draws(who, G, R, steps, D, eps, unif, xi0, with_S0, return_particles, seeded):
    """N, the draw arguments and what must stay alive: `_pack_particles` on the caller's arrays, or (seeded = (seed, noise,
    num_particles)) `_pack_seeded`'s N, seed, noise."""
    if seeded is None:
        return _pack_particles(who, G, R, steps, D, eps, unif, xi0, with_S0, return_particles)
    seed, noise, num_particles = seeded
    N, _, _, pargs = _pack_seeded(who, G, R, steps, D, num_particles, "bootstrap", "filter", seed, noise, 0, return_particles)
    return N, pargs, None


def _adaptive_records_given(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols, eps,
                            unif, xi0, ess_threshold, lengths, S0s, q_mode, Y_train_std, records_per_pass, return_particles, seeded=None):
    """The body of `filter_adaptive_records_grouped` and, with seeded = (seed, noise, num_particles), of `adaptive_records_seeded`."""
    shape = np.shape(Y_records)
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: Y_records: expected (R, steps, J) with at least one record and one row, got {shape}")
    G = len(U_vals)
    if x0s is None:
        raise ValueError(f"{who}: x0s: the start means are needed, ({shape[0]}, D) or ({G}, {shape[0]}, D)")
    thr = _ess_threshold(who, ess_threshold)
    xl, ci = _records_placeholders(G, Zs, kerns, shape[1])
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, xl, ci, 0, shape[1], Qs, None, q_mode)
    D, args = a["D"], a["args"]
    r = _pack_records(who, G, D, args[16], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    N, pargs, keep = _adaptive_draws(who, G, R, steps, D, eps, unif, xi0, r["S0"] is not None, return_particles, seeded)
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, extra, oargs = _particle_call(m, G, R, steps, D, N, bool(return_particles))
    ad, aargs = _adaptive_call(G, R, steps, N, bool(return_particles))
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    entry = "ffvd_particle_adaptive_records_grouped" if seeded is None else "ffvd_particle_adaptive_seeded_records_grouped"
    rc = getattr(_lib.load(), entry)(*args[:13], R, dp(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), *args[16:], dp(m["CC"]), dp(m["DD"]), dp(m["sd"]),
                                     m["J"], dp(m["Y"]), r["rpp"], *pargs, thr, *oargs, *aargs)
    _lib.check(rc, None, who)
    return _adaptive_dict(_particle_dict(r, G, out, extra, Y_train_std), r, ad)


def _adaptive_records_posterior(who, Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, xi0,
                                ess_threshold, lengths, x0s, S0s, q_mode, Y_train_std, jitter, groups_per_pass, records_per_pass,
                                return_particles, seeded=None):
    """The body of `posterior_filter_adaptive_records_grouped` and, with seeded = (seed, noise, num_particles), of
    `posterior_adaptive_records_seeded`."""
    thr = _ess_threshold(who, ess_threshold)
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, 0, 0, None, q_mode, jitter, groups_per_pass)
    G, D, args = a["G"], a["D"], a["args"]
    r = _pack_records(who, G, D, args[11], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    N, pargs, keep = _adaptive_draws(who, G, R, steps, D, eps, unif, xi0, r["S0"] is not None, return_particles, seeded)
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, extra, oargs = _particle_call(m, G, R, steps, D, N, bool(return_particles))
    ad, aargs = _adaptive_call(G, R, steps, N, bool(return_particles))
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    entry = "ffvd_posterior_particle_adaptive_records_grouped" if seeded is None else "ffvd_posterior_particle_adaptive_seeded_records_grouped"
    rc = getattr(_lib.load(), entry)(*args[:17], R, opt(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), steps, dp(m["CC"]), dp(m["DD"]), dp(m["sd"]),
                                     m["J"], dp(m["Y"]), r["rpp"], *pargs, thr, *oargs, *aargs, None)
    _lib.check(rc, None, who)
    return _adaptive_dict(_particle_dict(r, G, out, extra, Y_train_std), r, ad)


def filter_adaptive_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                    eps, unif, *, ess_threshold=0.5, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0,
                                    records_per_pass=0, return_particles=False):
    """Particle filtering of R observed records through G posteriors with ADAPTIVE resampling in ONE call
    (`ffvd_particle_adaptive_records_grouped`): `filter_particle_records_grouped` carrying a WEIGHTED set that is resampled only on
    the rows whose effective sample size falls below ess_threshold * N (Liu & Chen 1998), the textbook form.  Where rows have few or
    uninformative outputs the ESS stays high, and every resampling step saved there takes variance out of log_evidence and of the
    filtered moments and keeps the ancestry from thinning.  The parameters, the checks, the draws (the same arrays in the same
    layouts; unif[t] is not read on a row that does not resample) and the dict are `filter_particle_records_grouped`'s.
    Per track, with X the particles and a the log-weights carried into row t (largest entry exactly 0; a = 0 at the start),
    e_i = exp(a_i) and A = sum e: X^-_i as in the bootstrap call; m_pred, S_pred: the e-weighted mean and centred covariance of the
    X^-; lpd[t, j] = max_i(a_i + l_ij) + log(sum_i exp(a_i + l_ij - max) / A); b_i = a_i + L_i, lpd_joint[t] = max b +
    log(sum_i exp(b_i - max b) / A); W_i = exp(b_i - max b), m_filt / S_filt the W-weighted moments, ess = (sum W)^2 / sum W^2,
    weights[t, i] = W_i / sum W.  If ess < ess_threshold * N: the bootstrap call's systematic resampling with unif[t], then a = 0 and
    resampled[t] = 1; otherwise ancestors[t, i] = i, the X^- are carried, a_i = b_i - max b and resampled[t] = 0.  A row with nothing
    observed only propagates: m_filt = m_pred and S_filt = S_pred bit for bit, ess = A^2 / sum e^2, weights = e / A, a kept.
    log_evidence, the sum of lpd_joint over the observed rows, is the unbiased SMC estimate whether or not a row resamples.
    ess_threshold: a finite number >= 0; 0 never resamples (sequential importance sampling), any value above 1 always resamples and
    returns `filter_particle_records_grouped`'s arrays bit for bit in every key the two share.
    Returns that call's dict plus resampled (G, R, steps) int32 (-1 at and beyond a record's length) and, with return_particles,
    weights (G, R, steps, N) (NaN there): (particles[t], weights[t]) is the filtering approximation after every row, resampled or
    not; particles[t] is X^-.  A track's arrays are bit-identical whatever the other groups, the other records, their order and
    records_per_pass are.  Smoothing, backward simulation and forecasts on the weighted sets are not built (DESIGN.md section 9,
    "Adaptive resampling")."""
    return _adaptive_records_given("filter_adaptive_records_grouped", Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, ess_threshold, lengths, S0s, q_mode, Y_train_std,
                                   records_per_pass, return_particles)


def posterior_filter_adaptive_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, *,
                                              ess_threshold=0.5, xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference",
                                              Y_train_std=1.0, jitter=JITTER, groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and the filter of `filter_adaptive_records_grouped` in ONE call
    (`ffvd_posterior_particle_adaptive_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `filter_adaptive_records_grouped` computes, without the posteriors leaving the device.  The parameters are
    `posterior_filter_particle_records_grouped`'s plus ess_threshold; the returned dict is `filter_adaptive_records_grouped`'s."""
    return _adaptive_records_posterior("posterior_filter_adaptive_records_grouped", Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, ess_threshold, lengths, x0s, S0s, q_mode, Y_train_std,
                                       jitter, groups_per_pass, records_per_pass, return_particles)


def adaptive_records_seeded(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols, *, seed,
                            num_particles=256, ess_threshold=0.5, noise="shared", lengths=None, S0s=None, q_mode="reference",
                            Y_train_std=1.0, records_per_pass=0, return_particles=False):
    """`filter_adaptive_records_grouped` with SEEDED draws generated on the device (`ffvd_particle_adaptive_seeded_records_grouped`):
    seed, noise and num_particles are `particle_records_seeded`'s, and the call equals `filter_adaptive_records_grouped` on
    `particle_draws(seed, noise, G, R, steps, N, D, with_xi0=S0s is not None)` bit for bit in every key."""
    return _adaptive_records_given("adaptive_records_seeded", Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records,
                                   Qs, CC, DD, log_Rchols, None, None, None, ess_threshold, lengths, S0s, q_mode, Y_train_std,
                                   records_per_pass, return_particles, seeded=(seed, noise, num_particles))


def posterior_adaptive_records_seeded(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, *, seed,
                                      num_particles=256, ess_threshold=0.5, noise="shared", lengths=None, x0s=None, S0s=None,
                                      q_mode="reference", Y_train_std=1.0, jitter=JITTER, groups_per_pass=0, records_per_pass=0,
                                      return_particles=False):
    """The collapsed posterior of G groups and `adaptive_records_seeded` in ONE call
    (`ffvd_posterior_particle_adaptive_seeded_records_grouped`): neither the posteriors nor the draws ever exist on the host.  The
    model and start arguments are `posterior_filter_particle_records_grouped`'s; the rest and the dict are `adaptive_records_seeded`'s."""
    return _adaptive_records_posterior("posterior_adaptive_records_seeded", Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records,
                                       CC, DD, log_Rchols, None, None, None, ess_threshold, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles, seeded=(seed, noise, num_particles))


SMOOTH_PARTICLE_KEYS = ("m_smooth", "S_smooth", "ess_smooth")
SMOOTH_PARTICLE_STACKS = ("w_smooth", "weights", "trans_mean", "trans_var")


def _smooth_call(r, G, D, N, return_particles, adapted=False):
    """Output arrays and the trailing arguments (lengths, m_smooth .. trans_var) of the two particle smoothing entry points; with
    `adapted` of the two on the adapted sets, which have no `weights`."""
    import ctypes
    R, steps, dp = r["R"], r["steps"], _lib.dptr
    sm = dict(m_smooth=np.empty((G, R, steps, D)), S_smooth=np.empty((G, R, steps, D, D)), ess_smooth=np.empty((G, R, steps)))
    stacks = tuple(k for k in SMOOTH_PARTICLE_STACKS if not (adapted and k == "weights"))
    if return_particles:
        sm.update({k: np.empty((G, R, steps, N) + ((D,) if k.startswith("trans_") else ())) for k in stacks})
    sm["_lengths"] = np.ascontiguousarray(r["lengths"], dtype=np.int32)                 # (kept alive with the outputs)
    args = (sm["_lengths"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)),) + tuple(dp(sm[k]) for k in SMOOTH_PARTICLE_KEYS) + \
        tuple(dp(sm[k]) if return_particles else None for k in stacks)
    return sm, args


def _smooth_dict(res, r, sm):
    """`res` plus the arrays of the smoother or of the backward simulation, NaN (traj_index -1) at and beyond a record's length."""
    dead = ~r["live"]
    for k, v in sm.items():
        if not k.startswith("_"):
            rows = np.swapaxes(v, 2, 3) if k == "trajectories" else v          # (G, R, B, steps, D): a view with the rows third
            rows[:, dead] = -1 if k == "traj_index" else np.nan
            res[k] = v
    return res


def smooth_particle_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                    eps, unif, *, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0,
                                    return_particles=False):
    """`filter_particle_records_grouped` followed by the marginal particle smoother of every track in ONE call
    (`ffvd_particle_smooth_records_grouped`): the forward filter / backward smoother of Doucet, Godsill & Andrieu (2000) on the
    equally weighted sets the filter carries.  The parameters, their checks and every key of the returned dict are
    `filter_particle_records_grouped`'s (the filter's arrays bit for bit); no GP is evaluated beyond the filter's and no draw is
    added, so the result is a deterministic function of the filter's run.  Per track of n = lengths[r] rows, with X_t the set carried
    into row t, mu_t = X_t + m(X_t, c_t) the transition mean and s_t = v(X_t, c_t) + Q the transition variance (X^-_t = mu_t +
    eps[t] sqrt(s_t)), W_t the filter's weights and a_t its ancestors: w_smooth[n-1] = W_{n-1} / sum W_{n-1}; for t = n-2 .. 0, with
    x_j = X^-_{t+1,j}: log f_ij = -1/2 sum_d ((x_jd - mu_{t+1,id})^2 / s_{t+1,id} + log s_{t+1,id}), c_j = log sum_i exp log f_ij,
    omega_i = sum_j w_smooth[t+1, j] exp(log f_ij - c_j), w_smooth[t, k] = the sum of omega_i over the i with a_t[i] = k (exactly 0
    for a particle without offspring); nothing is renormalised inside the recursion.
    Adds to the dict, per track: m_smooth (G, R, steps, D) and S_smooth (G, R, steps, D, D), the w_smooth-weighted mean and centred
    covariance of the X^-_t (exactly symmetric), and ess_smooth (G, R, steps) = (sum w)^2 / sum w^2.  With return_particles also
    weights (W_t), w_smooth (G, R, steps, N), trans_mean and trans_var (G, R, steps, N, D) beside particles and ancestors.  NaN at and
    beyond a record's length; a record of one row returns its filtered row.  A track's arrays are bit-identical whatever the other
    groups, the other records, their order and records_per_pass are ("Particle smoothing").  The estimate
    converges at the usual 1 / sqrt(N) rate and does not collapse onto one path as the genealogy of `ancestors` does; joint
    trajectory draws (backward simulation) are `backsim_particle_records_grouped`'s."""
    return _particle_records_given("smooth_particle_records_grouped", True, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass,
                                   return_particles)


def posterior_smooth_particle_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, *,
                                              xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0, jitter=JITTER,
                                              groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and `smooth_particle_records_grouped` in ONE call
    (`ffvd_posterior_particle_smooth_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `smooth_particle_records_grouped` computes, without the posteriors leaving the device.  The parameters are
    `posterior_filter_particle_records_grouped`'s, the returned dict is `smooth_particle_records_grouped`'s."""
    return _particle_records_posterior("posterior_smooth_particle_records_grouped", True, Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles)


BACKSIM_MAX_B = 4096
BACKSIM_KEYS = ("trajectories", "traj_index", "m_traj", "S_traj", "lag_cov")
BACKSIM_STACKS = ("weights", "trans_mean", "trans_var")


def _smooth_or_backsim_call(who, r, G, D, N, return_particles, smooth, unif_bs, adapted=False):
    """`_smooth_call`, `_backsim_call` or nothing, by the form of the particle call"""
    if not smooth:
        return {}, ()
    return _smooth_call(r, G, D, N, return_particles, adapted) if unif_bs is None else \
        _backsim_call(who, r, G, D, N, return_particles, unif_bs, adapted)


def _backsim_call(who, r, G, D, N, return_particles, unif_bs, adapted=False):
    """Checks of `unif_bs` (before the library is loaded), output arrays and the trailing arguments (lengths, B, unif_bs and its
    strides, trajectories .. trans_var) of the two backward-simulation entry points; with `adapted` of the two on the adapted sets,
    which have no `weights`."""
    import ctypes
    R, steps, dp = r["R"], r["steps"], _lib.dptr
    u = np.asarray(unif_bs, dtype=np.float64)
    if u.ndim not in (2, 3, 4) or u.shape[-1] < 1:
        raise ValueError(f"{who}: unif_bs: expected ({steps}, B), ({R}, {steps}, B) or ({G}, {R}, {steps}, B), got {u.shape}")
    B = u.shape[-1]
    if B > BACKSIM_MAX_B:
        raise ValueError(f"{who}: unif_bs: the number of trajectories B must lie in [1, {BACKSIM_MAX_B}], got {B}")
    u, ug, ur = _particle_layout(who, "unif_bs", u, (steps, B), G, R)
    if np.any(u < 0.0) or np.any(u >= 1.0):
        raise ValueError(f"{who}: unif_bs: every uniform must lie in [0, 1)")
    if G * R * B >= 2 ** 31:
        raise ValueError(f"{who}: G * R * B = {G * R * B} must stay below 2^31")
    sm = dict(trajectories=np.empty((G, R, B, steps, D)), traj_index=np.empty((G, R, steps, B), dtype=np.int32), m_traj=np.empty((G, R, steps, D)),
              S_traj=np.empty((G, R, steps, D, D)), lag_cov=np.empty((G, R, steps, D, D)))
    stacks = tuple(k for k in BACKSIM_STACKS if not (adapted and k == "weights"))
    if return_particles:
        sm.update({k: np.empty((G, R, steps, N) + ((D,) if k.startswith("trans_") else ())) for k in stacks})
    sm["_lengths"], sm["_unif_bs"] = np.ascontiguousarray(r["lengths"], dtype=np.int32), u     # (kept alive with the outputs)
    ip = ctypes.POINTER(ctypes.c_int)
    args = (sm["_lengths"].ctypes.data_as(ip), B, dp(u), ug, ur, dp(sm["trajectories"]), sm["traj_index"].ctypes.data_as(ip)) + \
        tuple(dp(sm[k]) for k in BACKSIM_KEYS[2:]) + tuple(dp(sm[k]) if return_particles else None for k in stacks)
    return sm, args


def backsim_particle_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                     eps, unif, unif_bs, *, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0,
                                     records_per_pass=0, return_particles=False):
    """`filter_particle_records_grouped` followed by the backward simulation of B joint smoothed trajectories of every track in ONE
    call (`ffvd_particle_backsim_records_grouped`): forward filtering / backward simulation (Godsill, Doucet & West 2004) on the
    equally weighted sets the filter carries.  Where `smooth_particle_records_grouped` weights the particles of one row, this call
    draws whole paths, so a statistic of a path (an excursion, a first-passage time, a sum over a window, the increment x_{t+1} -
    x_t) has a sample, at B N density evaluations per row where the marginal smoother needs N^2.  The parameters, their checks and
    every key of the filter's dict are `filter_particle_records_grouped`'s (the filter's arrays bit for bit); no GP is evaluated
    beyond the filter's.  unif_bs: the caller's uniforms in [0, 1), (steps, B) shared by all tracks, (R, steps, B) shared by the
    groups, or (G, R, steps, B); B = unif_bs.shape[-1], 1 <= B <= 4096.
    Per track of n = lengths[r] rows and trajectory b, with u = unif_bs[t, b] and the notation of `smooth_particle_records_grouped`:
    row n-1: cdf = the running sum of W_{n-1} in index order, tot = cdf[N-1], k_{n-1} = min(#{k: cdf_k <= u tot}, N - 1); for
    t = n-2 .. 0, with x = X^-_{t+1, k_{t+1}}: log f_i = -1/2 sum_d ((x_d - mu_{t+1,id})^2 / s_{t+1,id} + log s_{t+1,id}), p_i =
    exp(log f_i - max_i log f_i) (so tot >= 1: nothing divides by a sum that can vanish), cdf the running sum of p, i* =
    min(#{i: cdf_i <= u tot}, N - 1) and k_t = ancestors[t, i*].  Conditional on the filter's run P(k_t = k) = w_smooth[t, k].
    Adds to the dict, per track: traj_index (G, R, steps, B) int32, k_t (-1 at and beyond a record's length); trajectories
    (G, R, B, steps, D) = particles[t, k_t], a gather, bit for bit; m_traj (G, R, steps, D), the mean over b; S_traj
    (G, R, steps, D, D), the centred covariance with divisor B (exactly symmetric); lag_cov (G, R, steps, D, D), lag_cov[t] =
    mean_b (x_t^b - m_traj[t]) (x_{t+1}^b - m_traj[t+1])^T, row index the component of x_t, not symmetric, NaN at the record's last
    row.  With return_particles also weights (W_t), trans_mean and trans_var beside particles and ancestors.  NaN at and beyond a
    record's length; a record of one row draws from its filtered weights.  Trajectory b depends on column b of unif_bs alone; a
    track's arrays are bit-identical whatever the other groups, the other records, their order and records_per_pass are (DESIGN.md
    section 9, "Particle backward simulation")."""
    return _particle_records_given("backsim_particle_records_grouped", True, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass,
                                   return_particles, _need(unif_bs, "backsim_particle_records_grouped"))


def posterior_backsim_particle_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif,
                                               unif_bs, *, xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0,
                                               jitter=JITTER, groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and `backsim_particle_records_grouped` in ONE call
    (`ffvd_posterior_particle_backsim_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `backsim_particle_records_grouped` computes, without the posteriors leaving the device.  The parameters are
    `posterior_filter_particle_records_grouped`'s plus unif_bs, the returned dict is `backsim_particle_records_grouped`'s."""
    return _particle_records_posterior("posterior_backsim_particle_records_grouped", True, Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles,
                                       _need(unif_bs, "posterior_backsim_particle_records_grouped"))


def smooth_adapted_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                   eps, unif, *, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0,
                                   return_particles=False):
    """`filter_adapted_records_grouped` followed by the marginal particle smoother of every track on the ADAPTED sets in ONE call
    (`ffvd_particle_adapted_smooth_records_grouped`).  The parameters and their checks are `smooth_particle_records_grouped`'s; every
    key of `filter_adapted_records_grouped`'s dict is returned bit for bit (the same draws); no GP is evaluated beyond the filter's
    and no draw is added.  Where the bootstrap filter collapses, `smooth_particle_records_grouped` inherits its collapsed sets and
    this call does not.
    Per track of n = lengths[r] rows, with P_t = particles[t] the equally weighted filtered set after row t and mu_t = trans_mean[t],
    s_t = trans_var[t] the filter's (mu, s) of the set carried into row t -- for t >= 1 the transition moments of P_{t-1}, particle by
    particle; row 0 belongs to the start set and is not read: w_smooth[n-1, i] = 1 / N; for t = n-2 .. 0, with x_j = P_{t+1,j}:
    log f_ij = -1/2 sum_d ((x_jd - mu_{t+1,id})^2 / s_{t+1,id} + log s_{t+1,id}), c_j = log sum_i exp log f_ij, w_smooth[t, i] =
    sum_j w_smooth[t+1, j] exp(log f_ij - c_j).  There is no fold through the ancestors and no emission weight (particle i of row t
    IS carried particle i of row t + 1, and the sets are equally weighted); nothing is renormalised.
    Adds to the dict, per track: m_smooth (G, R, steps, D) and S_smooth (G, R, steps, D, D), the w_smooth-weighted mean and centred
    covariance of P_t (exactly symmetric), and ess_smooth (G, R, steps) = (sum w)^2 / sum w^2.  With return_particles also w_smooth
    (G, R, steps, N), trans_mean and trans_var (G, R, steps, N, D) beside particles and ancestors; there is no `weights`.  NaN at and
    beyond a record's length.  A record of one row returns the plain mean and covariance of P_0: the unweighted particle estimate,
    not the Rao-Blackwellised m_filt / S_filt.  A record that is all NaN returns `smooth_particle_records_grouped`'s arrays bit for
    bit.  A track's arrays are bit-identical whatever the other groups, the other records, their order and records_per_pass are
    ("Adapted particle smoothing")."""
    return _particle_records_given("smooth_adapted_records_grouped", True, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass,
                                   return_particles, adapted=True)


def posterior_smooth_adapted_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif, *,
                                             xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0, jitter=JITTER,
                                             groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and `smooth_adapted_records_grouped` in ONE call
    (`ffvd_posterior_particle_adapted_smooth_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `smooth_adapted_records_grouped` computes, without the posteriors leaving the device.  The parameters are
    `posterior_filter_particle_records_grouped`'s, the returned dict is `smooth_adapted_records_grouped`'s."""
    return _particle_records_posterior("posterior_smooth_adapted_records_grouped", True, Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles, adapted=True)


def backsim_adapted_records_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols,
                                    eps, unif, unif_bs, *, xi0=None, lengths=None, S0s=None, q_mode="reference", Y_train_std=1.0,
                                    records_per_pass=0, return_particles=False):
    """`filter_adapted_records_grouped` followed by the backward simulation of B joint smoothed trajectories of every track on the
    ADAPTED sets in ONE call (`ffvd_particle_adapted_backsim_records_grouped`).  The parameters and their checks are
    `backsim_particle_records_grouped`'s; every key of `filter_adapted_records_grouped`'s dict is returned bit for bit.
    Per track of n = lengths[r] rows and trajectory b, with u = unif_bs[t, b] and the notation of `smooth_adapted_records_grouped`:
    k_{n-1} = min(#{k: k + 1 <= u N}, N - 1) (the filter's scan and search on unit weights); for t = n-2 .. 0, with
    x = P_{t+1, k_{t+1}}: p_i = exp(log f_i - max_i log f_i), cdf the running sum of p, k_t = min(#{i: cdf_i <= u tot}, N - 1): the
    searched index itself, without an ancestor indirection.  Conditional on the filter's run P(k_t = k) = w_smooth[t, k].
    Adds to the dict traj_index, trajectories (= particles[t, k_t], a gather, bit for bit), m_traj, S_traj and lag_cov with
    `backsim_particle_records_grouped`'s shapes and conventions.  With return_particles also trans_mean and trans_var beside
    particles and ancestors; there is no `weights`.  A record that is all NaN returns `backsim_particle_records_grouped`'s traj_index
    and trajectories for the same unif_bs bit for bit ("Adapted particle smoothing")."""
    return _particle_records_given("backsim_adapted_records_grouped", True, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records,
                                   Y_records, Qs, CC, DD, log_Rchols, eps, unif, xi0, lengths, S0s, q_mode, Y_train_std, records_per_pass,
                                   return_particles, _need(unif_bs, "backsim_adapted_records_grouped"), adapted=True)


def posterior_backsim_adapted_records_grouped(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, eps, unif,
                                              unif_bs, *, xi0=None, lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0,
                                              jitter=JITTER, groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and `backsim_adapted_records_grouped` in ONE call
    (`ffvd_posterior_particle_adapted_backsim_records_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `backsim_adapted_records_grouped` computes, without the posteriors leaving the device.  The parameters are
    `posterior_filter_particle_records_grouped`'s plus unif_bs, the returned dict is `backsim_adapted_records_grouped`'s."""
    return _particle_records_posterior("posterior_backsim_adapted_records_grouped", True, Zs, kerns, Xs, Qs, control_inputs, control_records,
                                       Y_records, CC, DD, log_Rchols, eps, unif, xi0, lengths, x0s, S0s, q_mode, Y_train_std, jitter,
                                       groups_per_pass, records_per_pass, return_particles,
                                       _need(unif_bs, "posterior_backsim_adapted_records_grouped"), adapted=True)


def _need(unif_bs, who):
    if unif_bs is None:
        raise ValueError(f"{who}: unif_bs: the uniforms of the backward simulation are needed, (steps, B), (R, steps, B) or (G, R, steps, B)")
    return unif_bs


PARTICLE_RULES = ("bootstrap", "adapted")
PARTICLE_STAGES = ("filter", "smooth", "backsim")
PARTICLE_NOISE = ("shared", "per_record", "independent")


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _seed_and_noise(who, seed, noise):
    """The checks of a seed (an integer in [0, 2^64)) and a noise mode; returns (seed, index of the mode)."""
    if not _is_int(seed) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"{who}: seed: expected an integer in [0, 2^64), got {seed!r}")
    if not isinstance(noise, str) or noise not in PARTICLE_NOISE:
        raise ValueError(f"{who}: noise: expected \"shared\", \"per_record\" or \"independent\", got {noise!r}")
    return int(seed), PARTICLE_NOISE.index(noise)


def particle_draws(seed, noise, G, R, steps, N, D, *, with_xi0=False, B=0):
    """The draws a seeded particle call uses (`ffvd_particle_draws`): generated on the device by Philox4x32-10 and downloaded, for
    inspection, for a reference, or to feed the calls that take the caller's arrays -- `particle_records_seeded(.., seed, noise)`
    equals its sibling on these arrays bit for bit.  An element is a pure function of (seed, stream, group, record, index in the
    block): the arrays of a call with fewer groups, records or steps are slices of a larger call's.  noise: "shared" (no leading
    dimensions), "per_record" (R,) or "independent" (G, R).  Returns a dict: eps lead + (steps, N, D) standard normal, unif
    lead + (steps,) in [0, 1), with_xi0 also xi0 lead + (N, D) standard normal, B >= 1 also unif_bs lead + (steps, B) in [0, 1)
    ("Device draws")."""
    who = "particle_draws"
    seed, mode = _seed_and_noise(who, seed, noise)
    for name, v, lo, hi in (("G", G, 1, None), ("R", R, 1, None), ("steps", steps, 1, None), ("N", N, PARTICLE_MIN_N, PARTICLE_MAX_N),
                            ("D", D, 1, 8), ("B", B, 0, BACKSIM_MAX_B)):
        if not _is_int(v) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"{who}: {name}: expected an integer " + (f"in [{lo}, {hi}]" if hi is not None else f">= {lo}") + f", got {v!r}")
    if not isinstance(with_xi0, (bool, np.bool_)):
        raise ValueError(f"{who}: with_xi0: expected a bool, got {with_xi0!r}")
    G, R, steps, N, D, B = (int(v) for v in (G, R, steps, N, D, B))
    if G * R * steps * N * D >= 2 ** 31:
        raise ValueError(f"{who}: G * R * steps * N * D = {G * R * steps * N * D} must stay below 2^31")
    if G * R * B >= 2 ** 31 or steps * B >= 2 ** 31:
        raise ValueError(f"{who}: G * R * B = {G * R * B} and steps * B = {steps * B} must stay below 2^31")
    lead = ((), (R,), (G, R))[mode]
    out = dict(eps=np.empty(lead + (steps, N, D)), unif=np.empty(lead + (steps,)))
    if with_xi0:
        out["xi0"] = np.empty(lead + (N, D))
    if B:
        out["unif_bs"] = np.empty(lead + (steps, B))
    dp = _lib.dptr
    rc = _lib.load().ffvd_particle_draws(seed, mode, G, R, steps, N, D, B, *(dp(out[k]) if k in out else None
                                                                            for k in ("eps", "unif", "xi0", "unif_bs")))
    _lib.check(rc, None, who)
    return out


def _pack_seeded(who, G, R, steps, D, num_particles, rule, stage, seed, noise, num_trajectories, return_particles):
    """The checks of the scalars of a seeded call (before the library is loaded).  Returns N, B and the leading arguments rule, stage
    and the middle ones N, seed, noise of the entry points."""
    if not isinstance(rule, str) or rule not in PARTICLE_RULES:
        raise ValueError(f"{who}: rule: expected \"bootstrap\" or \"adapted\", got {rule!r}")
    if not isinstance(stage, str) or stage not in PARTICLE_STAGES:
        raise ValueError(f"{who}: stage: expected \"filter\", \"smooth\" or \"backsim\", got {stage!r}")
    seed, mode = _seed_and_noise(who, seed, noise)
    N, B = num_particles, num_trajectories
    if not _is_int(N) or not PARTICLE_MIN_N <= N <= PARTICLE_MAX_N:
        raise ValueError(f"{who}: num_particles: expected an integer in [{PARTICLE_MIN_N}, {PARTICLE_MAX_N}], got {N!r}")
    if stage == "backsim":
        if not _is_int(B) or not 1 <= B <= BACKSIM_MAX_B:
            raise ValueError(f"{who}: num_trajectories: expected an integer in [1, {BACKSIM_MAX_B}] with stage=\"backsim\", got {B!r}")
    elif not _is_int(B) or B != 0:
        raise ValueError(f"{who}: num_trajectories: only stage=\"backsim\" draws trajectories, expected 0 with stage={stage!r}, got {B!r}")
    if not isinstance(return_particles, (bool, np.bool_)):
        raise ValueError(f"{who}: return_particles: expected a bool, got {return_particles!r}")
    N, B = int(N), int(B)
    if G * R * steps * N * D >= 2 ** 31:
        raise ValueError(f"{who}: G * R * steps * N * D = {G * R * steps * N * D} must stay below 2^31")
    if G * R * B >= 2 ** 31:
        raise ValueError(f"{who}: G * R * B = {G * R * B} must stay below 2^31")
    return N, B, (PARTICLE_RULES.index(rule), PARTICLE_STAGES.index(stage)), (N, seed, mode)


def _seeded_call(r, G, D, N, B, return_particles, stage, adapted):
    """Output arrays and the trailing arguments (lengths, B, trajectories .. trans_var, m_smooth .. w_smooth) of the two seeded entry
    points: the arrays of `_smooth_call` or `_backsim_call` by the stage, NULL for what the (rule, stage) does not produce."""
    import ctypes
    R, steps, dp, ip = r["R"], r["steps"], _lib.dptr, ctypes.POINTER(ctypes.c_int)
    sm, stacks = {}, ()
    if stage == "smooth":
        sm = dict(m_smooth=np.empty((G, R, steps, D)), S_smooth=np.empty((G, R, steps, D, D)), ess_smooth=np.empty((G, R, steps)))
        stacks = SMOOTH_PARTICLE_STACKS
    elif stage == "backsim":
        sm = dict(trajectories=np.empty((G, R, B, steps, D)), traj_index=np.empty((G, R, steps, B), dtype=np.int32),
                  m_traj=np.empty((G, R, steps, D)), S_traj=np.empty((G, R, steps, D, D)), lag_cov=np.empty((G, R, steps, D, D)))
        stacks = BACKSIM_STACKS
    if return_particles:
        sm.update({k: np.empty((G, R, steps, N) + ((D,) if k.startswith("trans_") else ())) for k in stacks if not (adapted and k == "weights")})
    lengths = None
    if stage != "filter":
        sm["_lengths"] = np.ascontiguousarray(r["lengths"], dtype=np.int32)                 # (kept alive with the outputs)
        lengths = sm["_lengths"].ctypes.data_as(ip)
    g = lambda k: dp(sm[k]) if k in sm else None
    args = (lengths, B, g("trajectories"), sm["traj_index"].ctypes.data_as(ip) if "traj_index" in sm else None) + \
        tuple(g(k) for k in ("m_traj", "S_traj", "lag_cov", "weights", "trans_mean", "trans_var", "m_smooth", "S_smooth", "ess_smooth", "w_smooth"))
    return sm, args


def particle_records_seeded(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_records, Y_records, Qs, CC, DD, log_Rchols, *, seed,
                            num_particles=256, rule="bootstrap", stage="filter", noise="shared", num_trajectories=0, lengths=None,
                            S0s=None, q_mode="reference", Y_train_std=1.0, records_per_pass=0, return_particles=False):
    """The six particle calls of many records with SEEDED draws generated on the device (`ffvd_particle_seeded_records_grouped`): no
    draw is generated, checked or uploaded by the host, so the cost of a call is what runs on the device and noise="independent" is
    bounded by the library's index limit (G * R * steps * N * D < 2^31) alone.  rule "bootstrap" / "adapted" and stage "filter" /
    "smooth" / "backsim" select the sibling -- `filter_particle_records_grouped`, `smooth_particle_records_grouped`,
    `backsim_particle_records_grouped`, `filter_adapted_records_grouped`, `smooth_adapted_records_grouped`,
    `backsim_adapted_records_grouped` -- whose positional operands (without eps, unif and unif_bs), other keywords, checks and
    returned dict these are.  seed: an integer in [0, 2^64); noise: "shared" (one set of draws for every track: common random
    numbers), "per_record" (one per record, shared by the groups) or "independent" (one per (group, record)); num_particles: N;
    num_trajectories: B, with stage="backsim" only; the start draws xi0 are generated exactly when S0s is given.
    The draws are Philox4x32-10 blocks addressed by (seed, stream, group, record, element) (`particle_draws` returns them): the call
    equals its sibling on `particle_draws(seed, noise, G, R, steps, N, D, ..)` bit for bit in every key, and a track's arrays do not
    depend on the other groups, the other records or records_per_pass ("Device draws")."""
    who = "particle_records_seeded"
    shape = np.shape(Y_records)
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{who}: Y_records: expected (R, steps, J) with at least one record and one row, got {shape}")
    G = len(U_vals)
    if x0s is None:
        raise ValueError(f"{who}: x0s: the start means are needed, ({shape[0]}, D) or ({G}, {shape[0]}, D)")
    xl, ci = _records_placeholders(G, Zs, kerns, shape[1])
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, xl, ci, 0, shape[1], Qs, None, q_mode)
    D, args = a["D"], a["args"]
    r = _pack_records(who, G, D, args[16], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    N, B, head, pargs = _pack_seeded(who, G, R, steps, D, num_particles, rule, stage, seed, noise, num_trajectories, return_particles)
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, extra, oargs = _particle_call(m, G, R, steps, D, N, bool(return_particles))
    sm, sargs = _seeded_call(r, G, D, N, B, bool(return_particles), stage, rule == "adapted")
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = _lib.load().ffvd_particle_seeded_records_grouped(*head, *args[:13], R, dp(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), *args[16:], dp(m["CC"]),
                                                          dp(m["DD"]), dp(m["sd"]), m["J"], dp(m["Y"]), r["rpp"], *pargs, *oargs, *sargs)
    _lib.check(rc, None, who)
    return _smooth_dict(_particle_dict(r, G, out, extra, Y_train_std), r, sm)


def posterior_particle_records_seeded(Zs, kerns, Xs, Qs, control_inputs, control_records, Y_records, CC, DD, log_Rchols, *, seed,
                                      num_particles=256, rule="bootstrap", stage="filter", noise="shared", num_trajectories=0,
                                      lengths=None, x0s=None, S0s=None, q_mode="reference", Y_train_std=1.0, jitter=JITTER,
                                      groups_per_pass=0, records_per_pass=0, return_particles=False):
    """The collapsed posterior of G groups and `particle_records_seeded` in ONE call
    (`ffvd_posterior_particle_seeded_records_grouped`): neither the posteriors nor the draws ever exist on the host.  The model and
    start arguments are `posterior_filter_particle_records_grouped`'s (x0s None: every record of group g starts at Xs[g][-1]); seed,
    num_particles, rule, stage, noise, num_trajectories and the returned dict are `particle_records_seeded`'s; the call equals the
    posterior sibling of its (rule, stage) on `particle_draws(..)` bit for bit."""
    who = "posterior_particle_records_seeded"
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, 0, 0, None, q_mode, jitter, groups_per_pass)
    G, D, args = a["G"], a["D"], a["args"]
    r = _pack_records(who, G, D, args[11], x0s, control_records, Y_records, lengths, S0s, records_per_pass)
    R, steps = r["R"], r["steps"]
    N, B, head, pargs = _pack_seeded(who, G, R, steps, D, num_particles, rule, stage, seed, noise, num_trajectories, return_particles)
    m = _pack_summary(who, D, R * steps, CC, DD, log_Rchols, r["Y"].reshape(R * steps, r["J"]))
    out, extra, oargs = _particle_call(m, G, R, steps, D, N, bool(return_particles))
    sm, sargs = _seeded_call(r, G, D, N, B, bool(return_particles), stage, rule == "adapted")
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = _lib.load().ffvd_posterior_particle_seeded_records_grouped(*head, *args[:17], R, opt(r["x0"]), opt(r["S0"]), opt(r["ctrl"]), steps,
                                                                    dp(m["CC"]), dp(m["DD"]), dp(m["sd"]), m["J"], dp(m["Y"]), r["rpp"], *pargs,
                                                                    *oargs, *sargs, None)
    _lib.check(rc, None, who)
    return _smooth_dict(_particle_dict(r, G, out, extra, Y_train_std), r, sm)


def _pack_forecast(who, n, horizon, origins=None, stride=1, model=None):
    """Horizon and forecast origins of a record of n rows, checked (before the library is loaded): 1 <= horizon <= n - 1; origins
    None: range(0, n - horizon, stride) with stride >= 1, else strictly ascending integers in [0, n - 1 - horizon], so that every
    track lies inside the record and its control rows exist.  model: (kind, M, P, D) for `_moment_limits` (LinearK is rejected).
    Returns horizon and the origins as a contiguous int32 array (B,)."""
    if model is not None:
        _moment_limits(who, *model)
    if isinstance(horizon, bool) or int(horizon) != horizon:
        raise ValueError(f"{who}: horizon: expected an integer, got {horizon!r}")
    h, n = int(horizon), int(n)
    if h < 1:
        raise ValueError(f"{who}: horizon: at least one step ahead is needed, got {h}")
    if n - h < 1:
        raise ValueError(f"{who}: horizon {h} does not fit a record of {n} rows (an origin and {h} rows after it are needed)")
    if origins is None:
        if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
            raise ValueError(f"{who}: stride: expected a positive integer, got {stride!r}")
        org = np.arange(0, n - h, int(stride), dtype=np.int32)
    else:
        o = np.asarray(origins)
        if o.ndim != 1 or o.size < 1 or not (np.issubdtype(o.dtype, np.integer) or np.array_equal(o, np.floor(o))):
            raise ValueError(f"{who}: origins: expected a non-empty sequence of integers")
        o = o.astype(np.int64)
        if o[0] < 0 or o[-1] > n - 1 - h or np.any(np.diff(o) <= 0) or np.any(o < 0) or np.any(o > n - 1 - h):
            raise ValueError(f"{who}: origins: expected strictly ascending rows in [0, {n - 1 - h}] (horizon {h}, {n} rows)")
        org = np.ascontiguousarray(o, dtype=np.int32)
    return h, org


_NO_FILTER_OUTPUTS = (None,) * 13
FORECAST_POOLED = ("predict_y", "predict_y_var_total", "lpd_mix", "lpd_gauss")


def _forecast_call(m, G, D, steps, h, org, return_tracks, return_filter, tracks_per_pass):
    """Output arrays (the filter's, the forecast's) and the arguments CC .. lpd_gauss and horizon .. fc_lpd_gauss of the two forecast
    entry points (U_means of the fused one goes between them)."""
    if isinstance(tracks_per_pass, bool) or int(tracks_per_pass) != tracks_per_pass or int(tracks_per_pass) < 0:
        raise ValueError(f"tracks_per_pass must be 0 (automatic) or a positive integer, got {tracks_per_pass!r}")
    import ctypes
    J, B, dp = m["J"], len(org), _lib.dptr
    if return_filter:
        fout, fargs = _filter_call(m, G, D, steps, False)
    else:
        fout, fargs = None, (dp(m["CC"]), dp(m["DD"]), dp(m["sd"]), J, dp(m["Y"])) + _NO_FILTER_OUTPUTS
    out = {k: np.empty((B, h, J)) for k in FORECAST_POOLED}
    if return_tracks:
        out.update(m_fc=np.empty((G, B, h, D)), S_fc=np.empty((G, B, h, D, D)))
    opt = lambda k: dp(out[k]) if k in out else None
    args = (h, org.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, int(tracks_per_pass), opt("m_fc"), opt("S_fc")) + \
        tuple(dp(out[k]) for k in FORECAST_POOLED)
    return fout, fargs, out, args


def _forecast_dict(m, org, h, fout, out, Y_train_std):
    """The dict the forecast functions return: origins, the arrays of `_forecast_call`, and the per-horizon curves over the observed
    targets Y[origins[b] + k] (formed here as `_filter_dict` forms ll): n_h, rmse_h, ll_h, ll_gauss_h, ll_h_original_units, each
    (h, J); a horizon or output without an observed target gives NaN and n_h = 0.  With the filter's outputs: the keys of
    `filter_grouped`, its four pooled one-step arrays as filter_predict_y, filter_predict_y_var_total, filter_lpd_mix,
    filter_lpd_gauss (the plain names are the forecast's here)."""
    Y = m["Y"]
    Yt = Y[org.astype(np.int64)[:, None] + 1 + np.arange(h)[None, :]]                     # (B, h, J)
    seen = ~np.isnan(Yt)
    n_h = np.sum(seen, axis=0).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = lambda x: np.where(n_h > 0, np.sum(np.where(seen, x, 0.0), axis=0) / n_h, np.nan)
        rmse_h = np.sqrt(over((Yt - out["predict_y"]) ** 2)) * Y_train_std
        ll_h, ll_gauss_h = over(out["lpd_mix"]), over(out["lpd_gauss"])
    res = {}
    if fout is not None:
        f = _filter_dict(m, fout, Y_train_std)
        res.update({("filter_" + k if k in FORECAST_POOLED else k): v for k, v in f.items()})
    res.update(out)
    res.update(origins=org.astype(np.int64), n_h=n_h, rmse_h=rmse_h, ll_h=ll_h, ll_gauss_h=ll_gauss_h,
               ll_h_original_units=ll_h - float(np.log(Y_train_std)))
    return res


def _forecast_given(who, symbol, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD,
                    log_Rchols, horizon, origins, stride, S0s, q_mode, Y_train_std, return_tracks, return_filter, tracks_per_pass):
    """The body of `forecast_grouped`, `forecast_linear_grouped` and `forecast_cubature_grouped`: `symbol` is the entry point (the
    propagation rule)."""
    steps = _filter_steps(who, Y_obs)
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode)
    h, org = _pack_forecast(who, steps, horizon, origins, stride, (a["args"][0], a["M"], a["args"][6], a["D"]))
    m = _pack_filter(who, a["D"], Y_obs, CC, DD, log_Rchols)
    fout, fargs, out, args = _forecast_call(m, a["G"], a["D"], steps, h, org, return_tracks, return_filter, tracks_per_pass)
    rc = getattr(_lib.load(), symbol)(*a["args"], *fargs, *args)
    _lib.check(rc, None, who)
    return _forecast_dict(m, org, h, fout, out, Y_train_std)


def _forecast_posterior(who, symbol, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, x0s, origins,
                        stride, S0s, q_mode, Y_train_std, return_tracks, return_filter, tracks_per_pass, jitter, groups_per_pass):
    """The body of `posterior_forecast_grouped`, `posterior_forecast_linear_grouped` and `posterior_forecast_cubature_grouped`"""
    steps = _filter_steps(who, Y_obs)
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass)
    h, org = _pack_forecast(who, steps, horizon, origins, stride, (a["args"][0], a["M"], a["args"][5], a["D"]))
    m = _pack_filter(who, a["D"], Y_obs, CC, DD, log_Rchols)
    x0 = None if x0s is None else _lib.as_f64(x0s, (a["G"], a["D"]), "x0s")
    fout, fargs, out, args = _forecast_call(m, a["G"], a["D"], steps, h, org, return_tracks, return_filter, tracks_per_pass)
    pre = a["args"][:17] + (None if x0 is None else _lib.dptr(x0),) + a["args"][17:]
    rc = getattr(_lib.load(), symbol)(*pre, *fargs, None, *args)
    _lib.check(rc, None, who)
    return _forecast_dict(m, org, h, fout, out, Y_train_std)


def forecast_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols,
                     horizon, *, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0, return_tracks=False,
                     return_filter=False, tracks_per_pass=0, method="moment"):
    """Rolling-origin multi-step forecasts of an observed record through G posteriors in ONE call (`ffvd_op_forecast_grouped`): the
    filter of `filter_grouped` (same arguments up to log_Rchols), then from every origin -- a row of the record -- `horizon` steps of
    `moment_grouped` started at the filtered state of that row.  All (group, origin) tracks advance in one launch per forecast
    step; the posteriors are prepared once and the filtered states never leave the device.  origins: strictly ascending rows in
    [0, n - 1 - horizon]; None: range(0, n - horizon, stride).
    Returns a dict.  origins (B,);  predict_y, predict_y_var_total, lpd_mix, lpd_gauss (B, horizon, J): entry [b, k - 1] is the
    equal-weight pool over the groups (the chains are not re-weighted by their likelihoods) of the k-step-ahead prediction of row
    origins[b] + k given rows 0 .. origins[b]; NaN densities where that target is unobserved.  Per-horizon curves over the observed
    targets, (horizon, J): n_h (count), rmse_h (times Y_train_std), ll_h, ll_gauss_h, ll_h_original_units (ll_h - log Y_train_std);
    NaN where n_h = 0.  With return_tracks: m_fc (G, B, horizon, D), S_fc (G, B, horizon, D, D), exactly symmetric.  With
    return_filter: the keys of `filter_grouped` without the smoothed ones, its pooled one-step arrays under filter_predict_y,
    filter_predict_y_var_total, filter_lpd_mix, filter_lpd_gauss.  A track is bit-identical to `moment_grouped` from
    x_lasts = m_filt[:, o], S0s = S_filt[:, o], ctrl_offset + o + 1, and does not depend on the other tracks, the other groups or
    tracks_per_pass (0: automatic; the number of origins that advance together).  method: "moment" only -- `filter_grouped`'s
    "linearised" raises ValueError here: the linearised rule has functions of its own, `forecast_linear_grouped` and
    `posterior_forecast_linear_grouped`."""
    who = "forecast_grouped"
    _filter_method(who, method, forecast=True)
    return _forecast_given(who, "ffvd_op_forecast_grouped", Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset,
                           Y_obs, Qs, CC, DD, log_Rchols, horizon, origins, stride, S0s, q_mode, Y_train_std, return_tracks, return_filter,
                           tracks_per_pass)


def posterior_forecast_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, *, x0s=None,
                               origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0, return_tracks=False,
                               return_filter=False, tracks_per_pass=0, jitter=JITTER, groups_per_pass=0, method="moment"):
    """The collapsed posterior of G groups and the forecasts of `forecast_grouped` in ONE call
    (`ffvd_op_posterior_forecast_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by `forecast_grouped`
    computes, without the posteriors leaving the device.  The arguments up to log_Rchols, x0s, jitter and groups_per_pass are
    `posterior_filter_grouped`'s; method: as `forecast_grouped`.  Returns the dict of `forecast_grouped`."""
    who = "posterior_forecast_grouped"
    _filter_method(who, method, forecast=True)
    return _forecast_posterior(who, "ffvd_op_posterior_forecast_grouped", Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD,
                               log_Rchols, horizon, x0s, origins, stride, S0s, q_mode, Y_train_std, return_tracks, return_filter,
                               tracks_per_pass, jitter, groups_per_pass)


def forecast_linear_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols,
                            horizon, *, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0, return_tracks=False,
                            return_filter=False, tracks_per_pass=0):
    """`forecast_grouped` under the linearised (extended Kalman) rule, in ONE call (`ffvd_op_forecast_linear_grouped`): the filter of
    `filter_grouped(method="linearised")`, then from every origin `horizon` steps of the same linearisation without a measurement
    update, started at the filtered state (mu, S) of that row: with m, v the mean and variance of the GP conditional at
    [mu, c_row] and J the Jacobian of m with respect to the state, A = I + J: mu' = mu + m, S' = A S A^T + diag(v + Q).  The
    parameters (without `method`) and the returned dict are `forecast_grouped`'s; the pooled arrays give the groups EQUAL weights (the
    chains are not re-weighted by their likelihoods).  The call's filter outputs are `filter_grouped(method="linearised")`'s bit for
    bit.  A track is what that filter computes over the record cut after its origin and continued by `horizon` all-NaN rows, to
    rounding and not bit for bit: the quadratic forms k^T Gamma k of all tracks that share a Gamma are one dense product on the fp64
    matrix cores here and are summed in another order.  A track does not depend on the other tracks, the other groups or
    tracks_per_pass; every S_fc is exactly symmetric ("Linearised forecasts")."""
    return _forecast_given("forecast_linear_grouped", "ffvd_op_forecast_linear_grouped", Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s,
                           control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols, horizon, origins, stride, S0s, q_mode, Y_train_std,
                           return_tracks, return_filter, tracks_per_pass)


def posterior_forecast_linear_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, *, x0s=None,
                                      origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0, return_tracks=False,
                                      return_filter=False, tracks_per_pass=0, jitter=JITTER, groups_per_pass=0):
    """The collapsed posterior of G groups and the forecasts of `forecast_linear_grouped` in ONE call
    (`ffvd_op_posterior_forecast_linear_grouped`): the parameters of `posterior_forecast_grouped` without `method`, the dict of
    `forecast_grouped`."""
    return _forecast_posterior("posterior_forecast_linear_grouped", "ffvd_op_posterior_forecast_linear_grouped", Zs, kerns, Xs, Qs,
                               control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, x0s, origins, stride, S0s, q_mode, Y_train_std,
                               return_tracks, return_filter, tracks_per_pass, jitter, groups_per_pass)


def forecast_cubature_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols,
                              horizon, *, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0, return_tracks=False,
                              return_filter=False, tracks_per_pass=0):
    """`forecast_grouped` under the third-degree spherical cubature rule, in ONE call (`ffvd_op_forecast_cubature_grouped`): the filter
    of `filter_cubature_records_grouped` over the one record, then from every origin `horizon` steps of the same propagation without
    a measurement update, started at the filtered state (mu, S) of that row: S = L L^T, the 2D points [mu +- sqrt(D) L[:, i], c_row]
    with equal weights, mu' and S' as in `filter_cubature_records_grouped`'s m^- and S^-.  The parameters and the returned dict are
    `forecast_linear_grouped`'s; the pooled arrays give the groups EQUAL weights.  The call's filter outputs are
    `filter_cubature_records_grouped`'s with R = 1 bit for bit (record axis dropped).  A track is what that filter computes over the
    record cut after its origin and continued by `horizon` all-NaN rows.  A track does not depend on the other tracks, the other
    groups or tracks_per_pass; every S_fc is exactly symmetric ("Cubature forecasts")."""
    return _forecast_given("forecast_cubature_grouped", "ffvd_op_forecast_cubature_grouped", Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts,
                           x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols, horizon, origins, stride, S0s, q_mode,
                           Y_train_std, return_tracks, return_filter, tracks_per_pass)


def posterior_forecast_cubature_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, *, x0s=None,
                                        origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0, return_tracks=False,
                                        return_filter=False, tracks_per_pass=0, jitter=JITTER, groups_per_pass=0):
    """The collapsed posterior of G groups and the forecasts of `forecast_cubature_grouped` in ONE call
    (`ffvd_op_posterior_forecast_cubature_grouped`): the parameters of `posterior_forecast_linear_grouped`, the dict of
    `forecast_grouped`."""
    return _forecast_posterior("posterior_forecast_cubature_grouped", "ffvd_op_posterior_forecast_cubature_grouped", Zs, kerns, Xs, Qs,
                               control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, x0s, origins, stride, S0s, q_mode, Y_train_std,
                               return_tracks, return_filter, tracks_per_pass, jitter, groups_per_pass)


def _fc_draw_layout(who, name, x, tail, lead):
    """One of the layouts of a draw array of the particle forecasts: `tail` (shared), or `tail` behind the last one, two, ... of the
    leading axes `lead`.  Returns the contiguous array and one stride in doubles per leading axis (0 = shared)."""
    a = np.asarray(x, dtype=np.float64)
    tail, lead = tuple(tail), tuple(lead)
    shapes = [lead[len(lead) - k:] + tail for k in range(len(lead) + 1)]
    if a.shape not in shapes:
        raise ValueError(f"{who}: {name}: expected " + " or ".join(str(s) for s in shapes) + f", got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: {name}: every draw must be finite")
    have = a.ndim - len(tail)
    strides, inner = [], int(np.prod(tail, dtype=np.int64))
    for k in range(len(lead)):                          # from the innermost leading axis outwards
        strides.append(inner if k < have else 0)
        inner *= lead[len(lead) - 1 - k] if k < have else 1
    return np.ascontiguousarray(a), tuple(reversed(strides))


def _pack_particle_forecast(who, G, B, steps, h, D, eps, unif, xi0, eps_fc, with_S0, return_particles):
    """Shape and value checks of the draws of `forecast_particle_grouped` (before the library is loaded): N from eps, the layouts of
    eps / unif / xi0 (shared or per group) and of eps_fc (shared, per origin, or per group and origin), unif in [0, 1), xi0 exactly
    when S0s is given, the 2^31 limits.  Returns N and the arguments N .. eps_fc_stride_b."""
    e = np.asarray(eps, dtype=np.float64)
    if e.ndim not in (3, 4) or e.shape[-1] != D:
        raise ValueError(f"{who}: eps: expected ({steps}, N, {D}) or ({G}, {steps}, N, {D}), got {e.shape}")
    N = e.shape[-2]
    if not PARTICLE_MIN_N <= N <= PARTICLE_MAX_N:
        raise ValueError(f"{who}: eps: the number of particles N must lie in [{PARTICLE_MIN_N}, {PARTICLE_MAX_N}], got {N}")
    e, (eg,) = _fc_draw_layout(who, "eps", e, (steps, N, D), (G,))
    u, (ug,) = _fc_draw_layout(who, "unif", unif, (steps,), (G,))
    if np.any(u < 0.0) or np.any(u >= 1.0):
        raise ValueError(f"{who}: unif: every uniform must lie in [0, 1)")
    if with_S0 != (xi0 is not None):
        raise ValueError(f"{who}: xi0: the start draws ({N}, {D}) are needed exactly when S0s is given (S0s "
                         f"{'given' if with_S0 else 'None'}, xi0 {'None' if xi0 is None else 'given'})")
    x, (xg,) = (None, (0,)) if xi0 is None else _fc_draw_layout(who, "xi0", xi0, (N, D), (G,))
    f, (fg, fb) = _fc_draw_layout(who, "eps_fc", eps_fc, (h, N, D), (G, B))
    if not isinstance(return_particles, (bool, np.bool_)):
        raise ValueError(f"{who}: return_particles: expected a bool, got {return_particles!r}")
    if G * steps * N * D >= 2 ** 31:
        raise ValueError(f"{who}: G * steps * N * D = {G * steps * N * D} must stay below 2^31")
    if G * B * h * N * D >= 2 ** 31:
        raise ValueError(f"{who}: G * B * horizon * N * D = {G * B * h * N * D} must stay below 2^31")
    dp = _lib.dptr
    return N, (N, dp(e), eg, dp(u), ug, None if x is None else dp(x), xg, dp(f), fg, fb), (e, u, x, f)


def _particle_forecast_call(m, G, D, steps, h, org, N, return_tracks, return_filter, return_particles, tracks_per_pass):
    """Output arrays and the arguments CC .. lpd_gauss, horizon .. tracks_per_pass and m_fc .. fc_particles of the two particle
    forecast entry points (U_means of the fused one goes behind the first block, the draws between the other two)."""
    if isinstance(tracks_per_pass, bool) or int(tracks_per_pass) != tracks_per_pass or int(tracks_per_pass) < 0:
        raise ValueError(f"tracks_per_pass must be 0 (automatic) or a positive integer, got {tracks_per_pass!r}")
    import ctypes
    J, B, dp = m["J"], len(org), _lib.dptr
    fout = None
    if return_filter:
        fout = dict(m_pred=np.empty((G, steps, D)), S_pred=np.empty((G, steps, D, D)), m_filt=np.empty((G, steps, D)),
                    S_filt=np.empty((G, steps, D, D)), lpd=np.empty((G, steps, J)), lpd_joint=np.empty((G, steps)),
                    predict_y=np.empty((steps, J)), predict_y_var_total=np.empty((steps, J)), lpd_mix=np.empty((steps, J)),
                    lpd_gauss=np.empty((steps, J)), ess=np.empty((G, steps)), log_evidence=np.empty((G,)))
    fo = lambda k: dp(fout[k]) if fout is not None and k in fout else None
    names = ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "lpd", "lpd_joint", "m_smooth", "S_smooth", "predict_y",
             "predict_y_var_total", "lpd_mix", "lpd_gauss")
    fargs = (dp(m["CC"]), dp(m["DD"]), dp(m["sd"]), J, dp(m["Y"])) + tuple(fo(k) for k in names)
    out = {k: np.empty((B, h, J)) for k in FORECAST_POOLED}
    out["lpd_fc"] = np.empty((G, B, h, J))
    if return_tracks:
        out.update(m_fc=np.empty((G, B, h, D)), S_fc=np.empty((G, B, h, D, D)))
    if return_particles:
        out["fc_particles"] = np.empty((G, B, h, N, D))
    opt = lambda k: dp(out[k]) if k in out else None
    hargs = (h, org.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), B, int(tracks_per_pass))
    oargs = (opt("m_fc"), opt("S_fc")) + tuple(dp(out[k]) for k in FORECAST_POOLED) + \
        (fo("ess"), fo("log_evidence"), dp(out["lpd_fc"]), opt("fc_particles"))
    return fout, fargs, out, hargs, oargs


def _particle_forecast_dict(m, org, h, fout, out, Y_train_std):
    """`_forecast_dict`; with the filter's outputs also ll_all (= ll: one record)."""
    res = _forecast_dict(m, org, h, fout, out, Y_train_std)
    if fout is not None:
        res["ll_all"] = res["ll"]
    return res


def forecast_particle_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols,
                              horizon, eps, unif, eps_fc, *, xi0=None, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0,
                              return_tracks=False, return_filter=False, return_particles=False, tracks_per_pass=0):
    """`forecast_grouped` by particles, in ONE call (`ffvd_op_forecast_particle_grouped`): the bootstrap particle filter of
    `filter_particle_records_grouped` over the one record, then from every origin o a track of N equally weighted particles started
    from the set the filter carries AFTER row o (the X^- of row o gathered through that row's ancestors; the identity for a row
    with nothing observed) and advanced `horizon` steps with the caller's forecast draws, without weighting or resampling: with
    (m_i, v_i) the GP conditional of the group at [X_i, c_row], X_i <- X_i + m_i + eps_fc[k - 1, i] sqrt(v_i + Q) for k = 1 .. h,
    control row ctrl_offset + o + k (the row the Gaussian fans use).  The positional model, record and emission arguments are
    `forecast_cubature_grouped`'s.  Every random draw is the caller's: eps (steps, N, D) or (G, steps, N, D), unif (steps,) or
    (G, steps) in [0, 1), xi0 (N, D) or (G, N, D), given exactly when S0s is; eps_fc (h, N, D), (B, h, N, D) or (G, B, h, N, D):
    the shared layouts are common random numbers across groups, or across groups and origins.  N = eps.shape[-2], 2 <= N <= 2048.
    Returns the dict of `forecast_grouped`: predict_y, predict_y_var_total and lpd_gauss pool the moments (m_fc, S_fc) of the
    particle sets over the groups with EQUAL weights as the Gaussian rules do; lpd_mix = log mean_g exp(lpd_fc[g]) is the density of
    the mixture of all G N particles' emissions, so ll_h is directly comparable with the three Gaussian fans'.  Always lpd_fc
    (G, B, h, J) = log mean_i N(Y[o + k, j]; CC[:, j] . X_i + DD_j, sd_j^2), NaN where that target is NaN; with return_tracks m_fc
    (G, B, h, D) and S_fc (G, B, h, D, D), the mean and centred covariance of the N particles, exactly symmetric; with
    return_particles fc_particles (G, B, h, N, D); with return_filter the keys of `filter_particle_records_grouped` with the record
    axis dropped, its pooled one-step arrays under filter_predict_y, filter_predict_y_var_total, filter_lpd_mix, filter_lpd_gauss.
    A track is bit for bit what `filter_particle_records_grouped` computes (m_pred, S_pred, particles at rows o + 1 .. o + h) over
    the record cut after its origin and continued by `horizon` all-NaN rows with the draws concatenated, and does not depend on the
    other tracks, the other groups or tracks_per_pass ("Particle forecasts").  SquaredExponential kernels
    only."""
    who = "forecast_particle_grouped"
    steps = _filter_steps(who, Y_obs)
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode)
    G, D = a["G"], a["D"]
    h, org = _pack_forecast(who, steps, horizon, origins, stride, (a["args"][0], a["M"], a["args"][6], D))
    m = _pack_filter(who, D, Y_obs, CC, DD, log_Rchols)
    N, pargs, keep = _pack_particle_forecast(who, G, len(org), steps, h, D, eps, unif, xi0, eps_fc, S0s is not None, return_particles)
    fout, fargs, out, hargs, oargs = _particle_forecast_call(m, G, D, steps, h, org, N, return_tracks, return_filter,
                                                             bool(return_particles), tracks_per_pass)
    rc = _lib.load().ffvd_op_forecast_particle_grouped(*a["args"], *fargs, *hargs, *pargs, *oargs)
    _lib.check(rc, None, who)
    return _particle_forecast_dict(m, org, h, fout, out, Y_train_std)


def posterior_forecast_particle_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, eps, unif, eps_fc,
                                        *, xi0=None, x0s=None, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0,
                                        return_tracks=False, return_filter=False, return_particles=False, tracks_per_pass=0, jitter=JITTER,
                                        groups_per_pass=0):
    """The collapsed posterior of G groups and the forecasts of `forecast_particle_grouped` in ONE call
    (`ffvd_op_posterior_forecast_particle_grouped`): what `conditionals_multi_output.collapse_u_mean_grouped` followed by
    `forecast_particle_grouped` computes, without the posteriors leaving the device.  The model and start arguments are
    `posterior_forecast_cubature_grouped`'s; the draws, the return_* flags and the returned dict are `forecast_particle_grouped`'s."""
    who = "posterior_forecast_particle_grouped"
    steps = _filter_steps(who, Y_obs)
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass)
    G, D = a["G"], a["D"]
    h, org = _pack_forecast(who, steps, horizon, origins, stride, (a["args"][0], a["M"], a["args"][5], D))
    m = _pack_filter(who, D, Y_obs, CC, DD, log_Rchols)
    x0 = None if x0s is None else _lib.as_f64(x0s, (G, D), "x0s")
    N, pargs, keep = _pack_particle_forecast(who, G, len(org), steps, h, D, eps, unif, xi0, eps_fc, S0s is not None, return_particles)
    fout, fargs, out, hargs, oargs = _particle_forecast_call(m, G, D, steps, h, org, N, return_tracks, return_filter,
                                                             bool(return_particles), tracks_per_pass)
    pre = a["args"][:17] + (None if x0 is None else _lib.dptr(x0),) + a["args"][17:]
    rc = _lib.load().ffvd_op_posterior_forecast_particle_grouped(*pre, *fargs, None, *hargs, *pargs, *oargs)
    _lib.check(rc, None, who)
    return _particle_forecast_dict(m, org, h, fout, out, Y_train_std)


def forecast_adapted_grouped(Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, Y_obs, Qs, CC, DD, log_Rchols,
                             horizon, eps, unif, eps_fc, *, xi0=None, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0,
                             return_tracks=False, return_filter=False, return_particles=False, tracks_per_pass=0):
    """`forecast_particle_grouped` on the sets of the fully adapted particle filter, in ONE call
    (`ffvd_particle_adapted_forecast_grouped`): the filter of `filter_adapted_records_grouped` over the one record, then from every
    origin o a track of N particles started from a straight copy of particles[o], the equally weighted FILTERED set that filter stores
    after row o (no ancestor is read).  For k = 1 .. h, with (mean_i, v_i) the GP conditional of the group at [X_i, c_row], control
    row ctrl_offset + o + k, mu_i = X_i + mean_i and s_i = v_i + Q:
      m_fc = mean_i mu_i,  S_fc = mean_i (mu_i - m_fc)(mu_i - m_fc)^T + diag(mean_i s_i)          (no draw enters)
      lpd_fc_j = log mean_i N(Y[o + k, j]; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + sd_j^2), NaN where that target is NaN
      X_i <- mu_i + eps_fc[k - 1, i] sqrt(s_i);  fc_particles[k - 1] is this advanced set.
    These are the adapted filter's Rao-Blackwellised m_pred / S_pred / lpd expressions: the last step's process noise is integrated
    in closed form at every horizon, the row k = 1 from origin o equals the filter's own prediction of row o + 1 bit for bit, and a
    track is bit for bit what `filter_adapted_records_grouped` computes (m_pred, S_pred, particles at rows o + 1 .. o + h) over the
    record cut after its origin and continued by `horizon` all-NaN rows with the draws concatenated.  A track does not depend on
    the other tracks, the other groups or tracks_per_pass ("Adapted particle forecasts").  The parameters, the
    draws and their layouts, the return_* flags and the keys of the returned dict are `forecast_particle_grouped`'s; with
    return_filter the filter keys are those of `filter_adapted_records_grouped` with the record axis dropped.  SquaredExponential
    kernels only."""
    who = "forecast_adapted_grouped"
    steps = _filter_steps(who, Y_obs)
    a = _pack_moment_groups(who, Lm_inverse_seqs, Zs, kerns, U_vals, q_sqrts, x0s, control_inputs, ctrl_offset, steps, Qs, S0s, q_mode)
    G, D = a["G"], a["D"]
    h, org = _pack_forecast(who, steps, horizon, origins, stride, (a["args"][0], a["M"], a["args"][6], D))
    m = _pack_filter(who, D, Y_obs, CC, DD, log_Rchols)
    N, pargs, keep = _pack_particle_forecast(who, G, len(org), steps, h, D, eps, unif, xi0, eps_fc, S0s is not None, return_particles)
    fout, fargs, out, hargs, oargs = _particle_forecast_call(m, G, D, steps, h, org, N, return_tracks, return_filter,
                                                             bool(return_particles), tracks_per_pass)
    rc = _lib.load().ffvd_particle_adapted_forecast_grouped(*a["args"], *fargs, *hargs, *pargs, *oargs)
    _lib.check(rc, None, who)
    return _particle_forecast_dict(m, org, h, fout, out, Y_train_std)


def posterior_forecast_adapted_grouped(Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, Y_obs, CC, DD, log_Rchols, horizon, eps, unif, eps_fc,
                                       *, xi0=None, x0s=None, origins=None, stride=1, S0s=None, q_mode="reference", Y_train_std=1.0,
                                       return_tracks=False, return_filter=False, return_particles=False, tracks_per_pass=0, jitter=JITTER,
                                       groups_per_pass=0):
    """The collapsed posterior of G groups and the forecasts of `forecast_adapted_grouped` in ONE call
    (`ffvd_posterior_particle_adapted_forecast_grouped`), without the posteriors leaving the device.  The parameters are
    `posterior_forecast_particle_grouped`'s; the returned dict is `forecast_adapted_grouped`'s."""
    who = "posterior_forecast_adapted_grouped"
    steps = _filter_steps(who, Y_obs)
    a = _pack_posterior_moment(who, Zs, kerns, Xs, Qs, control_inputs, ctrl_offset, steps, S0s, q_mode, jitter, groups_per_pass)
    G, D = a["G"], a["D"]
    h, org = _pack_forecast(who, steps, horizon, origins, stride, (a["args"][0], a["M"], a["args"][5], D))
    m = _pack_filter(who, D, Y_obs, CC, DD, log_Rchols)
    x0 = None if x0s is None else _lib.as_f64(x0s, (G, D), "x0s")
    N, pargs, keep = _pack_particle_forecast(who, G, len(org), steps, h, D, eps, unif, xi0, eps_fc, S0s is not None, return_particles)
    fout, fargs, out, hargs, oargs = _particle_forecast_call(m, G, D, steps, h, org, N, return_tracks, return_filter,
                                                             bool(return_particles), tracks_per_pass)
    pre = a["args"][:17] + (None if x0 is None else _lib.dptr(x0),) + a["args"][17:]
    rc = _lib.load().ffvd_posterior_particle_adapted_forecast_grouped(*pre, *fargs, None, *hargs, *pargs, *oargs)
    _lib.check(rc, None, who)
    return _particle_forecast_dict(m, org, h, fout, out, Y_train_std)


# ---- proper scores and quantiles of the pooled predictive mixtures (csrc/predict_score.h) -----------------------------------------------
SCORE_TILE = 256              # components per tile of the pair kernel (PSC_TILE)
SCORE_MAX_K = 65536
SCORE_MAX_Q = 16
SCORE_MAX_D_POINTS = 32
SCORE_LEVEL_MIN = 1e-9
SCORE_LEVELS = (0.05, 0.5, 0.95)
SCORE_USES = ("auto", "moments", "particles")


def _pack_levels(who, levels):
    """The quantile levels as a contiguous vector: at most 16, each in [1e-9, 1 - 1e-9] (NaN is refused)."""
    try:
        lv = np.asarray(levels, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: levels: expected a sequence of numbers, got {levels!r}") from None
    if lv.ndim != 1 or lv.size > SCORE_MAX_Q:
        raise ValueError(f"{who}: levels: expected at most {SCORE_MAX_Q} levels in one dimension, got shape {lv.shape}")
    if lv.size and not np.all((lv >= SCORE_LEVEL_MIN) & (lv <= 1.0 - SCORE_LEVEL_MIN)):
        raise ValueError(f"{who}: levels: every level must lie in [{SCORE_LEVEL_MIN}, 1 - {SCORE_LEVEL_MIN}], got {lv.tolist()}")
    return np.ascontiguousarray(lv)


def _pack_score(who, K, D, steps, CC, DD, log_Rchols, Y_test, levels, targets_per_pass):
    """Checks shared by the score functions (before the library is loaded): the emission and Y_test as `_pack_summary`, the levels,
    targets_per_pass, 1 <= K <= 65536 and the 2^31 limits."""
    if not 1 <= K <= SCORE_MAX_K:
        raise ValueError(f"{who}: the number of mixture components K must lie in [1, {SCORE_MAX_K}], got {K}")
    m = _pack_summary(who, D, steps, CC, DD, log_Rchols, Y_test)
    lv = _pack_levels(who, levels)
    if m["Y"] is None and lv.size == 0:
        raise ValueError(f"{who}: nothing to compute: Y_test is None and levels is empty")
    if isinstance(targets_per_pass, bool) or int(targets_per_pass) != targets_per_pass or int(targets_per_pass) < 0:
        raise ValueError(f"{who}: targets_per_pass must be 0 (automatic) or a positive integer, got {targets_per_pass!r}")
    if steps * m["J"] * K >= 2 ** 31:
        raise ValueError(f"{who}: steps * J * K = {steps * m['J'] * K} must stay below 2^31")
    m.update(levels=np.ascontiguousarray(lv), Q=lv.size, tpp=int(targets_per_pass))
    return m


def _score_call(m, steps):
    """Output arrays and the arguments CC .. quantiles of the two score entry points."""
    J, nt, Q, dp = m["J"], m["n_test"], m["Q"], _lib.dptr
    out = dict(quantiles=np.empty((steps, J, Q)))
    if m["Y"] is not None:
        out.update(crps=np.empty((nt, J)), pit=np.empty((nt, J)))
    opt = lambda k: dp(out[k]) if k in out and out[k].size else None
    args = (dp(m["CC"]), dp(m["DD"]), dp(m["sd"]), J, dp(m["Y"]) if nt else None, nt, dp(m["levels"]) if Q else None, Q, m["tpp"],
            opt("crps"), opt("pit"), opt("quantiles"))
    return out, args, any(a is not None for a in args[-3:])


def _coverage_pairs(levels):
    """(index of p, index of 1 - p) for every level p < 1/2 whose mirror image is a level too"""
    lv = np.asarray(levels, dtype=np.float64)
    pairs = []
    for i, p in enumerate(lv):
        if p < 0.5:
            hit = np.nonzero(np.abs(lv - (1.0 - p)) <= 1e-12)[0]
            if hit.size:
                pairs.append((i, int(hit[0])))
    return pairs


def _coverage(pit, seen, levels, axis=None):
    """Share of the observed targets (`seen`) with p <= pit <= 1 - p, per symmetric pair of levels (last axis), over all targets or
    along `axis`; NaN where nothing is observed.  Returns the shares and the lower levels p."""
    pairs = _coverage_pairs(levels)
    n = np.sum(seen, axis=axis)
    cov = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, k in pairs:
            inside = seen & (pit >= levels[i]) & (pit <= levels[k])
            cov.append(np.where(n > 0, np.sum(inside, axis=axis) / n, np.nan))
    shape = np.shape(n) + (len(pairs),)
    return (np.stack(cov, axis=-1) if pairs else np.empty(shape)), np.array([levels[i] for i, _ in pairs], dtype=np.float64)


def _score_dict(m, out, Y_train_std):
    """The dict the score functions return: quantiles (steps, J, Q) and levels (Q,); with Y_test crps and pit (n_test, J), NaN where
    the target is NaN, crps_mean over the observed targets (NaN without any), crps_mean_original_units (times Y_train_std),
    coverage (one share per symmetric pair of levels p, 1 - p: the observed targets with p <= pit <= 1 - p) and coverage_levels
    (the p of each pair); without Y_test those are None."""
    res = dict(crps=None, pit=None, quantiles=out["quantiles"], levels=m["levels"], crps_mean=None, crps_mean_original_units=None,
               coverage=None, coverage_levels=None)
    if m["Y"] is not None:
        crps, pit = out["crps"], out["pit"]
        seen = ~np.isnan(m["Y"])
        mean = float(np.sum(crps[seen]) / np.sum(seen)) if np.any(seen) else float("nan")
        cov, low = _coverage(pit, seen, m["levels"])
        res.update(crps=crps, pit=pit, crps_mean=mean, crps_mean_original_units=mean * float(Y_train_std), coverage=cov,
                   coverage_levels=low)
    return res


def _score_points(who, x, K1, K2, steps, D, strides, CC, DD, log_Rchols, Y_test, levels, Y_train_std, targets_per_pass):
    """The body of `rollout_score` and `particle_score`: x contiguous, component k = k1 * K2 + k2 at the strides given."""
    if not 1 <= D <= SCORE_MAX_D_POINTS:
        raise ValueError(f"{who}: 1 <= D <= {SCORE_MAX_D_POINTS} is needed, got {D}")
    if x.size >= 2 ** 31:
        raise ValueError(f"{who}: the stack holds {x.size} numbers: it must stay below 2^31")
    m = _pack_score(who, K1 * K2, D, steps, CC, DD, log_Rchols, Y_test, levels, targets_per_pass)
    out, args, work = _score_call(m, steps)
    if work:
        rc = _lib.load().ffvd_score_points(_lib.dptr(x), K1, K2, steps, D, *strides, *args)
        _lib.check(rc, None, who)
    return _score_dict(m, out, Y_train_std)


def rollout_score(predict_x, CC, DD, log_Rchols, Y_test=None, *, levels=SCORE_LEVELS, Y_train_std=1.0, targets_per_pass=0):
    """CRPS, PIT and predictive quantiles of the held-out predictive distribution of rollouts on the GPU (`ffvd_score_points`): the
    sibling of `rollout_summary` on the stack the caller holds.  For row t and output j the distribution is the equal-weight mixture
    of the K = N (or G R) Gaussians N(CC[:, j] . predict_x[k, t] + DD_j, sd_j^2), the mixture whose log density `rollout_summary`
    returns as lpd.  With A(d, v) = E|N(d, v)|: crps = mean_k A(y - mu_k, v_k) - (1 / (2 K^2)) sum_kl A(mu_k - mu_l, v_k + v_l),
    pit = F(y) with F the mixture's distribution function, quantiles[t, j, q] = the x with F(x) = levels[q] (for every row: they
    need no target).  predict_x (N, steps, D) or (G, R, steps, D), D <= 32, K <= 65536; CC, DD, log_Rchols and Y_test
    (n_test <= steps, J; NaN = unobserved) as `rollout_summary`; levels: at most 16 numbers in [1e-9, 1 - 1e-9]; targets_per_pass:
    0 (automatic) or the number of targets whose pair sums share a pass of the scratch -- no result depends on it.  Returns the
    dict of `_score_dict`: crps, pit, quantiles, levels, crps_mean, crps_mean_original_units, coverage, coverage_levels.  The stack
    is not scanned for non-finite values: such a component makes the outputs of its row NaN and nothing else."""
    who = "rollout_score"
    px = _lib.as_f64(predict_x)
    if px.ndim not in (3, 4):
        raise ValueError(f"{who}: predict_x: expected (N, steps, D) or (G, R, steps, D), got {px.shape}")
    steps, D = px.shape[-2:]
    K = int(np.prod(px.shape[:-2]))
    if K < 1 or steps < 1 or D < 1:
        raise ValueError(f"{who}: at least one rollout, one step and one latent dim are needed, got {px.shape}")
    return _score_points(who, px, K, 1, steps, D, (steps * D, 0, D), CC, DD, log_Rchols, Y_test, levels, Y_train_std, targets_per_pass)


def particle_score(particles, CC, DD, log_Rchols, Y_test=None, *, levels=SCORE_LEVELS, Y_train_std=1.0, targets_per_pass=0):
    """`rollout_score` on particle sets: particles (G, T, N, D), the layout of `fc_particles` of the particle forecasts with its
    (origin, horizon) axes flattened and of the filters' `particles` with the record and row axes flattened.  Row t is scored by
    the mixture of the K = G N particles' emissions, component k = g N + i; read through strides, no copy is made.  The other
    parameters and the returned dict are `rollout_score`'s; the same components in the same order give the same bits in either
    layout."""
    who = "particle_score"
    p = _lib.as_f64(particles)
    if p.ndim != 4:
        raise ValueError(f"{who}: particles: expected (G, T, N, D), got {p.shape}")
    G, T, N, D = p.shape
    if G < 1 or T < 1 or N < 1 or D < 1:
        raise ValueError(f"{who}: at least one group, one row, one particle and one latent dim are needed, got {p.shape}")
    return _score_points(who, p, G, N, T, D, (T * N * D, D, N * D), CC, DD, log_Rchols, Y_test, levels, Y_train_std, targets_per_pass)


def moment_score(m_x, S_x, CC, DD, log_Rchols, Y_test=None, *, levels=SCORE_LEVELS, Y_train_std=1.0, targets_per_pass=0):
    """`rollout_score` for Gaussian states (`ffvd_score_moments`): the sibling of `moment_summary`.  m_x (G, steps, D), S_x
    (G, steps, D, D), D <= 8; row t and output j are scored by the mixture of the G Gaussians N(CC_j^T m_g + DD_j,
    CC_j^T S_g CC_j + sd_j^2), the components of `moment_summary`'s lpd.  The other parameters and the returned dict are
    `rollout_score`'s."""
    who = "moment_score"
    m, S = _lib.as_f64(m_x), _lib.as_f64(S_x)
    if m.ndim != 3 or S.shape != m.shape + (m.shape[2],):
        raise ValueError(f"{who}: expected m_x (G, steps, D) and S_x (G, steps, D, D), got {m.shape} and {S.shape}")
    G, steps, D = m.shape
    if G < 1 or steps < 1 or not 1 <= D <= MOMENT_MAX_D:
        raise ValueError(f"{who}: at least one group, one step and 1 <= D <= {MOMENT_MAX_D} are needed, got {m.shape}")
    if S.size >= 2 ** 31:
        raise ValueError(f"{who}: G * steps * D * D = {S.size} must stay below 2^31")
    s = _pack_score(who, G, D, steps, CC, DD, log_Rchols, Y_test, levels, targets_per_pass)
    out, args, work = _score_call(s, steps)
    if work:
        rc = _lib.load().ffvd_score_moments(_lib.dptr(m), _lib.dptr(S), G, steps, D, *args)
        _lib.check(rc, None, who)
    return _score_dict(s, out, Y_train_std)


def forecast_score(fan, Y_obs, CC, DD, log_Rchols, *, levels=SCORE_LEVELS, use="auto", Y_train_std=1.0):
    """CRPS, PIT and predictive quantiles of a forecast fan: `fan` is the dict one of the six forecast functions returned with
    return_tracks=True (m_fc, S_fc) or return_particles=True (fc_particles); Y_obs (n, J) is the record that was forecast.  The
    targets are Y_obs[origins[b] + k], k = 1 .. h, as in that dict's curves.  use: "particles" scores the mixture of the G N
    particles' emissions (`particle_score`), "moments" the mixture of the G per-group Gaussians (`moment_score`), "auto" the
    particles when the fan has them, else the moments.  For the adapted rule fc_particles is the set AFTER the draw: its point
    mixture is the sampled form of the Rao-Blackwellised predictive whose density that fan reports, and use="moments" scores the
    per-chain Gaussians instead.  Returns a dict: crps, pit (B, h, J), NaN where the target is unobserved; quantiles (B, h, J, Q);
    levels; crps_mean, crps_mean_original_units, coverage, coverage_levels over all observed targets; the curves over the origins
    n_h (h, J), crps_h (h, J) and coverage_h (h, J, pairs), NaN where n_h = 0; origins; used ("moments" or "particles")."""
    who = "forecast_score"
    if use not in SCORE_USES:
        raise ValueError(f"{who}: use: expected one of {list(SCORE_USES)}, got {use!r}")
    if not isinstance(fan, dict) or "origins" not in fan:
        raise ValueError(f"{who}: fan: expected the dict a forecast function returned (with origins)")
    has_p, has_m = fan.get("fc_particles") is not None, fan.get("m_fc") is not None and fan.get("S_fc") is not None
    if use == "particles" and not has_p:
        raise ValueError(f"{who}: use=\"particles\" needs fc_particles: call the forecast with return_particles=True")
    if use == "moments" and not has_m:
        raise ValueError(f"{who}: use=\"moments\" needs m_fc and S_fc: call the forecast with return_tracks=True")
    if not (has_p or has_m):
        raise ValueError(f"{who}: fan holds neither fc_particles nor m_fc / S_fc: call the forecast with return_particles=True or "
                         "return_tracks=True")
    used = "particles" if (use == "particles" or (use == "auto" and has_p)) else "moments"
    org = np.asarray(fan["origins"])
    if org.ndim != 1 or org.size < 1 or not np.issubdtype(org.dtype, np.integer):
        raise ValueError(f"{who}: fan[\"origins\"]: expected a non-empty vector of integers")
    org, B = org.astype(np.int64), org.size
    if used == "particles":
        stack = _lib.as_f64(fan["fc_particles"])
        if stack.ndim != 5 or stack.shape[1] != B:
            raise ValueError(f"{who}: fc_particles: expected (G, {B}, h, N, D), got {stack.shape}")
        G, _, h, N, D = stack.shape
    else:
        stack, S = _lib.as_f64(fan["m_fc"]), _lib.as_f64(fan["S_fc"])
        if stack.ndim != 4 or stack.shape[1] != B or S.shape != stack.shape + (stack.shape[3],):
            raise ValueError(f"{who}: expected m_fc (G, {B}, h, D) and S_fc (G, {B}, h, D, D), got {stack.shape} and {S.shape}")
        G, _, h, D = stack.shape
    Y = np.asarray(Y_obs, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.ndim != 2:
        raise ValueError(f"{who}: Y_obs: expected (n, J), got {Y.shape}")
    if h < 1 or org[0] < 0 or np.any(np.diff(org) <= 0) or org[-1] + h > Y.shape[0] - 1:
        raise ValueError(f"{who}: origins and horizon {h} do not fit a record of {Y.shape[0]} rows")
    J = Y.shape[1]
    Yt = Y[org[:, None] + 1 + np.arange(h)[None, :]]                                         # (B, h, J), as `_forecast_dict`
    kw = dict(levels=levels, Y_train_std=Y_train_std)
    if used == "particles":
        r = particle_score(stack.reshape(G, B * h, N, D), CC, DD, log_Rchols, Yt.reshape(B * h, J), **kw)
    else:
        r = moment_score(stack.reshape(G, B * h, D), S.reshape(G, B * h, D, D), CC, DD, log_Rchols, Yt.reshape(B * h, J), **kw)
    crps, pit = r["crps"].reshape(B, h, J), r["pit"].reshape(B, h, J)
    seen = ~np.isnan(Yt)
    n_h = np.sum(seen, axis=0).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        crps_h = np.where(n_h > 0, np.sum(np.where(seen, crps, 0.0), axis=0) / n_h, np.nan)
    coverage_h, _ = _coverage(pit, seen, r["levels"], axis=0)
    r.update(crps=crps, pit=pit, quantiles=r["quantiles"].reshape(B, h, J, -1), n_h=n_h, crps_h=crps_h, coverage_h=coverage_h,
             origins=org, used=used)
    return r


def pg_sweep(Lm_inverse_seq, Z, kern, U_val, X_ref, Y, control_inputs, CC, DD, Rchols, Q, x0, eps, unif):
    """One particle-Gibbs sweep over the latent trajectory: the INTENT of BaseModel.PG_for_X_speedup
    (base_model.py:78-138; the op as written never updates X, see include/ffvd_abi.h `ffvd_op_pg_sweep`).

    X_ref (X_N, D): the current trajectory = the reference particle; Y (>= X_N-1, Ydim); control_inputs (>= X_N-1, C) or
    None; Rchols (Ydim, Ydim) = likelihood.Rchols = exp(log_Rchols), lower triangular; Q (D,);
    x0 (PG_particles-1, D): the N(0, I) start of :79; eps (X_N-1, PG_particles-1, D): the normal draws of :101;
    unif (X_N-1, PG_particles-1) in [0, 1): the categorical draws of :113 as inverse-CDF uniforms.
    Returns particles (X_N, PG_particles-1, D) (`resampled_X`, :133) and idx (X_N-1, PG_particles-1)."""
    kind, _, logvar, loglen = stack_hypers(kern)
    D = len(kern)
    Z = _lib.as_f64(Z)
    M, P = Z.shape
    C = P - D
    X_ref = _lib.as_f64(X_ref)
    if X_ref.ndim != 2 or X_ref.shape[1] != D:
        raise ValueError(f"X_ref: expected (X_N, {D}), got {X_ref.shape}")
    XN = X_ref.shape[0]
    steps = XN - 1
    x0 = _lib.as_f64(x0)
    if x0.ndim != 2 or x0.shape[1] != D or x0.shape[0] < 1:
        raise ValueError(f"x0: expected (PG_particles - 1, {D}), got {x0.shape}")
    R = x0.shape[0]
    eps = _lib.as_f64(eps, (steps, R, D), "eps")
    unif = _lib.as_f64(unif, (steps, R), "unif")
    if unif.size and (unif.min() < 0.0 or unif.max() >= 1.0):
        raise ValueError("unif: the categorical draws are inverse-CDF uniforms in [0, 1)")
    Y = _lib.as_f64(Y)
    if Y.ndim != 2 or Y.shape[0] < steps:
        raise ValueError(f"Y: need at least {steps} rows")
    Ydim = Y.shape[1]
    Yc = np.ascontiguousarray(Y[:steps])
    ctrl = None
    if C > 0:
        ci = _lib.as_f64(control_inputs)
        if ci.ndim != 2 or ci.shape[1] != C or ci.shape[0] < steps:
            raise ValueError(f"control_inputs: need at least {steps} rows of {C} columns")
        ctrl = np.ascontiguousarray(ci[:steps])
    W = _lib.as_f64(np.stack([np.asarray(w) for w in Lm_inverse_seq]), (D, M, M), "Lm_inverse_seq")
    f = _lib.as_f64(U_val, (M, D), "U_val")
    CC = _lib.as_f64(CC, (D, Ydim), "CC")
    DD = _lib.as_f64(np.asarray(DD).reshape(-1), (Ydim,), "DD")
    Rch = _lib.as_f64(Rchols, (Ydim, Ydim), "Rchols")
    log_Q = np.log(_lib.as_f64(Q, (D,), "Q"))
    parts = np.empty((XN, R, D))
    idx = np.zeros((max(steps, 0), R), dtype=np.int32)
    rc = _lib.load().ffvd_op_pg_sweep(kind, _lib.dptr(W), _lib.dptr(Z), M, P, D, _lib.dptr(logvar),
                                      None if loglen is None else _lib.dptr(loglen), _lib.dptr(f), _lib.dptr(X_ref), XN,
                                      _lib.dptr(Yc), Ydim, None if ctrl is None else _lib.dptr(ctrl), C, _lib.dptr(CC),
                                      _lib.dptr(DD), _lib.dptr(Rch), _lib.dptr(log_Q), R, _lib.dptr(x0), _lib.dptr(eps),
                                      _lib.dptr(unif), _lib.dptr(parts), idx.ctypes.data)
    _lib.check(rc, None, "ffvd_op_pg_sweep")
    return parts, idx
