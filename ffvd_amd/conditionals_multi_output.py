"""GP conditional operators for D independent kernels -- counterpart of vfegpssm/conditionals_multi_output.py.

Same function names and argument order as the reference; NumPy in/out; all arithmetic in libffvd_hip.so.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .kernels import stack_hypers

JITTER = 1e-5      # conditionals_multi_output.py:108,159


def kernel_pre_cal(X, kern):
    """Per kernel d: L_d = chol(K_d(X) + 1e-5 I); returns the list of L_d^{-T} (upper triangular)
    (conditionals_multi_output.py:124-169)."""
    lib = _lib.load()
    kind, _, logvar, loglen = stack_hypers(kern)
    X = _lib.as_f64(X)
    M, P = X.shape
    D = len(kern)
    out = np.empty((D, M, M))
    rc = lib.ffvd_op_kernel_pre_cal(kind, _lib.dptr(X), M, P, D, _lib.dptr(logvar),
                                    None if loglen is None else _lib.dptr(loglen), JITTER, _lib.dptr(out))
    _lib.check(rc, None, "kernel_pre_cal")
    return [out[d] for d in range(D)]


def collapse_after_kernel_precalculation(Lm_inverse_seq, X_combine, X, Z, kern, Q, batch_size, Y_N):
    """Collapsed-U ELBO terms (-term1/Y_N, -term2/Y_N, -trace/Y_N) (conditionals_multi_output.py:230-257)."""
    lib = _lib.load()
    kind, _, logvar, loglen = stack_hypers(kern)
    D = len(kern)
    Z = _lib.as_f64(Z)
    M, P = Z.shape
    X = _lib.as_f64(X)
    T = X.shape[0] - 1
    Xc = _lib.as_f64(X_combine, (T, P), "X_combine")
    X = _lib.as_f64(X, (T + 1, D), "X")
    W = _lib.as_f64(np.stack([np.asarray(w) for w in Lm_inverse_seq]), (D, M, M), "Lm_inverse_seq")
    Q = _lib.as_f64(Q, (D,), "Q")
    out = np.zeros(3)
    rc = lib.ffvd_op_collapse(kind, _lib.dptr(W), _lib.dptr(Xc), _lib.dptr(X), _lib.dptr(Z), T, M, P, D,
                              _lib.dptr(logvar), None if loglen is None else _lib.dptr(loglen), _lib.dptr(Q),
                              float(batch_size), float(Y_N), _lib.dptr(out))
    _lib.check(rc, None, "collapse_after_kernel_precalculation")
    return float(out[0]), float(out[1]), float(out[2])


def _qsqrt_slice0(q_sqrt, M, D, who):
    """The M x M matrix q0 that inflates EVERY dim: slice 0 of a D x M x M stack (the reference hands the whole stack to every dim
    and keeps index 0), or diag(q_sqrt[:, 0]) of an M x D one.  Shapes are checked before any device call."""
    q = np.asarray(q_sqrt, dtype=np.float64)
    if q.ndim == 3 and q.shape == (D, M, M):
        return np.ascontiguousarray(q[0])
    if q.ndim == 2 and q.shape == (M, D):
        return np.diag(q[:, 0])
    raise ValueError(f"{who}: Bad dimension for q_sqrt: expected ({D}, {M}, {M}) or ({M}, {D}), got {q.shape}")


def _cov_outputs(N, D, full_cov):
    return np.empty((N, D)), (np.empty((D, N, N)) if full_cov else np.empty((N, D)))


def conditional(Xnew, X, kern, f, *, full_cov=False, q_sqrt=None, white=False, return_Lm=False, jitter=JITTER):
    """Mean (N x D) and variance of D independent GPs at Xnew given whitened values f at X
    (conditionals_multi_output.py:73-120 -> base_conditional :6-70).  white=True only (return_Lm=True is broken in the
    reference).

    With F_d = K_d(Xnew, X) L_d^-T, L_d = chol(K_d(X, X) + jitter I):
      full_cov=False: var is N x D, var[:, d] = Kdiag_d(Xnew) - sum_j F_d[:, j]^2.
      full_cov=True:  var is D x N x N (GPflow's R x N x N layout), var[d] = K_d(Xnew, Xnew) - F_d F_d^T, exactly symmetric; the
                      mean is the full_cov=False mean.  Stated departure: the reference's final stacking
                      (`np.asarray(f_var)[:, :, 0].T`, :120) is written for N x 1 blocks and does not return a covariance for
                      N x N ones; it is not reproduced.
      q_sqrt: D x M x M or M x D.  As in conditional_after_kernel_precalculation, slice 0 inflates EVERY dim: with
              q0 = q_sqrt[0] as given (no triangle mask), or q0 = diag(q_sqrt[:, 0]), E_d = F_d q0 adds sum_j E_d[:, j]^2 to the
              per-point variance and E_d E_d^T to the covariance.  Open point: the reference's base_conditional q_sqrt block
              (:50-63) may mask q_sqrt to its lower triangle (GPflow's band_part); that cannot be checked here.  The precalc
              form does not mask; for a lower-triangular q_sqrt both readings agree."""
    if not white or return_Lm:
        raise NotImplementedError("conditional: only white=True, return_Lm=False")
    lib = _lib.load()
    kind, _, logvar, loglen = stack_hypers(kern)
    D = len(kern)
    X = _lib.as_f64(X)
    M, P = X.shape
    Xnew = _lib.as_f64(Xnew)
    if Xnew.ndim != 2 or Xnew.shape[1] != P:
        raise ValueError(f"Xnew: expected (N, {P}), got {Xnew.shape}")
    N = Xnew.shape[0]
    f = _lib.as_f64(f, (M, D), "f")
    if not full_cov and q_sqrt is None:
        mean, var = np.empty((N, D)), np.empty((N, D))
        rc = lib.ffvd_op_conditional(kind, _lib.dptr(Xnew), N, _lib.dptr(X), M, P, D, _lib.dptr(logvar),
                                     None if loglen is None else _lib.dptr(loglen), _lib.dptr(f), float(jitter),
                                     _lib.dptr(mean), _lib.dptr(var))
        _lib.check(rc, None, "conditional")
        return mean, var
    qs = None if q_sqrt is None else _qsqrt_slice0(q_sqrt, M, D, "conditional")
    mean, var = _cov_outputs(N, D, full_cov)
    rc = lib.ffvd_op_conditional_cov(kind, _lib.dptr(Xnew), N, _lib.dptr(X), M, P, D, _lib.dptr(logvar),
                                     None if loglen is None else _lib.dptr(loglen), _lib.dptr(f),
                                     None if qs is None else _lib.dptr(qs), int(bool(full_cov)), float(jitter),
                                     _lib.dptr(mean), _lib.dptr(var))
    _lib.check(rc, None, "conditional")
    return mean, var


def collapse_u_mean_after_kernel_precalculation(Lm_inverse_seq, X_combine, X, Z, kern, Q):
    """Posterior mean of the whitened inducing outputs (M x D) and the stack of L_H^{-T} (D x M x M)
    (conditionals_multi_output.py:206-227)."""
    lib = _lib.load()
    kind, _, logvar, loglen = stack_hypers(kern)
    D = len(kern)
    Z = _lib.as_f64(Z)
    M, P = Z.shape
    X = _lib.as_f64(X)
    T = X.shape[0] - 1
    Xc = _lib.as_f64(X_combine, (T, P), "X_combine")
    X = _lib.as_f64(X, (T + 1, D), "X")
    W = _lib.as_f64(np.stack([np.asarray(w) for w in Lm_inverse_seq]), (D, M, M), "Lm_inverse_seq")
    Q = _lib.as_f64(Q, (D,), "Q")
    U_mean, Hinv = np.empty((M, D)), np.empty((D, M, M))
    rc = lib.ffvd_op_collapse_u_mean(kind, _lib.dptr(W), _lib.dptr(Xc), _lib.dptr(X), _lib.dptr(Z), T, M, P, D,
                                     _lib.dptr(logvar), None if loglen is None else _lib.dptr(loglen), _lib.dptr(Q),
                                     _lib.dptr(U_mean), _lib.dptr(Hinv))
    _lib.check(rc, None, "collapse_u_mean_after_kernel_precalculation")
    return U_mean, Hinv


def conditional_after_kernel_precalculation(Lm_inverse_seq, Xnew, Z, kern, f, *, full_cov=False, q_sqrt=None,
                                            white=False, return_Lm=False):
    """conditional() with the pre-computed L^{-T} stack (conditionals_multi_output.py:306-387); mean N x D, var N x D or, with
    full_cov=True, D x N x N (the layout and the stated departure of conditional()).

    q_sqrt may be a D x M x M stack: as in the reference, slice d = 0 inflates the variance of EVERY dim
    (the stack is handed to every dim at :317 and `[:, :, 0]` at :322 keeps slice 0).  An M x D q_sqrt
    inflates by diag(q_sqrt[:, 0]) (:369, column 0 kept the same way)."""
    if not white or return_Lm:
        raise NotImplementedError("conditional_after_kernel_precalculation: only white=True, return_Lm=False")
    lib = _lib.load()
    kind, _, logvar, loglen = stack_hypers(kern)
    D = len(kern)
    Z = _lib.as_f64(Z)
    M, P = Z.shape
    Xnew = _lib.as_f64(Xnew)
    if Xnew.ndim != 2 or Xnew.shape[1] != P:
        raise ValueError(f"Xnew: expected (N, {P}), got {Xnew.shape}")
    N = Xnew.shape[0]
    f = _lib.as_f64(f, (M, D), "f")
    W = _lib.as_f64(np.stack([np.asarray(w) for w in Lm_inverse_seq]), (D, M, M), "Lm_inverse_seq")
    qs = None
    if q_sqrt is not None:
        q = np.asarray(q_sqrt, dtype=np.float64)
        if q.ndim == 3 and q.shape[1:] == (M, M):
            qs = np.ascontiguousarray(q[0])
        elif q.ndim == 2 and q.shape == (M, D):
            qs = np.diag(q[:, 0])
        else:
            raise ValueError(f"Bad dimension for q_sqrt: expected (D, {M}, {M}) or ({M}, {D}), got {q.shape}")
    if full_cov:
        mean, var = _cov_outputs(N, D, True)
        rc = lib.ffvd_op_conditional_precalc_cov(kind, _lib.dptr(W), _lib.dptr(Xnew), N, _lib.dptr(Z), M, P, D,
                                                 _lib.dptr(logvar), None if loglen is None else _lib.dptr(loglen),
                                                 _lib.dptr(f), None if qs is None else _lib.dptr(qs), 1, _lib.dptr(mean),
                                                 _lib.dptr(var))
        _lib.check(rc, None, "conditional_after_kernel_precalculation")
        return mean, var
    mean, var = np.empty((N, D)), np.empty((N, D))
    rc = lib.ffvd_op_conditional_precalc(kind, _lib.dptr(W), _lib.dptr(Xnew), N, _lib.dptr(Z), M, P, D,
                                         _lib.dptr(logvar), None if loglen is None else _lib.dptr(loglen),
                                         _lib.dptr(f), None if qs is None else _lib.dptr(qs), _lib.dptr(mean),
                                         _lib.dptr(var))
    _lib.check(rc, None, "conditional_after_kernel_precalculation")
    return mean, var


def pack_posterior_groups(Zs, kerns, Xs, control_inputs, Qs, who):
    """The packed inputs of the grouped posterior operators (`ffvd_op_posterior_grouped`, `ffvd_op_posterior_rollout_grouped`), with
    every shape checked before any device call.  `Zs` / `kerns`: one model (an (M, P) array and a list of D kernels: shared by all
    groups) or a length-G sequence of them; `Xs`: G trajectories (T+1, D); `Qs`: G vectors (D,), or one for all groups;
    control_inputs: rows [0, T) are used ((>= T, C); None or no columns when P = D)."""
    G = len(Xs)
    if G < 1:
        raise ValueError(f"{who}: at least one group is needed")
    one_model = len(kerns) > 0 and not isinstance(kerns[0], (list, tuple))
    if one_model:
        if np.ndim(Zs) != 2:
            raise ValueError(f"{who}: Zs: one list of kernels goes with one (M, P) array, got an array of {np.ndim(Zs)} dimensions")
        Zl, kl = [Zs], [kerns]
    else:
        Zl, kl = list(Zs), list(kerns)
        if len(Zl) != len(kl):
            raise ValueError(f"{who}: Zs: expected {len(kl)} models (one per kernel list), got {len(Zl)}")
    n_models = len(kl)
    if n_models not in (1, G):
        raise ValueError(f"{who}: n_models: expected 1 or {G} (one per group of Xs), got {n_models}")
    hy = [stack_hypers(k) for k in kl]
    kind, D = hy[0][0], len(kl[0])
    Z0 = np.asarray(Zl[0])
    if Z0.ndim != 2:
        raise ValueError(f"{who}: Zs[0]: expected (M, P), got {Z0.shape}")
    M, P = Z0.shape
    C = P - D
    if C < 0:
        raise ValueError(f"{who}: Zs: {P} input columns for {D} latent dims")
    Z = np.empty((n_models, M, P))
    logvar = np.empty((n_models, D))
    loglen = None if hy[0][3] is None else np.empty((n_models, D, P))
    for m in range(n_models):
        if hy[m][0] != kind:
            raise ValueError(f"{who}: kerns[{m}]: every group must use the same kernel type")
        if len(kl[m]) != D:
            raise ValueError(f"{who}: kerns[{m}]: expected {D} kernels (one per latent dim), got {len(kl[m])}")
        Z[m] = _lib.as_f64(Zl[m], (M, P), f"Zs[{m}]")
        logvar[m] = _lib.as_f64(hy[m][2], (D,), f"kerns[{m}] logvariance")
        if loglen is not None:
            loglen[m] = _lib.as_f64(hy[m][3], (D, P), f"kerns[{m}] loglengthscales")
    X0 = np.asarray(Xs[0])
    if X0.ndim != 2 or X0.shape[1] != D or X0.shape[0] < 2:
        raise ValueError(f"{who}: Xs[0]: expected (T + 1, {D}) with T >= 1, got {X0.shape}")
    T = X0.shape[0] - 1
    X = np.empty((G, T + 1, D))
    for g in range(G):
        X[g] = _lib.as_f64(Xs[g], (T + 1, D), f"Xs[{g}]")
    Qa = np.asarray(Qs, dtype=np.float64)
    if Qa.shape == (D,):
        Qa = np.broadcast_to(Qa, (G, D))
    if Qa.shape != (G, D):
        raise ValueError(f"{who}: Qs: expected {G} groups of ({D},), got {Qa.shape}")
    log_Q = np.ascontiguousarray(np.log(Qa))
    ctrl = None
    if C > 0:
        ci = _lib.as_f64(control_inputs)
        if ci.ndim != 2 or ci.shape[1] != C or ci.shape[0] < T:
            raise ValueError(f"{who}: control_inputs: need at least {T} rows of {C} columns")
        ctrl = np.ascontiguousarray(ci[:T])
    return dict(kind=kind, G=G, n_models=n_models, M=M, P=P, D=D, C=C, T=T, Z=Z, logvar=logvar, loglen=loglen, X=X, log_Q=log_Q,
                ctrl=ctrl)


def collapse_u_mean_grouped(Zs, kerns, Xs, control_inputs, Qs, *, jitter=JITTER, groups_per_pass=0, return_factors=True):
    """kernel_pre_cal + collapse_u_mean_after_kernel_precalculation (conditionals_multi_output.py:124-169, :206-227, as
    base_model.py:243-256 calls them) for G groups in one call (`ffvd_op_posterior_grouped`): one group per chain (`Zs`, `kerns` one
    model) or per SG-HMC sample (length-G sequences).  Xs: G trajectories (T+1, D); X_combine of group g is [Xs[g][:T], control_inputs[:T]].
    Returns (U_means (G, M, D), H_inv_sqrts (G, D, M, M), Lm_inverse (n_models, D, M, M)); with return_factors=False the two stacks
    are neither packed nor downloaded and come back as None.  groups_per_pass: see include/ffvd_abi.h (0 = automatic)."""
    who = "collapse_u_mean_grouped"
    a = pack_posterior_groups(Zs, kerns, Xs, control_inputs, Qs, who)
    if int(groups_per_pass) < 0:
        raise ValueError(f"{who}: groups_per_pass must be 0 (automatic) or positive")
    G, nm, M, D = a["G"], a["n_models"], a["M"], a["D"]
    U = np.empty((G, M, D))
    Hinv = np.empty((G, D, M, M)) if return_factors else None
    Lm = np.empty((nm, D, M, M)) if return_factors else None
    dp = _lib.dptr
    rc = _lib.load().ffvd_op_posterior_grouped(a["kind"], G, nm, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]),
                                               None if a["loglen"] is None else dp(a["loglen"]), dp(a["X"]),
                                               None if a["ctrl"] is None else dp(a["ctrl"]), a["C"], a["T"], dp(a["log_Q"]),
                                               float(jitter), int(groups_per_pass), None if Lm is None else dp(Lm), dp(U),
                                               None if Hinv is None else dp(Hinv))
    _lib.check(rc, None, who)
    return U, Hinv, Lm


Q_MODES = {"reference": 0, "intent": 1}


def check_conditional_query(who, Xnew, P, q_mode, rows_per_pass, per_group, summary):
    """Xnew as a contiguous (N, P) array and the q_mode code of the grouped conditionals, checked before any device call."""
    if q_mode not in Q_MODES:
        raise ValueError(f"{who}: q_mode: expected one of {sorted(Q_MODES)}, got {q_mode!r}")
    if int(rows_per_pass) < 0:
        raise ValueError(f"{who}: rows_per_pass must be 0 (automatic) or positive")
    if not per_group and not summary:
        raise ValueError(f"{who}: per_group=False and summary=False leave nothing to compute")
    Xnew = _lib.as_f64(Xnew)
    if Xnew.ndim != 2 or Xnew.shape[1] != P:
        raise ValueError(f"{who}: Xnew: expected (N, {P}), got {Xnew.shape}")
    return Xnew, Q_MODES[q_mode]


def pack_conditional_groups(who, Lm_inverse_seqs, Zs, kerns, fs, q_sqrts, Xnew, q_mode, rows_per_pass, per_group, summary):
    """The packed inputs of the grouped conditional operators (`ffvd_op_conditional_grouped`, `ffvd_op_conditional_grad_grouped`), with
    every shape checked before any device call.  The pointer tables `Wt` / `qt` refer to the arrays kept under `keep`."""
    G = len(fs)
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
        raise ValueError(f"{who}: n_models: expected 1 or {G} (one per group of fs), got {nm}")
    hy = [stack_hypers(k) for k in kl]
    kind, D = hy[0][0], len(kl[0])
    Z0 = np.asarray(Zl[0])
    if Z0.ndim != 2:
        raise ValueError(f"{who}: Zs[0]: expected (M, P), got {Z0.shape}")
    M, P = Z0.shape
    if P < D:
        raise ValueError(f"{who}: Zs: {P} input columns for {D} latent dims")
    Xnew, qm = check_conditional_query(who, Xnew, P, q_mode, rows_per_pass, per_group, summary)
    Z, logvar = np.empty((nm, M, P)), np.empty((nm, D))
    loglen = None if hy[0][3] is None else np.empty((nm, D, P))
    Wm, qmats = [], []                                   # (keeps the matrices alive until the call returns)
    for m in range(nm):
        if hy[m][0] != kind:
            raise ValueError(f"{who}: kerns[{m}]: every group must use the same kernel type")
        if len(kl[m]) != D:
            raise ValueError(f"{who}: kerns[{m}]: expected {D} kernels (one per latent dim), got {len(kl[m])}")
        Z[m] = _lib.as_f64(Zl[m], (M, P), f"Zs[{m}]")
        logvar[m] = _lib.as_f64(hy[m][2], (D,), f"kerns[{m}] logvariance")
        if loglen is not None:
            loglen[m] = _lib.as_f64(hy[m][3], (D, P), f"kerns[{m}] loglengthscales")
        if len(Wl[m]) != D:
            raise ValueError(f"{who}: Lm_inverse_seqs[{m}]: expected {D} matrices, got {len(Wl[m])}")
        for d in range(D):
            Wm.append(_lib.as_f64(Wl[m][d], (M, M), f"Lm_inverse_seqs[{m}][{d}]"))
    f = np.empty((G, M, D))
    for g in range(G):
        f[g] = _lib.as_f64(fs[g], (M, D), f"fs[{g}]")
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
    return dict(kind=kind, G=G, n_models=nm, M=M, P=P, D=D, N=Xnew.shape[0], Z=Z, logvar=logvar, loglen=loglen, f=f, Xnew=Xnew, q_mode=qm,
                Wt=Wt, qt=qt, keep=(Wm, qmats))


def conditional_grouped(Lm_inverse_seqs, Zs, kerns, fs, q_sqrts, Xnew, *, q_mode="reference", per_group=True, summary=True,
                        rows_per_pass=0):
    """conditional_after_kernel_precalculation (conditionals_multi_output.py:306-387, white=True, full_cov=False) for G posteriors at
    the same N inputs in one call (`ffvd_op_conditional_grouped`): the transition function f(x, c) of every chain or SG-HMC sample.

    `Zs` / `kerns` / `Lm_inverse_seqs`: one model (an (M, P) array, a list of D kernels, D matrices L^-T: shared by the groups) or
    length-G sequences of them; fs: G arrays (M, D), the whitened inducing outputs; q_sqrts: None (explicit U: no third variance
    term) or G stacks (D, M, M); Xnew (N, P).  q_mode "reference": slice 0 of a group's stack inflates every dim (what
    the reference and the rollouts do); "intent": slice d inflates dim d.
    Returns (means, vars, mix_mean, mix_var): (G, N, D) per group (None unless per_group) and the equal-weight mixture over the
    groups, (N, D): mix_mean = mean_g(mean), mix_var = mean_g(var + mean^2) - mix_mean^2 (None unless summary).
    rows_per_pass: see include/ffvd_abi.h (0 = automatic)."""
    who = "conditional_grouped"
    a = pack_conditional_groups(who, Lm_inverse_seqs, Zs, kerns, fs, q_sqrts, Xnew, q_mode, rows_per_pass, per_group, summary)
    G, N, D = a["G"], a["N"], a["D"]
    means, vars_ = (np.empty((G, N, D)), np.empty((G, N, D))) if per_group else (None, None)
    mm, mv = (np.empty((N, D)), np.empty((N, D))) if summary else (None, None)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = _lib.load().ffvd_op_conditional_grouped(a["kind"], G, a["n_models"], a["Wt"], dp(a["Z"]), a["M"], a["P"], D, dp(a["logvar"]),
                                                 opt(a["loglen"]), dp(a["f"]), a["qt"], a["q_mode"], dp(a["Xnew"]), N, int(rows_per_pass),
                                                 opt(means), opt(vars_), opt(mm), opt(mv))
    _lib.check(rc, None, who)
    return means, vars_, mm, mv


GRAD_KEYS = ("mean", "var", "dmean", "dvar", "mix_mean", "mix_var", "mix_dmean", "mix_dvar")


def grad_outputs(G, N, D, P, per_group, summary, variance):
    """The output arrays of the linearisation operators as a dict over GRAD_KEYS (None where not asked for): per group (G, N, D) and
    (G, N, D, P), the mixture (N, D) and (N, D, P); the mixture values come as a pair, so summary=True forms the variance side."""
    out = dict.fromkeys(GRAD_KEYS)
    if per_group:
        out["mean"], out["dmean"] = np.empty((G, N, D)), np.empty((G, N, D, P))
        if variance:
            out["var"], out["dvar"] = np.empty((G, N, D)), np.empty((G, N, D, P))
    if summary:
        out["mix_mean"], out["mix_var"], out["mix_dmean"] = np.empty((N, D)), np.empty((N, D)), np.empty((N, D, P))
        if variance:
            out["mix_dvar"] = np.empty((N, D, P))
    return out


def check_se_only(who, kind):
    if kind != 0:
        raise ValueError(f"{who}: the input gradients are closed-form for the SE kernel only (a linear kernel's Jacobian is constant)")


def conditional_grad_grouped(Lm_inverse_seqs, Zs, kerns, fs, q_sqrts, Xnew, *, q_mode="reference", per_group=True, summary=True,
                             variance=True, rows_per_pass=0):
    """`conditional_grouped` with the gradients of mean and variance with respect to the rows of Xnew, in one call
    (`ffvd_op_conditional_grad_grouped`): the linearisation of the transition function f(x, c) of every chain or SG-HMC sample.
    SE-ARD kernels only.  Arguments as `conditional_grouped`.

    Returns a dict: mean, var (G, N, D), dmean, dvar (G, N, D, P) with dmean[g, n, d, p] = d mean[g, n, d] / d Xnew[n, p] (the first D
    columns are d/dx, the last C are d/dc) (None unless per_group); mix_mean, mix_var (N, D), mix_dmean, mix_dvar (N, D, P): the
    equal-weight mixture over the groups and its gradients (None unless summary).  variance=False: var, dvar and mix_dvar are None and,
    with summary=False, the variance side is not computed at all.  The local linear model of x' = x + f(x, c) is
    A = I + dmean[..., :D], B = dmean[..., D:].  rows_per_pass: see include/ffvd_abi.h (0 = automatic)."""
    who = "conditional_grad_grouped"
    a = pack_conditional_groups(who, Lm_inverse_seqs, Zs, kerns, fs, q_sqrts, Xnew, q_mode, rows_per_pass, per_group, summary)
    check_se_only(who, a["kind"])
    G, N, D, P = a["G"], a["N"], a["D"], a["P"]
    out = grad_outputs(G, N, D, P, per_group, summary, variance)
    dp = _lib.dptr
    opt = lambda x: None if x is None else dp(x)
    rc = _lib.load().ffvd_op_conditional_grad_grouped(a["kind"], G, a["n_models"], a["Wt"], dp(a["Z"]), a["M"], P, D, dp(a["logvar"]),
                                                      opt(a["loglen"]), dp(a["f"]), a["qt"], a["q_mode"], dp(a["Xnew"]), N,
                                                      int(rows_per_pass), *[opt(out[k]) for k in GRAD_KEYS])
    _lib.check(rc, None, who)
    return out
