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
