"""Argument limits of the prediction entry points, without a GPU: ffvd_op_rollout, ffvd_op_pg_sweep and
ffvd_op_conditional_precalc return FFVD_EINVAL before any device work when M > 2048 (the cap of the step kernels and of
qsqrt_inflation's 2048-double row), P > 32 (MAXP, the LDS layout), P != D + C, n_free + 1 > 1024 particles or Ydim > 8.

Every array is allocated at the size the rejected argument implies, and every other argument is valid: the rejected
argument is the only reason for the status, and a missing check could not make the call read past an array."""
import numpy as np
import pytest

from ffvd_amd import _lib

E = _lib.FFVD_EINVAL
BIG_M = 2049
BIG_P = 33            # MAXP + 1


def _rollout(*, M=4, D=2, C=1, P=None, R=2, steps=3):
    P = D + C if P is None else P
    lib, dp = _lib.load(), _lib.dptr
    W, Z, f, q = np.zeros((D, M, M)), np.zeros((M, P)), np.zeros((M, D)), np.zeros((M, M))
    lv, ll, lq, xl = np.zeros(D), np.zeros((D, P)), np.zeros(D), np.zeros(D)
    ctrl, eps = np.zeros((steps, max(C, 1))), np.zeros((steps, R, D))
    px, pv = np.zeros((R, steps, D)), np.zeros((R, steps, D))
    return lib.ffvd_op_rollout(0, dp(W), dp(Z), M, P, D, dp(lv), dp(ll), dp(f), dp(q), dp(xl), R, dp(ctrl), C, steps, dp(lq),
                               dp(eps), dp(px), dp(pv))


def _pg_sweep(*, M=4, D=2, C=1, P=None, n_free=3, XN=4, Ydim=1):
    P = D + C if P is None else P
    lib, dp = _lib.load(), _lib.dptr
    W, Z, U = np.zeros((D, M, M)), np.zeros((M, P)), np.zeros((M, D))
    lv, ll, lq = np.zeros(D), np.zeros((D, P)), np.zeros(D)
    Xr, Y, ctrl = np.zeros((XN, D)), np.zeros((XN - 1, Ydim)), np.zeros((XN - 1, max(C, 1)))
    CC, DD, Rch = np.zeros((D, Ydim)), np.zeros(Ydim), np.eye(Ydim)
    x0, eps, u = np.zeros((n_free, D)), np.zeros((XN - 1, n_free, D)), np.zeros((XN - 1, n_free))
    parts, idx = np.zeros((XN, n_free, D)), np.zeros((XN - 1, n_free), dtype=np.int32)
    return lib.ffvd_op_pg_sweep(0, dp(W), dp(Z), M, P, D, dp(lv), dp(ll), dp(U), dp(Xr), XN, dp(Y), Ydim, dp(ctrl), C, dp(CC),
                                dp(DD), dp(Rch), dp(lq), n_free, dp(x0), dp(eps), dp(u), dp(parts), idx.ctypes.data)


def _precalc(*, M=4, D=2, P=3, N=2):
    lib, dp = _lib.load(), _lib.dptr
    W, X, Z, f, q = np.zeros((D, M, M)), np.zeros((N, P)), np.zeros((M, P)), np.zeros((M, D)), np.zeros((M, M))
    lv, ll = np.zeros(D), np.zeros((D, P))
    mean, var = np.zeros((N, D)), np.zeros((N, D))
    return lib.ffvd_op_conditional_precalc(0, dp(W), dp(X), N, dp(Z), M, P, D, dp(lv), dp(ll), dp(f), dp(q), dp(mean), dp(var))


def _rejected(rc, who):
    assert rc == E, rc
    assert f"{who}: bad argument".encode() in _lib.load().ffvd_last_error(None)


@pytest.mark.parametrize("case", ["M=2049", "P=33"])
def test_prediction_entry_points_reject_m_and_p_beyond_their_caps(case):
    ov = dict(M=BIG_M) if case == "M=2049" else dict(D=2, C=BIG_P - 2)
    _rejected(_rollout(**ov), "ffvd_op_rollout")
    _rejected(_pg_sweep(**ov), "ffvd_op_pg_sweep")
    _rejected(_precalc(**(dict(M=BIG_M) if case == "M=2049" else dict(P=BIG_P))), "ffvd_op_conditional_precalc")


def test_step_loops_reject_p_other_than_d_plus_c():
    for P in (2, 4):                                     # D = 2, C = 1
        _rejected(_rollout(P=P), "ffvd_op_rollout")
        _rejected(_pg_sweep(P=P), "ffvd_op_pg_sweep")


def test_pg_sweep_rejects_more_than_1024_particles_and_ydim_above_8():
    _rejected(_pg_sweep(n_free=1024), "ffvd_op_pg_sweep")      # PG_particles = n_free + 1 = 1025
    _rejected(_pg_sweep(Ydim=9), "ffvd_op_pg_sweep")
