"""Argument checks of the full-covariance conditional and the joint draw, without a GPU: the C entry points reject bad
arguments with FFVD_EINVAL before any device work, the Python layer raises ValueError on a wrong q_sqrt / var shape before
any device call."""
import ctypes as C

import numpy as np
import pytest

from ffvd_amd import _lib, conditionals_multi_output as cmo, utils
from ffvd_amd.kernels import SquaredExponential

E = _lib.FFVD_EINVAL


def test_cov_entry_points_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    dp = _lib.dptr
    N, M, P, D = 3, 4, 2, 2
    x, z, f = np.zeros((N, P)), np.zeros((M, P)), np.zeros((M, D))
    lv, ll, q = np.zeros(D), np.zeros((D, P)), np.zeros((M, M))
    W = np.zeros((D, M, M))
    mean, var = np.zeros((N, D)), np.zeros((D, N, N))
    big = 2049
    zb, fb, qb = np.zeros((big, P)), np.zeros((big, D)), np.zeros((1, 1))

    def cov(*, kind=0, X=x, n=N, Z=z, m=M, d=D, f_=f, qs=None, full=1, out_m=mean, out_v=var, loglen=ll):
        return lib.ffvd_op_conditional_cov(kind, None if X is None else dp(X), n, None if Z is None else dp(Z), m, P, d, dp(lv),
                                           None if loglen is None else dp(loglen), None if f_ is None else dp(f_),
                                           None if qs is None else dp(qs), full, 1e-5, None if out_m is None else dp(out_m),
                                           None if out_v is None else dp(out_v))

    assert cov(X=None) == E
    assert cov(Z=None) == E
    assert cov(f_=None) == E
    assert cov(out_m=None) == E
    assert cov(out_v=None) == E
    assert cov(loglen=None) == E                      # SE without lengthscales
    assert cov(kind=7) == E
    assert cov(n=-1) == E
    assert cov(full=2) == E and cov(full=-1) == E
    assert cov(Z=zb, m=big, f_=fb, qs=qb) == E         # q_sqrt needs M <= 2048 (the pointer is not read: validation comes first)
    assert b"ffvd_op_conditional_cov: bad argument" in lib.ffvd_last_error(None)

    def pre(*, W_=W, X=x, n=N, full=1, qs=None, m=M):
        return lib.ffvd_op_conditional_precalc_cov(0, None if W_ is None else dp(W_), None if X is None else dp(X), n, dp(z), m, P,
                                                   D, dp(lv), dp(ll), dp(f), None if qs is None else dp(qs), full, dp(mean),
                                                   dp(var))

    assert pre(W_=None) == E
    assert pre(X=None) == E
    assert pre(n=-5) == E
    assert pre(full=3) == E
    assert pre(m=big, qs=qb) == E
    assert b"ffvd_op_conditional_precalc_cov: bad argument" in lib.ffvd_last_error(None)

    eps, out = np.zeros((N, D)), np.zeros((N, D))
    g = lib.ffvd_op_get_rand_full_cov
    assert g(None, dp(var), dp(eps), N, D, 1e-7, dp(out)) == E
    assert g(dp(mean), None, dp(eps), N, D, 1e-7, dp(out)) == E
    assert g(dp(mean), dp(var), None, N, D, 1e-7, dp(out)) == E
    assert g(dp(mean), dp(var), dp(eps), N, D, 1e-7, None) == E
    assert g(dp(mean), dp(var), dp(eps), -1, D, 1e-7, dp(out)) == E
    assert g(dp(mean), dp(var), dp(eps), N, 0, 1e-7, dp(out)) == E
    assert g(dp(mean), dp(var), dp(eps), N, D, -1.0, dp(out)) == E
    assert g(dp(mean), dp(var), dp(eps), N, D, float("nan"), dp(out)) == E
    assert b"ffvd_op_get_rand_full_cov: bad argument" in lib.ffvd_last_error(None)


def _setup(M=5, P=2, D=3, N=4):
    rng = np.random.default_rng(3)
    kern = [SquaredExponential(P, variance=1.0, lengthscales=np.ones(P)) for _ in range(D)]
    return rng.standard_normal((N, P)), rng.standard_normal((M, P)), kern, rng.standard_normal((M, D))


@pytest.mark.parametrize("shape", [(3, 5), (5, 5), (5,), (2, 5, 5), (3, 5, 4), (5, 2), (3, 5, 5, 1)])
def test_python_layer_rejects_bad_q_sqrt_shapes(shape):
    X, Z, kern, f = _setup()
    q = np.zeros(shape)
    for full_cov in (False, True):
        with pytest.raises(ValueError):
            cmo.conditional(X, Z, kern, f, full_cov=full_cov, q_sqrt=q, white=True)
    W = [np.eye(5)] * 3
    if shape not in ((2, 5, 5),):                      # (a precalc stack needs only M x M slices: slice 0 is kept)
        with pytest.raises(ValueError):
            cmo.conditional_after_kernel_precalculation(W, X, Z, kern, f, full_cov=True, q_sqrt=q, white=True)


def test_get_rand_full_cov_rejects_bad_shapes():
    mean, eps = np.zeros((4, 2)), np.zeros((4, 2))
    for var in (np.zeros((4, 2)), np.zeros((2, 4, 3)), np.zeros((4, 4, 2)), np.zeros((1, 4, 4))):
        with pytest.raises(ValueError):
            utils.get_rand((mean, var), eps, full_cov=True)
    with pytest.raises(ValueError):
        utils.get_rand((mean, np.zeros((2, 4, 4))), np.zeros((4, 3)), full_cov=True)
    with pytest.raises(ValueError):
        utils.get_rand((np.zeros(4), np.zeros((1, 4, 4))), np.zeros(4), full_cov=True)
