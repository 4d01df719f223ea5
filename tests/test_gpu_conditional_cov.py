"""Full-covariance GP conditionals and joint posterior draws (conditionals_multi_output.py:6-120, :306-387; utils.py:4-11)
against NumPy fp64 restatements on the oracle's kernels: Sigma_d = K_d(Xnew, Xnew) - F_d F_d^T (+ E_d E_d^T), F_d = K_d(Xnew, Z)
L_d^-T, E_d = F_d q0 with q0 = slice 0 of q_sqrt for every dim (the convention of the precalc form)."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

from ffvd_amd import conditionals, conditionals_multi_output as cmo, synthetic, utils
from ffvd_amd.kernels import LinearK, SquaredExponential
from oracle import ffvd_oracle as orc

pytestmark = pytest.mark.gpu


def workload(name):
    params, Y, c, meta = synthetic.make_named(name)
    X0 = params["X"][0]
    xc = np.concatenate((X0[:-1], c[: meta["T"]]), axis=1)
    D, P = meta["D"], meta["P"]
    if meta["kernel_type"] == "LinearK":
        kern = [LinearK(P, variance=np.exp(params["logvariance"][d])) for d in range(D)]
    else:
        kern = [SquaredExponential(P, variance=np.exp(params["logvariance"][d]),
                                   lengthscales=np.exp(params["loglengthscales"][d])) for d in range(D)]
    okern = orc.make_kernels(params, meta["kernel_type"])
    return params, meta, xc, kern, okern


def restate(Xnew, Z, okern, f, *, q0=None, jitter=1e-5, W=None):
    """mean N x D and Sigma D x N x N in fp64 (white=True)."""
    M = Z.shape[0]
    means, covs = [], []
    for d, k in enumerate(okern):
        if W is None:
            L = np.linalg.cholesky(k.K(Z) + jitter * np.eye(M))
            F = solve_triangular(L, k.K(Z, Xnew), lower=True).T         # A^T, :34
        else:
            F = k.K(Xnew, Z) @ W[d]                                     # (L^-T)^T K_mn, :349
        S = k.K(Xnew) - F @ F.T
        if q0 is not None:
            E = F @ q0
            S = S + E @ E.T
        means.append(F @ f[:, d])
        covs.append(S)
    return np.stack(means, axis=1), np.stack(covs)


def check_cov(mean, var, ref_mean, ref_var, *, atol=1e-10):
    np.testing.assert_allclose(var, ref_var, rtol=1e-7, atol=atol)
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-7, atol=atol)
    for d in range(var.shape[0]):
        assert np.array_equal(var[d], var[d].T)


@pytest.mark.parametrize("name", ["tiny", "ragged", "small", "small_lin"])
def test_full_cov_matches_restatement(name):
    params, meta, xc, kern, okern = workload(name)
    Z, U = params["Z"], params["U"]
    mean, var = cmo.conditional(xc, Z, kern, U, full_cov=True, white=True)
    N, D = xc.shape[0], meta["D"]
    assert mean.shape == (N, D) and var.shape == (D, N, N)
    rm, rv = restate(xc, Z, okern, U)
    check_cov(mean, var, rm, rv)
    m0, v0 = cmo.conditional(xc, Z, kern, U, white=True)
    assert np.array_equal(mean, m0)                                    # the full_cov=False mean, bit for bit
    for d in range(D):
        np.testing.assert_allclose(np.diagonal(var[d]), v0[:, d], rtol=1e-10)


@pytest.mark.parametrize("N", [1, 0])
def test_full_cov_one_and_no_rows(N):
    params, meta, xc, kern, okern = workload("ragged")
    Z, U = params["Z"], params["U"]
    mean, var = cmo.conditional(xc[:N], Z, kern, U, full_cov=True, white=True)
    assert mean.shape == (N, meta["D"]) and var.shape == (meta["D"], N, N)
    if N:
        rm, rv = restate(xc[:N], Z, okern, U)
        check_cov(mean, var, rm, rv)


@pytest.mark.parametrize("form", ["3d", "2d"])
@pytest.mark.parametrize("full_cov", [False, True])
def test_q_sqrt_inflates_every_dim_by_slice_0(form, full_cov):
    params, meta, xc, kern, okern = workload("ragged")
    Z, U = params["Z"], params["U"]
    M, D = Z.shape[0], meta["D"]
    rng = np.random.default_rng(11)
    if form == "3d":
        q = np.stack([np.tril(rng.standard_normal((M, M))) * (0.2 / (1 + d)) for d in range(D)])
        q0 = q[0]
    else:
        q = 0.5 * rng.random((M, D)) + 0.1 * np.arange(D)
        q0 = np.diag(q[:, 0])
    mean, var = cmo.conditional(xc, Z, kern, U, full_cov=full_cov, q_sqrt=q, white=True)
    rm, rv = restate(xc, Z, okern, U, q0=q0)
    if full_cov:
        check_cov(mean, var, rm, rv)
    else:
        np.testing.assert_allclose(var, np.stack([np.diagonal(s) for s in rv], axis=1), rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(mean, rm, rtol=1e-7, atol=1e-10)
    # slice 0 for every dim, not each dim's own slice: dim 1 differs from what its own slice would give
    _, own = restate(xc, Z, okern, U, q0=(q[1] if form == "3d" else np.diag(q[:, 1])))
    d1 = var[1] if full_cov else var[:, 1]
    own1 = own[1] if full_cov else np.diagonal(own[1])
    assert not np.allclose(d1, own1, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_precalc_full_cov_with_posterior_q_sqrt(name):
    params, meta, xc, kern, okern = workload(name)
    Z = params["Z"]
    Q = np.exp(params["log_Q"])
    W = cmo.kernel_pre_cal(Z, kern)
    Um, Hinv = cmo.collapse_u_mean_after_kernel_precalculation(W, xc, params["X"][0], Z, kern, Q)   # H_inv_sqrt: upper triangular
    xs = xc[: min(len(xc), 257)]
    mean, var = cmo.conditional_after_kernel_precalculation(W, xs, Z, kern, Um, full_cov=True, q_sqrt=Hinv, white=True)
    m0, v0 = cmo.conditional_after_kernel_precalculation(W, xs, Z, kern, Um, q_sqrt=Hinv, white=True)
    assert np.array_equal(mean, m0)
    for d in range(meta["D"]):
        np.testing.assert_allclose(np.diagonal(var[d]), v0[:, d], rtol=1e-10)
    rm, rv = restate(xs, Z, okern, Um, q0=Hinv[0], W=np.stack(W))
    check_cov(mean, var, rm, rv)


def test_full_cov_at_c2_size():
    """M = 512, D = 4 (config 2's inducing inputs and kernels), N = 2048: 16 x 16 output tiles of 128, depth 2 x 512."""
    params, meta, xc, kern, okern = workload("c2")
    Z, U = params["Z"], params["U"]
    M = Z.shape[0]
    xs = xc[:2048]
    rng = np.random.default_rng(5)
    q = np.stack([np.tril(rng.standard_normal((M, M))) * 0.02 for _ in range(meta["D"])])
    mean, var = cmo.conditional(xs, Z, kern, U, full_cov=True, q_sqrt=q, white=True)
    rm, rv = restate(xs, Z, okern, U, q0=q[0])
    s2 = float(np.max(np.exp(params["logvariance"])))
    check_cov(mean, var, rm, rv, atol=1e-10 * s2)


def test_get_rand_full_cov_joint_draw():
    params, meta, xc, kern, okern = workload("tiny")
    mean, var = cmo.conditional(xc, params["Z"], kern, params["U"], full_cov=True, white=True)
    eps = np.random.default_rng(2).standard_normal(mean.shape)
    out = utils.get_rand((mean, var), eps, full_cov=True)
    N = mean.shape[0]
    ref = np.stack([mean[:, d] + np.linalg.cholesky(var[d] + 1e-7 * np.eye(N)) @ eps[:, d] for d in range(mean.shape[1])],
                   axis=1)
    np.testing.assert_allclose(out, ref, rtol=1e-7, atol=1e-9 * np.max(np.abs(ref)))
    # a bigger one, with the q_sqrt inflation: ragged (N = 301, not a multiple of the block size)
    p2, m2, xc2, kern2, _ = workload("ragged")
    M = p2["Z"].shape[0]
    q = np.tril(np.random.default_rng(4).standard_normal((M, M))) * 0.1
    mean2, var2 = cmo.conditional(xc2, p2["Z"], kern2, p2["U"], full_cov=True, q_sqrt=np.stack([q] * m2["D"]), white=True)
    eps2 = np.random.default_rng(6).standard_normal(mean2.shape)
    out2 = utils.get_rand((mean2, var2), eps2, full_cov=True, jitter=1e-6)
    N2 = mean2.shape[0]
    ref2 = np.stack([mean2[:, d] + np.linalg.cholesky(var2[d] + 1e-6 * np.eye(N2)) @ eps2[:, d] for d in range(m2["D"])], axis=1)
    np.testing.assert_allclose(out2, ref2, rtol=1e-6, atol=1e-8 * np.max(np.abs(ref2)))


def test_get_rand_full_cov_rejects_an_indefinite_covariance():
    N, D = 70, 3
    var = np.stack([np.eye(N), -np.eye(N), np.eye(N)])
    with pytest.raises(np.linalg.LinAlgError, match="latent dim 1"):
        utils.get_rand((np.zeros((N, D)), var), np.zeros((N, D)), full_cov=True)


def test_single_kernel_conditional_full_cov():
    params, meta, xc, kern, okern = workload("tiny")
    R = params["U"].shape[1]
    mean, var = conditionals.conditional(xc[:40], params["Z"], kern[0], params["U"], full_cov=True, white=True)
    assert var.shape == (R, 40, 40)
    rm, rv = restate(xc[:40], params["Z"], [okern[0]] * R, params["U"], jitter=1e-7)
    np.testing.assert_allclose(var, rv, rtol=1e-5, atol=1e-9)          # (jitter 1e-7: the tolerances of test_conditional_matches_oracle)
    np.testing.assert_allclose(mean, rm, rtol=1e-6, atol=1e-7)
