"""The extended-precision Cholesky reference (tests/cholesky_ref.py) checked on the CPU: the long double factor against LAPACK, the
backward-error statistic of LAPACK's own factor against its textbook bound, the inputs that are not positive definite against the
info they are built to produce, and -- what gives the GPU criterion its meaning -- a NumPy emulation of the blocked algorithm that
passes the criterion with its refinement step and misses it without, on the very matrices the GPU tests factorise."""
import numpy as np
import pytest

import cholesky_ref as cr


def test_long_double_is_extended():
    assert float(np.finfo(np.longdouble).eps) < 1e-18          # fail, do not skip: without it nothing below is a reference


@pytest.mark.parametrize("n", [1, 17, 65, 130, 320])
def test_chol_ld_agrees_with_lapack(n):
    """On the well-conditioned family the two factors differ by fp64 rounding: |L_ld - L_lapack| <= gamma_{n+1} |L| |L|^T-sized
    perturbations of A move L by at most kappa-many of them; kappa(W) < 1e4 up to n = 320."""
    for seed in cr.seeds(n, 2):
        A = cr.family("W", n, seed)
        L, bad = cr.chol_ld(A)
        ref = np.linalg.cholesky(A)
        assert bad == 0 and L.dtype == np.longdouble
        assert np.all(np.triu(L, 1) == 0)
        kappa = np.linalg.cond(A)
        assert np.max(np.abs(L.astype(np.float64) - ref)) <= kappa * cr.gamma(n + 1) * np.max(np.abs(ref))
        assert cr.omega(A, L) < 1e-18 * (n + 1)                # the long double factor's own backward error: ~ n eps_ld
    # a stack gives what the matrices give one by one
    A = cr.stack("W", n, 2)
    Ls, bads = cr.chol_ld(A)
    assert np.array_equal(bads, [0, 0]) and np.array_equal(Ls[1], cr.chol_ld(A[1])[0])


def test_omega_definition():
    """omega is the smallest number with |A - L L^T| <= omega |L||L|^T; exact factors have omega = 0; where |L||L|^T vanishes the
    residual must vanish too."""
    L = np.array([[2.0, 0.0], [1.0, 3.0]])
    A = L @ L.T
    assert cr.omega(A, L) == 0.0
    A2 = A.copy()
    A2[1, 0] += 0.5                                           # |L||L|^T[1, 0] = 2
    assert cr.omega(A2, L) == 0.25
    R, S = cr.residual(A2, L)
    assert cr.within(R, S, 0.25) and not cr.within(R, S, 0.2499)
    D = np.diag([1.0, 2.0])
    A3 = D @ D
    A3[1, 0] = 1e-30                                          # S[1, 0] = 0, R[1, 0] > 0
    assert cr.omega(A3, D) == float("inf") and not cr.within(*cr.residual(A3, D), 1e6)
    assert cr.omega(A, np.full((2, 2), np.nan)) == float("inf")
    # the blocked product of the triangular factor is the plain one
    Lw = np.linalg.cholesky(cr.family("W", 70, 1)).astype(np.longdouble)
    assert np.array_equal(cr.residual(np.zeros((70, 70)), Lw)[0], np.abs(np.tril(Lw @ Lw.T)))


@pytest.mark.parametrize("fam,n,batch", cr.accuracy_keys(), ids=lambda v: str(v))
def test_lapack_factor_is_within_its_textbook_bound(fam, n, batch):
    """Every family and size the GPU tests use: the input factors in long double, and omega of LAPACK's factor -- the yardstick of
    the GPU criterion -- is below gamma_{n+1} (Higham, theorem 10.3); measured 0.01 ... 0.1 gamma_{n+1}."""
    A = cr.stack(fam, n, batch)
    assert not np.any(cr.chol_ld(A)[1])
    sd = cr.seeds(n, batch)
    for b in cr.extended_subset(n, batch):
        w = cr.lapack_omega(fam, n, sd[b])
        assert w < cr.gamma(n + 1), (fam, n, b, w / cr.gamma(n + 1))
        assert n == 1 or w > 0.0


def test_extended_subsets():
    assert cr.extended_subset(130, 33) == list(range(33)) and cr.extended_subset(320, 2) == [0, 1]
    for n, batch in ((320, 52), (130, 257)):
        sub = cr.extended_subset(n, batch)
        assert len(sub) >= 8 and {0, 7, 8, batch - 1} <= set(sub) and all(0 <= i < batch for i in sub)
    assert {255, 256} <= set(cr.extended_subset(130, 257))


def test_non_pd_builders_produce_the_intended_info():
    good40, bad40, info40, good7, bad7, info7 = cr.nonpd_batches()
    want = {1: 1, 8: 16, 15: 17, 16: 64, 31: 65, 32: 130, 39: 101}
    assert {b: int(info40[b]) for b in np.flatnonzero(info40)} == want
    assert np.array_equal(cr.chol_ld(bad40)[1], info40)
    assert np.array_equal(info7, [1, 16, 17, 64, 65, 130, 101]) and np.array_equal(cr.chol_ld(bad7)[1], info7)
    assert not np.any(cr.chol_ld(good40)[1]) and not np.any(cr.chol_ld(good7)[1])
    for seed in cr.seeds(cr.NONPD_N, cr.NONPD_BATCH):        # the good neighbours are held to the accuracy criterion: its yardstick
        assert 0.0 < cr.lapack_omega("W", cr.NONPD_N, seed) < cr.gamma(cr.NONPD_N + 1)
    for b in range(cr.NONPD_BATCH):                           # a bad matrix replaces one matrix, the others are untouched
        assert (b in want) != np.array_equal(bad40[b], good40[b], equal_nan=True)
    # each builder on its own, at both ends of a matrix
    A = cr.family("W", 20, 3)
    for p in (0, 7, 19):
        assert cr.chol_ld(cr.bad_negative_pivot(A, p)[0])[1] == p + 1
        assert cr.chol_ld(cr.bad_zero_pivot(20, p)[0])[1] == p + 1
        assert cr.chol_ld(cr.bad_nan_pivot(A, p)[0])[1] == p + 1
    assert cr.chol_ld(cr.bad_inf_entry(A, 12, 4)[0])[1] == 13
    assert cr.chol_ld(cr.bad_inf_entry(A, 19, 0)[0])[1] == 20


def test_emulation_factorises():
    """The emulation is a Cholesky: on the well-conditioned family both forms agree with LAPACK to rounding."""
    for n in (16, 65, 130):
        A = cr.family("W", n, n)
        ref = np.linalg.cholesky(A)
        for refine in (True, False):
            np.testing.assert_allclose(cr.blocked_emulation(A, refine), ref, rtol=1e-11, atol=1e-12)


ILL = [(fam, n, batch) for fam, n, batch in cr.accuracy_keys() if fam in ("K8", "K9")]


@pytest.mark.parametrize("fam,n,batch", ILL, ids=lambda v: str(v))
def test_criterion_separates_refined_from_unrefined_substitution(fam, n, batch):
    """The power of the GPU criterion, on the seeds of every ill-conditioned GPU batch: the blocked algorithm with one refinement step
    per inverted sub-block passes on every matrix (measured 0.6 ... 1.3 x LAPACK's omega), the same algorithm without it misses the
    bound on at least one matrix of the batch (3 ... 110 x).  A kernel that loses its refinement step cannot pass."""
    A = cr.stack(fam, n, batch)
    missed = 0
    for b, seed in enumerate(cr.seeds(n, batch)):
        bound = cr.bound_for(cr.lapack_omega(fam, n, seed))
        R, S = cr.residual(A[b], cr.blocked_emulation(A[b], True))
        assert cr.within(R, S, bound), (fam, n, b, cr.omega_of(R, S) / cr.lapack_omega(fam, n, seed))
        missed += not cr.within(*cr.residual(A[b], cr.blocked_emulation(A[b], False)), bound)
    assert missed >= 1


def test_well_conditioned_family_cannot_see_the_refinement():
    """Why the ill-conditioned families are needed: on B B^T + 0.5 I the unrefined algorithm passes as well."""
    A = cr.stack("W", 130, 6)
    for b, seed in enumerate(cr.seeds(130, 6)):
        assert cr.within(*cr.residual(A[b], cr.blocked_emulation(A[b], False)), cr.bound_for(cr.lapack_omega("W", 130, seed)))
