"""Extended-precision reference for the batched Cholesky (NumPy only): the factor in `np.longdouble`, the componentwise backward
error of a computed factor, the seeded input families and non-positive-definite inputs the GPU tests use, and a NumPy emulation
of the blocked algorithm of `potrf.hip` / `potrf_flow.hip` (with and without its refinement step) that shows what the accuracy
criterion can tell apart.

The criterion: a factor L of A passes when, on the lower triangle,

    |A - L L^T|  <=  max(4 omega_LAPACK(A), 4 u) * |L| |L|^T,        u = 2^-53,

where omega_LAPACK(A) is the same statistic of `np.linalg.cholesky(A)` for that matrix -- the reference's own error.  Both sides are
evaluated in extended precision, without dividing (where |L||L|^T is zero the residual must be zero).  The factor 4 is the margin
for another summation order and the reciprocal-square-root pivots; the floor 4 u covers inputs LAPACK factors exactly."""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                     # unit roundoff of fp64
NB, SB = 64, 16                    # block and sub-block size of the GPU algorithm (kernels.h NB; the inverted diagonal sub-blocks)


def _require_extended():
    """The reference is only a reference where long double is wider than double (x87: eps 1.08e-19)."""
    eps = float(np.finfo(LD).eps)
    assert eps < 1e-18, f"np.longdouble has eps {eps:.3g}: no extended precision on this platform, the Cholesky reference is void"


def gamma(k):
    """gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return k * U / (1.0 - k * U)


def chol_ld(A):
    """Column-by-column Cholesky in np.longdouble of the lower triangle of A (n x n, or a stack ... x n x n).
    Returns (L, bad): bad = 0, or 1 + the index of the first pivot that is not > 0 (NaN included); an int for one matrix, an int
    array for a stack.  Behind a bad pivot L holds NaN."""
    _require_extended()
    A = np.asarray(A)
    single = A.ndim == 2
    S = np.tril(A.astype(LD)).reshape((-1,) + A.shape[-2:])
    n = S.shape[-1]
    L = np.zeros_like(S)
    bad = np.zeros(S.shape[0], dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(n):
            col = S[:, j:, j] - np.einsum("bik,bk->bi", L[:, j:, :j], L[:, j, :j])
            piv = col[:, 0]
            ok = piv > 0
            bad[(~ok) & (bad == 0)] = j + 1
            d = np.sqrt(np.where(ok, piv, LD(np.nan)))
            L[:, j, j] = d
            L[:, j + 1:, j] = col[:, 1:] / d[:, None]
    if single:
        return L[0], int(bad[0])
    return L.reshape(A.shape), bad.reshape(A.shape[:-2])


def _tril_gram(X, bs=32):
    """tril(X X^T) of a lower-triangular X: block (I, J) needs the columns left of J's end only (a third of the full product; the
    long double product has no BLAS behind it)."""
    n = X.shape[0]
    out = np.zeros_like(X)
    for i0 in range(0, n, bs):
        for j0 in range(0, i0 + 1, bs):
            je = min(j0 + bs, n)
            out[i0:i0 + bs, j0:je] = X[i0:i0 + bs, :je] @ X[j0:je, :je].T
    return np.tril(out)


def residual(A, L):
    """(R, S) = (|tril(A) - tril(L L^T)|, tril(|L| |L|^T)) of one matrix and the lower triangle of L, in long double."""
    _require_extended()
    A = np.asarray(A).astype(LD)
    L = np.tril(np.asarray(L).astype(LD))
    with np.errstate(all="ignore"):
        R = np.abs(np.tril(A) - _tril_gram(L))
        S = _tril_gram(np.abs(L))
    return R, S


def within(R, S, bound):
    """R <= bound * S everywhere, compared without dividing (S = 0 demands R = 0; a NaN anywhere fails)."""
    return bool(np.all(R <= R.dtype.type(bound) * S))


def omega_of(R, S):
    """The smallest omega with R <= omega S: inf where S = 0 < R, NaN entries count as inf."""
    if np.isnan(R).any() or np.isnan(S).any() or np.any((S == 0) & (R > 0)):
        return float("inf")
    pos = S > 0
    return float(np.max(R[pos] / S[pos])) if pos.any() else 0.0


def omega(A, L):
    """Componentwise backward error of the factor L of A, in extended precision."""
    return omega_of(*residual(A, L))


# ------------------------------------------------------------------------------------------------------------------------------
# input families, all seeded
# ------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("W", "K5", "K8", "K9", "G")
JITTER = {"K5": 1e-5, "K8": 1e-8, "K9": 1e-9}


def _se(rng, n, jitter):
    z = np.cumsum(0.1 * rng.standard_normal((n, 2)), axis=0)
    return 0.5 * np.exp(-((z[:, None, :] - z[None, :, :]) ** 2).sum(-1) / 8.0) + jitter * np.eye(n)


def family(name, n, seed):
    """One n x n matrix.  W: B B^T + 0.5 I, B of shape n x (n + 2) (well conditioned, the family of the operator tests);
    K5 / K8 / K9: 0.5 exp(-|z_a - z_b|^2 / 8) + j I with z = cumsum(0.1 randn(n, 2)), j = 1e-5 / 1e-8 / 1e-9 (condition ~1e6 ... 1e10);
    G: D K5 D with D = diag(2^k), k uniform in [-200, 200] (no absolute tolerance or range assumption may hide in the pivots)."""
    rng = np.random.default_rng(seed)
    if name == "W":
        B = rng.standard_normal((n, n + 2))
        return B @ B.T + 0.5 * np.eye(n)
    if name in JITTER:
        return _se(rng, n, JITTER[name])
    if name == "G":
        K = _se(rng, n, JITTER["K5"])
        d = np.ldexp(1.0, rng.integers(-200, 201, n))
        return d[:, None] * K * d[None, :]            # powers of two: exact
    raise ValueError(name)


def seeds(n, batch):
    return [1000 * n + s for s in range(batch)]


@functools.lru_cache(maxsize=None)
def _stack(name, n, batch):
    A = np.stack([family(name, n, s) for s in seeds(n, batch)])
    A.setflags(write=False)
    return A


def stack(name, n, batch):
    """batch matrices of one family with the seeds 1000 n + s, s = 0 .. batch - 1 (shared, read-only)."""
    return _stack(name, n, batch)


# (n, batch, families): what every forced variant factorises in the accuracy tests (tests/test_gpu_cholesky_variants.py says what
# each row reaches)
ACCURACY_CASES = tuple((n, 3, ("W", "K5")) for n in (1, 16, 17, 63, 64, 65)) + (
    (130, 6, ("W", "K5", "K8", "K9", "G")),
    (200, 6, ("K9",)),
    (320, 2, ("W", "K8")),
    (130, 33, ("K8",)),
    (320, 52, ("W",)),
    (130, 257, ("W",)),
)


def accuracy_keys():
    return [(fam, n, batch) for n, batch, fams in ACCURACY_CASES for fam in fams]


def extended_subset(n, batch):
    """Indices of the matrices whose criterion is evaluated in extended precision: all of them up to n = 200 and 33 matrices, a
    fixed subset of at least 8 beyond (the others get the same inequality in fp64, enlarged by the evaluation's own rounding)."""
    if n <= 200 and batch <= 64:
        return list(range(batch))
    want = [0, 7, 8, batch - 1, 255, 256, 3, 21, 29, 41, 100, 130]
    out = []
    for i in want:
        if 0 <= i < batch and i not in out:
            out.append(i)
    return sorted(out[:8]) if batch >= 8 else list(range(batch))


@functools.lru_cache(maxsize=None)
def lapack_omega(name, n, seed):
    """omega of np.linalg.cholesky's factor of family(name, n, seed): the reference's own error."""
    A = family(name, n, seed)
    return omega(A, np.linalg.cholesky(A))


def bound_for(w_lapack):
    return max(4.0 * w_lapack, 4.0 * U)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs that are not positive definite, each with the info it must produce (1 + first bad pivot)
# ------------------------------------------------------------------------------------------------------------------------------
def bad_negative_pivot(A, p):
    """(a) the Schur complement at pivot p becomes -1 (up to rounding): A[p, p] = sum_{k<p} L0[p, k]^2 - 1, L0 the factor of A."""
    L0, bad = chol_ld(A)
    assert bad == 0
    out = np.array(A, dtype=np.float64)
    out[p, p] = float((L0[p, :p] ** 2).sum()) - 1.0
    return out, p + 1


def bad_zero_pivot(n, p):
    """(b) an exactly zero pivot: the identity with A[p, p] = 0."""
    out = np.eye(n)
    out[p, p] = 0.0
    return out, p + 1


def bad_nan_pivot(A, p):
    """(c) A[p, p] = NaN."""
    out = np.array(A, dtype=np.float64)
    out[p, p] = np.nan
    return out, p + 1


def bad_inf_entry(A, i, j):
    """(d) A[i, j] = +inf for one i > j (lower triangle only): L[i, j] is infinite and pivot i is the first that is not > 0."""
    assert i > j
    out = np.array(A, dtype=np.float64)
    out[i, j] = np.inf
    return out, i + 1


NONPD_N, NONPD_BATCH = 130, 40
# b -> (builder, arguments): the table of the issue; the same seven, in this order, form the batch of 7
NONPD_TABLE = ((1, "a", (0,)), (8, "b", (15,)), (15, "c", (16,)), (16, "a", (63,)), (31, "a", (64,)), (32, "a", (129,)),
               (39, "d", (100, 20)))


def _bad(kind, A, args):
    if kind == "a":
        return bad_negative_pivot(A, *args)
    if kind == "b":
        return bad_zero_pivot(A.shape[0], *args)
    if kind == "c":
        return bad_nan_pivot(A, *args)
    return bad_inf_entry(A, *args)


@functools.lru_cache(maxsize=None)
def nonpd_batches():
    """(good40, bad40, info40, good7, bad7, info7): W matrices of n = 130; bad40 = good40 with the seven matrices of NONPD_TABLE
    replaced, bad7 = those seven alone (good7: the matrices they were made from)."""
    good40 = stack("W", NONPD_N, NONPD_BATCH)
    bad40 = np.array(good40)
    info40 = np.zeros(NONPD_BATCH, dtype=np.int32)
    for b, kind, args in NONPD_TABLE:
        bad40[b], info40[b] = _bad(kind, good40[b], args)
    idx = [b for b, _, _ in NONPD_TABLE]
    out = (good40, bad40, info40, np.ascontiguousarray(good40[idx]), np.ascontiguousarray(bad40[idx]), info40[idx].copy())
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# inputs of kernel_pre_cal (the factorisation with identity rows riding through it)
# ------------------------------------------------------------------------------------------------------------------------------
def kpc_inputs(M, nk):
    """(Z, logvariance, loglengthscales): M inducing points of the synthetic "c2" workload with two latent dimensions (P = 3 inputs)
    and nk squared-exponential kernels over them -- the workload's own two, or for nk > 2 its rule variance 0.5, lengthscales
    2 + 0.1 d continued (P = D + C is capped at 32, so 33 kernels cannot come from 33 latent dimensions)."""
    from ffvd_amd import synthetic             # NumPy only
    cfg = dict(synthetic.CONFIGS["c2"], D=2)
    cfg.update(M=M, T=max(cfg["T"], M + 64))
    params, _, _, meta = synthetic.make_workload(**cfg)
    d = np.arange(nk, dtype=np.float64)
    logvar = np.log(np.full(nk, 0.5))
    loglen = np.log(np.repeat((2.0 + 0.1 * d)[:, None], meta["P"], axis=1))
    if nk == 2:
        assert np.array_equal(logvar, params["logvariance"]) and np.array_equal(loglen, params["loglengthscales"])
    return params["Z"], logvar, loglen


# ------------------------------------------------------------------------------------------------------------------------------
# the blocked algorithm in NumPy (fp64): proves that the criterion separates a refined substitution from an unrefined one
# ------------------------------------------------------------------------------------------------------------------------------
def _chol_unblocked(T):
    n = T.shape[0]
    L = np.zeros_like(T)
    for j in range(n):
        col = T[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L


def _inv_lower(T):
    """Inverse of a lower-triangular block by running the identity through the forward substitution (as diag_block_finish)."""
    n = T.shape[0]
    X = np.zeros_like(T)
    for r in range(n):
        X[r] = ((np.arange(n) == r) - T[r, :r] @ X[:r]) / T[r, r]
    return X


def blocked_emulation(A, refine):
    """Right-looking blocked Cholesky as the GPU kernels do it: NB = 64 block columns on the identity-padded matrix; the panel below a
    diagonal block is solved by MULTIPLYING with the explicitly inverted 16 x 16 diagonal sub-blocks of L_kk, with (refine) or without
    one step of iterative refinement per sub-block, and block updates between the sub-blocks.  fp64 throughout."""
    n = A.shape[0]
    m = -(-n // NB) * NB
    S = np.eye(m)
    S[:n, :n] = np.tril(A) + np.tril(A, -1).T
    for k0 in range(0, m, NB):
        k1 = k0 + NB
        Lkk = _chol_unblocked(S[k0:k1, k0:k1])
        S[k0:k1, k0:k1] = Lkk
        if k1 == m:
            break
        R = S[k1:, k0:k1]
        for s in range(0, NB, SB):
            Lss = Lkk[s:s + SB, s:s + SB]
            inv = _inv_lower(Lss)
            B = R[:, s:s + SB].copy()
            X = B @ inv.T
            if refine:
                X = X + (B - X @ Lss.T) @ inv.T
            R[:, s:s + SB] = X
            R[:, s + SB:] -= X @ Lkk[s + SB:, s:s + SB].T
        S[k1:, k1:] -= R @ R.T
    return np.tril(S[:n, :n])
