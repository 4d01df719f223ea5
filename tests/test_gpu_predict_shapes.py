"""GPU parity of the prediction side at M from 128 to 2100: the GP operators, the posterior rollouts and the particle-Gibbs sweep
against the NumPy oracle on identical inputs, at shapes chosen to cross the boundaries the small goldens (M <= 96, Mp <= 128) never
reach:

  - Mp = M (no padding: `upload_stack` hands the caller's array over as it is) and Mp > M (identity-padded stack), SE and LinearK;
  - Mp > 512: `launch_project` writes ng = Mp / 512 partial row sums, `conditional_finish` adds them (ng = 2 at Mp = 640, 5 at 2112);
  - Mp > 2048: the second 2048-wide tile of y in `matvec_kernel` (U_mean of `ffvd_op_collapse_u_mean`);
  - the resident rollout loop (`rollout_resident_kernel`, M <= 512, D <= 8, P <= 8, R <= 64; the default up to R = 32, FFVD_STEP_LOOP=2
    up to 64) with 1 to 4 row tiles of 16 rollouts and 32 slabs of L^-T (and of W q_sqrt) in LDS;
  - the skinny step product (`skinny_gemm_xcd_kernel`) with more than 32 * cnt (slab, row group) pairs, so that its reversed half runs;
  - the tiled step (more than 512 rollouts or free particles: `launch_kfu_build` + `launch_proj_gemm` + `launch_qsqrt_inflation`).

Every rollout / sweep / precalc call gets the oracle's own L^-T, U_mean and L_H^-T, so that what is compared is the operator under
test and not an error of `kernel_pre_cal` on a K_uu of condition ~1e8 (that operator is checked on its own, in units of eps kappa).
Inputs come from `synthetic.make_named`; the operators run on a few hundred rows, the rollouts for a few steps and the sweeps over
X[:17] ... X[:33], so that the oracle stays cheap."""
import functools
import warnings

import numpy as np
import pytest

from ffvd_amd import _lib, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import pg_sweep, rollout
from oracle import ffvd_oracle as orc
from oracle import ffvd_pg_oracle as pgo

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
JITTER = cmo.JITTER
T_OPS = 300              # rows of X_combine handed to the operators (collapse is O(T M^2) per dim in the oracle)
ROLL = dict(rtol=1e-8, atol=1e-9)          # rollouts: test_gpu_ops.test_rollout_matches_oracle
ROLL_VAR = dict(rtol=1e-8, atol=1e-10)


@functools.lru_cache(maxsize=None)
def case(name, M, **ov):
    """Inputs of shape `name` with M inducing points (T raised to M + 64 where the draw of Z needs it), the kernels on both sides and
    the oracle's L^-T, U_mean and L_H^-T (from the first T_OPS rows)."""
    cfg = dict(synthetic.CONFIGS[name], **ov)
    cfg.update(M=M, T=max(cfg["T"], M + 64))
    params, Y, c, meta = synthetic.make_workload(**cfg)
    D, C = meta["D"], meta["C"]
    lin = meta["kernel_type"] == "LinearK"
    okern = orc.make_kernels(params, kernel_type=meta["kernel_type"])
    if lin:
        kern = [LinearK(D + C, variance=np.exp(params["logvariance"][d])) for d in range(D)]
    else:
        kern = [SquaredExponential(D + C, variance=np.exp(params["logvariance"][d]),
                                   lengthscales=np.exp(params["loglengthscales"][d])) for d in range(D)]
    X = params["X"][0]
    xc = np.concatenate((X[:-1], c), axis=1)
    Q = np.exp(params["log_Q"])
    Z = params["Z"]
    L = orc.kernel_pre_cal(Z, okern)
    U, H = orc.collapse_u_mean_after_kernel_precalculation(L, xc[:T_OPS], X[:T_OPS + 1], Z, okern, Q)
    return dict(params=params, Y=Y, c=c, meta=meta, okern=okern, kern=kern, X=X, xc=xc, Q=Q, Z=Z, L=L, U=U, H=H, lin=lin)


def dense_q(k, seed=17):
    """A q_sqrt that is not triangular: L_H^-T (slice 0) plus 5 % noise -- both forms of the step must then take the full k range."""
    H0 = k["H"][:1]
    rng = np.random.default_rng(seed)
    return H0 + 0.05 * rng.standard_normal(H0.shape) * np.abs(H0).max()


def assert_close(got, want, rtol, atol, what=""):
    """assert_allclose with an elementwise absolute tolerance (LinearK variances: atol proportional to K_ii)."""
    err, bound = np.abs(np.asarray(got) - want), atol + rtol * np.abs(want)
    assert got.shape == want.shape and np.all(err <= bound), f"{what}: worst error {np.max(err / bound):.3g} x its bound"


def kuu(k, d):
    return k["okern"][d].K(k["Z"]) + JITTER * np.eye(k["Z"].shape[0])


def cond(A):
    """kappa of a symmetric positive definite matrix."""
    ev = np.linalg.eigvalsh(A)
    return ev[-1] / ev[0]


# ------------------------------------------------------------------------------------------------------------------------------
# operators
# ------------------------------------------------------------------------------------------------------------------------------
KPC_CASES = [("c2", 128, {}), ("c2", 200, {}), ("c2", 512, {}), ("c2", 600, {}), ("c2", 1024, dict(D=2)),
             ("c2", 2048, dict(D=2)), ("small_lin", 600, dict(D=3))]


@pytest.mark.parametrize("name,M,ov", KPC_CASES, ids=[f"{n}-M{m}" for n, m, _ in KPC_CASES])
def test_kernel_pre_cal_at_large_m(name, M, ov):
    """kernel_pre_cal (Mp = 128 unpadded, 256 padded, 512, 640, 1024, 2048; SE and LinearK at Mp = 640) on its own: its defining
    property W^T (K_uu + jI) W = I, an exactly zero strict lower triangle, and closeness to the oracle's L^-T.  Both bounds are in
    units of eps kappa(K_uu + jI) (the unit of tools/factor_acc.py and DESIGN section 7): the computed inverse of a Cholesky factor has a
    relative error of a small multiple of eps kappa, which the product W^T K W shows up to that bound too."""
    k = case(name, M, **ov)
    W = cmo.kernel_pre_cal(k["Z"], k["kern"])
    for d in range(k["meta"]["D"]):
        A = kuu(k, d)
        kappa = cond(A)
        assert np.all(np.tril(W[d], -1) == 0.0)
        res = np.abs(W[d].T @ A @ W[d] - np.eye(M)).max()
        assert res < 4 * EPS * kappa, (d, res, kappa)
        rel = np.abs(W[d] - k["L"][d]).max() / np.abs(k["L"][d]).max()
        assert rel < 4 * EPS * kappa, (d, rel, kappa)


OP_CASES = [("c2", 128, {}), ("c2", 200, {}), ("c2", 512, {}), ("c2", 600, {}), ("c2", 1024, dict(D=2)), ("c2", 2048, dict(D=2)),
            ("small_lin", 600, dict(D=3))]


@pytest.mark.parametrize("name,M,ov", OP_CASES, ids=[f"{n}-M{m}" for n, m, _ in OP_CASES])
def test_collapse_and_posterior_u_at_large_m(name, M, ov):
    """collapse_after_kernel_precalculation and collapse_u_mean_after_kernel_precalculation with the oracle's L^-T (Mp = 128 unpadded,
    256 padded, 512: ng = 1, 640: ng = 2 partial row sums of the projection, 1024, 2048; LinearK at Mp = 640), tolerances of
    test_gpu_ops (collapse 1e-9, U_mean / L_H^-T 1e-8 / 1e-10).  At one large M the mini-batch factor batch_size != Y_N as well."""
    k = case(name, M, **ov)
    n = T_OPS
    xc, X = k["xc"][:n], k["X"][:n + 1]
    for bs, yn in ((n, n),) + (((n, 4.0 * n),) if M == 1024 else ()):
        got = cmo.collapse_after_kernel_precalculation(k["L"], xc, X, k["Z"], k["kern"], k["Q"], bs, yn)
        ref = orc.collapse_after_kernel_precalculation(k["L"], xc, X, k["Z"], k["okern"], k["Q"], bs, yn)
        np.testing.assert_allclose(got, ref, rtol=1e-9)
    Ug, Hg = cmo.collapse_u_mean_after_kernel_precalculation(k["L"], xc, X, k["Z"], k["kern"], k["Q"])
    np.testing.assert_allclose(Ug, k["U"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(Hg, k["H"], rtol=1e-8, atol=1e-10)
    assert all(np.all(np.tril(Hg[d], -1) == 0.0) for d in range(Hg.shape[0]))


def test_posterior_u_beyond_2048_inducing_points():
    """collapse_u_mean_after_kernel_precalculation at M = 2100 (Mp = 2112, not capped): the second 2048-wide tile of y in matvec_kernel
    (U_mean = L_H^-T (L_H^-1 b)) and ng = 5 partial row sums of the projection.  Tolerances of test_gpu_ops."""
    k = case("c2", 2100, D=2)
    n = T_OPS
    Ug, Hg = cmo.collapse_u_mean_after_kernel_precalculation(k["L"], k["xc"][:n], k["X"][:n + 1], k["Z"], k["kern"], k["Q"])
    np.testing.assert_allclose(Ug, k["U"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(Hg, k["H"], rtol=1e-8, atol=1e-10)


COND_CASES = [("c2", 128, {}), ("c2", 200, {}), ("c2", 512, {}), ("c2", 600, {}), ("c2", 2048, dict(D=2)), ("c2", 2100, dict(D=2)),
              ("small_lin", 600, dict(D=3))]


@pytest.mark.parametrize("name,M,ov", COND_CASES, ids=[f"{n}-M{m}" for n, m, _ in COND_CASES])
def test_conditional_at_large_m(name, M, ov):
    """conditional (its own factorisation of K_uu) at N = 1, 65, 257 new points: Mp = 128, 256, 512 (ng = 1), 640 (ng = 2), 2048,
    2112 (ng = 5, no cap on M); LinearK at Mp = 640.  Mean to rtol 1e-8 / atol 1e-9 and variance to rtol 1e-7 / atol 1e-10 (the
    tolerances of test_gpu_ops) -- for LinearK the variance is a cancellation to ~1e-6 K_ii (cov.hip), so its absolute tolerance is
    1e-10 K_ii."""
    k = case(name, M, **ov)
    rng = np.random.default_rng(M)
    for N in (1, 65, 257):
        Xn = k["xc"][rng.choice(k["xc"].shape[0], N, replace=False)]
        mean, var = cmo.conditional(Xn, k["Z"], k["kern"], k["params"]["U"], white=True)
        mo, vo = orc.conditional(Xn, k["Z"], k["okern"], k["params"]["U"], white=True)
        np.testing.assert_allclose(mean, mo, rtol=1e-8, atol=1e-9)
        kdiag = np.stack([kk.Kdiag(Xn) for kk in k["okern"]], axis=1)
        assert_close(var, vo, 1e-7, 1e-10 * (kdiag if k["lin"] else 1.0), f"var N={N}")


PRE_CASES = [("c2", 128, {}), ("c2", 200, {}), ("c2", 512, {}), ("c2", 600, {}), ("c2", 1024, dict(D=2)), ("c2", 2048, dict(D=2)),
             ("small_lin", 600, dict(D=3))]


@pytest.mark.parametrize("name,M,ov", PRE_CASES, ids=[f"{n}-M{m}" for n, m, _ in PRE_CASES])
def test_conditional_precalc_at_large_m(name, M, ov):
    """conditional_after_kernel_precalculation with the oracle's L^-T and U_mean at N = 1, 65, 257 points, three ways: no q_sqrt, the
    reference's upper-triangular L_H^-T and a dense q_sqrt (qsqrt_inflation stages a row of F in its 2048-double array: M up to the
    cap).  Mp = 128 unpadded, 256 padded, 512, 640 (ng = 2), 1024, 2048; LinearK at Mp = 640.  Tolerances of test_gpu_ops (mean
    1e-9 / 1e-11, variance 1e-8 / 1e-11; LinearK variance atol 1e-11 K_ii)."""
    k = case(name, M, **ov)
    rng = np.random.default_rng(M + 1)
    for N in (1, 65, 257):
        Xn = k["xc"][rng.choice(k["xc"].shape[0], N, replace=False)]
        kdiag = np.stack([kk.Kdiag(Xn) for kk in k["okern"]], axis=1)
        for q in (None, k["H"][:1], dense_q(k)):
            m, v = cmo.conditional_after_kernel_precalculation(k["L"], Xn, k["Z"], k["kern"], k["U"], q_sqrt=q, white=True)
            mo, vo = orc.conditional_after_kernel_precalculation(k["L"], Xn, k["Z"], k["okern"], k["U"], q_sqrt=q)
            np.testing.assert_allclose(m, mo, rtol=1e-9, atol=1e-11)
            assert_close(v, vo, 1e-8, 1e-11 * (kdiag if k["lin"] else 1.0), f"var N={N}")


# ------------------------------------------------------------------------------------------------------------------------------
# rollouts
# ------------------------------------------------------------------------------------------------------------------------------
def run_rollout(k, R, steps, q, seed=5):
    """GPU and oracle rollouts of R posterior draws for `steps` steps from X[-1], the oracle's L^-T / U_mean / q_sqrt on both sides."""
    D, C, T = k["meta"]["D"], k["meta"]["C"], k["meta"]["T"]
    rng = np.random.default_rng(seed)
    ctrl = np.concatenate((k["c"], rng.standard_normal((steps, C))))
    eps = rng.standard_normal((steps, R, D))
    args = (k["Z"], k["kern"], k["U"], q, k["X"][-1], ctrl, T, steps, k["Q"], eps)
    before = _lib.load().ffvd_op_rollout_fallbacks()
    got = rollout(k["L"], *args)
    moved = _lib.load().ffvd_op_rollout_fallbacks() - before
    ref = orc.rollout(k["L"], k["Z"], k["okern"], k["U"], q, k["X"][-1], ctrl, T, steps, k["Q"], eps)
    return got, ref, moved


def check_rollout(got, ref):
    assert got[0].shape == ref[0].shape and np.all(got[1] > 0)
    np.testing.assert_allclose(got[0], ref[0], **ROLL)
    np.testing.assert_allclose(got[1], ref[1], **ROLL_VAR)


RESIDENT = [(16, "H", None, "RT = 1, default"), (17, None, None, "RT = 2, default"), (17, "H", None, "RT = 2, default"),
            (33, None, "2", "RT = 3"), (33, "H", "2", "RT = 3"), (64, "H", "2", "RT = 4"), (64, "dense", "2", "RT = 4")]


@pytest.mark.parametrize("R,qk,loop,what", RESIDENT, ids=[f"R{r}-{q}-{w.split(',')[0].replace(' ', '')}" for r, q, _, w in RESIDENT])
def test_resident_rollouts_at_config2(R, qk, loop, what, monkeypatch):
    """Config 2 (M = Mp = 512, D = 4, P = 5): the resident rollout loop with 32 slabs of L^-T per dim in LDS (and all of W q_sqrt:
    ~143 KiB per workgroup), 1 to 4 row tiles of 16 rollouts (RT = 1 at 16, 2 at 17, 3 at 33, 4 at 64 -- the wavefront roles nkp /
    rt / kp of each), the default up to 32 rollouts and FFVD_STEP_LOOP=2 beyond.  The fallback counter must stand still: the
    resident form is what ran.  Rollout tolerances (1e-8 / 1e-9)."""
    if loop is not None:
        monkeypatch.setenv("FFVD_STEP_LOOP", loop)
    else:
        monkeypatch.delenv("FFVD_STEP_LOOP", raising=False)
    k = case("c2", 512)
    q = {None: None, "H": k["H"][:1], "dense": dense_q(k)}[qk]
    got, ref, moved = run_rollout(k, R, 6, q)
    assert moved == 0, _lib.load().ffvd_last_error(None)
    check_rollout(got, ref)


def test_resident_rollouts_whole_chip(monkeypatch):
    """Mp = 512, D = 8, P = 8 (C = 0), 32 rollouts with q_sqrt: 8 x 32 = 256 workgroups of ~143 KiB LDS each, one per CU -- the
    whole chip.  Another tenant can keep a workgroup from being resident and force the per-step launches; that is reported, not
    failed, and the result is held to the oracle either way."""
    monkeypatch.delenv("FFVD_STEP_LOOP", raising=False)
    k = case("c2", 512, D=8, C=0)
    got, ref, moved = run_rollout(k, 32, 5, k["H"][:1])
    if moved:
        warnings.warn("whole-chip resident rollout fell back to the per-step launches: " + str(_lib.load().ffvd_last_error(None)))
    check_rollout(got, ref)


LAUNCH = [("c2", 512, {}, 100, "H", "skinny, reversed half (by nbx >= 64)"), ("c2", 512, {}, 100, "dense", "skinny, full k range"),
          ("c2", 512, {}, 512, "H", "skinny, 16 row groups"), ("c2", 512, {}, 512, "dense", "skinny, 16 row groups"),
          ("c2", 512, {}, 100, None, "skinny without q_sqrt"),
          ("c2", 600, {}, 16, "H", "Mp = 640 > 512: launches"),
          ("c2", 128, dict(D=3, C=2), 20, "dense", "Mp = 128 unpadded, resident"),
          ("c2", 200, dict(D=3, C=2), 20, "dense", "Mp = 256 padded, resident"),
          ("c2", 512, {}, 513, "H", "tiled"), ("c2", 512, {}, 600, None, "tiled"), ("c2", 512, {}, 600, "dense", "tiled"),
          ("c2", 2048, dict(D=2), 8, "H", "largest M"),
          ("c2", 512, dict(C=5), 20, "H", "P = 9 > 8: launches"),
          ("small_lin", 512, dict(T=1024), 20, "H", "LinearK, resident"), ("small_lin", 512, dict(T=1024), 100, "H", "LinearK, skinny")]


@pytest.mark.parametrize("name,M,ov,R,qk,what", LAUNCH, ids=[f"{n}-M{m}-R{r}-{q}" for n, m, _, r, q, _ in LAUNCH])
def test_rollouts_at_large_m(name, M, ov, R, qk, what, monkeypatch):
    """Rollouts against the oracle in the default dispatch: the skinny step product at 100 and 512 rollouts of config 2 (more than
    32 cnt (slab, row group) pairs: the reversed half of skinny_gemm_xcd_kernel; the q_upper shortcut with 32 slabs), Mp = 640 (no
    resident loop), Mp = 128 unpadded and 256 padded (dense q_sqrt, resident), the tiled step at 513 and 600 rollouts (proj_gemm +
    qsqrt_inflation), M = 2048 (the cap), P = 9 (no resident loop) and LinearK at M = 512.  A case the resident loop takes must not
    fall back.  Rollout tolerances (1e-8 / 1e-9)."""
    monkeypatch.delenv("FFVD_STEP_LOOP", raising=False)
    k = case(name, M, **ov)
    q = {None: None, "H": k["H"][:1], "dense": dense_q(k)}[qk]
    got, ref, moved = run_rollout(k, R, 5, q)
    assert moved == 0, _lib.load().ffvd_last_error(None)
    check_rollout(got, ref)


@pytest.mark.parametrize("R", [16, 33])
def test_resident_loop_equals_launches_at_config2(R, monkeypatch):
    """Config 2 (Mp = 512, 32 slabs), 16 and 33 rollouts, with and without q_sqrt: the resident loop (FFVD_STEP_LOOP=2) against the
    per-step launches (FFVD_STEP_LOOP=0) to 1e-9 -- the same values, another summation order inside a row of F
    (test_gpu_ops.test_step_loops_equal_the_per_step_launches at M <= 96)."""
    k = case("c2", 512)
    for q in (None, k["H"][:1]):
        out = {}
        for mode in ("2", "0"):
            monkeypatch.setenv("FFVD_STEP_LOOP", mode)
            got, _, moved = run_rollout(k, R, 8, q, seed=R)
            assert moved == 0
            out[mode] = got
        np.testing.assert_allclose(out["2"][0], out["0"][0], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(out["2"][1], out["0"][1], rtol=1e-9, atol=1e-10)


# ------------------------------------------------------------------------------------------------------------------------------
# particle-Gibbs sweep
# ------------------------------------------------------------------------------------------------------------------------------
SWEEP = [("c2", 512, {}, 33, 1, 17), ("c2", 512, {}, 101, 3, 17), ("c2", 512, {}, 513, 3, 17), ("c2", 512, {}, 700, 1, 17),
         ("c2", 600, {}, 101, 3, 25), ("c2", 600, {}, 700, 3, 17), ("c2", 2048, dict(D=2), 33, 1, 33), ("c2", 2048, dict(D=2), 513, 1, 17),
         ("small_lin", 512, dict(T=1024), 101, 1, 25), ("small_lin", 512, dict(T=1024), 700, 3, 17)]


@pytest.mark.parametrize("name,M,ov,N,Ydim,XN", SWEEP, ids=[f"{n}-M{m}-N{p}-Y{y}" for n, m, _, p, y, _ in SWEEP])
def test_pg_sweep_at_large_m(name, M, ov, N, Ydim, XN):
    """One particle-Gibbs sweep over X[:XN] against the oracle with the same draws, at M = 512 (config 2), 600 (Mp = 640) and 2048
    (the cap), SE and LinearK: 32 and 100 free particles (skinny product, fast step), 512 (skinny product at its 512-row edge,
    N D > 2048: the general step) and 699 (the tiled step: kfu_build + proj_gemm); Ydim 1 and 3.  Identical ancestor indices, particle
    states to 1e-9 / 1e-10 on the skinny product and 1e-7 / 1e-8 on the tiled one (test_gpu_ops.test_pg_sweep_matches_oracle).  Also:
    a particle that drew the reference's index carries the reference's state, and u -> 1 returns X itself from t = 1 on.

    At M = 2048 the absolute tolerance is eps kappa(K_uu + jI) (kappa ~ 6e7 there, against ~1e7 at M = 512): the first step of the
    512-particle sweep is off by 6e-12, and the difference then grows about 1.5 x per step with the trajectory (1.4e-9 after 16
    steps, measured; 3e-10 after 32 steps with 32 particles), where at M = 512 the same sweep ends at 5e-11."""
    k = case(name, M, **ov)
    D, T = k["meta"]["D"], XN - 1
    X, c = k["X"][:XN], k["c"][:T]
    p = k["params"]
    rng = np.random.default_rng(N + M)
    CC, DD, Rch, Y = p["CC"], p["DD"], np.exp(p["log_Rchols"]), k["Y"][:T]
    if Ydim > 1:
        CC = rng.standard_normal((D, Ydim)) * 0.5
        DD = rng.standard_normal(Ydim) * 0.1
        Rch = np.tril(rng.standard_normal((Ydim, Ydim)) * 0.2) + np.diag(0.4 + rng.random(Ydim))
        Y = X[1:] @ CC + DD + 0.4 * rng.standard_normal((T, Ydim))
    x0, eps, u = rng.standard_normal((N - 1, D)), rng.standard_normal((T, N - 1, D)), rng.random((T, N - 1))
    args = (k["Z"], k["kern"], p["U"], X, Y, c, CC, DD, Rch, k["Q"], x0, eps)
    pg, ig = pg_sweep(k["L"], *args, u)
    po, io = pgo.pg_sweep(k["L"], k["Z"], k["okern"], p["U"], X, Y, c, CC, DD, Rch, k["Q"], x0, eps, u)
    assert pg.shape == (XN, N - 1, D) and ig.shape == (T, N - 1)
    np.testing.assert_array_equal(ig, io)
    tol = dict(rtol=1e-7, atol=1e-8) if N - 1 > 512 else dict(rtol=1e-9, atol=1e-10)
    if M == 2048:
        tol["atol"] = max(tol["atol"], EPS * max(cond(kuu(k, d)) for d in range(D)))
    np.testing.assert_allclose(pg, po, **tol)
    np.testing.assert_array_equal(pg[0], x0)
    hits = np.argwhere(ig == N - 1)
    assert len(hits)
    for t, i in hits[:: max(1, len(hits) // 16)]:
        np.testing.assert_array_equal(pg[t + 1, i], X[t + 1])
    p1, i1 = pg_sweep(k["L"], *args, np.full_like(u, 1.0 - 1e-16))
    assert np.all(i1 == N - 1)
    np.testing.assert_array_equal(p1[1:], np.repeat(X[1:, None, :], N - 1, axis=1))
