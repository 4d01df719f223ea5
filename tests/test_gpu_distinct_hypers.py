"""GPU parity with hyper-parameters that differ along every axis (tests/distinct_hypers.py): per-(d, p) ARD lengthscales, a variance
and a Q per latent dim, C / d / R per output.  Every synthetic workload of the other GPU tests has lengthscales uniform over p, one
variance for every d and proportional outputs, so a kernel that reads `loglengthscales[d][p']` with the wrong p', `logvariance`
without the `d_begin` offset of a latent-dim shard or the wrong column of C / d / log_Rchols passes them all;
tests/test_distinct_hypers.py shows on the CPU that each of those mistakes moves the nll of these cases by at least 1000 x the
tolerances used here.

Every comparison is against the CPU oracle on identical inputs, never against another GPU path (the sum-to-whole checks of the shard
tests are second assertions).  Tolerances are the ones the project already states for each path:
  forward, reference route 1e-9 with assert_terms' floors (test_gpu_elbo); one-launch path 1e-10 (test_gpu_tiny); Gram route the
  predicted 4 eps cond(K_uu) (gram_route_tolerance) times max(1, |term|) -- with these variances some terms are of order 10;
  gradients, multi-kernel schedule 1e-6 for Z / lengthscales / variance and 1e-7 otherwise (test_gradient_matches_autograd); one-launch
  path 2e-6 for Z and 1e-7 otherwise (test_gpu_tiny); explicit-U branch 1e-8 (test_explicit_u_gradient_matches_autograd).
A gradient bound is never below 10 x the disagreement of the two CPU references (closed form, torch autograd) on that case and key
(distinct_hypers.grad_bound): that value is a property of the references, not of the HIP result.  The per-latent-dim arrays
(logvariance, log_Q, loglengthscales) are normalised row by row.  Every test prints its worst error per key."""
import functools

import numpy as np
import pytest

import distinct_hypers as dh
from ffvd_amd import _lib
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.engine import ElboEngine
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import pg_sweep, rollout
from oracle import ffvd_grad_oracle as gorc
from oracle import ffvd_optim_oracle as oo
from oracle import ffvd_oracle as orc
from oracle import ffvd_pg_oracle as pgo

pytestmark = pytest.mark.gpu

RTOL = 1e-9                   # reference route (test_gpu_elbo.RTOL)
RTOL_ONE_LAUNCH = 1e-10       # test_gpu_tiny
ONE_LAUNCH_CASES = ("tiny", "ragged", "p8", "ragged_y3")          # SE kernel, P <= 8, Mp <= 128: what tiny.hip takes
GRAD_KEYS, TERMS_B, TERMS_A = dh.GRAD_KEYS, dh.TERMS_B, dh.TERMS_A


def engine(case, monkeypatch, schedule, **kw):
    """An engine for the case on the asked schedule (FFVD_NO_TINY is read when a handle is created); asserts that the schedule is
    the one that runs."""
    params, Y, c, meta = dh.workload(case)
    if schedule == "multi_kernel":
        monkeypatch.setenv("FFVD_NO_TINY", "1")
    else:
        monkeypatch.delenv("FFVD_NO_TINY", raising=False)
    kw.setdefault("S", params["X"].shape[0])
    S = kw.pop("S")
    e = ElboEngine(meta["T"], meta["D"], meta["C"], meta["M"], S, Ydim=meta["Ydim"], kernel_type=meta["kernel_type"], **kw)
    assert (int(e.lib.ffvd_single_launch(e._h)) != 0) == (schedule == "one_launch"), (case, schedule)
    e.set_data(Y, c)
    return e


def report(what, errs):
    print(f"{what}: " + ", ".join(f"{k}={v:.1e}" for k, v in errs.items()))


def check_forward(what, got, ref, names, path, gram_tol=None):
    """All named terms and nll_per_chain against the oracle at the tolerance of `path`."""
    errs, bad = {}, []
    for n in names:
        r = float(ref[n])
        errs[n] = abs(got[n] - r)
        if path == "gram":
            bound = gram_tol * max(1.0, abs(r))
        else:
            rtol = RTOL_ONE_LAUNCH if path == "one_launch" else RTOL
            # the trace term is a cancellation (T sigma^2 - |F|^2): its absolute floor is set by |F|^2 eps (test_gpu_elbo.assert_terms)
            bound = max(rtol * abs(r), 1e-11 if n != "nll_reg_trace_inverse_Q_B" else 1e-10)
        if not errs[n] <= bound:
            bad.append((n, got[n], r, errs[n], bound))
    pc = np.abs(got["nll_per_chain"] - ref["nll_per_chain"])
    errs["nll_per_chain"] = float(pc.max())
    report(f"forward {what} [{path}" + (f", 4 eps cond = {gram_tol:.1e}" if path == "gram" else "") + "] abs.err", errs)
    assert not bad, bad
    if path == "gram":
        assert np.all(pc <= gram_tol * np.maximum(1.0, np.abs(ref["nll_per_chain"])))
    else:
        np.testing.assert_allclose(got["nll_per_chain"], ref["nll_per_chain"], rtol=RTOL_ONE_LAUNCH if path == "one_launch" else RTOL)


def grad_tolerance(key, schedule, collapse):
    if not collapse:
        return 1e-8
    if schedule == "one_launch":
        return 2e-6 if key == "Z" else 1e-7
    return 1e-6 if key in ("Z", "loglengthscales", "logvariance") else 1e-7


def check_grad(what, case, collapse, schedule, got, ref, keys=None):
    keys = keys or (GRAD_KEYS + (() if collapse else ("U",)))
    errs = dh.grad_errors(got, ref, keys)
    report(f"gradient {what} {case} {'B' if collapse else 'A'} [{schedule}] rel.err", errs)
    for k in keys:
        assert errs[k] < dh.grad_bound(case, collapse, k, grad_tolerance(k, schedule, collapse)), (k, errs[k])


# ------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------
FORWARD = ([(c, "one_launch", p) for c in ONE_LAUNCH_CASES for p in ("B", "A")]
           + [(c, "multi_kernel", p) for c in ("tiny", "ragged", "p8", "p9", "ragged_y3", "lin_y2") for p in ("B", "gram", "A")]
           + [("m256", "multi_kernel", "gram"), ("m600", "multi_kernel", "B"), ("m600", "multi_kernel", "gram"), ("m600", "multi_kernel", "A")])


@pytest.mark.parametrize("case,schedule,path", FORWARD, ids=["-".join(f) for f in FORWARD])
def test_forward(case, schedule, path, monkeypatch):
    """nll and every named term: branch B in the reference's op order, branch B on the Gram route, branch A; on the one-launch path
    (P = 3, 5, 8) and on the multi-kernel schedule (also P = 9: the generic-P K build; M = 256: the Gram kernel's pair combos; M =
    600: two column groups; LinearK with two outputs)."""
    params, Y, c, meta = dh.workload(case)
    collapse = path != "A"
    ref = dh.forward_reference(case, collapse)
    with engine(case, monkeypatch, schedule, U_collapse=collapse, route="gram" if path == "gram" else "reference") as e:
        got = e.nll_terms(params)
    names = TERMS_B if collapse else TERMS_A
    if path == "gram":
        check_forward(case, got, ref, names, "gram", dh.gram_route_tolerance(params, meta))
    else:
        check_forward(case, got, ref, names, "one_launch" if schedule == "one_launch" else "reference")


# ------------------------------------------------------------------------------------------------------------------------------
# gradients
# ------------------------------------------------------------------------------------------------------------------------------
GRAD_CASES = dh.GRAD_CASES                      # tiny, ragged, p8, p9, m256, ragged with three outputs
GRADS = ([(c, "one_launch", b) for c in GRAD_CASES if c in ONE_LAUNCH_CASES for b in ("B", "A")]
         + [(c, "multi_kernel", b) for c in GRAD_CASES for b in ("B", "A")])
AUTOGRAD_CASES = ("tiny", "p8", "p9")           # the three smallest shapes: also against torch autograd


@pytest.mark.parametrize("case,schedule,branch", GRADS, ids=["-".join(g) for g in GRADS])
def test_gradient(case, schedule, branch, monkeypatch):
    """d nll / d every parameter (and U in branch A) against the closed-form oracle, on the three smallest shapes against torch
    autograd as well: per-(d, p) lengthscales inside dK/dX, dK/dZ and the Hadamard chain rule on the fused (P <= 6), the P <= 8 and
    the generic-P path, and three outputs with their own C, d and R."""
    params, Y, c, meta = dh.workload(case)
    collapse = branch == "B"
    with engine(case, monkeypatch, schedule, U_collapse=collapse, route="gram" if collapse else "reference", grad=True) as e:
        terms, g = e.nll_and_grad(params)
    ref_nll = dh.forward_reference(case, collapse)["nll"]
    assert terms["nll"] == pytest.approx(ref_nll, rel=1e-8 if collapse else 1e-9)
    check_grad("vs closed form", case, collapse, schedule, g, dh.grad_reference(case, collapse))
    if case in AUTOGRAD_CASES:
        check_grad("vs autograd", case, collapse, schedule, g, dh.autograd_reference(case, collapse))


@pytest.mark.parametrize("case", ["ragged", "p9"])
def test_gradient_reference_route(case, monkeypatch):
    """The backward pass behind the reference-route forward (what the fp32-contraction backward shares) at its own tolerances
    (test_gpu_f32c.test_reference_route_gradient_fp64: 1e-6 / 1e-7)."""
    params, Y, c, meta = dh.workload(case)
    with engine(case, monkeypatch, "multi_kernel", route="reference", grad=True) as e:
        terms, g = e.nll_and_grad(params)
    assert terms["nll"] == pytest.approx(dh.forward_reference(case, True)["nll"], rel=1e-9)
    check_grad("reference route", case, True, "multi_kernel", g, dh.grad_reference(case, True))


@pytest.mark.parametrize("branch", ["B", "A"])
def test_gradient_linear_kernel_two_outputs(branch, monkeypatch):
    """LinearK with Ydim = 2 against torch autograd (the closed form is SE only), at the bound of
    test_collapsed_gradient_linear_kernel: K_uu has rank P << M, only the jitter makes it positive definite."""
    params, Y, c, meta = dh.workload("lin_y2")
    collapse = branch == "B"
    with engine("lin_y2", monkeypatch, "multi_kernel", U_collapse=collapse, route="gram" if collapse else "reference", grad=True) as e:
        terms, g = e.nll_and_grad(params)
    ref = dh.autograd_reference("lin_y2", collapse)
    errs = dh.grad_errors(g, ref, tuple(ref))
    report(f"gradient lin_y2 {branch} vs autograd rel.err", errs)
    for k, v in errs.items():
        assert v < 1e-5, (k, v)
    assert not np.any(g["loglengthscales"])


# ------------------------------------------------------------------------------------------------------------------------------
# latent-dim shards with d_begin > 0
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["one_launch", "multi_kernel"])
@pytest.mark.parametrize("branch", ["B", "A"])
def test_dim_shards_against_the_oracle(branch, schedule, monkeypatch):
    """A shard that does not start at latent dim 0 (d_begin = 1 with D - 1 dims, d_begin = D - 1 with one) against the ORACLE's share
    for those dims (orc.nll_terms_shard) and the oracle's gradient rows for the dims it owns; shard sums that are only compared with
    the whole engine cancel a missing d_begin offset when every dim has the same variance.  Second assertion: with its complement the
    shard adds up to the whole."""
    case = "ragged"
    params, Y, c, meta = dh.workload(case)
    collapse = branch == "B"
    S, D, T = meta["S"], meta["D"], meta["T"]
    path = "one_launch" if schedule == "one_launch" else "reference"
    gref = dh.grad_reference(case, collapse)
    own = ("logvariance", "log_Q", "loglengthscales")

    def run(d0, dc, shared):
        with engine(case, monkeypatch, schedule, U_collapse=collapse, d_begin=d0, d_count=dc, shared_terms=shared) as e:
            sums = e.elbo_sums(params)
        with engine(case, monkeypatch, schedule, U_collapse=collapse, d_begin=d0, d_count=dc, shared_terms=shared,
                    route="gram" if collapse else "reference", grad=True) as e:
            g = e.nll_and_grad(params, S_total=S)[1]
        return sums, g

    whole_sums, whole_g = run(0, D, True)
    names = TERMS_B if collapse else TERMS_A
    for (d0, dc), (c0, cc) in (((1, D - 1), (0, 1)), ((D - 1, 1), (0, D - 1))):
        sums, g = run(d0, dc, False)
        assert sums[7] == 0                                      # the chains are counted where the shared terms are
        ref = None
        for s in range(S):
            t = orc.nll_terms_shard(dict(params, X=params["X"][s]), Y, c, d0, dc, False, U_collapse=collapse)
            ref = t if ref is None else {k: ref[k] + t[k] for k in t}
        got = {n: sums[i] / S for i, n in enumerate(TERMS_B)}
        got["nll_per_chain"] = ref["nll_per_chain"] = np.zeros(1)
        check_forward(f"shard d_begin={d0} d_count={dc} {branch}", got, {k: (v / S if k != "nll_per_chain" else v) for k, v in ref.items()},
                      names, path)
        sl = slice(d0, d0 + dc)
        rows_got = {k: g[k][sl] for k in own}
        rows_ref = {k: gref[k][sl] for k in own}
        keys = own
        if not collapse:
            rows_got["U"], rows_ref["U"] = g["U"][:, sl], gref["U"][:, sl]
            keys = own + ("U",)
        check_grad(f"rows of shard d_begin={d0} d_count={dc}", case, collapse, schedule, rows_got, rows_ref, keys)
        for k in own:                                           # the rows of other owners stay zero for the all-reduce
            assert not np.any(np.delete(g[k], np.arange(d0, d0 + dc), axis=0)), k
        csums, cg = run(c0, cc, True)
        np.testing.assert_allclose(sums + csums, whole_sums, rtol=1e-12, atol=1e-13)
        for k in GRAD_KEYS + (() if collapse else ("U",)):
            np.testing.assert_allclose(g[k] + cg[k], whole_g[k], rtol=1e-9, atol=1e-9 * np.max(np.abs(whole_g[k])) + 1e-300, err_msg=k)


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 contractions, T-shards, training
# ------------------------------------------------------------------------------------------------------------------------------
def test_f32c_forward_and_gradient(monkeypatch):
    """fp32 contractions (T = 301, M = 77, D = 3, C = 2, S = 2) at test_gpu_f32c's own tolerances: every term within 1e-5 absolute and
    the nll within 1e-4 relative; gradients within 1e-2 (Z, kernel hyper-parameters), 1e-3 (X), 1e-4 (log_Q), 1e-9 (C, d, R)."""
    case = "ragged"
    params, Y, c, meta = dh.workload(case)
    ref = dh.forward_reference(case, True)
    with engine(case, monkeypatch, "multi_kernel", dtype="f32c", grad=True) as e:
        got = e.nll_terms(params)
        _, g = e.nll_and_grad(params)
    errs = {n: abs(got[n] - ref[n]) for n in TERMS_B}
    report("forward f32c abs.err", errs)
    for n in TERMS_B:
        assert errs[n] <= 1e-5, (n, got[n], ref[n])
    assert errs["nll"] <= 1e-4 * abs(ref["nll"])
    np.testing.assert_allclose(got["nll_per_chain"], ref["nll_per_chain"], rtol=0, atol=1e-5)
    gerrs = dh.grad_errors(g, dh.grad_reference(case, True), GRAD_KEYS)
    report("gradient f32c rel.err", gerrs)
    tol = dict(X=1e-3, Z=1e-2, logvariance=1e-2, loglengthscales=1e-2, log_Q=1e-4, CC=1e-9, DD=1e-9, log_Rchols=1e-9)
    for k, v in gerrs.items():
        assert v < tol[k], (k, v)


def test_time_shards_against_the_oracle():
    """Four T-shard engines (ragged with S = 2, D = 1: S * D < ranks), their exchange buffers added as the all-reduce would: the nll
    of every shard (1e-7, test_time_shards_sum_to_the_single_engine_nll) and the assembled gradient (multi-kernel tolerances) against
    the oracle at the fixture's values."""
    from ffvd_amd.distributed import shard_range
    case, nshard = "tshard", 4
    params, Y, c, meta = dh.workload(case)
    T, S = meta["T"], meta["S"]
    ref = dh.forward_reference(case, True)
    engines = []
    try:
        for r in range(nshard):
            t0, tc = shard_range(T, nshard, r)
            e = ElboEngine(tc, meta["D"], meta["C"], meta["M"], S, route="gram", t_shard=(t0, T), grad=True)
            e.set_data(Y[t0: t0 + tc], c[t0: t0 + tc])
            e.set_params(dict(params, X=np.ascontiguousarray(params["X"][:, t0: t0 + tc + 1])))
            engines.append(e)
        total = np.sum([e.tshard_local() for e in engines], axis=0)
        block = np.sum([e.tshard_finish_grad(total) for e in engines], axis=0)
        dX = np.zeros_like(params["X"])
        for r, e in enumerate(engines):
            t0, tc = shard_range(T, nshard, r)
            sums, g = e.tshard_grad_fetch(block)
            assert sums[7] == S and sums[6] / S == pytest.approx(ref["nll"], rel=1e-7)
            dX[:, t0: t0 + tc + 1] += g["X"]
            check_grad(f"T-shard {r}", case, True, "multi_kernel", g, dh.grad_reference(case, True), GRAD_KEYS[1:])
        check_grad("T-shards, assembled dX", case, True, "multi_kernel", dict(X=dX), dh.grad_reference(case, True), ("X",))
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("branch", ["B", "A"])
def test_three_adam_steps_from_the_fixture(branch, monkeypatch):
    """Three device-resident Adam steps from the fixture's values against the closed-form gradient + the Adam oracle on the CPU
    (test_device_resident_training_matches_oracle_loop and its tolerance), collapsed and explicit-U."""
    from ffvd_amd import optim
    case = "tiny"
    params, Y, c, meta = dh.workload(case)
    collapse = branch == "B"
    keys = GRAD_KEYS + (() if collapse else ("U",))
    fn = gorc.nll_grad if collapse else gorc.nll_grad_explicit_u
    lr = optim.decayed_learning_rate()
    ref = {k: np.array(params[k], dtype=np.float64) for k in keys}
    m = {k: np.zeros_like(ref[k]) for k in keys}
    v = {k: np.zeros_like(ref[k]) for k in keys}
    with engine(case, monkeypatch, "one_launch", U_collapse=collapse, route="gram" if collapse else "reference", grad=True) as e:
        e.set_params(params)
        nlls = []
        for t in range(1, 4):
            nlls.append(e.adam_step(lr)["nll"])
            p = dict(params, **ref)
            g = dh.mean_over_chains(lambda q: fn(q, Y, c), p)
            for k in keys:
                ref[k], m[k], v[k] = oo.adam_step(ref[k], g[k], m[k], v[k], t, lr)
        got = e.get_params()
    assert nlls[0] > nlls[-1]
    errs = {k: float(np.max(np.abs(got[k] - ref[k]))) for k in keys}
    report(f"three Adam steps {branch} abs.err (lr = {lr:.2e})", errs)
    for k in keys:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=2e-5 * lr + 1e-9 * np.max(np.abs(ref[k])), err_msg=k)
    if collapse:
        np.testing.assert_array_equal(got["U"], params["U"])


# ------------------------------------------------------------------------------------------------------------------------------
# operators: kernels built from the fixture's parameters, the oracle's L^-T, U_mean and L_H^-T handed in
# ------------------------------------------------------------------------------------------------------------------------------
T_OPS = 300
ROLL = dict(rtol=1e-8, atol=1e-9)             # test_gpu_ops.test_rollout_matches_oracle
ROLL_VAR = dict(rtol=1e-8, atol=1e-10)


@functools.lru_cache(maxsize=None)
def op_case(case):
    params, Y, c, meta = dh.workload(case)
    D, P = meta["D"], meta["P"]
    okern = orc.make_kernels(params, kernel_type=meta["kernel_type"])
    if meta["kernel_type"] == "LinearK":
        kern = [LinearK(P, variance=np.exp(params["logvariance"][d])) for d in range(D)]
    else:
        kern = [SquaredExponential(P, variance=np.exp(params["logvariance"][d]), lengthscales=np.exp(params["loglengthscales"][d]))
                for d in range(D)]
    X = params["X"][0]
    xc = np.concatenate((X[:-1], c), axis=1)
    n = min(T_OPS, meta["T"])
    Q = np.exp(params["log_Q"])
    L = orc.kernel_pre_cal(params["Z"], okern)
    U, H = orc.collapse_u_mean_after_kernel_precalculation(L, xc[:n], X[:n + 1], params["Z"], okern, Q)
    return dict(params=params, Y=Y, c=c, meta=meta, okern=okern, kern=kern, X=X, xc=xc, Q=Q, Z=params["Z"], L=L, U=U, H=H, n=n)


def worst(got, want, rtol, atol):
    """Worst error in units of its bound atol + rtol |want|."""
    return float(np.max(np.abs(np.asarray(got) - want) / (atol + rtol * np.abs(want))))


def check_close(what, got, want, rtol, atol):
    assert np.shape(got) == np.shape(want), what
    w = worst(got, want, rtol, atol)
    print(f"{what}: worst error {w:.2e} x its bound (rtol {rtol:g}, atol {atol:g})")
    assert w <= 1.0, what


@pytest.mark.parametrize("case", ["ragged", "p9"])
def test_conditional_operators(case):
    """conditional (its own factorisation), conditional_after_kernel_precalculation without q_sqrt, with L_H^-T and with a dense
    q_sqrt, collapse_after_kernel_precalculation and collapse_u_mean_after_kernel_precalculation, at the tolerances of test_gpu_ops /
    test_gpu_predict_shapes."""
    k = op_case(case)
    n = k["n"]
    xc, X, Z = k["xc"][:n], k["X"][:n + 1], k["Z"]
    mean, var = cmo.conditional(xc, Z, k["kern"], k["params"]["U"], white=True)
    mo, vo = orc.conditional(xc, Z, k["okern"], k["params"]["U"], white=True)
    check_close("conditional mean", mean, mo, 1e-8, 1e-9)
    check_close("conditional var", var, vo, 1e-7, 1e-10)
    rng = np.random.default_rng(17)
    dense = k["H"][:1] + 0.05 * rng.standard_normal(k["H"][:1].shape) * np.abs(k["H"][:1]).max()
    for name, q in (("no q_sqrt", None), ("L_H^-T", k["H"][:1]), ("dense q_sqrt", dense)):
        m, v = cmo.conditional_after_kernel_precalculation(k["L"], xc[:65], Z, k["kern"], k["U"], q_sqrt=q, white=True)
        mo, vo = orc.conditional_after_kernel_precalculation(k["L"], xc[:65], Z, k["okern"], k["U"], q_sqrt=q)
        check_close(f"precalc conditional mean, {name}", m, mo, 1e-9, 1e-11)
        check_close(f"precalc conditional var, {name}", v, vo, 1e-8, 1e-11)
    got = cmo.collapse_after_kernel_precalculation(k["L"], xc, X, Z, k["kern"], k["Q"], n, n)
    ref = orc.collapse_after_kernel_precalculation(k["L"], xc, X, Z, k["okern"], k["Q"], n, n)
    check_close("collapse", np.asarray(got), np.asarray(ref), 1e-9, 0.0)
    Ug, Hg = cmo.collapse_u_mean_after_kernel_precalculation(k["L"], xc, X, Z, k["kern"], k["Q"])
    check_close("U_mean", Ug, k["U"], 1e-8, 1e-10)
    check_close("L_H^-T", Hg, k["H"], 1e-8, 1e-10)


def test_conditional_full_cov():
    """conditional with full_cov=True against the fp64 restatement Sigma_d = K_d(Xnew, Xnew) - F_d F_d^T (test_gpu_conditional_cov:
    rtol 1e-7, atol 1e-10)."""
    from scipy.linalg import solve_triangular
    k = op_case("ragged")
    xs, Z, U = k["xc"][:97], k["Z"], k["params"]["U"]
    mean, var = cmo.conditional(xs, Z, k["kern"], U, full_cov=True, white=True)
    means, covs = [], []
    for d, kk in enumerate(k["okern"]):
        Lc = np.linalg.cholesky(kk.K(Z) + 1e-5 * np.eye(Z.shape[0]))
        F = solve_triangular(Lc, kk.K(Z, xs), lower=True).T
        means.append(F @ U[:, d])
        covs.append(kk.K(xs) - F @ F.T)
    check_close("full_cov mean", mean, np.stack(means, axis=1), 1e-7, 1e-10)
    check_close("full_cov Sigma", var, np.stack(covs), 1e-7, 1e-10)


ROLLOUTS = [("ragged", 70, "H"), ("ragged", 20, "H"), ("d9", 5, "H"), ("m512", 16, "H")]


@pytest.mark.parametrize("case,R,qk", ROLLOUTS, ids=[f"{c}-R{r}" for c, r, _ in ROLLOUTS])
def test_rollouts(case, R, qk, monkeypatch):
    """Posterior rollouts at P = 5 (70 rollouts: per-step launches; 20: the resident loop), with more than eight inputs (D = 9,
    C = 2) and through the resident loop at M = 512 with 16 rollouts for 5 steps (the fallback counter must stand still); rollout
    tolerances 1e-8 / 1e-9 (mean) and 1e-8 / 1e-10 (variance)."""
    monkeypatch.delenv("FFVD_STEP_LOOP", raising=False)
    k = op_case(case)
    D, C, T = k["meta"]["D"], k["meta"]["C"], k["meta"]["T"]
    steps = 5
    rng = np.random.default_rng(5)
    ctrl = np.concatenate((k["c"], rng.standard_normal((steps, C))))
    eps = rng.standard_normal((steps, R, D))
    q = k["H"][:1]
    before = _lib.load().ffvd_op_rollout_fallbacks()
    px, pv = rollout(k["L"], k["Z"], k["kern"], k["U"], q, k["X"][-1], ctrl, T, steps, k["Q"], eps)
    moved = _lib.load().ffvd_op_rollout_fallbacks() - before
    pxo, pvo = orc.rollout(k["L"], k["Z"], k["okern"], k["U"], q, k["X"][-1], ctrl, T, steps, k["Q"], eps)
    assert moved == 0, _lib.load().ffvd_last_error(None)
    assert np.all(pv > 0)
    check_close(f"rollout {case} R={R} states", px, pxo, **ROLL)
    check_close(f"rollout {case} R={R} variances", pv, pvo, **ROLL_VAR)


SWEEPS = [("tiny", 12, None), ("m600", 101, 17)]


@pytest.mark.parametrize("case,N,XN", SWEEPS, ids=[f"{c}-N{n}" for c, n, _ in SWEEPS])
def test_pg_sweep(case, N, XN):
    """One particle-Gibbs sweep with the oracle's draws: identical ancestor indices, particle states to 1e-9 / 1e-10
    (test_pg_sweep_matches_oracle); `tiny` over the whole trajectory, M = 600 over X[:17]."""
    k = op_case(case)
    p = k["params"]
    D = k["meta"]["D"]
    XN = XN or k["X"].shape[0]
    T = XN - 1
    X, c, Y = k["X"][:XN], k["c"][:T], k["Y"][:T]
    rng = np.random.default_rng(N)
    Rch = np.exp(p["log_Rchols"])
    x0, eps, u = rng.standard_normal((N - 1, D)), rng.standard_normal((T, N - 1, D)), rng.random((T, N - 1))
    args = (k["Z"], k["kern"], p["U"], X, Y, c, p["CC"], p["DD"], Rch, k["Q"], x0, eps)
    pg, ig = pg_sweep(k["L"], *args, u)
    po, io = pgo.pg_sweep(k["L"], k["Z"], k["okern"], p["U"], X, Y, c, p["CC"], p["DD"], Rch, k["Q"], x0, eps, u)
    assert pg.shape == (XN, N - 1, D) and ig.shape == (T, N - 1)
    np.testing.assert_array_equal(ig, io)
    check_close(f"pg_sweep {case} particle states", pg, po, 1e-9, 1e-10)
