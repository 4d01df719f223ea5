"""Grouped GP conditionals on the device: the transition function f(x, c) of G posteriors at common inputs, explicit form
(`ffvd_op_conditional_grouped`, conditionals_multi_output.conditional_grouped), fused with the collapsed posteriors
(`ffvd_op_posterior_conditional_grouped`, prediction.posterior_conditional_grouped) and through DGPSSM.predict_transition.

Reference and rule.  The reference is the oracle, group by group: orc.kernel_pre_cal -> orc.collapse_u_mean_after_kernel_precalculation
-> orc.conditional_after_kernel_precalculation(..., q_sqrt=H) for q_mode "reference"; for "intent" the last call runs per dim d with
q_sqrt=H[d:d+1] and column d is kept.  The yardstick is the existing one-group device operator
(cmo.conditional_after_kernel_precalculation) on the same inputs -- for the explicit form the oracle's posteriors, which are also what
the new operator is given; for the fused form the whole composed device path (cmo.kernel_pre_cal, then
cmo.collapse_u_mean_after_kernel_precalculation, then the one-group operator).  Its largest absolute error against the oracle is
e_ref, per array, and the new path must satisfy  error <= max(4 e_ref, floor)  (the factor 4 is tests/test_gpu_posterior_grouped.py's).
The floors are the tolerances tests/test_gpu_ops.py applies to this operator (rtol 1e-9 / atol 1e-11 on the mean, rtol 1e-8 /
atol 1e-11 on the variance), taken at the array's largest reference magnitude: 1e-11 + 1e-9 max|ref| for means,
1e-11 + 1e-8 max|ref| for var and mix_var.  Mixture references are formed from the per-group reference arrays.  Both errors are
printed per case.

Xnew is seeded (default_rng(7)): N - N // 4 rows are GP input rows of chain 0, [X[0][:T], c[:T]], plus 0.05 N(0, 1); N // 4 rows are
3 N(0, 1), far from the data, where the variance returns to Kdiag.  On these inputs chains, dims and q slices differ by 1e-3 and
more (checked with the oracle), so a wrong group, dim or slice index is many orders above any bound used here."""
import functools

import numpy as np
import pytest

from ffvd_amd import _lib, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import posterior_conditional_grouped
from oracle import ffvd_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = {"tiny": ("tiny", {}), "ragged": ("ragged", {}), "small200": ("small", dict(M=200, S=3)), "tiny64": ("tiny", dict(M=64)),
          "tiny_noctrl": ("tiny", dict(C=0)), "small_lin": ("small_lin", dict(S=3))}
MODES = ("reference", "intent")


def floor(key, ref):
    return 1e-11 + (1e-9 if key in ("mean", "mix_mean") else 1e-8) * float(np.max(np.abs(ref)))


def rule(what, key, new, dev, ref):
    """error of the new path <= max(4 x error of the one-group device operator, the project's floor for this array)"""
    e_new, e_ref = float(np.max(np.abs(np.asarray(new) - ref))), float(np.max(np.abs(np.asarray(dev) - ref)))
    bound = max(4.0 * e_ref, floor(key, ref))
    print(f"{what}: {key}: new path {e_new:.3e}, one-group operator e_ref {e_ref:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(new)), f"{what}: {key}"
    assert e_new <= bound, f"{what}: {key}: {e_new:.3e} > max(4 x {e_ref:.3e}, {floor(key, ref):.3e})"


def _kernels(p, meta):
    D, P = meta["D"], meta["P"]
    if meta["kernel_type"] == "LinearK":
        return [LinearK(P, variance=np.exp(p["logvariance"][d])) for d in range(D)]
    return [SquaredExponential(P, variance=np.exp(p["logvariance"][d]), lengthscales=np.exp(p["loglengthscales"][d]))
            for d in range(D)]


def _group(p, c, meta, X):
    """One group: its model, trajectory and Q, and -- computed once -- the oracle's posterior and the composed device path's."""
    T = meta["T"]
    okern, kern, Q = orc.make_kernels(p, kernel_type=meta["kernel_type"]), _kernels(p, meta), np.exp(p["log_Q"])
    xc = np.concatenate((X[:T], c[:T]), axis=1)
    Lo = orc.kernel_pre_cal(p["Z"], okern)
    Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, xc, X, p["Z"], okern, Q)
    Ld = cmo.kernel_pre_cal(p["Z"], kern)
    Ud, Hd = cmo.collapse_u_mean_after_kernel_precalculation(Ld, xc, X, p["Z"], kern, Q)
    return dict(Z=p["Z"], kern=kern, okern=okern, X=X, Q=Q, orc=dict(L=list(Lo), U=Uo, H=np.asarray(Ho)),
                dev=dict(L=list(Ld), U=Ud, H=np.asarray(Hd)))


@functools.lru_cache(maxsize=None)
def case(shape, per_model, G=None):
    """Shared model: the workload's own S chains.  One model per group: G groups under the seeded perturbations of case(shape, True, G)
    in tests/test_gpu_posterior_grouped.py (log-hyper-parameters + 0.05 N(0,1), Z + 0.01 N(0,1), log Q + 0.05 N(0,1), a different
    chain + 0.1 N(0,1) as X; default_rng(1000 + g))."""
    name, ov = SHAPES[shape]
    if G is not None:
        ov = dict(ov, S=G)
    params, Y, c, meta = synthetic.make_named(name, **ov)
    gs = []
    for g in range(meta["S"]):
        q, X = dict(params), params["X"][g]
        if per_model:
            rng = np.random.default_rng(1000 + g)
            q["logvariance"] = params["logvariance"] + 0.05 * rng.standard_normal(params["logvariance"].shape)
            q["loglengthscales"] = params["loglengthscales"] + 0.05 * rng.standard_normal(params["loglengthscales"].shape)
            q["Z"] = params["Z"] + 0.01 * rng.standard_normal(params["Z"].shape)
            q["log_Q"] = params["log_Q"] + 0.05 * rng.standard_normal(params["log_Q"].shape)
            X = X + 0.1 * rng.standard_normal(X.shape)
        gs.append(_group(q, c, meta, X))
    return gs, c, meta, per_model


def make_xnew(X0, c, T, N):
    rng = np.random.default_rng(7)
    rows = np.concatenate((X0[:T], c[:T]), axis=1)
    near = N - N // 4
    pick = rng.choice(T, size=near, replace=near > T)
    return np.concatenate((rows[pick] + 0.05 * rng.standard_normal((near, rows.shape[1])),
                           3.0 * rng.standard_normal((N // 4, rows.shape[1]))))


def _oracle_cond(g, L, U, H, Xnew, mode, kern_key="okern", fn=None):
    """mean, var of one group from (L, U, H) with the oracle (or, fn = the device's one-group operator, kern_key = "kern")"""
    fn = fn or orc.conditional_after_kernel_precalculation
    kern = g[kern_key]
    if H is None or mode == "reference":
        return fn(L, Xnew, g["Z"], kern, U, q_sqrt=H, white=True)
    D = len(kern)
    outs = [fn(L, Xnew, g["Z"], kern, U, q_sqrt=H[d:d + 1], white=True) for d in range(D)]
    return outs[0][0], np.stack([outs[d][1][:, d] for d in range(D)], axis=1)


@functools.lru_cache(maxsize=None)
def refs(shape, per_model, G, N, mode, with_q=True):
    """Per group: the oracle's mean / var (`ref`), the one-group device operator on the oracle's posterior (`dev_explicit`) and on
    the composed device path's posterior (`dev_fused`).  Computed once per (case, N, mode), shared by the tests, never modified."""
    gs, c, meta, _ = case(shape, per_model, G)
    Xnew = make_xnew(gs[0]["X"], c, meta["T"], N)
    dev_op = cmo.conditional_after_kernel_precalculation
    out = dict(Xnew=Xnew, ref=[], dev_explicit=[], dev_fused=[])
    for g in gs:
        o, dv = g["orc"], g["dev"]
        out["ref"].append(_oracle_cond(g, o["L"], o["U"], o["H"] if with_q else None, Xnew, mode))
        out["dev_explicit"].append(_oracle_cond(g, o["L"], o["U"], o["H"] if with_q else None, Xnew, mode, "kern", dev_op))
        out["dev_fused"].append(_oracle_cond(g, dv["L"], dv["U"], dv["H"] if with_q else None, Xnew, mode, "kern", dev_op))
    return out


def mixture(pairs):
    m, v = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    mm = m.sum(axis=0) / len(pairs)
    return mm, (v + m * m).sum(axis=0) / len(pairs) - mm * mm


def check(what, r, yard, means, vars_, mm, mv):
    G = len(r["ref"])
    if means is not None:
        assert means.shape == vars_.shape == (G,) + r["ref"][0][0].shape
        for g in range(G):
            rule(f"{what} group {g}", "mean", means[g], r[yard][g][0], r["ref"][g][0])
            rule(f"{what} group {g}", "var", vars_[g], r[yard][g][1], r["ref"][g][1])
    if mm is not None:
        (rm, rv), (dm, dv) = mixture(r["ref"]), mixture(r[yard])
        rule(what, "mix_mean", mm, dm, rm)
        rule(what, "mix_var", mv, dv, rv)


def _models(cs):
    gs, c, meta, per_model = cs
    if per_model:
        return [g["Z"] for g in gs], [g["kern"] for g in gs]
    return gs[0]["Z"], gs[0]["kern"]


def run_explicit(cs, Xnew, mode, src="orc", with_q=True, groups=None, **kw):
    gs, c, meta, per_model = cs
    idx = range(len(gs)) if groups is None else groups
    sel = [gs[i] for i in idx]
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in sel], [g["kern"] for g in sel], [g[src]["L"] for g in sel]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    return cmo.conditional_grouped(Ls, Zs, kerns, [g[src]["U"] for g in sel], [g[src]["H"] for g in sel] if with_q else None, Xnew,
                                   q_mode=mode, **kw)


def run_fused(cs, Xnew, mode, **kw):
    gs, c, meta, _ = cs
    Zs, kerns = _models(cs)
    return posterior_conditional_grouped(Zs, kerns, [g["X"] for g in gs], [g["Q"] for g in gs], c, Xnew, q_mode=mode, **kw)


# the smallest shapes at which the kernel can go wrong: one tile with everything ragged; two row tiles; Mp = 256 (two column tiles:
# the triangular k cut and the column-tile partial sum); the exact tile edge; a single row; LinearK; no control inputs
CASES = [("tiny", False, None, 37), ("ragged", False, None, 130), ("small200", False, None, 130), ("tiny64", False, None, 37),
         ("tiny", False, None, 1), ("small_lin", False, None, 37), ("tiny_noctrl", False, None, 37),
         ("tiny", True, 5, 37), ("ragged", True, 5, 130), ("small200", True, 5, 130), ("tiny_noctrl", True, 5, 37)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G,N", CASES, ids=lambda v: str(v))
def test_explicit_form_against_the_oracle(shape, per_model, G, N, mode):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, N, mode)
    means, vars_, mm, mv = run_explicit(cs, r["Xnew"], mode)
    assert np.all(vars_ > 0)
    check(f"{shape} N={N} {mode} explicit", r, "dev_explicit", means, vars_, mm, mv)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G,N", CASES, ids=lambda v: str(v))
def test_fused_form_against_the_oracle(shape, per_model, G, N, mode):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, N, mode)
    means, vars_, mm, mv, U = run_fused(cs, r["Xnew"], mode, return_U=True)
    assert np.all(vars_ > 0) and U.shape == (len(cs[0]), cs[2]["M"], cs[2]["D"])
    check(f"{shape} N={N} {mode} fused", r, "dev_fused", means, vars_, mm, mv)


def test_the_two_q_modes_differ_where_they_should():
    """d = 0 is slice 0 in both modes (identical bits); the other dims use different slices"""
    cs = case("tiny", False)
    Xnew = refs("tiny", False, None, 37, "reference")["Xnew"]
    a, b = run_explicit(cs, Xnew, "reference"), run_explicit(cs, Xnew, "intent")
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1][:, :, 0], b[1][:, :, 0])
    assert np.max(np.abs(a[1][:, :, 1:] - b[1][:, :, 1:])) > 1e-3


@pytest.mark.parametrize("form", ["explicit", "fused"])
@pytest.mark.parametrize("mode", MODES)
def test_three_row_passes_equal_one_pass_bit_for_bit(form, mode):
    """N = 257 in passes of 128, 128 and 1 rows: F and the partial sums are reused between the passes"""
    cs, r = case("small200", False), refs("small200", False, None, 257, mode)
    run = run_explicit if form == "explicit" else run_fused
    one, three = run(cs, r["Xnew"], mode), run(cs, r["Xnew"], mode, rows_per_pass=128)
    check(f"small200 N=257 {mode} {form} passes of 128", r, "dev_" + form, *three)
    for x, y in zip(one, three):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("mode", MODES)
def test_dense_q_slices(mode):
    """An upper-triangular slice plus a seeded strict lower part takes the full k range: same rule.  With the lower part set to zero
    the dense path is not taken -- so one group keeps a dense slice and the others, whose slices ARE triangular, must come out of the
    full-range launch with the bits of the triangular launch."""
    gs, c, meta, _ = case("small200", False)
    M, D = meta["M"], meta["D"]
    r = refs("small200", False, None, 130, mode)
    Xnew, rng = r["Xnew"], np.random.default_rng(21)
    Ws, Us = gs[0]["orc"]["L"], [g["orc"]["U"] for g in gs]
    dense = [g["orc"]["H"] + 0.01 * np.tril(rng.standard_normal((D, M, M)), -1) for g in gs]
    means, vars_, _, _ = cmo.conditional_grouped(Ws, gs[0]["Z"], gs[0]["kern"], Us, dense, Xnew, q_mode=mode)
    dev_op = cmo.conditional_after_kernel_precalculation
    for i, g in enumerate(gs):
        ref = _oracle_cond(g, Ws, Us[i], dense[i], Xnew, mode)
        dev = _oracle_cond(g, Ws, Us[i], dense[i], Xnew, mode, "kern", dev_op)
        rule(f"dense q, {mode}, group {i}", "mean", means[i], dev[0], ref[0])
        rule(f"dense q, {mode}, group {i}", "var", vars_[i], dev[1], ref[1])
        assert np.max(np.abs(ref[1] - r["ref"][i][1])) > 1e-6 * np.max(np.abs(ref[1]))          # the lower part is seen
    tri = cmo.conditional_grouped(Ws, gs[0]["Z"], gs[0]["kern"], Us, [g["orc"]["H"] for g in gs], Xnew, q_mode=mode)
    zeroed = cmo.conditional_grouped(Ws, gs[0]["Z"], gs[0]["kern"], Us, [np.triu(q) for q in dense], Xnew, q_mode=mode)
    for x, y in zip(zeroed, tri):
        np.testing.assert_array_equal(x, y)
    mixed = cmo.conditional_grouped(Ws, gs[0]["Z"], gs[0]["kern"], Us, [dense[0]] + [g["orc"]["H"] for g in gs[1:]], Xnew, q_mode=mode)
    np.testing.assert_array_equal(mixed[0], tri[0])
    np.testing.assert_array_equal(mixed[1][1:], tri[1][1:])
    np.testing.assert_array_equal(mixed[1][0], vars_[0])


@pytest.mark.parametrize("shape,per_model,N", [("tiny", True, 37), ("small200", True, 130), ("ragged", False, 130)])
def test_a_group_alone_equals_the_group_among_the_others(shape, per_model, N):
    G = 5 if per_model else None
    cs = case(shape, per_model, G)
    for mode in MODES:
        Xnew = refs(shape, per_model, G, N, mode)["Xnew"]
        means, vars_, _, _ = run_explicit(cs, Xnew, mode)
        for g in range(len(cs[0])):
            m1, v1, _, _ = run_explicit(cs, Xnew, mode, groups=[g])
            np.testing.assert_array_equal(m1[0], means[g])
            np.testing.assert_array_equal(v1[0], vars_[g])


def test_two_identical_fused_calls_are_equal():
    for cs, key in ((case("ragged", False), ("ragged", False, None)), (case("tiny", True, 5), ("tiny", True, 5))):
        Xnew = refs(*key, 37 if key[0] == "tiny" else 130, "intent")["Xnew"]
        a, b = run_fused(cs, Xnew, "intent", return_U=True), run_fused(cs, Xnew, "intent", return_U=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("shape,per_model,G,N", [("tiny", False, None, 37), ("small200", True, 5, 130), ("small_lin", False, None, 37)],
                         ids=lambda v: str(v))
def test_explicit_u_without_q_sqrt(shape, per_model, G, N):
    """q_sqrts=None: per group what the one-group operator gives without q_sqrt"""
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, N, "reference", False)
    check(f"{shape} no q_sqrt", r, "dev_explicit", *run_explicit(cs, r["Xnew"], "reference", with_q=False))
    with_q = refs(shape, per_model, G, N, "reference")
    assert np.max(np.abs(with_q["ref"][0][1] - r["ref"][0][1])) > 1e-6


@pytest.mark.parametrize("form", ["explicit", "fused"])
def test_unrequested_outputs_change_nothing_in_the_others(form):
    cs, r = case("ragged", False), refs("ragged", False, None, 130, "reference")
    run = run_explicit if form == "explicit" else run_fused
    full = run(cs, r["Xnew"], "reference")
    only_groups, only_mix = run(cs, r["Xnew"], "reference", summary=False), run(cs, r["Xnew"], "reference", per_group=False)
    assert only_groups[2] is None and only_groups[3] is None and only_mix[0] is None and only_mix[1] is None
    for i in (0, 1):
        np.testing.assert_array_equal(only_groups[i], full[i])
    for i in (2, 3):
        np.testing.assert_array_equal(only_mix[i], full[i])


def test_a_k_uu_that_is_not_positive_definite_is_named_and_nothing_is_written():
    """jitter = -2 max(variance): the first pivot of every K_uu + jitter I is negative by construction."""
    gs, c, meta, _ = case("tiny", False)
    Zs, kerns, Xs, Qs = gs[0]["Z"], gs[0]["kern"], [g["X"] for g in gs], [g["Q"] for g in gs]
    a = cmo.pack_posterior_groups(Zs, kerns, Xs, c, Qs, "test")
    G, M, D, N = a["G"], a["M"], a["D"], 9
    jitter = -2.0 * float(np.max(np.exp(a["logvar"])))
    lib, dp = _lib.load(), _lib.dptr
    Xnew = np.zeros((N, a["P"]))
    outs = [np.full((G, N, D), 7.0), np.full((G, N, D), 7.0), np.full((N, D), 7.0), np.full((N, D), 7.0), np.full((G, M, D), 7.0)]
    rc = lib.ffvd_op_posterior_conditional_grouped(a["kind"], G, 1, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]), dp(a["loglen"]), dp(a["X"]),
                                                   dp(a["ctrl"]), a["C"], a["T"], dp(a["log_Q"]), jitter, 0, 0, dp(Xnew), N, 0,
                                                   *[dp(o) for o in outs])
    assert rc == _lib.FFVD_ENOTPD, rc
    msg = lib.ffvd_last_error(None).decode()
    assert "K_uu" in msg and "group 0" in msg and "latent dim 0" in msg, msg
    for out in outs:
        assert np.all(out == 7.0)
    with pytest.raises(np.linalg.LinAlgError, match="K_uu"):
        posterior_conditional_grouped(Zs, kerns, Xs, Qs, c, Xnew, jitter=jitter)


def _model(params, Y, cc, meta, num_chains, U_collapse):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd.likelihoods import Gaussian
    D, M, P = meta["D"], meta["M"], meta["P"]
    kern = [SquaredExponential(P, ARD=True, variance=np.exp(params["logvariance"][d]),
                               lengthscales=np.exp(params["loglengthscales"][d]), kernel_optimization=False) for d in range(D)]
    lik = Gaussian(1, D, CC=params["CC"], DD=params["DD"], RR_chol=np.exp(params["log_Rchols"]))
    X = params["X"][0]
    kw = dict(case_val=5, route="gram", grad=True) if U_collapse else dict(case_val=1)
    return DGPSSM(Y, [D], M, [kern], lik, QQ_chol=np.exp(0.5 * params["log_Q"]), ZZ=params["Z"], control_inputs=cc,
                  U_ini=params["U"], X_0_ini=X[0], X_train_ini=X[1:], kernel_optimization=False, U_optimization=False,
                  U_collapse=U_collapse, Z_optimization=True, prior_type="normal", num_chains=num_chains, **kw)


@pytest.mark.parametrize("mode", MODES)
def test_predict_transition_of_a_collapsed_model(mode):
    params, Y, c, meta = synthetic.make_named("tiny", S=3)
    cs, r = case("tiny", False), refs("tiny", False, None, 37, mode)
    mod = _model(params, Y, c, meta, 3, True)
    mod.set_X(params["X"])
    out = mod.predict_transition(r["Xnew"], q_mode=mode)
    assert set(out) == {"mean", "var", "mix_mean", "mix_var"} and out["mean"].shape == (3, 37, meta["D"])
    check(f"predict_transition {mode}", r, "dev_fused", out["mean"], out["var"], out["mix_mean"], out["mix_var"])
    pooled = mod.predict_transition(r["Xnew"], q_mode=mode, per_chain=False)
    assert pooled["mean"] is None and pooled["var"] is None
    np.testing.assert_array_equal(pooled["mix_mean"], out["mix_mean"])
    np.testing.assert_array_equal(pooled["mix_var"], out["mix_var"])


def test_predict_transition_of_an_explicit_u_model():
    """one group, whatever the number of chains: f does not depend on X; no q_sqrt term"""
    params, Y, c, meta = synthetic.make_named("tiny", S=3)
    Xnew = make_xnew(params["X"][0], c, meta["T"], 37)
    mod = _model(params, Y, c, meta, 3, False)
    out = mod.predict_transition(Xnew)
    assert out["mean"].shape == out["var"].shape == (1, 37, meta["D"])
    okern, kern = orc.make_kernels(params, kernel_type=meta["kernel_type"]), _kernels(params, meta)
    Lo = orc.kernel_pre_cal(params["Z"], okern)
    ref = orc.conditional_after_kernel_precalculation(Lo, Xnew, params["Z"], okern, params["U"], white=True)
    dev = cmo.conditional_after_kernel_precalculation(cmo.kernel_pre_cal(params["Z"], kern), Xnew, params["Z"], kern, params["U"], white=True)
    rule("explicit-U model", "mean", out["mean"][0], dev[0], ref[0])
    rule("explicit-U model", "var", out["var"][0], dev[1], ref[1])
    rule("explicit-U model", "mix_mean", out["mix_mean"], dev[0], ref[0])
    rule("explicit-U model", "mix_var", out["mix_var"], dev[1], ref[1])
