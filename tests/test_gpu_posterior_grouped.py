"""Grouped collapsed posteriors on the device (`ffvd_op_posterior_grouped`, conditionals_multi_output.collapse_u_mean_grouped) and
their fusion with the grouped rollouts (`ffvd_op_posterior_rollout_grouped`, prediction.posterior_rollout_grouped), through DGPSSM as
well (collect_samples_chains(fused=True), rollout_mode="intent-fused").

Reference and rule.  The reference is the oracle, group by group: orc.kernel_pre_cal -> orc.collapse_u_mean_after_kernel_precalculation
-> orc.rollout.  L^-T is ill-conditioned (kappa ~ 1e6; the project compares it at rtol 1e-6 / atol 1e-7) and the whitened posterior
inherits that, so no tolerance is fixed in advance: every test also runs the COMPOSED device path (cmo.kernel_pre_cal, then
cmo.collapse_u_mean_after_kernel_precalculation per group, then rollout_grouped) on the same inputs and takes its largest absolute
error e_ref against the oracle, per array.  The new path must satisfy  error <= max(4 e_ref, floor),  the floor being the project's
own absolute tolerance for that array (1e-10 U_mean / L_H^-T, 1e-7 L^-T, 1e-9 rollout states, 1e-10 rollout variances); the factor 4
covers a different order of summation in a split Gram launch and nothing else.  Both errors are printed per case."""
import functools

import numpy as np
import pytest

from ffvd_amd import _lib, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import posterior_rollout_grouped, rollout_grouped
from oracle import ffvd_oracle as orc

pytestmark = pytest.mark.gpu

FLOOR = dict(U=1e-10, H=1e-10, L=1e-7, px=1e-9, pv=1e-10)
SHAPES = {"tiny": ("tiny", {}), "ragged": ("ragged", {}), "small": ("small", {}), "tiny64": ("tiny", dict(M=64)),
          "tiny_noctrl": ("tiny", dict(C=0)), "small_lin": ("small_lin", {})}


def _kernels(p, meta):
    D, P = meta["D"], meta["P"]
    if meta["kernel_type"] == "LinearK":
        return [LinearK(P, variance=np.exp(p["logvariance"][d])) for d in range(D)]
    return [SquaredExponential(P, variance=np.exp(p["logvariance"][d]), lengthscales=np.exp(p["loglengthscales"][d]))
            for d in range(D)]


def _group(p, c, meta, X):
    """One group: its model (Z, kernels for the device and for the oracle), trajectory, Q -- and, computed once, the oracle's posterior
    and the composed device path's."""
    T = meta["T"]
    okern, kern, Q = orc.make_kernels(p, kernel_type=meta["kernel_type"]), _kernels(p, meta), np.exp(p["log_Q"])
    xc = np.concatenate((X[:T], c[:T]), axis=1)
    Lo = orc.kernel_pre_cal(p["Z"], okern)
    Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, xc, X, p["Z"], okern, Q)
    Ld = cmo.kernel_pre_cal(p["Z"], kern)
    Ud, Hd = cmo.collapse_u_mean_after_kernel_precalculation(Ld, xc, X, p["Z"], kern, Q)
    return dict(Z=p["Z"], kern=kern, okern=okern, X=X, Q=Q, orc=dict(L=np.stack(Lo), U=Uo, H=np.asarray(Ho)),
                dev=dict(L=np.stack(Ld), U=Ud, H=np.asarray(Hd)))


@functools.lru_cache(maxsize=None)
def case(shape, per_model, G=None):
    """Shared model: the workload's own S chains (or G of them).  One model per group: G groups, each the workload's parameters under
    a seeded perturbation (log-hyper-parameters + 0.05 N(0,1), Z + 0.01 N(0,1), log Q + 0.05 N(0,1)) and a different chain + 0.1 N(0,1)
    as its X -- a mixed-up group or dim index moves the results by many orders more than any tolerance."""
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


def _model_args(cs):
    gs, c, meta, per_model = cs
    if per_model:
        return [g["Z"] for g in gs], [g["kern"] for g in gs], [g["X"] for g in gs], [g["Q"] for g in gs]
    return gs[0]["Z"], gs[0]["kern"], [g["X"] for g in gs], [g["Q"] for g in gs]


def rule(what, key, new, dev, ref):
    """error of the new path <= max(4 x error of the composed device path, the project's floor for this array)"""
    e_new, e_ref = float(np.max(np.abs(np.asarray(new) - ref))), float(np.max(np.abs(np.asarray(dev) - ref)))
    print(f"{what}: {key}: new path {e_new:.3e}, composed path e_ref {e_ref:.3e}, bound {max(4 * e_ref, FLOOR[key]):.3e}")
    assert np.all(np.isfinite(new)), f"{what}: {key}"
    assert e_new <= max(4.0 * e_ref, FLOOR[key]), f"{what}: {key}: {e_new:.3e} > max(4 x {e_ref:.3e}, {FLOOR[key]:.0e})"


def _check_posterior(what, cs, U, H, L):
    gs, _, _, per_model = cs
    for g, grp in enumerate(gs):
        rule(f"{what} group {g}", "U", U[g], grp["dev"]["U"], grp["orc"]["U"])
        if H is not None:
            rule(f"{what} group {g}", "H", H[g], grp["dev"]["H"], grp["orc"]["H"])
        if L is not None and (per_model or g == 0):
            rule(f"{what} group {g}", "L", L[g], grp["dev"]["L"], grp["orc"]["L"])


def _posterior(cs, **kw):
    Zs, kerns, Xs, Qs = _model_args(cs)
    return cmo.collapse_u_mean_grouped(Zs, kerns, Xs, cs[1], Qs, **kw)


@pytest.mark.parametrize("shape", ["tiny", "ragged", "small", "tiny64"])
def test_posterior_of_the_chains_of_one_model(shape):
    cs = case(shape, False)
    gs, _, meta, _ = cs
    U, H, L = _posterior(cs)
    assert U.shape == (meta["S"], meta["M"], meta["D"]) and H.shape == (meta["S"], meta["D"], meta["M"], meta["M"])
    assert L.shape == (1, meta["D"], meta["M"], meta["M"])
    _check_posterior(shape, cs, U, H, L)


@pytest.mark.parametrize("shape", ["tiny", "ragged"])
def test_posterior_with_one_model_per_group(shape):
    cs = case(shape, True, 5)
    U, H, L = _posterior(cs)
    assert L.shape[0] == 5
    _check_posterior(shape, cs, U, H, L)


@pytest.mark.parametrize("shape,per_model", [("tiny", True), ("ragged", True), ("tiny", False)])
def test_passes_of_two_groups_with_a_short_last_pass(shape, per_model):
    """G = 5 in passes of 2, 2 and 1: F and the H slabs are reused between the passes.  Also prints the largest difference between
    the groups of this call, of the one-pass call and of each group computed alone (the header does not promise them equal)."""
    cs = case(shape, per_model, 5)
    U, H, L = _posterior(cs, groups_per_pass=2)
    _check_posterior(f"{shape} passes of 2", cs, U, H, L)
    U1, H1, _ = _posterior(cs)
    dU, dH = np.max(np.abs(U - U1)), np.max(np.abs(H - H1))
    Zs, kerns, Xs, Qs = _model_args(cs)
    aU = aH = 0.0
    for g in range(5):
        Ua, Ha, _ = cmo.collapse_u_mean_grouped(Zs[g] if per_model else Zs, kerns[g] if per_model else kerns, Xs[g:g + 1], cs[1],
                                                Qs[g:g + 1])
        rule(f"{shape} group {g} alone", "U", Ua[0], cs[0][g]["dev"]["U"], cs[0][g]["orc"]["U"])
        rule(f"{shape} group {g} alone", "H", Ha[0], cs[0][g]["dev"]["H"], cs[0][g]["orc"]["H"])
        aU, aH = max(aU, np.max(np.abs(Ua[0] - U1[g]))), max(aH, np.max(np.abs(Ha[0] - H1[g])))
    print(f"{shape} per_model={per_model}: passes of 2 against one pass: max |dU| = {dU:.3e}, max |dL_H^-T| = {dH:.3e}; "
          f"a group alone against the group among five: max |dU| = {aU:.3e}, max |dL_H^-T| = {aH:.3e}")


@pytest.mark.parametrize("shape,per_model", [("ragged", False), ("tiny", True)])
def test_u_mean_does_not_depend_on_whether_the_factors_are_asked_for(shape, per_model):
    cs = case(shape, per_model, 5 if per_model else None)
    U, H, L = _posterior(cs)
    U2, H2, L2 = _posterior(cs, return_factors=False)
    assert H2 is None and L2 is None
    np.testing.assert_array_equal(U2, U)


def _ctrl(c, meta, steps, seed=5):
    return np.concatenate((c, np.random.default_rng(seed).standard_normal((steps, meta["C"]))))


def _fused_against_the_oracle(what, cs, R, steps, **kw):
    gs, c, meta, _ = cs
    G, D, T = len(gs), meta["D"], meta["T"]
    ctrl = _ctrl(c, meta, steps)
    eps = np.random.default_rng(11).standard_normal((steps, G, R, D))
    Zs, kerns, Xs, Qs = _model_args(cs)
    px, pv, U = posterior_rollout_grouped(Zs, kerns, Xs, Qs, ctrl, T, steps, eps, return_U=True, **kw)
    assert px.shape == pv.shape == (G, R, steps, D) and U.shape == (G, meta["M"], D)
    assert np.all(pv > 0)
    # the composed device path of today: its own posteriors (computed with the case) through rollout_grouped
    dx, dv = rollout_grouped([list(g["dev"]["L"]) for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs],
                             [g["dev"]["U"] for g in gs], [g["dev"]["H"] for g in gs], [g["X"][-1] for g in gs], ctrl, T, steps,
                             [g["Q"] for g in gs], eps)
    for i, g in enumerate(gs):
        o = g["orc"]
        po, vo = orc.rollout(list(o["L"]), g["Z"], g["okern"], o["U"], o["H"], g["X"][-1], ctrl, T, steps, g["Q"], eps[:, i])
        rule(f"{what} group {i}", "U", U[i], g["dev"]["U"], o["U"])
        rule(f"{what} group {i}", "px", px[i], dx[i], po)
        rule(f"{what} group {i}", "pv", pv[i], dv[i], vo)
    return px, pv, U


@pytest.mark.parametrize("R,steps", [(1, 7), (9, 5)])
@pytest.mark.parametrize("shape", ["tiny", "ragged", "small", "tiny64"])
def test_fused_rollouts_of_the_chains_of_one_model(shape, R, steps):
    _fused_against_the_oracle(f"{shape} R={R}", case(shape, False), R, steps)


@pytest.mark.parametrize("shape", ["tiny", "ragged"])
def test_fused_rollouts_with_one_model_per_group(shape):
    _fused_against_the_oracle(f"{shape} per model", case(shape, True, 5), 3, 5)
    _fused_against_the_oracle(f"{shape} per model, passes of 2", case(shape, True, 5), 3, 5, groups_per_pass=2)


def test_fused_rollouts_without_control_inputs():
    _fused_against_the_oracle("tiny C=0", case("tiny_noctrl", False), 9, 5)
    _fused_against_the_oracle("tiny C=0 per model", case("tiny_noctrl", True, 5), 3, 5)


def test_linear_kernels():
    cs = case("small_lin", False)
    U, H, L = _posterior(cs)
    _check_posterior("small_lin", cs, U, H, L)
    _fused_against_the_oracle("small_lin", cs, 3, 5)


def test_two_identical_fused_calls_are_equal():
    for cs, R in ((case("ragged", False), 9), (case("tiny", True, 5), 1)):
        gs, c, meta, _ = cs
        steps = 6
        ctrl = _ctrl(c, meta, steps)
        eps = np.random.default_rng(12).standard_normal((steps, len(gs), R, meta["D"]))
        Zs, kerns, Xs, Qs = _model_args(cs)
        a = posterior_rollout_grouped(Zs, kerns, Xs, Qs, ctrl, meta["T"], steps, eps, return_U=True)
        b = posterior_rollout_grouped(Zs, kerns, Xs, Qs, ctrl, meta["T"], steps, eps, return_U=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        U1, H1, L1 = _posterior(cs)
        U2, H2, L2 = _posterior(cs)
        for x, y in ((U1, U2), (H1, H2), (L1, L2), (a[2], U1)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("fused", [False, True], ids=["posterior", "fused"])
def test_a_k_uu_that_is_not_positive_definite_is_named_and_nothing_is_written(fused):
    """jitter = -2 max(variance): the first pivot of every K_uu + jitter I is negative by construction."""
    cs = case("tiny", False)
    gs, c, meta, _ = cs
    Zs, kerns, Xs, Qs = _model_args(cs)
    a = cmo.pack_posterior_groups(Zs, kerns, Xs, c, Qs, "test")
    G, M, D, R, steps = a["G"], a["M"], a["D"], 2, 3
    jitter = -2.0 * float(np.max(np.exp(a["logvar"])))
    lib, dp = _lib.load(), _lib.dptr
    U, H, L = np.full((G, M, D), 7.0), np.full((G, D, M, M), 7.0), np.full((1, D, M, M), 7.0)
    px, pv = np.full((G, R, steps, D), 7.0), np.full((G, R, steps, D), 7.0)
    eps, ctrl = np.zeros((steps, G, R, D)), np.zeros((steps, a["C"]))
    if fused:
        rc = lib.ffvd_op_posterior_rollout_grouped(a["kind"], G, 1, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]), dp(a["loglen"]), dp(a["X"]),
                                                   dp(a["ctrl"]), a["C"], a["T"], dp(a["log_Q"]), jitter, 0, R, dp(ctrl), steps, dp(eps),
                                                   dp(px), dp(pv), dp(U))
    else:
        rc = lib.ffvd_op_posterior_grouped(a["kind"], G, 1, dp(a["Z"]), M, a["P"], D, dp(a["logvar"]), dp(a["loglen"]), dp(a["X"]),
                                           dp(a["ctrl"]), a["C"], a["T"], dp(a["log_Q"]), jitter, 0, dp(L), dp(U), dp(H))
    assert rc == _lib.FFVD_ENOTPD, rc
    msg = lib.ffvd_last_error(None).decode()
    assert "K_uu" in msg and "group 0" in msg and "latent dim 0" in msg, msg
    for out in (U, H, L, px, pv):
        assert np.all(out == 7.0)
    with pytest.raises(np.linalg.LinAlgError, match="K_uu"):
        cmo.collapse_u_mean_grouped(Zs, kerns, Xs, c, Qs, jitter=jitter)


def _case5_model(params, Y, cc, meta, num_chains=1):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd.likelihoods import Gaussian
    D, M, P = meta["D"], meta["M"], meta["P"]
    kern = [SquaredExponential(P, ARD=True, variance=np.exp(params["logvariance"][d]),
                               lengthscales=np.exp(params["loglengthscales"][d]), kernel_optimization=False) for d in range(D)]
    lik = Gaussian(1, D, CC=params["CC"], DD=params["DD"], RR_chol=np.exp(params["log_Rchols"]))
    X = params["X"][0]
    return DGPSSM(Y, [D], M, [kern], lik, QQ_chol=np.exp(0.5 * params["log_Q"]), ZZ=params["Z"], control_inputs=cc,
                  U_ini=params["U"], X_0_ini=X[0], X_train_ini=X[1:], kernel_optimization=False, U_optimization=False,
                  U_collapse=True, Z_optimization=True, case_val=5, prior_type="normal", route="gram", grad=True,
                  num_chains=num_chains)


def _oracle_rollouts(params, meta, X, cc, test_len, eps_g):
    okern, Q, T = orc.make_kernels(params, kernel_type=meta["kernel_type"]), np.exp(params["log_Q"]), meta["T"]
    Lo = orc.kernel_pre_cal(params["Z"], okern)
    Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, np.concatenate((X[:T], cc[:T]), axis=1), X, params["Z"], okern, Q)
    return orc.rollout(Lo, params["Z"], okern, Uo, Ho, X[-1], cc, T, test_len, Q, eps_g) + (Uo,)


def test_collect_samples_chains_fused():
    params, Y, c, meta = synthetic.make_named("tiny", S=3)
    D, S, test_len, R = meta["D"], 3, 6, 4
    cc = np.concatenate((c, np.random.default_rng(5).standard_normal((test_len, meta["C"]))))
    mod = _case5_model(params, Y, cc, meta, num_chains=S)
    mod.set_X(params["X"])
    eps = np.random.default_rng(10).standard_normal((test_len, S, R, D))
    old = mod.collect_samples_chains(R, cc, test_len, Y_train=Y, eps=eps)
    new = mod.collect_samples_chains(R, cc, test_len, Y_train=Y, eps=eps, fused=True)
    assert set(new) == set(old)
    assert new["predict_x"].shape == (S, R, test_len, D) and np.all(new["predict_x_var"] > 0)
    assert len(new["U_vals"]) == S
    for s in range(S):
        po, vo, Uo = _oracle_rollouts(params, meta, params["X"][s], cc, test_len, eps[:, s])
        rule(f"chain {s}", "U", new["U_vals"][s], old["U_vals"][s], Uo)
        rule(f"chain {s}", "px", new["predict_x"][s], old["predict_x"][s], po)
        rule(f"chain {s}", "pv", new["predict_x_var"][s], old["predict_x_var"][s], vo)
    summary = orc.predict_y_summary(new["predict_x"].reshape(S * R, test_len, D), new["predict_x_var"].reshape(S * R, test_len, D),
                                    params["CC"], params["DD"], params["log_Rchols"])
    np.testing.assert_allclose(new["predict_y"], summary["predict_y"], rtol=1e-12, atol=1e-12)


def test_intent_fused_against_intent_batched():
    """Two identically built and seeded case-5 models: the same sampler sequence (identical recorded variables); the rollouts under
    the rule, the oracle being run on each sample's recorded hyper-parameters."""
    params, Y, c, meta = synthetic.make_named("tiny", S=1)
    D, test_len, num, spacing = meta["D"], 6, 3, 2
    cc = np.concatenate((c, np.random.default_rng(5).standard_normal((test_len, meta["C"]))))
    eps = np.random.default_rng(9).standard_normal((test_len, num, D))
    outs = {}
    for mode in ("intent-batched", "intent-fused"):
        mod = _case5_model(params, Y, cc, meta)
        mod.seed(42)
        outs[mode] = mod.collect_samples_formal(num, spacing, cc, test_len, sghmc_var_len=2, U_collapse=True, Y_train=Y, eps=eps,
                                                rollout_mode=mode)
    a, b = outs["intent-batched"], outs["intent-fused"]
    assert set(a) == set(b)
    assert set(a["mc_posterior_samples"]) == set(b["mc_posterior_samples"]) == {"logvariance", "loglengthscales"}
    for k in a["mc_posterior_samples"]:
        np.testing.assert_array_equal(a["mc_posterior_samples"][k], b["mc_posterior_samples"][k], err_msg=k)
    assert b["predict_x"].shape == (num, test_len, D)
    for i in range(num):
        q = dict(params, logvariance=b["mc_posterior_samples"]["logvariance"][i],
                 loglengthscales=b["mc_posterior_samples"]["loglengthscales"][i])
        po, vo, Uo = _oracle_rollouts(q, meta, params["X"][0], cc, test_len, eps[:, i:i + 1])
        rule(f"sample {i}", "px", b["predict_x"][i], a["predict_x"][i], po[0])
        rule(f"sample {i}", "pv", b["predict_x_var"][i], a["predict_x_var"][i], vo[0])
        if i == num - 1:
            rule(f"sample {i}", "U", b["U_val"], a["U_val"], Uo)
