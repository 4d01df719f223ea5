"""Grouped posterior rollouts (`ffvd_op_rollout_grouped`, prediction.rollout_grouped): G independent posteriors -- one per SG-HMC
sample or per chain -- advanced by one launch per step.  Against the CPU restatement group by group, bit-exact independence of a
group from the others, against the one-posterior operator, and through DGPSSM (rollout_mode="intent-batched",
collect_samples_chains).

Tolerances are the project's own for this loop (tests/test_gpu_ops.py::test_rollout_matches_oracle): rtol 1e-8, atol 1e-9 for the
states and 1e-10 for the variances."""
import functools

import numpy as np
import pytest

from ffvd_amd import synthetic
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import rollout, rollout_grouped
from oracle import ffvd_oracle as orc

pytestmark = pytest.mark.gpu

ROLL = dict(rtol=1e-8, atol=1e-9)
ROLL_VAR = dict(rtol=1e-8, atol=1e-10)
T_OPS = 300              # rows of X_combine behind the posterior (the oracle's collapse is O(T M^2) per dim)


def _kernels(p, meta):
    D, P = meta["D"], meta["P"]
    if meta["kernel_type"] == "LinearK":
        return [LinearK(P, variance=np.exp(p["logvariance"][d])) for d in range(D)]
    return [SquaredExponential(P, variance=np.exp(p["logvariance"][d]), lengthscales=np.exp(p["loglengthscales"][d]))
            for d in range(D)]


def _posterior(p, c, meta, seed, perturb=True):
    """One group: the workload's parameters under a seeded perturbation (log-hyper-parameters + 0.05 N(0,1), Z + 0.01 N(0,1),
    log_Q + 0.05 N(0,1), a start state of its own) and the oracle's posterior L^-T, U_mean, L_H^-T of those parameters."""
    rng = np.random.default_rng(seed)
    q = dict(p)
    X = p["X"][0]
    x_last = X[-1].copy()
    if perturb:
        q["logvariance"] = p["logvariance"] + 0.05 * rng.standard_normal(p["logvariance"].shape)
        q["loglengthscales"] = p["loglengthscales"] + 0.05 * rng.standard_normal(p["loglengthscales"].shape)
        q["Z"] = p["Z"] + 0.01 * rng.standard_normal(p["Z"].shape)
        q["log_Q"] = p["log_Q"] + 0.05 * rng.standard_normal(p["log_Q"].shape)
        x_last = x_last + 0.1 * rng.standard_normal(x_last.shape)
    okern = orc.make_kernels(q, kernel_type=meta["kernel_type"])
    Q = np.exp(q["log_Q"])
    n = min(T_OPS, meta["T"])
    xc = np.concatenate((X[:n], c[:n]), axis=1)
    L = orc.kernel_pre_cal(q["Z"], okern)
    U, H = orc.collapse_u_mean_after_kernel_precalculation(L, xc, X[:n + 1], q["Z"], okern, Q)
    return dict(L=L, Z=q["Z"], okern=okern, kern=_kernels(q, meta), U=U, H=H, x_last=x_last, Q=Q)


@functools.lru_cache(maxsize=None)
def groups_of(name, n, **ov):
    params, Y, c, meta = synthetic.make_named(name, **ov)
    return [_posterior(params, c, meta, 1000 + g) for g in range(n)], c, meta


def _ctrl(c, meta, steps, seed=5):
    return np.concatenate((c, np.random.default_rng(seed).standard_normal((steps, meta["C"]))))


def _grouped(gs, qs, ctrl, T, steps, eps):
    return rollout_grouped([g["L"] for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs], [g["U"] for g in gs],
                           qs, [g["x_last"] for g in gs], ctrl, T, steps, [g["Q"] for g in gs], eps)


def _oracle(g, q, ctrl, T, steps, eps_g):
    return orc.rollout(g["L"], g["Z"], g["okern"], g["U"], q, g["x_last"], ctrl, T, steps, g["Q"], eps_g)


def _check(px, pv, gs, qs, ctrl, T, steps, eps, which=None):
    assert np.all(pv > 0)
    for i in (range(len(gs)) if which is None else which):
        po, vo = _oracle(gs[i], None if qs is None else qs[i], ctrl, T, steps, eps[:, i])
        dx, dv = np.max(np.abs(px[i] - po)), np.max(np.abs(pv[i] - vo))
        print(f"group {i}: max |dx| = {dx:.3e}, max |dvar| = {dv:.3e}")
        np.testing.assert_allclose(px[i], po, err_msg=f"group {i}", **ROLL)
        np.testing.assert_allclose(pv[i], vo, err_msg=f"group {i}", **ROLL_VAR)


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "noq"])
@pytest.mark.parametrize("G,R,steps", [(1, 1, 7), (5, 1, 7), (7, 3, 5), (3, 20, 5)])
@pytest.mark.parametrize("name", ["tiny", "ragged", "small"])
def test_grouped_rollout_matches_oracle_group_by_group(name, G, R, steps, with_q):
    """Every group of a grouped call against orc.rollout on that group's own posterior, same injected noise; keeps the d = 0
    q_sqrt quirk (a14).  All R take the same path (8 rollouts per workgroup; 20 rollouts = three chunks)."""
    gs, c, meta = groups_of(name, 7)
    gs = gs[:G]
    ctrl = _ctrl(c, meta, steps)
    eps = np.random.default_rng(11).standard_normal((steps, G, R, meta["D"]))
    qs = [g["H"] for g in gs] if with_q else None
    px, pv = _grouped(gs, qs, ctrl, meta["T"], steps, eps)
    assert px.shape == pv.shape == (G, R, steps, meta["D"])
    _check(px, pv, gs, qs, ctrl, meta["T"], steps, eps)


@pytest.mark.parametrize("name,R", [("tiny", 1), ("small", 3), ("ragged", 9)])
def test_a_group_does_not_depend_on_the_others(name, R):
    """Exact: each slab of a G = 7 call equals the G = 1 call of that group alone; two identical calls are equal; G copies of
    one posterior with equal noise give G identical slabs."""
    gs, c, meta = groups_of(name, 7)
    steps, D, T = 6, meta["D"], meta["T"]
    ctrl = _ctrl(c, meta, steps)
    eps = np.random.default_rng(12).standard_normal((steps, 7, R, D))
    for qs in ([g["H"] for g in gs], None):
        px, pv = _grouped(gs, qs, ctrl, T, steps, eps)
        px2, pv2 = _grouped(gs, qs, ctrl, T, steps, eps)
        np.testing.assert_array_equal(px, px2)
        np.testing.assert_array_equal(pv, pv2)
        for i in range(7):
            p1, v1 = _grouped(gs[i:i + 1], None if qs is None else qs[i:i + 1], ctrl, T, steps, eps[:, i:i + 1])
            np.testing.assert_array_equal(px[i], p1[0], err_msg=f"group {i}")
            np.testing.assert_array_equal(pv[i], v1[0], err_msg=f"group {i}")
        same = [gs[2]] * 5
        e5 = np.repeat(eps[:, 2:3], 5, axis=1)
        p5, v5 = _grouped(same, None if qs is None else [gs[2]["H"]] * 5, ctrl, T, steps, e5)
        for i in range(1, 5):
            np.testing.assert_array_equal(p5[i], p5[0])
            np.testing.assert_array_equal(v5[i], v5[0])
        np.testing.assert_array_equal(p5[0], px[2])
    # a dense q_sqrt among triangular ones changes which rows the others' second product walks (exact zeros): not their results
    rng = np.random.default_rng(3)
    qd = [g["H"] for g in gs]
    qd[4] = qd[4] + 0.05 * rng.standard_normal(qd[4].shape) * np.abs(qd[4]).max()
    pxd, pvd = _grouped(gs, qd, ctrl, T, steps, eps)
    pxt, pvt = _grouped(gs, [g["H"] for g in gs], ctrl, T, steps, eps)
    for i in (0, 3, 6):
        np.testing.assert_array_equal(pxd[i], pxt[i])
        np.testing.assert_array_equal(pvd[i], pvt[i])
    assert not np.array_equal(pvd[4], pvt[4])


@pytest.mark.parametrize("R", [1, 5])
def test_grouped_agrees_with_the_one_posterior_operator(R):
    """G = 1 against prediction.rollout on the same posterior: 1e-9, the agreement the header states between the loop forms."""
    gs, c, meta = groups_of("small", 7)
    g = gs[1]
    steps, D, T = 8, meta["D"], meta["T"]
    ctrl = _ctrl(c, meta, steps)
    eps = np.random.default_rng(13).standard_normal((steps, 1, R, D))
    for q in (g["H"], None):
        px, pv = _grouped([g], None if q is None else [q], ctrl, T, steps, eps)
        p1, v1 = rollout(g["L"], g["Z"], g["kern"], g["U"], q, g["x_last"], ctrl, T, steps, g["Q"], eps[:, 0])
        np.testing.assert_allclose(px[0], p1, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(pv[0], v1, rtol=1e-9, atol=1e-9)


def test_grouped_with_more_than_eight_inputs_linear_kernels_and_dense_q():
    """D = 9, C = 2 (P = 11 > 8, D > 8); LinearK groups (Kdiag reads the whole input row); a dense, non-triangular q_sqrt slice:
    both products then walk every row."""
    for name, ov, G, R, steps in (("tiny", dict(D=9, C=2), 3, 5, 6), ("small_lin", {}, 4, 3, 6)):
        gs, c, meta = groups_of(name, G, **ov)
        ctrl = _ctrl(c, meta, steps)
        eps = np.random.default_rng(14).standard_normal((steps, G, R, meta["D"]))
        qs = [g["H"] for g in gs]
        px, pv = _grouped(gs, qs, ctrl, meta["T"], steps, eps)
        _check(px, pv, gs, qs, ctrl, meta["T"], steps, eps)
    gs, c, meta = groups_of("small", 7)
    gs = gs[:3]
    rng = np.random.default_rng(17)
    steps, R = 9, 20
    qd = [g["H"] + 0.05 * rng.standard_normal(g["H"].shape) * np.abs(g["H"]).max() for g in gs]
    assert not np.all(np.tril(qd[0][0], -1) == 0.0)
    ctrl = _ctrl(c, meta, steps)
    eps = rng.standard_normal((steps, 3, R, meta["D"]))
    px, pv = _grouped(gs, qd, ctrl, meta["T"], steps, eps)
    _check(px, pv, gs, qd, ctrl, meta["T"], steps, eps)


def test_grouped_at_the_config2_operator_shape():
    """M = 512, D = 4, P = 5 with G = 128 posteriors, R = 1, 8 steps (8 distinct posteriors, every group a start state of its
    own); four seeded groups against the oracle."""
    params, Y, c, meta = synthetic.make_workload(**dict(synthetic.CONFIGS["c2"], T=1024, S=1))
    base = [_posterior(params, c, meta, 2000 + i) for i in range(8)]
    rng = np.random.default_rng(21)
    G, steps = 128, 8
    gs = [dict(base[i % 8], x_last=base[i % 8]["x_last"] + 0.05 * rng.standard_normal(meta["D"])) for i in range(G)]
    ctrl = _ctrl(c, meta, steps)
    eps = rng.standard_normal((steps, G, 1, meta["D"]))
    qs = [g["H"] for g in gs]
    px, pv = _grouped(gs, qs, ctrl, meta["T"], steps, eps)
    assert px.shape == (G, 1, steps, meta["D"])
    _check(px, pv, gs, qs, ctrl, meta["T"], steps, eps, which=[int(i) for i in rng.choice(G, 4, replace=False)])


def test_grouped_at_the_largest_m():
    """M = 2048 (the cap), D = 2: two groups on one posterior with their own start state and Q."""
    cfg = dict(synthetic.CONFIGS["c2"], D=2, M=2048, T=2048 + 64, S=1)
    params, Y, c, meta = synthetic.make_workload(**cfg)
    g0 = _posterior(params, c, meta, 0, perturb=False)
    rng = np.random.default_rng(22)
    gs = [g0, dict(g0, x_last=g0["x_last"] + 0.1 * rng.standard_normal(2), Q=g0["Q"] * 1.1)]
    steps, R = 4, 2
    ctrl = _ctrl(c, meta, steps)
    eps = rng.standard_normal((steps, 2, R, 2))
    qs = [g["H"] for g in gs]
    px, pv = _grouped(gs, qs, ctrl, meta["T"], steps, eps)
    _check(px, pv, gs, qs, ctrl, meta["T"], steps, eps)


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


def test_intent_batched_equals_intent():
    """Two identically built and seeded case-5 models: "intent" (one rollout call per sample) and "intent-batched" (one grouped
    call): the same sampler sequence (identical recorded variables), predict_x to the rollout tolerance."""
    params, Y, c, meta = synthetic.make_named("tiny", S=1)
    T, D = meta["T"], meta["D"]
    test_len, num, spacing = 6, 3, 2
    cc = np.concatenate((c, np.random.default_rng(5).standard_normal((test_len, meta["C"]))))
    eps = np.random.default_rng(9).standard_normal((test_len, num, D))
    outs = {}
    for mode in ("intent", "intent-batched"):
        mod = _case5_model(params, Y, cc, meta)
        mod.seed(42)
        outs[mode] = mod.collect_samples_formal(num, spacing, cc, test_len, sghmc_var_len=2, U_collapse=True, Y_train=Y, eps=eps,
                                                rollout_mode=mode)
    a, b = outs["intent"], outs["intent-batched"]
    assert set(a["mc_posterior_samples"]) == set(b["mc_posterior_samples"]) == {"logvariance", "loglengthscales"}
    for k in a["mc_posterior_samples"]:
        np.testing.assert_array_equal(a["mc_posterior_samples"][k], b["mc_posterior_samples"][k], err_msg=k)
    assert b["predict_x"].shape == (num, test_len, D)
    np.testing.assert_allclose(b["predict_x"], a["predict_x"], **ROLL)
    np.testing.assert_allclose(b["predict_x_var"], a["predict_x_var"], **ROLL_VAR)
    np.testing.assert_allclose(b["predict_y"], a["predict_y"], rtol=1e-8, atol=1e-9)


def test_collect_samples_chains():
    """A three-chain model: one posterior per chain, R rollouts each from the chain's own last state, against the oracle chain by
    chain; chain 0 against collect_samples_formal with the same noise."""
    params, Y, c, meta = synthetic.make_named("tiny", S=3)
    T, D, S = meta["T"], meta["D"], 3
    test_len, R = 6, 4
    cc = np.concatenate((c, np.random.default_rng(5).standard_normal((test_len, meta["C"]))))
    mod = _case5_model(params, Y, cc, meta, num_chains=S)
    mod.set_X(params["X"])
    eps = np.random.default_rng(10).standard_normal((test_len, S, R, D))
    out = mod.collect_samples_chains(R, cc, test_len, Y_train=Y, eps=eps)
    assert out["predict_x"].shape == out["predict_x_var"].shape == (S, R, test_len, D)
    assert out["predict_y"].shape == (test_len,) and np.all(out["predict_x_var"] > 0)
    okern = orc.make_kernels(params)
    Q = np.exp(params["log_Q"])
    Lo = orc.kernel_pre_cal(params["Z"], okern)
    for s in range(S):
        Xs = params["X"][s]
        Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, np.concatenate((Xs[:-1], cc[:T]), axis=1), Xs, params["Z"],
                                                                 okern, Q)
        po, vo = orc.rollout(Lo, params["Z"], okern, Uo, Ho, Xs[-1], cc, T, test_len, Q, eps[:, s])
        np.testing.assert_allclose(out["predict_x"][s], po, err_msg=f"chain {s}", **ROLL)
        np.testing.assert_allclose(out["predict_x_var"][s], vo, err_msg=f"chain {s}", **ROLL_VAR)
    one = mod.collect_samples_formal(R, 0, cc, test_len, U_collapse=True, Y_train=Y, eps=eps[:, 0])
    np.testing.assert_allclose(out["predict_x"][0], one["predict_x"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["predict_x_var"][0], one["predict_x_var"], rtol=1e-9, atol=1e-9)
    summary = orc.predict_y_summary(out["predict_x"].reshape(S * R, test_len, D), out["predict_x_var"].reshape(S * R, test_len, D),
                                    params["CC"], params["DD"], params["log_Rchols"])
    np.testing.assert_allclose(out["predict_y"], summary["predict_y"], rtol=1e-12, atol=1e-12)
