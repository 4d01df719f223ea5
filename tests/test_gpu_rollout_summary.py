"""Rollout summaries on the device (`ffvd_op_rollout_summary`, prediction.rollout_summary) and their fusion with the grouped
rollouts (`ffvd_op_rollout_grouped_summary`, `ffvd_op_posterior_rollout_grouped_summary`), through DGPSSM and Model.fit as well
(collect_samples_chains(summary="device"), evaluate_heldout, fit(eval_every=k)).

Decomposition under test (predict_summary.h): a wavefront owns a chunk of PS_CHUNK = 32 rollouts and a tile of PS_TILE = 64 steps;
the chunks are merged in ascending order by a second launch.  The shapes below sit at 1 and 2 rollouts, one below / at / one above
the chunk (31, 32, 33) and two chunks plus 3 (67); at 1 and 7 steps and one above the tile (65).

Reference: an fp64 NumPy restatement (`reference` below: scipy's logsumexp for lpd, `var(axis=0)` for the spread); for J = 1 also
oracle.predict_y_summary.  Tolerances ("Parity"): y_mean, y_var 1e-11 + 1e-9 max|ref|; y_var_total
1e-11 + 1e-9 max(s^2 + mean_n p^2); lpd, lpd_gauss 1e-9 (1 + max|ref|).  Every measured error is printed before it is asserted."""
import functools

import numpy as np
import pytest
from scipy.special import logsumexp

from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import synthetic
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import (posterior_rollout_grouped, posterior_rollout_grouped_summary, rollout_grouped, rollout_grouped_summary,
                                 rollout_summary)
from oracle import ffvd_oracle as orc

pytestmark = pytest.mark.gpu

PS_CHUNK, PS_TILE = 32, 64
ARRAYS = ("predict_y", "predict_y_var", "predict_y_var_total", "lpd", "lpd_gauss")
LOG_2PI = np.log(2.0 * np.pi)


def reference(px, pv, CC, DD, log_Rchols, Y=None):
    """The quantities of the issue in plain NumPy, fp64; returns the arrays and the absolute tolerance of each."""
    D = px.shape[-1]
    px, pv = px.reshape(-1, px.shape[-2], D), pv.reshape(-1, px.shape[-2], D)
    N, steps, J = px.shape[0], px.shape[1], CC.shape[1]
    lr = np.asarray(log_Rchols, dtype=np.float64)
    s = np.exp(lr[0] if lr.ndim == 2 else lr.reshape(J))                 # row 0: the row the likelihood uses
    p = np.einsum("ntk,kj->ntj", px, CC)
    ref = {"predict_y": p.mean(axis=0) + DD, "predict_y_var": np.einsum("ntk,kj->ntj", pv, CC ** 2).mean(axis=0) + s ** 2,
           "predict_y_var_total": s ** 2 + p.var(axis=0)}
    tol = {"predict_y": 1e-11 + 1e-9 * np.max(np.abs(ref["predict_y"])),
           "predict_y_var": 1e-11 + 1e-9 * np.max(np.abs(ref["predict_y_var"])),
           "predict_y_var_total": 1e-11 + 1e-9 * np.max(s ** 2 + np.mean(p ** 2, axis=0))}
    if Y is not None:
        nt = Y.shape[0]
        e = -0.5 * ((Y[None] - p[:, :nt] - DD) / s) ** 2
        ref["lpd"] = logsumexp(e, axis=0) - np.log(N) - np.log(s) - 0.5 * LOG_2PI
        vt, ym = ref["predict_y_var_total"][:nt], ref["predict_y"][:nt]
        ref["lpd_gauss"] = -0.5 * (LOG_2PI + np.log(vt)) - 0.5 * (Y - ym) ** 2 / vt
        for k in ("lpd", "lpd_gauss"):
            tol[k] = 1e-9 * (1.0 + (np.max(np.abs(ref[k])) if nt else 0.0))
    return ref, tol


def check(what, out, px, pv, CC, DD, lr, Y):
    ref, tol = reference(px, pv, CC, DD, lr, Y)
    steps, J = px.shape[-2], CC.shape[1]
    assert set(out) == set(ref) | ({"RMSE", "ll", "ll_original_units"} if Y is not None else set()), sorted(out)
    for k in ARRAYS:
        if k not in ref:
            continue
        got = out[k].reshape(ref[k].shape)                      # (predict_y* come flattened; every entry is compared)
        assert got.size == ref[k].size and np.all(np.isfinite(got)), f"{what}: {k}"
        err = float(np.max(np.abs(got - ref[k]))) if got.size else 0.0
        print(f"{what}: {k}: max error {err:.3e}, tolerance {tol[k]:.3e}")
        assert err <= tol[k], f"{what}: {k}: {err:.3e} > {tol[k]:.3e}"
    if Y is not None and Y.shape[0]:
        assert out["ll"] == pytest.approx(float(np.mean(ref["lpd"])), abs=tol["lpd"])
    return ref


def _emission(rng, D, J):
    return rng.standard_normal((D, J)), rng.standard_normal(J), np.log(0.2 + 0.3 * rng.random((J, J)))


# ---- 1. the standalone operator on random stacks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 7, PS_TILE + 1])
@pytest.mark.parametrize("N", [1, 2, PS_CHUNK - 1, PS_CHUNK, PS_CHUNK + 1, 2 * PS_CHUNK + 3])
def test_standalone_summary_against_numpy(N, steps):
    for D in (1, 3, 4, 16):
        rng = np.random.default_rng(1000 * N + 10 * steps + D)
        px = 2.0 + rng.standard_normal((N, steps, D))           # a mean of 2: E[p^2] - E[p]^2 would cancel
        pv = 0.05 + 0.1 * rng.random((N, steps, D))
        for J in (1, 3):
            CC, DD, lr = _emission(rng, D, J)
            for n_test in sorted({0, 1, steps}):
                Y = 2.0 * rng.standard_normal((n_test, J))
                out = rollout_summary(px, pv, CC, DD, lr, Y, 1.7)
                ref = check(f"N={N} steps={steps} D={D} J={J} n_test={n_test}", out, px, pv, CC, DD, lr, Y)
                if J == 1:
                    o = orc.predict_y_summary(px, pv, CC, DD, lr.reshape(-1), Y if n_test == steps else None, 1.7)
                    np.testing.assert_allclose(out["predict_y"], o["predict_y"], rtol=0, atol=1e-11 + 1e-9 * np.max(np.abs(o["predict_y"])))
                    np.testing.assert_allclose(out["predict_y_var"], o["predict_y_var"], rtol=0,
                                               atol=1e-11 + 1e-9 * np.max(np.abs(o["predict_y_var"])))
                    if n_test == steps:
                        assert out["RMSE"] == pytest.approx(o["RMSE"], abs=1.7 * (1e-11 + 1e-9 * np.max(np.abs(o["predict_y"]))))
                if n_test:
                    assert out["ll_original_units"] == out["ll"] - np.log(1.7)
            none = rollout_summary(px, pv, CC, DD, lr)
            assert set(none) == {"predict_y", "predict_y_var", "predict_y_var_total"}
            for k in none:
                np.testing.assert_array_equal(none[k], out[k], err_msg=k)      # the moments do not depend on the held-out data


def test_four_axis_stacks_are_the_flattened_ones():
    rng = np.random.default_rng(3)
    px, pv = rng.standard_normal((3, 12, 7, 4)), 0.1 + rng.random((3, 12, 7, 4))
    CC, DD, lr = _emission(rng, 4, 3)
    Y = rng.standard_normal((5, 3))
    a, b = rollout_summary(px, pv, CC, DD, lr, Y), rollout_summary(px.reshape(36, 7, 4), pv.reshape(36, 7, 4), CC, DD, lr, Y)
    for k in ARRAYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    check("four axes", a, px, pv, CC, DD, lr, Y)


# ---- 2. every component at least 40 noise standard deviations away ------------------------------------------------------------------
def test_density_of_a_far_point_is_finite():
    """Y_test = max_n(p + DD) + 40 s_j: every exponent is below -800 and exp(-800) = 0 in fp64 -- an unshifted sum gives -inf."""
    rng = np.random.default_rng(5)
    N, steps, D, J = 2 * PS_CHUNK + 3, 7, 3, 3
    px, pv = 2.0 + rng.standard_normal((N, steps, D)), 0.05 + 0.1 * rng.random((N, steps, D))
    CC, DD, lr = _emission(rng, D, J)
    s = np.exp(lr[0])
    Y = np.max(np.einsum("ntk,kj->ntj", px, CC), axis=0) + DD + 40.0 * s
    assert np.all(-0.5 * ((Y[None] - np.einsum("ntk,kj->ntj", px, CC) - DD) / s) ** 2 <= -799.999)
    with np.errstate(divide="ignore"):
        naive = np.log(np.mean(np.exp(-0.5 * ((Y[None] - np.einsum("ntk,kj->ntj", px, CC) - DD) / s) ** 2), axis=0))
    assert np.all(np.isneginf(naive))
    out = rollout_summary(px, pv, CC, DD, lr, Y)
    assert out["lpd"].shape == (steps, J) and np.all(np.isfinite(out["lpd"])) and np.all(out["lpd"] < -790.0)
    check("far point", out, px, pv, CC, DD, lr, Y)


# ---- 3. the fused calls against the standalone operator -----------------------------------------------------------------------------
SHAPES = {"tiny": ("tiny", {}, False), "small M=64, a model per group": ("small", dict(M=64, S=3), True),
          "tiny, no control inputs": ("tiny", dict(C=0), False), "tiny, no control inputs, a model per group": ("tiny", dict(C=0), True),
          "LinearK": ("small_lin", dict(S=2), False)}


def _kernels(p, meta):
    D, P = meta["D"], meta["P"]
    if meta["kernel_type"] == "LinearK":
        return [LinearK(P, variance=np.exp(p["logvariance"][d])) for d in range(D)]
    return [SquaredExponential(P, variance=np.exp(p["logvariance"][d]), lengthscales=np.exp(p["loglengthscales"][d])) for d in range(D)]


@functools.lru_cache(maxsize=None)
def case(shape):
    """G groups: the workload's chains under one model, or each under a seeded perturbation of it (as test_gpu_posterior_grouped);
    with each group the posterior of the composed device path, for the calls that take posteriors."""
    name, ov, per_model = SHAPES[shape]
    params, _, c, meta = synthetic.make_named(name, **ov)
    T, gs = meta["T"], []
    for g in range(meta["S"]):
        q, X = dict(params), params["X"][g]
        if per_model:
            rng = np.random.default_rng(1000 + g)
            q["logvariance"] = params["logvariance"] + 0.05 * rng.standard_normal(params["logvariance"].shape)
            q["loglengthscales"] = params["loglengthscales"] + 0.05 * rng.standard_normal(params["loglengthscales"].shape)
            q["Z"] = params["Z"] + 0.01 * rng.standard_normal(params["Z"].shape)
            q["log_Q"] = params["log_Q"] + 0.05 * rng.standard_normal(params["log_Q"].shape)
            X = X + 0.1 * rng.standard_normal(X.shape)
        kern, Q = _kernels(q, meta), np.exp(q["log_Q"])
        L = cmo.kernel_pre_cal(q["Z"], kern)
        U, H = cmo.collapse_u_mean_after_kernel_precalculation(L, np.concatenate((X[:T], c[:T]), axis=1), X, q["Z"], kern, Q)
        gs.append(dict(Z=q["Z"], kern=kern, X=X, Q=Q, L=L, U=U, H=H))
    return gs, c, meta, per_model


def _equal(what, a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    for k in ("ll", "ll_original_units", "RMSE"):
        assert a[k] == b[k], f"{what}: {k}"


@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fused_summaries_are_the_standalone_summary_of_their_own_stacks(shape, J):
    gs, c, meta, per_model = case(shape)
    G, D, T, C, R, steps, nt = len(gs), meta["D"], meta["T"], meta["C"], 12, 6, 4          # G * R = 24 or 36: below / above a chunk
    rng = np.random.default_rng(17)
    ctrl = np.concatenate((c, rng.standard_normal((steps, C))))
    eps = rng.standard_normal((steps, G, R, D))
    CC, DD, lr = _emission(rng, D, J)
    Y = rng.standard_normal((nt, J))
    em = (CC, DD, lr, Y, 1.3)
    both = ARRAYS + ("predict_x", "predict_x_var")
    # posteriors formed in the call
    model = ([g["Z"] for g in gs], [g["kern"] for g in gs]) if per_model else (gs[0]["Z"], gs[0]["kern"])
    head = model + ([g["X"] for g in gs], [g["Q"] for g in gs], ctrl, T, steps, eps)
    a = posterior_rollout_grouped_summary(*head, *em, return_rollouts=True)
    px, pv = posterior_rollout_grouped(*head)
    np.testing.assert_array_equal(a["predict_x"], px)
    np.testing.assert_array_equal(a["predict_x_var"], pv)
    assert a["predict_x"].shape == (G, R, steps, D) and np.all(np.isfinite(px)) and np.all(pv > 0)
    _equal(f"{shape}: fused against standalone", a, rollout_summary(px, pv, *em), ARRAYS)
    b = posterior_rollout_grouped_summary(*head, *em)
    assert "predict_x" not in b and "predict_x_var" not in b
    _equal(f"{shape}: fused, nothing downloaded", b, a, ARRAYS)
    _equal(f"{shape}: fused, second call", posterior_rollout_grouped_summary(*head, *em, return_rollouts=True), a, both)
    check(f"{shape} J={J}: fused", b, px, pv, CC, DD, lr, Y)
    # posteriors handed over
    head = ([g["L"] for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs], [g["U"] for g in gs], [g["H"] for g in gs],
            [g["X"][-1] for g in gs], ctrl, T, steps, [g["Q"] for g in gs], eps)
    a = rollout_grouped_summary(*head, *em, return_rollouts=True)
    px, pv = rollout_grouped(*head)
    np.testing.assert_array_equal(a["predict_x"], px)
    np.testing.assert_array_equal(a["predict_x_var"], pv)
    _equal(f"{shape}: grouped against standalone", a, rollout_summary(px, pv, *em), ARRAYS)
    b = rollout_grouped_summary(*head, *em)
    assert "predict_x" not in b
    _equal(f"{shape}: grouped, nothing downloaded", b, a, ARRAYS)
    _equal(f"{shape}: grouped, second call", rollout_grouped_summary(*head, *em, return_rollouts=True), a, both)
    check(f"{shape} J={J}: grouped", b, px, pv, CC, DD, lr, Y)


# ---- 4. model level: the actuator fixture with S = 3 chains ----------------------------------------------------------------------------
N_TRAIN, TEST_LEN, S = 400, 40, 3


def _regression_model(params, c, U_collapse=True):
    from ffvd_amd.models import RegressionModel
    m = RegressionModel("normal")
    A = m.ARGS
    A.CC, A.DD = params["CC"], params["DD"]
    A.QQ_chol, A.RR_chol = np.exp(0.5 * params["log_Q"]), np.exp(params["log_Rchols"])
    A.lengthscales, A.variance = np.exp(params["loglengthscales"]), np.exp(params["logvariance"])
    A.UU_ini, A.XX_0_ini, A.x_initialization = params["U"], params["X"][0], params["X"][1:N_TRAIN + 1]
    A.control_inputs, A.num_inducing, A.x_dims, A.ZZ = c, 100, [4], params["Z"]
    A.U_collapse, A.kernel_optimization, A.case_val = U_collapse, True, 4 if U_collapse else 1
    if not U_collapse:
        A.U_optimization, A.Z_optimization = True, True
    return m


def _chains(params):
    X = params["X"][:N_TRAIN + 1]
    return np.stack([X + 0.05 * np.random.default_rng(40 + s).standard_normal(X.shape) * (s > 0) for s in range(S)])


@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_device_summary_of_the_chains_against_the_host_summary(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    R, D = 12, 4
    eps = np.random.default_rng(11).standard_normal((TEST_LEN, S, R, D))
    Yt = Y[N_TRAIN:N_TRAIN + TEST_LEN]
    kw = dict(Y_test=Yt, Y_train_std=1.7, Y_train=Y[:N_TRAIN], eps=eps)
    for fused in ((False, True) if U_collapse else (False,)):
        host = mod.collect_samples_chains(R, c, TEST_LEN, fused=fused, **kw)
        dev = mod.collect_samples_chains(R, c, TEST_LEN, fused=fused, summary="device", **kw)
        assert set(host) < set(dev) and set(dev) - set(host) == {"predict_y_var_total", "lpd", "lpd_gauss", "ll", "ll_original_units"}
        np.testing.assert_array_equal(dev["predict_x"], host["predict_x"])
        np.testing.assert_array_equal(dev["predict_x_var"], host["predict_x_var"])
        for k in ("predict_y", "predict_y_var"):
            err, tol = np.max(np.abs(dev[k] - host[k])), 1e-11 + 1e-9 * np.max(np.abs(host[k]))
            print(f"fused={fused}: {k}: device against host {err:.3e}, tolerance {tol:.3e}")
            assert dev[k].shape == host[k].shape and err <= tol
        assert dev["RMSE"] == pytest.approx(host["RMSE"], abs=1.7 * (1e-11 + 1e-9 * np.max(np.abs(host["predict_y"]))))
        lik = mod.likelihood
        check(f"chains fused={fused}", {k: v for k, v in dev.items() if k not in ("predict_x", "predict_x_var", "U_vals")},
              dev["predict_x"], dev["predict_x_var"], lik.CC, lik.DD, lik.log_Rchols, Yt)
        assert np.all(dev["predict_y_var_total"] > np.exp(2 * lik.log_Rchols[0, 0]))
    ev = mod.evaluate_heldout(Yt, c, R, Y_train_std=1.7, eps=eps)
    assert "predict_x" not in ev and "predict_x_var" not in ev
    _equal("evaluate_heldout against the device summary of the same call", ev, dev, ARRAYS)
    assert np.isfinite(ev["ll"]) and np.isfinite(ev["RMSE"])


def test_fit_records_held_out_metrics(actuator):
    params, Y, c = actuator
    Yt = Y[N_TRAIN:N_TRAIN + TEST_LEN]
    runs = {}
    for name, kw in (("plain", {}), ("eval_every=0", dict(Y_test=Yt, eval_every=0)), ("eval_every=1", dict(Y_test=Yt, eval_every=1, Ystd=1.7))):
        m = _regression_model(params, c)
        m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=2, route="gram", grad=True, num_chains=S, **kw)
        runs[name] = m
    for name in ("plain", "eval_every=0"):
        assert runs[name].rmse_seq == [] and runs[name].ll_seq == []
    np.testing.assert_array_equal(np.asarray(runs["eval_every=0"].nll_seq), np.asarray(runs["plain"].nll_seq))
    m = runs["eval_every=1"]
    assert len(m.rmse_seq) == 2 and len(m.ll_seq) == 2 and np.all(np.isfinite(m.rmse_seq)) and np.all(np.isfinite(m.ll_seq))
    np.testing.assert_array_equal(np.asarray(m.nll_seq), np.asarray(runs["plain"].nll_seq))     # evaluating does not disturb training
    print("held-out RMSE per round", m.rmse_seq, "log predictive density per round", m.ll_seq)
