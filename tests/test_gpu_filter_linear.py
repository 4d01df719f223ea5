"""Linearised (extended Kalman) filtering and RTS smoothing on the device: method="linearised" of prediction.filter_grouped
(`ffvd_op_filter_linear_grouped`), of prediction.posterior_filter_grouped (`ffvd_op_posterior_filter_linear_grouped`) and
DGPSSM.filter_heldout_linearised.

The shapes, the seven cases, the observations with their gaps, the emissions and the helpers are those of
tests/test_gpu_filter_grouped.py and tests/test_gpu_moment_grouped.py, imported: M = 130 leaves 2 of 16 rows in the last slab
(Mp = 192), D = 8 fills the D x D products, per-model and q-slice cases give every group its own Gamma unit.  None of them passes 256
inducing points, where the kernel's column loop takes a second stride: `test_a_second_column_stride` adds M = 300.  `run_filter` of
the sibling calls prediction.filter_grouped without a method; `run_linear` hands it that function with the method bound.

Reference and rule.  filter_ref.filter with linear_filter_ref.ekf_transition in fp64 on the oracle's posterior, then filter_ref.smooth
(pinned in tests/test_linear_filter_ref.py).  e_ref is that reference against itself in np.longdouble; per array
error <= max(4 e_ref, floor), floors 1e-11 + 1e-9 max|ref| on means and 1e-11 + 1e-8 max|ref| on covariances and cross-covariances
(`rule` of tests/test_gpu_moment_grouped.py).  Densities and pooled arrays against NumPy on the device's own predicted stacks at
1e-9 (1 + max|ref|).  Every measured error is printed; DESIGN.md section 9, "Linearised filtering", has the largest."""
import functools
from unittest import mock

import numpy as np
import pytest

import filter_ref as fr
import linear_filter_ref as lf
import moment_ref as mr
import transition_grad_ref as tg
from ffvd_amd import prediction as pr, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_conditional_grouped import _group, floor
from test_gpu_filter_grouped import (CASES, COVS, KEYS, MOMENTS, NAN, emission, key_of, numpy_densities, observations, run_filter)
from test_gpu_moment_grouped import (MODES, N_TRAIN, S, STEPS, TEST_LEN, WIDE, _chains, _fused_args, _q, _regression_model, case, rule,
                                     start_cov)

pytestmark = pytest.mark.gpu


def run_linear(*args, method="linearised", **kw):
    """`run_filter` of tests/test_gpu_filter_grouped.py with `method` bound on the function it calls.
    Indirection to keep in mind: `run_filter` takes no method, and it works only because the sibling looks the function up as the
    attribute `pr.filter_grouped` of the module at call time (patched here for the duration of the call).  Should the sibling ever
    bind the function at import, the patch would do nothing and the run would be moment matching:
    `test_the_default_is_moment_matching_and_the_linearised_rule_differs_from_it` and the accuracy tests fail then."""
    with mock.patch.object(pr, "filter_grouped", functools.partial(pr.filter_grouped, method=method)):
        return run_filter(*args, **kw)


def _start(cs, with_S0):
    return start_cov(len(cs[0]), cs[2]["D"]) if with_S0 else None


def reference(gs, ctrl, Y, CC, DD, sd, qs, S0, mode):
    """Per array: the linearised restatement in fp64 stacked over the groups and its error against np.longdouble"""
    ref, e_ref = {k: [] for k in MOMENTS}, {k: 0.0 for k in MOMENTS}
    for i, g in enumerate(gs):
        res = {}
        for t in (np.float64, np.longdouble) if WIDE else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
            f = fr.filter(g["X"][-1], S0[i], Y, CC, DD, sd, g["Q"], lf.ekf_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t), dtype=t)
            f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=t)
            res[t] = f
        for k in MOMENTS:
            ref[k].append(res[np.float64][k])
            if WIDE:
                e_ref[k] = max(e_ref[k], float(np.max(np.abs(res[np.float64][k] - res[np.longdouble][k]))))
    return {k: np.stack(v) for k, v in ref.items()}, e_ref


@functools.lru_cache(maxsize=None)
def linear_refs(shape, per_model, G, qkind, mode, J, with_S0):
    """`reference` of a case on the oracle's posterior.  Computed once per case, shared by the tests, never modified."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(shape, per_model, G, qkind, mode, J, with_S0)
    CC, DD, _ = emission(cs, J)
    S0 = start_cov(len(gs), meta["D"]) if with_S0 else np.zeros((len(gs), meta["D"], meta["D"]))
    return reference(gs, call[meta["T"]: meta["T"] + STEPS], Y, CC, DD, sd, _q(cs, qkind), S0, mode)


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case, shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    Y, _ = observations(shape, per_model, G, qkind, mode, J, with_S0)
    return run_linear(cs, qkind, mode, Y, emission(cs, J), _start(cs, with_S0))


# ---- accuracy, exact symmetry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_moments_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Linearised filtering"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    ref, e_ref = linear_refs(*args)
    out = device(*args)
    assert set(out) == KEYS
    for k in MOMENTS:
        assert out[k].shape == ref[k].shape, k
        rule(f"linearised {shape} q={qkind} {mode} J={J}: {k}", key_of(k), out[k], ref[k], e_ref[k])
    for k in COVS:
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)
    np.testing.assert_array_equal(out["m_smooth"][:, -1], out["m_filt"][:, -1])
    np.testing.assert_array_equal(out["S_smooth"][:, -1], out["S_filt"][:, -1])
    low = min(float(np.min(np.linalg.eigvalsh(out[k]))) for k in COVS)
    print(f"linearised {shape}: smallest eigenvalue of the covariances {low:.3e}")
    assert low > 0.0


def test_a_second_column_stride():
    """M = 300: the kernel row and the quadratic form take a second stride of 256 columns (none of the shared shapes does), 19 slabs
    with 12 of 16 rows in the last one; two chains of one model, q slices, a start covariance, six rows with a gap."""
    params, _, c, meta = synthetic.make_named("tiny", M=300, T=320, S=2)
    gs = [_group(params, c, meta, params["X"][g]) for g in range(2)]
    T, D, n = meta["T"], meta["D"], 6
    call = np.concatenate((c, np.random.default_rng(3).standard_normal((n, meta["C"]))), axis=0)
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    sd = np.exp(np.asarray(lr)[0])
    Y = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(31).standard_normal((n, CC.shape[1]))
    Y[2] = NAN
    S0, qs = start_cov(2, D), [g["orc"]["H"] for g in gs]
    ref, e_ref = reference(gs, call[T: T + n], Y, CC, DD, sd, qs, S0, "intent")
    out = pr.filter_grouped(gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], qs, [g["X"][-1] for g in gs], call, T, Y,
                            [g["Q"] for g in gs], CC, DD, lr, S0s=S0, q_mode="intent", smooth=True, method="linearised")
    for k in MOMENTS:
        rule(f"linearised M=300: {k}", key_of(k), out[k], ref[k], e_ref[k])
    for k in COVS:
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)


# ---- densities and pooled arrays -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_densities_against_numpy_on_the_device_stacks(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out = case(shape, per_model, G), device(*args)
    (Y, sd), (CC, DD, _) = observations(*args), emission(cs, J)
    want, seen = numpy_densities(out, Y, CC, DD, sd), ~np.isnan(Y)
    n = out["m_pred"].shape[0]
    nan_at = dict(lpd=np.broadcast_to(~seen, (n,) + seen.shape), lpd_joint=np.broadcast_to(~seen.any(axis=1), (n, Y.shape[0])),
                  lpd_mix=~seen, lpd_gauss=~seen, predict_y=np.zeros_like(seen), predict_y_var_total=np.zeros_like(seen))
    assert set(want) == {"lpd", "lpd_joint", "predict_y", "predict_y_var_total", "lpd_mix", "lpd_gauss"}
    for k, w in want.items():
        got = out[k]
        assert got.shape == w.shape, k
        np.testing.assert_array_equal(np.isnan(got), nan_at[k], err_msg=k)
        ok = ~nan_at[k]
        tol = 1e-9 * (1.0 + float(np.max(np.abs(w[ok]))))
        err = float(np.max(np.abs(got[ok] - w[ok])))
        print(f"linearised {shape} J={J}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    assert out["ll"] == pytest.approx(float(np.mean(want["lpd_mix"][seen])), abs=1e-9 * (1.0 + np.max(np.abs(want["lpd_mix"][seen]))))


# ---- the first step from a point is the conditional ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [c for c in CASES if not c[6]], ids=str)
def test_first_step_from_a_point_is_the_conditional(shape, per_model, G, qkind, mode, J, with_S0):
    """S0 = None: m_pred[:, 0] - x0 and diag(S_pred[:, 0]) - Q against `mean` and `var` of conditional_grad_grouped at [x0, c_0], by
    the project's rule: difference <= max(4 e_ref, floor) with the floors 1e-11 + 1e-9 max|mean| and 1e-11 + 1e-8 max|var| of the
    conditional's own values, and e_ref the error of the fp64 restatement of that conditional (transition_grad_ref.linearize on the
    oracle's posterior at the same rows) against itself in np.longdouble, never anything measured on the device.  The off-diagonal
    of S_pred[:, 0] and cross[:, 0] are exact zeros.
    Measured on one MI355X: mean at most 6.2e-15; var 2.3e-14 (tiny), 2.4e-14 (ragged), 2.9e-13 (small), 5.6e-16 (d8), all below
    their floors (5e-10 .. 4e-9), and 1.3e-10 at m130, where the floor is 1.0e-11 and e_ref 7.4e-11 (bound 3.0e-10): the variance
    at a training point is 3e-7 = 1 - 0.9999997 with Gamma entries near 1e5, and the two device paths add the same products in
    different orders (128 x 128 MFMA tiles there, slabs of 16 rows here)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out = case(shape, per_model, G), device(*args)
    gs, call, meta = cs[0], cs[1], cs[2]
    D, qs = meta["D"], _q(cs, qkind)
    xc = np.stack([np.concatenate((g["X"][-1], call[meta["T"]])) for g in gs])                  # row g: [x0 of group g, c_0]
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g["orc"]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0]["orc"]["L"]
    lin = cmo.conditional_grad_grouped(Ls, Zs, kerns, [g["orc"]["U"] for g in gs], qs, xc, q_mode=mode, summary=False)
    idx = np.arange(len(gs))
    mean, var = lin["mean"][idx, idx], lin["var"][idx, idx]                                     # (G, D): group g at its own row
    got_m = out["m_pred"][:, 0] - np.stack([g["X"][-1] for g in gs])
    got_v = np.diagonal(out["S_pred"][:, 0], axis1=-2, axis2=-1) - np.stack([g["Q"] for g in gs])
    e_m = e_v = 0.0
    if WIDE:                                                      # the reference's own error at these rows, per group
        for i, g in enumerate(gs):
            r = {}
            for t in (np.float64, np.longdouble):
                beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
                r[t] = tg.linearize(xc[i:i + 1], g["Z"], g["okern"], beta, Gam, dtype=t)
            e_m = max(e_m, float(np.max(np.abs(r[np.float64][0] - r[np.longdouble][0]))))
            e_v = max(e_v, float(np.max(np.abs(r[np.float64][1] - r[np.longdouble][1]))))
    rule(f"linearised {shape}: first step against conditional_grad_grouped", "mean", got_m, mean, e_m)
    rule(f"linearised {shape}: first step against conditional_grad_grouped", "var", got_v, var, e_v)
    off = out["S_pred"][:, 0] * (1.0 - np.eye(D))
    np.testing.assert_array_equal(off, np.zeros_like(off))
    np.testing.assert_array_equal(out["cross"][:, 0], np.zeros_like(off))


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_two_calls_a_group_alone_and_a_shuffled_order_are_equal(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a = case(shape, per_model, G), device(*args)
    Y, em, S0 = observations(*args)[0], emission(cs, J), _start(cs, with_S0)
    b = run_linear(cs, qkind, mode, Y, em, S0)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    per_group = MOMENTS + ("lpd", "lpd_joint")
    for g in range(len(cs[0])):
        one = run_linear(cs, qkind, mode, Y, em, S0, groups=[g])
        for k in per_group:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k} group {g}")
    order = list(np.random.default_rng(3).permutation(len(cs[0])))
    if order == sorted(order):
        order = order[::-1]
    mixed = run_linear(cs, qkind, mode, Y, em, S0, groups=[int(g) for g in order])
    for k in per_group:
        for i, g in enumerate(order):
            np.testing.assert_array_equal(mixed[k][i], a[k][g], err_msg=f"{k} group {g} at place {i}")


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
def test_the_default_is_moment_matching_and_the_linearised_rule_differs_from_it():
    args = CASES[1]                                               # tiny, one model per group, dense q, J = 3, a start covariance
    cs = case(*args[:3])
    Y, em, S0 = observations(*args)[0], emission(cs, args[5]), _start(cs, True)
    default, moment = run_filter(cs, args[3], args[4], Y, em, S0), run_linear(cs, args[3], args[4], Y, em, S0, method="moment")
    for k in KEYS:
        np.testing.assert_array_equal(default[k], moment[k], err_msg=k)
    lin, (ref, _) = device(*args), linear_refs(*args)
    diff, fl = float(np.max(np.abs(lin["m_filt"] - moment["m_filt"]))), floor("mean", ref["m_filt"])
    print(f"largest |m_filt(linearised) - m_filt(moment)| {diff:.3e}, accuracy floor {fl:.3e}")
    assert diff > fl


def test_without_observations_and_without_steps():
    """trailing and whole all-NaN records are the propagation-only use: filtered = predicted bit for bit, NaN densities"""
    cs = case("tiny")
    em = emission(cs, 3)
    out = run_linear(cs, "upper", "reference", np.full((4, 3), NAN), em, start_cov(3, 2))
    np.testing.assert_array_equal(out["m_filt"], out["m_pred"])
    np.testing.assert_array_equal(out["S_filt"], out["S_pred"])
    assert np.all(np.isnan(out["lpd"])) and np.all(np.isnan(out["lpd_joint"])) and np.all(np.isnan(out["lpd_mix"]))
    assert all(np.all(np.isfinite(out[k])) for k in MOMENTS)
    none = run_linear(cs, "upper", "reference", np.zeros((0, 3)), em)
    assert none["m_pred"].shape == none["m_smooth"].shape == (3, 0, 2) and none["S_filt"].shape == none["cross"].shape == (3, 0, 2, 2)


# ---- fused with the posteriors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J, mode):
    """posterior_filter_grouped(method="linearised") against collapse_u_mean_grouped followed by filter_grouped(method="linearised"),
    as tests/test_gpu_filter_grouped.py::test_fused_form_against_the_two_calls: the reference is the restatement on the device's own
    posterior (np.longdouble where that is wider), the yardstick the two-call route.  Whether the bits coincide is printed."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])          # (data only: any posterior's will do)
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    fused = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode, smooth=True, method="linearised")
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, meta["T"], Y, Qs, CC, DD, lr, q_mode=mode,
                            smooth=True, method="linearised")
    assert set(fused) == KEYS
    print(f"linearised {shape} {mode}: fused and two-call routes bit-identical: "
          f"{all(np.array_equal(fused[k], two[k], equal_nan=True) for k in KEYS)}")
    t = np.longdouble if WIDE else np.float64
    ctrl = call[meta["T"]: meta["T"] + STEPS]
    for i, g in enumerate(gs):
        beta, Gam = mr.posterior_terms(Lm[i if per_model else 0], U[i], Hinv[i], mode, dtype=t)
        f = fr.filter(g["X"][-1], np.zeros((meta["D"],) * 2), Y, CC, DD, sd, g["Q"], lf.ekf_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t),
                      dtype=t)
        f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=t)
        for k in MOMENTS:
            ref = f[k].astype(np.float64)
            e_f, e_t = float(np.max(np.abs(fused[k][i] - ref))), float(np.max(np.abs(two[k][i] - ref)))
            bound = max(4.0 * e_t, floor(key_of(k), ref))
            print(f"linearised {shape} {mode} group {i}: {k}: fused {e_f:.3e}, two calls {e_t:.3e}, bound {bound:.3e}")
            assert np.all(np.isfinite(fused[k][i])) and e_f <= bound, k
    for k in COVS:
        np.testing.assert_array_equal(fused[k], np.swapaxes(fused[k], -1, -2), err_msg=k)
    again = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode, smooth=True, method="linearised")
    for k in KEYS:
        np.testing.assert_array_equal(again[k], fused[k], err_msg=k)


# ---- model level: the actuator fixture with three chains -----------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_heldout_linearised(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = np.array(Y[N_TRAIN:N_TRAIN + TEST_LEN])
    Yt[7] = NAN
    Yt[-5:] = NAN
    out = mod.filter_heldout_linearised(Yt, c, smooth=True, Y_train_std=1.7)
    assert set(out) == KEYS and all(np.all(np.isfinite(out[k])) for k in MOMENTS)
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        direct = pr.posterior_filter_grouped(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, c, N_TRAIN, Yt, lik.CC, lik.DD,
                                             lik.log_Rchols, smooth=True, Y_train_std=1.7, method="linearised")
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        direct = pr.filter_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [mod._X_chains[s][-1] for s in range(S)], c, N_TRAIN, Yt, mod.Q,
                                   lik.CC, lik.DD, lik.log_Rchols, smooth=True, Y_train_std=1.7, method="linearised")
    for k in KEYS:
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
    mm = mod.filter_heldout(Yt, c, smooth=True, Y_train_std=1.7)
    assert float(np.max(np.abs(mm["m_filt"] - out["m_filt"]))) > 0.0
    print(f"U_collapse={U_collapse}: one step ahead, linearised: ll {out['ll']:.6f}, ll_joint {out['ll_joint']:.6f}, RMSE {out['RMSE']:.6f}; "
          f"moment matching: ll {mm['ll']:.6f}, ll_joint {mm['ll_joint']:.6f}, RMSE {mm['RMSE']:.6f}")
