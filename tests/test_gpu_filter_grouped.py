"""Gaussian filtering and RTS smoothing on the device: `ffvd_op_filter_grouped` (prediction.filter_grouped), fused with the collapsed
posteriors (`ffvd_op_posterior_filter_grouped`, prediction.posterior_filter_grouped) and DGPSSM.filter_heldout.

Reference and rule.  The reference is tests/filter_ref.py in fp64 (pinned in tests/test_filter_ref.py; its update is the joint form,
the device runs scalar updates), on the oracle's posterior.  Its own error e_ref is measured against the same restatement in
np.longdouble, never on the device; the device must satisfy, per array,  error <= max(4 e_ref, floor)  with the floors
1e-11 + 1e-9 max|ref| on means and 1e-11 + 1e-8 max|ref| on covariances and cross-covariances; where np.longdouble is no wider the
floor alone applies (tests/test_gpu_moment_grouped.py: its shapes, cases and helpers are imported).  Densities are compared with NumPy
on the device's own predicted stacks, tolerance 1e-9 (1 + max|ref|).  Every measured error is printed.

Observations: the no-observation propagation's predicted mean through the emission (mean over the groups) plus half a predictive
standard deviation of seeded noise; row 3 is missing, the last three rows are missing, and for J = 3 row 5 lacks one entry and row
6 has one entry only.  J = 1 is the fixture's emission, J = 3 a seeded CC, DD with sd = (0.4, 0.05, 1.3)."""
import functools

import numpy as np
import pytest

import filter_ref as fr
import moment_ref as mr
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_conditional_grouped import floor
from test_gpu_moment_grouped import (MODES, N_TRAIN, S, STEPS, TEST_LEN, WIDE, _chains, _fused_args, _q, _regression_model, case, refs, rule,
                                     run_explicit, start_cov)

pytestmark = pytest.mark.gpu

NAN = np.nan
MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "m_smooth", "S_smooth")
COVS = ("S_pred", "S_filt", "S_smooth")
POOLED = ("predict_y", "predict_y_var_total", "lpd_mix", "lpd_gauss")
KEYS = set(MOMENTS) | {"lpd", "lpd_joint", "ll", "ll_joint", "ll_original_units", "RMSE"} | set(POOLED)
# shape, per_model, G, q_sqrt, q_mode, J, start covariance
CASES = [("tiny", False, None, "upper", "reference", 1, False), ("tiny", True, 3, "dense", "intent", 3, True),
         ("ragged", False, None, "upper", "intent", 3, False), ("small", True, 3, "upper", "reference", 1, False),
         ("m130", False, 3, "none", "reference", 1, False), ("d8", False, 1, "dense", "reference", 3, False),
         ("tiny", False, 1, "none", "intent", 3, True)]


def key_of(k):
    return "mean" if k.startswith("m_") else "var"


def emission(cs, J):
    """J = 1: the fixture's; J = 3: seeded, sd = (0.4, 0.05, 1.3).  Returns CC (D, J), DD (J,), log_Rchols as the model holds it."""
    params, D = cs[4], cs[2]["D"]
    if J == 1:
        return params["CC"], params["DD"], params["log_Rchols"]
    rng = np.random.default_rng(17)
    return rng.standard_normal((D, J)), rng.standard_normal(J), np.log(np.asarray((0.4, 0.05, 1.3)))


def gaps(Y):
    Y = np.array(Y)
    Y[3, :] = NAN
    Y[-3:, :] = NAN
    if Y.shape[1] > 1:
        Y[5, 1] = NAN
        Y[6, :2] = NAN
    return Y


@functools.lru_cache(maxsize=None)
def observations(shape, per_model, G, qkind, mode, J, with_S0):
    """Y_obs (STEPS, J) with its gaps, from the reference's propagation without observations (shared with the moment tests)."""
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, qkind, mode, STEPS, with_S0)
    CC, DD, lr = emission(cs, J)
    sd = np.exp(np.asarray(lr).reshape(-1)[:J]) if J > 1 else np.exp(np.asarray(lr)[0])
    m = np.mean(np.einsum("gtk,kj->gtj", r["m"], CC) + DD, axis=0)
    s2 = np.mean(np.einsum("kj,gtkl,lj->gtj", CC, r["S"], CC) + sd ** 2, axis=0)
    return gaps(m + 0.5 * np.sqrt(s2) * np.random.default_rng(29).standard_normal(m.shape)), sd


@functools.lru_cache(maxsize=None)
def filter_refs(shape, per_model, G, qkind, mode, J, with_S0):
    """Per array: the restatement in fp64 stacked over the groups (`ref`) and its error against np.longdouble (`e_ref`).  Computed
    once per case, shared by the tests, never modified."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(shape, per_model, G, qkind, mode, J, with_S0)
    CC, DD, _ = emission(cs, J)
    qs, S0 = _q(cs, qkind), start_cov(len(gs), meta["D"]) if with_S0 else np.zeros((len(gs), meta["D"], meta["D"]))
    ctrl = call[meta["T"]: meta["T"] + STEPS]
    ref, e_ref = {k: [] for k in MOMENTS}, {k: 0.0 for k in MOMENTS}
    for i, g in enumerate(gs):
        res = {}
        for t in (np.float64, np.longdouble) if WIDE else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
            f = fr.filter(g["X"][-1], S0[i], Y, CC, DD, sd, g["Q"], fr.gp_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t), dtype=t)
            f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=t)
            res[t] = f
        for k in MOMENTS:
            ref[k].append(res[np.float64][k])
            if WIDE:
                e_ref[k] = max(e_ref[k], float(np.max(np.abs(res[np.float64][k] - res[np.longdouble][k]))))
    return {k: np.stack(v) for k, v in ref.items()}, e_ref


def run_filter(cs, qkind, mode, Y, em, S0=None, smooth=True, groups=None, src="orc"):
    gs, call, meta, per_model = cs[0], cs[1], cs[2], cs[3]
    idx = list(range(len(gs))) if groups is None else groups
    sel, qs = [gs[i] for i in idx], _q(cs, qkind, src)
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in sel], [g["kern"] for g in sel], [g[src]["L"] for g in sel]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    return pr.filter_grouped(Ls, Zs, kerns, [g[src]["U"] for g in sel], None if qs is None else [qs[i] for i in idx],
                             [g["X"][-1] for g in sel], call, meta["T"], Y, [g["Q"] for g in sel], *em,
                             S0s=None if S0 is None else S0[idx], q_mode=mode, smooth=smooth)


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case, shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    Y, _ = observations(shape, per_model, G, qkind, mode, J, with_S0)
    S0 = start_cov(len(cs[0]), cs[2]["D"]) if with_S0 else None
    return run_filter(cs, qkind, mode, Y, emission(cs, J), S0)


def numpy_densities(out, Y, CC, DD, sd):
    """lpd, lpd_joint (by the joint form) and the pooled one-step summary, from the device's own predicted stacks"""
    mp, Sp = out["m_pred"], out["S_pred"]
    G, n, J = mp.shape[0], Y.shape[0], Y.shape[1]
    ym = np.einsum("gtk,kj->gtj", mp, CC) + DD
    yv = np.einsum("kj,gtkl,lj->gtj", CC, Sp, CC) + sd ** 2
    lpd = -0.5 * (np.log(2 * np.pi) + np.log(yv)) - 0.5 * (Y[None] - ym) ** 2 / yv
    lj = np.full((G, n), NAN)
    for g in range(G):
        for i in range(n):
            idx = np.flatnonzero(~np.isnan(Y[i]))
            if idx.size:
                H = CC[:, idx]
                Sy, e = H.T @ Sp[g, i] @ H + np.diag(sd[idx] ** 2), Y[i, idx] - ym[g, i, idx]
                lj[g, i] = -0.5 * (idx.size * np.log(2 * np.pi) + np.linalg.slogdet(Sy)[1] + e @ np.linalg.solve(Sy, e))
    pooled = mr.summary(mp, Sp, CC, DD, sd, Y)
    return dict(lpd=lpd, lpd_joint=lj, predict_y=pooled["y_mean"], predict_y_var_total=pooled["y_var_total"], lpd_mix=pooled["lpd"],
                lpd_gauss=pooled["lpd_gauss"])


# ---- 1. moments, 2. densities, 7. properties -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_moments_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Filtering and smoothing"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    ref, e_ref = filter_refs(*args)
    out = device(*args)
    assert set(out) == KEYS
    for k in MOMENTS:
        assert out[k].shape == ref[k].shape, k
        rule(f"{shape} q={qkind} {mode} J={J}: {k}", key_of(k), out[k], ref[k], e_ref[k])
    for k in COVS:
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)
    np.testing.assert_array_equal(out["m_smooth"][:, -1], out["m_filt"][:, -1])
    np.testing.assert_array_equal(out["S_smooth"][:, -1], out["S_filt"][:, -1])
    # properties: conditioning does not add variance, every covariance is positive definite
    fl = floor("var", ref["S_pred"])
    up, sm = float(np.max(np.linalg.eigvalsh(out["S_filt"] - out["S_pred"]))), float(np.max(np.linalg.eigvalsh(out["S_smooth"] - out["S_filt"])))
    low = min(float(np.min(np.linalg.eigvalsh(out[k]))) for k in COVS)
    print(f"{shape}: lambda_max(S - S^-) {up:.3e}, lambda_max(S^s - S) {sm:.3e} (floor {fl:.3e}), smallest eigenvalue {low:.3e}")
    assert up <= fl and sm <= fl and low > 0.0


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_densities_against_numpy_on_the_device_stacks(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out = case(shape, per_model, G), device(*args)
    (Y, sd), (CC, DD, _) = observations(*args), emission(cs, J)
    want, seen = numpy_densities(out, Y, CC, DD, sd), ~np.isnan(Y)
    nGroups = out["m_pred"].shape[0]
    nan_at = dict(lpd=np.broadcast_to(~seen, (nGroups,) + seen.shape), lpd_joint=np.broadcast_to(~seen.any(axis=1), (nGroups, Y.shape[0])),
                  lpd_mix=~seen, lpd_gauss=~seen, predict_y=np.zeros_like(seen), predict_y_var_total=np.zeros_like(seen))
    for k, w in want.items():
        got = out[k]
        assert got.shape == w.shape, k
        np.testing.assert_array_equal(np.isnan(got), nan_at[k], err_msg=k)
        ok = ~nan_at[k]
        tol = 1e-9 * (1.0 + float(np.max(np.abs(w[ok]))))
        err = float(np.max(np.abs(got[ok] - w[ok])))
        print(f"{shape} J={J}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    assert out["ll"] == pytest.approx(float(np.mean(want["lpd_mix"][seen])), abs=1e-9 * (1.0 + np.max(np.abs(want["lpd_mix"][seen]))))
    rows = seen.any(axis=1)
    lj = want["lpd_joint"][:, rows]
    llj = float(np.mean(np.log(np.mean(np.exp(lj - lj.max(axis=0)), axis=0)) + lj.max(axis=0)))
    assert out["ll_joint"] == pytest.approx(llj, abs=1e-9 * (1.0 + abs(llj)))
    s30 = seen[:30]
    assert out["RMSE"] == pytest.approx(float(np.sqrt(np.mean((Y[:30][s30] - want["predict_y"][:30][s30]) ** 2))), rel=1e-9)


# ---- 3. no observations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[5]], ids=str)
def test_without_observations_the_filter_is_the_propagation(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs = case(shape, per_model, G)
    S0 = start_cov(len(cs[0]), cs[2]["D"]) if with_S0 else None
    m_x, S_x = run_explicit(cs, qkind, mode, STEPS, S0)
    out = run_filter(cs, qkind, mode, np.full((STEPS, J), NAN), emission(cs, J), S0)
    for k, w in (("m_pred", m_x), ("m_filt", m_x), ("S_pred", S_x), ("S_filt", S_x)):
        np.testing.assert_array_equal(out[k], w, err_msg=k)
    assert np.all(np.isnan(out["lpd"])) and np.all(np.isnan(out["lpd_joint"])) and np.all(np.isnan(out["lpd_mix"]))
    assert np.isnan(out["ll"]) and np.isnan(out["ll_joint"]) and np.isnan(out["RMSE"])
    mixed, (Y, _) = device(*args), observations(*args)                          # row-wise, where a whole row is missing
    for i in np.flatnonzero(np.all(np.isnan(Y), axis=1)):
        np.testing.assert_array_equal(mixed["m_filt"][:, i], mixed["m_pred"][:, i])
        np.testing.assert_array_equal(mixed["S_filt"][:, i], mixed["S_pred"][:, i])


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_two_calls_are_equal_and_a_group_alone_equals_the_group_among_the_others(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a = case(shape, per_model, G), device(*args)
    Y, em = observations(*args)[0], emission(cs, J)
    S0 = start_cov(len(cs[0]), cs[2]["D"]) if with_S0 else None
    b = run_filter(cs, qkind, mode, Y, em, S0)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(len(cs[0])):
        one = run_filter(cs, qkind, mode, Y, em, S0, groups=[g])
        for k in MOMENTS + ("lpd", "lpd_joint"):
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k} group {g}")


def test_one_step_smoothed_is_the_filter_and_no_steps_returns_empty_arrays():
    cs = case("tiny")
    em = emission(cs, 3)
    y = np.asarray([[0.3, NAN, -0.2]])
    one, plain = run_filter(cs, "upper", "reference", y, em), run_filter(cs, "upper", "reference", y, em, smooth=False)
    np.testing.assert_array_equal(one["m_smooth"], one["m_filt"])
    np.testing.assert_array_equal(one["S_smooth"], one["S_filt"])
    assert set(plain) == KEYS - {"m_smooth", "S_smooth"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], one[k], err_msg=k)
    none = run_filter(cs, "upper", "reference", np.zeros((0, 3)), em)
    assert none["m_pred"].shape == none["m_smooth"].shape == (3, 0, 2) and none["S_filt"].shape == none["cross"].shape == (3, 0, 2, 2)
    assert none["lpd"].shape == (3, 0, 3) and none["lpd_joint"].shape == (3, 0) and none["lpd_mix"].shape == (0, 3)
    fused = pr.posterior_filter_grouped(*_fused_args(cs, 0)[:6], np.zeros((0, 3)), *em, smooth=True)
    assert fused["m_smooth"].shape == (3, 0, 2) and fused["S_pred"].shape == (3, 0, 2, 2)


# ---- 5. fused with the posteriors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J, mode):
    """posterior_filter_grouped against collapse_u_mean_grouped followed by filter_grouped, as
    tests/test_gpu_moment_grouped.py::test_fused_form_against_the_two_calls: the reference is the restatement on the device's own
    posterior (np.longdouble where that is wider), the yardstick the two-call route.  Whether the bits coincide is printed."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])          # (data only: any posterior's will do)
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    fused = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode, smooth=True)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, meta["T"], Y, Qs, CC, DD, lr, q_mode=mode,
                            smooth=True)
    print(f"{shape} {mode}: fused and two-call routes bit-identical: {all(np.array_equal(fused[k], two[k], equal_nan=True) for k in KEYS)}")
    t = np.longdouble if WIDE else np.float64
    ctrl = call[meta["T"]: meta["T"] + STEPS]
    for i, g in enumerate(gs):
        beta, Gam = mr.posterior_terms(Lm[i if per_model else 0], U[i], Hinv[i], mode, dtype=t)
        f = fr.filter(g["X"][-1], np.zeros((meta["D"],) * 2), Y, CC, DD, sd, g["Q"], fr.gp_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t),
                      dtype=t)
        f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=t)
        for k in MOMENTS:
            ref = f[k].astype(np.float64)
            e_f, e_t = float(np.max(np.abs(fused[k][i] - ref))), float(np.max(np.abs(two[k][i] - ref)))
            bound = max(4.0 * e_t, floor(key_of(k), ref))
            print(f"{shape} {mode} group {i}: {k}: fused {e_f:.3e}, two calls {e_t:.3e}, bound {bound:.3e}")
            assert np.all(np.isfinite(fused[k][i])) and e_f <= bound, k
    for k in COVS:
        np.testing.assert_array_equal(fused[k], np.swapaxes(fused[k], -1, -2), err_msg=k)
    again = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode, smooth=True)
    for k in KEYS:
        np.testing.assert_array_equal(again[k], fused[k], err_msg=k)
    # a start given by the caller: the chains' own last states reproduce the default
    given = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode, smooth=True,
                                        x0s=np.stack([g["X"][-1] for g in gs]))
    for k in KEYS:
        np.testing.assert_array_equal(given[k], fused[k], err_msg=k)


# ---- 6. an outlier -------------------------------------------------------------------------------------------------------------------
def test_an_outlier_forty_deviations_away_stays_finite():
    args = ("ragged", False, None, "upper", "intent", 3, False)
    cs, base = case(*args[:3]), device(*args)
    Y, sd = observations(*args)
    CC, DD, lr = emission(cs, 3)
    s2 = np.einsum("kj,gkl,lj->gj", CC, base["S_pred"][:, 4], CC) + sd ** 2
    m = np.einsum("gk,kj->gj", base["m_pred"][:, 4], CC) + DD
    Y = np.array(Y)
    Y[4, 0] = np.max(m[:, 0]) + 40.0 * np.sqrt(np.max(s2[:, 0]))
    out = run_filter(cs, "upper", "intent", Y, (CC, DD, lr))
    seen = ~np.isnan(Y)
    for k in MOMENTS:
        assert np.all(np.isfinite(out[k])), k
    assert np.all(np.isfinite(out["lpd"][:, seen])) and np.all(np.isfinite(out["lpd_joint"][:, seen.any(axis=1)]))
    assert np.all(np.isfinite(out["lpd_mix"][seen])) and np.all(out["lpd"][:, 4, 0] < -700.0)
    assert np.isfinite(out["ll"]) and np.isfinite(out["ll_joint"])
    print(f"outlier: lpd of the entry {out['lpd'][:, 4, 0]}, ll_joint {out['ll_joint']:.3f}")


# ---- 8. model level: the actuator fixture with three chains --------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_heldout(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = np.array(Y[N_TRAIN:N_TRAIN + TEST_LEN])
    Yt[7] = NAN
    Yt[-5:] = NAN
    J, D = Yt.shape[1], 4
    out = mod.filter_heldout(Yt, c, smooth=True, Y_train_std=1.7)
    assert set(out) == KEYS
    for k in MOMENTS:
        assert out[k].shape == ((S, TEST_LEN, D) if k.startswith("m_") else (S, TEST_LEN, D, D)), k
    assert out["lpd"].shape == (S, TEST_LEN, J) and out["lpd_joint"].shape == (S, TEST_LEN)
    assert all(out[k].shape == (TEST_LEN, J) for k in POOLED)
    seen = ~np.isnan(Yt)
    assert all(np.all(np.isfinite(out[k])) for k in MOMENTS) and np.all(np.isfinite(out["lpd_mix"][seen]))
    assert all(np.isfinite(out[k]) for k in ("ll", "ll_joint", "ll_original_units", "RMSE"))
    assert out["ll_original_units"] == out["ll"] - float(np.log(1.7))
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        direct = pr.posterior_filter_grouped(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, c, N_TRAIN, Yt, lik.CC, lik.DD,
                                             lik.log_Rchols, smooth=True, Y_train_std=1.7)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        direct = pr.filter_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [mod._X_chains[s][-1] for s in range(S)], c, N_TRAIN, Yt, mod.Q,
                                   lik.CC, lik.DD, lik.log_Rchols, smooth=True, Y_train_std=1.7)
    again = mod.filter_heldout(Yt, c, smooth=True, Y_train_std=1.7)
    for k in KEYS:
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    plain = mod.filter_heldout(Yt, c, Y_train_std=1.7)
    assert set(plain) == KEYS - {"m_smooth", "S_smooth"}
    # a fresh record: a start given by the caller
    fresh = mod.filter_heldout(Yt, c, x0=np.zeros(D), S0=0.5 * np.eye(D), Y_train_std=1.7)
    assert fresh["m_pred"].shape == (S, TEST_LEN, D) and np.all(np.isfinite(fresh["m_filt"]))
    free = mod.evaluate_heldout(Y[N_TRAIN:N_TRAIN + TEST_LEN], c, 8, Y_train_std=1.7, method="moment")
    print(f"U_collapse={U_collapse}: one step ahead: ll {out['ll']:.6f}, ll_joint {out['ll_joint']:.6f}, RMSE {out['RMSE']:.6f}; "
          f"free run (evaluate_heldout, moment): ll {free['ll']:.6f}, RMSE {free['RMSE']:.6f}")
