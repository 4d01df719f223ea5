"""Rolling-origin multi-step forecasts on the device: `ffvd_op_forecast_grouped` (prediction.forecast_grouped), fused with the collapsed
posteriors (`ffvd_op_posterior_forecast_grouped`, prediction.posterior_forecast_grouped) and DGPSSM.forecast_heldout.

Record, horizon, origins.  The 12-row record of tests/test_gpu_filter_grouped.py with its gaps (row 3 missing, the last three rows
missing, for J = 3 rows 5 and 6 partial), h = 3, origins 0 .. 8: for output 0 that leaves 6 / 5 / 4 observed targets at k = 1 / 2 / 3
(asserted through n_h).  The cases are the filter's: the smallest shapes at which the track indexing can go wrong.

What is exact and what is not.  A track runs the expressions of the propagation on the filtered state the filter stored, so it must be
array_equal to `moment_grouped` from that state (and to a filter over the truncated record followed by all-NaN rows).  Accuracy is
judged independently of the device: the reference is tests/filter_ref.py followed by tests/moment_ref.py's propagation from its
filtered states, in fp64; its own error e_ref is measured against the same composition in np.longdouble; the device must satisfy
error <= max(4 e_ref, floor) (the rule and floors of tests/test_gpu_moment_grouped.py).  The pooled arrays are compared with NumPy on
the device's own stacks, tolerance 1e-9 (1 + max|ref|).  Every measured error is printed."""
import functools

import numpy as np
import pytest

import filter_ref as fr
import moment_ref as mr
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_conditional_grouped import floor
from test_gpu_filter_grouped import CASES, MOMENTS, POOLED, device as filter_device, emission, filter_refs, observations, run_filter
from test_gpu_moment_grouped import (N_TRAIN, S, STEPS, TEST_LEN, WIDE, _chains, _fused_args, _q, _regression_model, case, rule,
                                     start_cov)

pytestmark = pytest.mark.gpu

NAN = np.nan
H = 3
ORIGINS = list(range(STEPS - H))                 # 0 .. 8
FILTER_KEYS = tuple(k for k in MOMENTS if "smooth" not in k) + ("lpd", "lpd_joint")
CURVES = ("n_h", "rmse_h", "ll_h", "ll_gauss_h", "ll_h_original_units")
KEYS = {"origins"} | set(POOLED) | set(CURVES)
FULL_KEYS = KEYS | {"m_fc", "S_fc"} | set(FILTER_KEYS) | {"filter_" + k for k in POOLED} | {"ll", "ll_joint", "ll_original_units", "RMSE"}


def _posteriors(cs, qkind, groups=None, src="orc"):
    gs, per_model = cs[0], cs[3]
    idx = list(range(len(gs))) if groups is None else groups
    sel, qs = [gs[i] for i in idx], _q(cs, qkind, src)
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in sel], [g["kern"] for g in sel], [g[src]["L"] for g in sel]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    return idx, sel, (Ls, Zs, kerns, [g[src]["U"] for g in sel], None if qs is None else [qs[i] for i in idx])


def run_forecast(cs, qkind, mode, Y, em, S0=None, groups=None, h=H, **kw):
    call, meta = cs[1], cs[2]
    idx, sel, post = _posteriors(cs, qkind, groups)
    return pr.forecast_grouped(*post, [g["X"][-1] for g in sel], call, meta["T"], Y, [g["Q"] for g in sel], *em, h,
                               S0s=None if S0 is None else S0[idx], q_mode=mode, **kw)


def run_moment(cs, qkind, mode, x_lasts, S0s, offset, steps):
    """moment_grouped on the case's posteriors from the given states, control rows from `offset`"""
    call = cs[1]
    _, sel, post = _posteriors(cs, qkind)
    return pr.moment_grouped(*post, list(x_lasts), call, offset, steps, [g["Q"] for g in sel], S0s=S0s, q_mode=mode)


def _S0(cs, with_S0):
    return start_cov(len(cs[0]), cs[2]["D"]) if with_S0 else None


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case (every origin, tracks and the filter's outputs), shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    Y, _ = observations(shape, per_model, G, qkind, mode, J, with_S0)
    return run_forecast(cs, qkind, mode, Y, emission(cs, J), _S0(cs, with_S0), return_tracks=True, return_filter=True)


def targets(Y, origins=ORIGINS, h=H):
    return np.stack([Y[o + 1: o + 1 + h] for o in origins])                     # (B, h, J)


# ---- 1. bit-identity with the existing propagation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_are_the_propagation_from_the_filtered_states_bit_for_bit(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, flt = case(shape, per_model, G), device(*args), filter_device(*args)
    nG, D, T = len(cs[0]), cs[2]["D"], cs[2]["T"]
    assert set(out) == FULL_KEYS
    assert out["origins"].tolist() == ORIGINS
    assert out["m_fc"].shape == (nG, len(ORIGINS), H, D) and out["S_fc"].shape == (nG, len(ORIGINS), H, D, D)
    for k in FILTER_KEYS + ("ll", "ll_joint", "ll_original_units", "RMSE"):                  # the call's own filter is filter_grouped's
        np.testing.assert_array_equal(out[k], flt[k], err_msg=k)
    for k in POOLED:
        np.testing.assert_array_equal(out["filter_" + k], flt[k], err_msg=k)
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"]))
    for b, i in enumerate(ORIGINS):
        m_x, S_x = run_moment(cs, qkind, mode, out["m_filt"][:, i], out["S_filt"][:, i], T + i + 1, H)
        np.testing.assert_array_equal(out["m_fc"][:, b], m_x, err_msg=f"m_fc, origin {i}")
        np.testing.assert_array_equal(out["S_fc"][:, b], S_x, err_msg=f"S_fc, origin {i}")


# ---- 2. the user-facing meaning -----------------------------------------------------------------------------------------------------
def test_a_track_is_the_filter_of_the_truncated_record_followed_by_unobserved_rows():
    args = CASES[1]
    shape, per_model, G, qkind, mode, J, with_S0 = args
    cs, out = case(shape, per_model, G), device(*args)
    Y, em = observations(*args)[0], emission(cs, J)
    for b, i in enumerate(ORIGINS):
        Yi = np.concatenate((Y[:i + 1], np.full((H, J), NAN)), axis=0)
        f = run_filter(cs, qkind, mode, Yi, em, _S0(cs, with_S0), smooth=False)
        np.testing.assert_array_equal(out["m_fc"][:, b], f["m_pred"][:, i + 1: i + 1 + H], err_msg=f"origin {i}")
        np.testing.assert_array_equal(out["S_fc"][:, b], f["S_pred"][:, i + 1: i + 1 + H], err_msg=f"origin {i}")


# ---- 3. horizon 1 against the filter's own prediction, 4. accuracy -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forecast_refs(shape, per_model, G, qkind, mode, J, with_S0):
    """filter_ref.filter followed by moment_ref.propagate from its filtered states, stacked (G, B, H, ...) in fp64 (`ref`), and its
    error against the same composition in np.longdouble (`e_ref`).  Computed once per case, never modified."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(shape, per_model, G, qkind, mode, J, with_S0)
    CC, DD, _ = emission(cs, J)
    qs, S0 = _q(cs, qkind), start_cov(len(gs), meta["D"]) if with_S0 else np.zeros((len(gs), meta["D"], meta["D"]))
    ctrl = call[meta["T"]: meta["T"] + STEPS]
    ref, e_ref = dict(m=[], S=[]), dict(m=0.0, S=0.0)
    for gi, g in enumerate(gs):
        res = {}
        for t in (np.float64, np.longdouble) if WIDE else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[gi], mode, dtype=t)
            f = fr.filter(g["X"][-1], S0[gi], Y, CC, DD, sd, g["Q"], fr.gp_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t), dtype=t)
            tracks = [mr.propagate(f["m_filt"][i], f["S_filt"][i], ctrl[i + 1:], g["Z"], g["okern"], beta, Gam, g["Q"], H, dtype=t) for i in ORIGINS]
            res[t] = np.stack([m for m, _ in tracks]), np.stack([s for _, s in tracks])
        ref["m"].append(res[np.float64][0])
        ref["S"].append(res[np.float64][1])
        if WIDE:
            e_ref["m"] = max(e_ref["m"], float(np.max(np.abs(res[np.float64][0] - res[np.longdouble][0]))))
            e_ref["S"] = max(e_ref["S"], float(np.max(np.abs(res[np.float64][1] - res[np.longdouble][1]))))
    return {k: np.stack(v) for k, v in ref.items()}, e_ref


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Rolling-origin forecasts"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    out, (ref, e_ref) = device(*args), forecast_refs(*args)
    what = f"{shape} q={qkind} {mode} J={J}"
    assert out["m_fc"].shape == ref["m"].shape and out["S_fc"].shape == ref["S"].shape
    rule(f"{what}: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
    rule(f"{what}: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    low = float(np.min(np.linalg.eigvalsh(out["S_fc"])))
    print(f"{what}: smallest eigenvalue of S_fc {low:.3e}")
    assert low > 0.0
    # horizon 1 is the filter's own one-step prediction of the next row: judged against the filter's reference, by the same rule
    fref, fe = filter_refs(*args)
    rows = [i + 1 for i in ORIGINS]
    rule(f"{what}: horizon 1 against m_pred", "mean", out["m_fc"][:, :, 0], fref["m_pred"][:, rows], fe["m_pred"])
    rule(f"{what}: horizon 1 against S_pred", "var", out["S_fc"][:, :, 0], fref["S_pred"][:, rows], fe["S_pred"])
    rule(f"{what}: horizon 1 against the device's m_pred", "mean", out["m_fc"][:, :, 0], out["m_pred"][:, rows], fe["m_pred"])
    rule(f"{what}: horizon 1 against the device's S_pred", "var", out["S_fc"][:, :, 0], out["S_pred"][:, rows], fe["S_pred"])
    same = np.array_equal(out["m_fc"][:, :, 0], out["m_pred"][:, rows]) and np.array_equal(out["S_fc"][:, :, 0], out["S_pred"][:, rows])
    print(f"{what}: horizon 1 and the filter's m_pred / S_pred of the next row bit-identical: {same}")


# ---- 5. the pooled arrays and the horizon curves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_pooled_arrays_and_curves_against_numpy_on_the_device_stacks(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out = case(shape, per_model, G), device(*args)
    (Y, sd), (CC, DD, _) = observations(*args), emission(cs, J)
    nG, B, D = out["m_fc"].shape[0], len(ORIGINS), cs[2]["D"]
    Yt = targets(Y)
    seen = ~np.isnan(Yt)
    ref = mr.summary(out["m_fc"].reshape(nG, B * H, D), out["S_fc"].reshape(nG, B * H, D, D), CC, DD, np.asarray(sd).reshape(-1), Yt.reshape(B * H, J))
    want = dict(predict_y=ref["y_mean"], predict_y_var_total=ref["y_var_total"], lpd_mix=ref["lpd"], lpd_gauss=ref["lpd_gauss"])
    nan_at = dict(predict_y=np.zeros_like(seen), predict_y_var_total=np.zeros_like(seen), lpd_mix=~seen, lpd_gauss=~seen)
    for k in POOLED:
        got, w = out[k], want[k].reshape(B, H, J)
        assert got.shape == (B, H, J), k
        np.testing.assert_array_equal(np.isnan(got), nan_at[k], err_msg=k)
        ok = ~nan_at[k]
        tol, err = 1e-9 * (1.0 + float(np.max(np.abs(w[ok])))), float(np.max(np.abs(got[ok] - w[ok])))
        print(f"{shape} J={J}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    # the curves, from the device's own pooled arrays
    n_h = seen.sum(axis=0)
    np.testing.assert_array_equal(out["n_h"], n_h)
    assert out["n_h"].shape == (H, J) and np.issubdtype(out["n_h"].dtype, np.integer)
    assert n_h[:, 0].tolist() == ([6, 5, 4] if J == 3 else [7, 6, 5]) and np.all(n_h > 0)      # no horizon is silently empty (J = 3: row 6 too)
    for k, src in (("rmse_h", None), ("ll_h", "lpd_mix"), ("ll_gauss_h", "lpd_gauss")):
        w = np.empty((H, J))
        for kk in range(H):
            for j in range(J):
                s = seen[:, kk, j]
                w[kk, j] = np.sqrt(np.mean((Yt[s, kk, j] - out["predict_y"][s, kk, j]) ** 2)) if src is None else np.mean(out[src][s, kk, j])
        tol, err = 1e-9 * (1.0 + float(np.max(np.abs(w)))), float(np.max(np.abs(out[k] - w)))
        print(f"{shape} J={J}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert out[k].shape == (H, J) and np.all(np.isfinite(out[k])) and err <= tol, k
    np.testing.assert_array_equal(out["ll_h_original_units"], out["ll_h"])          # Y_train_std = 1


def test_curves_in_original_units_and_horizons_without_a_target():
    args = CASES[2]
    shape, per_model, G, qkind, mode, J, with_S0 = args
    cs, base = case(shape, per_model, G), device(*args)
    Y, em = observations(*args)[0], emission(cs, J)
    out = run_forecast(cs, qkind, mode, Y, em, Y_train_std=1.7)
    assert set(out) == KEYS
    np.testing.assert_allclose(out["rmse_h"], 1.7 * base["rmse_h"], rtol=1e-15)
    np.testing.assert_array_equal(out["ll_h"], base["ll_h"])
    np.testing.assert_array_equal(out["ll_h_original_units"], out["ll_h"] - float(np.log(1.7)))
    # origins 6 .. 8: the targets at k = 3 (rows 9 .. 11) are all missing
    late = run_forecast(cs, qkind, mode, Y, em, origins=[6, 7, 8])
    assert late["n_h"][2].tolist() == [0] * J and np.all(np.isnan(late["rmse_h"][2])) and np.all(np.isnan(late["ll_h"][2]))
    assert np.all(np.isnan(late["ll_gauss_h"][2])) and np.all(np.isfinite(late["rmse_h"][0])) and np.all(np.isfinite(late["predict_y"]))
    assert np.all(np.isfinite(late["predict_y_var_total"])) and np.all(np.isnan(late["lpd_mix"][:, 2]))


# ---- 6. determinism and independence of the decomposition ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_results_do_not_depend_on_the_call_the_groups_the_origins_or_the_pass_size(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a = case(shape, per_model, G), device(*args)
    Y, em, S0 = observations(*args)[0], emission(cs, J), _S0(cs, with_S0)
    kw = dict(return_tracks=True, return_filter=True)
    b = run_forecast(cs, qkind, mode, Y, em, S0, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(len(cs[0])):                                                     # a group alone
        one = run_forecast(cs, qkind, mode, Y, em, S0, groups=[g], return_tracks=True)
        np.testing.assert_array_equal(one["m_fc"][0], a["m_fc"][g], err_msg=f"group {g}")
        np.testing.assert_array_equal(one["S_fc"][0], a["S_fc"][g], err_msg=f"group {g}")
    for i in (0, 5, 8):                                                             # an origin alone
        one = run_forecast(cs, qkind, mode, Y, em, S0, origins=[i], return_tracks=True)
        assert one["origins"].tolist() == [i]
        for k in ("m_fc", "S_fc"):
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, i], err_msg=f"{k}, origin {i}")
        for k in POOLED:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=f"{k}, origin {i}")
    for tpp in (1, 2, 4):                                                           # passes of 1, 2 (a ragged last pass) and 4 origins
        p = run_forecast(cs, qkind, mode, Y, em, S0, tracks_per_pass=tpp, **kw)
        for k in FULL_KEYS:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, tracks_per_pass {tpp}")
    some = run_forecast(cs, qkind, mode, Y, em, S0, origins=[0, 4, 8], return_tracks=True)
    strided = run_forecast(cs, qkind, mode, Y, em, S0, stride=4, return_tracks=True, tracks_per_pass=2)
    for o in (some, strided):
        assert o["origins"].tolist() == [0, 4, 8]
        for k in ("m_fc", "S_fc"):
            np.testing.assert_array_equal(o[k], a[k][:, [0, 4, 8]], err_msg=k)
        for k in POOLED:
            np.testing.assert_array_equal(o[k], a[k][[0, 4, 8]], err_msg=k)


def test_horizon_one_from_the_last_possible_origin():
    args = CASES[0]
    shape, per_model, G, qkind, mode, J, with_S0 = args
    cs, flt = case(shape, per_model, G), filter_device(*args)
    Y, em = observations(*args)[0], emission(cs, J)
    out = run_forecast(cs, qkind, mode, Y, em, h=1, origins=[STEPS - 2], return_tracks=True)
    nG, D = len(cs[0]), cs[2]["D"]
    assert out["m_fc"].shape == (nG, 1, 1, D) and out["S_fc"].shape == (nG, 1, 1, D, D) and out["predict_y"].shape == (1, 1, J)
    m_x, S_x = run_moment(cs, qkind, mode, flt["m_filt"][:, STEPS - 2], flt["S_filt"][:, STEPS - 2], cs[2]["T"] + STEPS - 1, 1)
    np.testing.assert_array_equal(out["m_fc"][:, 0], m_x)
    np.testing.assert_array_equal(out["S_fc"][:, 0], S_x)
    assert out["n_h"].tolist() == [[0] * J] and np.all(np.isnan(out["ll_h"]))       # row 11 is missing
    full = run_forecast(cs, qkind, mode, Y, em, h=STEPS - 1, return_tracks=True)    # the longest horizon: one origin, row 0
    assert full["origins"].tolist() == [0] and full["m_fc"].shape == (nG, 1, STEPS - 1, D) and np.all(np.isfinite(full["S_fc"]))


# ---- 7. fused with the posteriors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_forecast_grouped against collapse_u_mean_grouped followed by forecast_grouped, as
    tests/test_gpu_filter_grouped.py::test_fused_form_against_the_two_calls: the reference is the restatement on the device's own
    posterior (np.longdouble where that is wider), the yardstick the two-call route.  Whether the bits coincide is printed."""
    mode = "reference"
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])          # (data only: any posterior's will do)
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(q_mode=mode, return_tracks=True, return_filter=True)
    fused = pr.posterior_forecast_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, H, **kw)
    assert set(fused) == FULL_KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.forecast_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, meta["T"], Y, Qs, CC, DD, lr, H, **kw)
    print(f"{shape}: fused and two-call routes bit-identical: {all(np.array_equal(fused[k], two[k], equal_nan=True) for k in FULL_KEYS)}")
    t = np.longdouble if WIDE else np.float64
    ctrl = call[meta["T"]: meta["T"] + STEPS]
    for i, g in enumerate(gs):
        beta, Gam = mr.posterior_terms(Lm[i if per_model else 0], U[i], Hinv[i], mode, dtype=t)
        f = fr.filter(g["X"][-1], np.zeros((meta["D"],) * 2), Y, CC, DD, sd, g["Q"], fr.gp_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t),
                      dtype=t)
        tracks = [mr.propagate(f["m_filt"][o], f["S_filt"][o], ctrl[o + 1:], g["Z"], g["okern"], beta, Gam, g["Q"], H, dtype=t) for o in ORIGINS]
        for k, key, ref in (("m_fc", "mean", np.stack([m for m, _ in tracks])), ("S_fc", "var", np.stack([s for _, s in tracks]))):
            ref = ref.astype(np.float64)
            e_f, e_t = float(np.max(np.abs(fused[k][i] - ref))), float(np.max(np.abs(two[k][i] - ref)))
            bound = max(4.0 * e_t, floor(key, ref))
            print(f"{shape} group {i}: {k}: fused {e_f:.3e}, two calls {e_t:.3e}, bound {bound:.3e}")
            assert np.all(np.isfinite(fused[k][i])) and e_f <= bound, k
    np.testing.assert_array_equal(fused["S_fc"], np.swapaxes(fused["S_fc"], -1, -2))
    plain = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode)
    for k in FILTER_KEYS:                                                           # the fused call's own filter is the fused filter's
        np.testing.assert_array_equal(fused[k], plain[k], err_msg=k)
    again = pr.posterior_forecast_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, H, tracks_per_pass=2, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(again[k], fused[k], err_msg=k)


# ---- 8. model level: the actuator fixture with three chains --------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_forecast_heldout(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = np.array(Y[N_TRAIN:N_TRAIN + TEST_LEN])
    Yt[7] = NAN
    Yt[-5:] = NAN
    J, D, h = Yt.shape[1], 4, 5
    B = TEST_LEN - h
    out = mod.forecast_heldout(Yt, c, h, Y_train_std=1.7, return_tracks=True)
    assert set(out) == KEYS | {"m_fc", "S_fc"}
    assert out["origins"].tolist() == list(range(B)) and out["m_fc"].shape == (S, B, h, D) and out["S_fc"].shape == (S, B, h, D, D)
    assert all(out[k].shape == (B, h, J) for k in POOLED) and all(out[k].shape == (h, J) for k in CURVES)
    assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"])) and np.all(np.isfinite(out["predict_y"]))
    assert np.all(out["n_h"] > 0) and all(np.all(np.isfinite(out[k])) for k in CURVES)
    np.testing.assert_array_equal(out["ll_h_original_units"], out["ll_h"] - float(np.log(1.7)))
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        direct = pr.posterior_forecast_grouped(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, c, N_TRAIN, Yt, lik.CC, lik.DD,
                                               lik.log_Rchols, h, Y_train_std=1.7, return_tracks=True)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        direct = pr.forecast_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [mod._X_chains[s][-1] for s in range(S)], c, N_TRAIN, Yt, mod.Q,
                                     lik.CC, lik.DD, lik.log_Rchols, h, Y_train_std=1.7, return_tracks=True)
    again = mod.forecast_heldout(Yt, c, h, Y_train_std=1.7, return_tracks=True)
    for k in out:
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    lean = mod.forecast_heldout(Yt, c, h, stride=7, Y_train_std=1.7)
    assert set(lean) == KEYS and lean["origins"].tolist() == list(range(0, B, 7))
    np.testing.assert_array_equal(lean["predict_y"], out["predict_y"][::7])
    one = mod.filter_heldout(Yt, c, Y_train_std=1.7)
    print(f"U_collapse={U_collapse}: one step ahead (filter_heldout): ll {one['ll']:.6f}, RMSE {one['RMSE']:.6f}; horizons 1 .. {h}: "
          f"rmse_h {np.round(out['rmse_h'][:, 0], 6).tolist()}, ll_h {np.round(out['ll_h'][:, 0], 6).tolist()}, n_h {out['n_h'][:, 0].tolist()}")
