"""Rolling-origin multi-step forecasts under the linearised (extended Kalman) rule on the device: prediction.forecast_linear_grouped
(`ffvd_op_forecast_linear_grouped`), fused with the collapsed posteriors (prediction.posterior_forecast_linear_grouped,
`ffvd_op_posterior_forecast_linear_grouped`) and DGPSSM.forecast_heldout_linearised.

Fixtures.  The seven cases, the 12-row record with its gaps, H = 3 and origins 0 .. 8 of tests/test_gpu_forecast_grouped.py, with its
helpers imported: `run_forecast` there takes no rule, `run_linear_forecast` hands it the linearised function in place of
`pr.forecast_grouped` for the duration of the call (the indirection of tests/test_gpu_filter_linear.py::run_linear; should the sibling
ever bind the function at import the patch would do nothing, and the accuracy tests and the comparison with the linearised filter
fail then).  Two fixtures reach tile edges of the product kernel that the shared cases do not: M = 300 (a ragged last column tile)
and the 140-row record of tests/forecast_linear_ref.py (138 origins: a second row tile).

Reference and rule.  tests/forecast_linear_ref.py (pinned in tests/test_forecast_linear_ref.py) in fp64 on the oracle's posterior; e_ref
is that reference against the same composition in np.longdouble; the device must satisfy error <= max(4 e_ref, floor) with `rule` and
the floors of tests/test_gpu_moment_grouped.py.  The pooled arrays are compared with NumPy on the device's own stacks at
1e-9 (1 + max|ref|).  Every measured error is printed; DESIGN.md section 9, "Linearised forecasts", has the largest."""
import functools
from unittest import mock

import numpy as np
import pytest

import filter_ref as fr
import forecast_linear_ref as flr
import linear_filter_ref as lf
import moment_ref as mr
from ffvd_amd import prediction as pr, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_conditional_grouped import _group, _kernels, floor
from test_gpu_filter_grouped import CASES, POOLED, emission, observations
from test_gpu_filter_linear import device as linear_filter_device
from test_gpu_forecast_grouped import CURVES, FILTER_KEYS, FULL_KEYS, H, KEYS, ORIGINS, _S0, run_forecast, targets
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, TEST_LEN, WIDE, _chains, _fused_args, _q, _regression_model, case, rule, start_cov

pytestmark = pytest.mark.gpu

NAN = np.nan


def run_linear_forecast(*args, **kw):
    """`run_forecast` of tests/test_gpu_forecast_grouped.py with the linearised function under the name it looks up at call time"""
    with mock.patch.object(pr, "forecast_grouped", pr.forecast_linear_grouped):
        return run_forecast(*args, **kw)


def bound(key, ref, e_ref):
    """the rule's bound for an array: max(4 e_ref, floor), the floor alone where np.longdouble is no wider"""
    return max(4.0 * e_ref, floor(key, ref)) if WIDE else floor(key, ref)


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case (every origin, tracks and the filter's outputs), shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    Y, _ = observations(shape, per_model, G, qkind, mode, J, with_S0)
    return run_linear_forecast(cs, qkind, mode, Y, emission(cs, J), _S0(cs, with_S0), return_tracks=True, return_filter=True)


@functools.lru_cache(maxsize=None)
def forecast_refs(shape, per_model, G, qkind, mode, J, with_S0):
    """The reference of a case on the oracle's posterior and its own error.  Computed once per case, never modified."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(shape, per_model, G, qkind, mode, J, with_S0)
    CC, DD, _ = emission(cs, J)
    S0 = start_cov(len(gs), meta["D"]) if with_S0 else np.zeros((len(gs), meta["D"], meta["D"]))
    return flr.reference(gs, call[meta["T"]: meta["T"] + STEPS], Y, CC, DD, sd, _q(cs, qkind), S0, mode, ORIGINS, H, WIDE)


# ---- 1. accuracy, the call's own filter, symmetry, horizon 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Linearised forecasts"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, (ref, e_ref), flt = case(shape, per_model, G), device(*args), forecast_refs(*args), linear_filter_device(*args)
    what = f"linearised {shape} q={qkind} {mode} J={J}"
    nG, D = len(cs[0]), cs[2]["D"]
    assert set(out) == FULL_KEYS and out["origins"].tolist() == ORIGINS
    assert out["m_fc"].shape == ref["m"].shape == (nG, len(ORIGINS), H, D) and out["S_fc"].shape == ref["S"].shape
    rule(f"{what}: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
    rule(f"{what}: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    low = float(np.min(np.linalg.eigvalsh(out["S_fc"])))
    print(f"{what}: smallest eigenvalue of S_fc {low:.3e}")
    assert low > 0.0
    # the call's own filter is filter_grouped(method="linearised") bit for bit
    for k in FILTER_KEYS + ("ll", "ll_joint", "ll_original_units", "RMSE"):
        np.testing.assert_array_equal(out[k], flt[k], err_msg=k)
    for k in POOLED:
        np.testing.assert_array_equal(out["filter_" + k], flt[k], err_msg=k)
    # horizon 1 against the filter's own prediction of the next row: the quadratic form is summed in column tiles here and in slabs of
    # 16 rows there, so the bits may differ; both lie within the rule's bound of one reference, so they are within twice that bound
    rows = [i + 1 for i in ORIGINS]
    dm = float(np.max(np.abs(out["m_fc"][:, :, 0] - out["m_pred"][:, rows])))
    dS = float(np.max(np.abs(out["S_fc"][:, :, 0] - out["S_pred"][:, rows])))
    bm, bS = 2.0 * bound("mean", ref["m"], e_ref["m"]), 2.0 * bound("var", ref["S"], e_ref["S"])
    same = np.array_equal(out["m_fc"][:, :, 0], out["m_pred"][:, rows]) and np.array_equal(out["S_fc"][:, :, 0], out["S_pred"][:, rows])
    print(f"{what}: horizon 1 against the filter's m_pred {dm:.3e} (2 x bound {bm:.3e}), S_pred {dS:.3e} (2 x bound {bS:.3e}), "
          f"bit-identical: {same}")
    assert dm <= bm and dS <= bS


# ---- 2. determinism and independence of the decomposition ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_results_do_not_depend_on_the_call_the_groups_the_origins_or_the_pass_size(shape, per_model, G, qkind, mode, J, with_S0):
    """a track must not depend on the other rows of its tile, on the other groups or on the pass it is in"""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a = case(shape, per_model, G), device(*args)
    Y, em, S0 = observations(*args)[0], emission(cs, J), _S0(cs, with_S0)
    kw = dict(return_tracks=True, return_filter=True)
    b = run_linear_forecast(cs, qkind, mode, Y, em, S0, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(len(cs[0])):                                                     # a group alone
        one = run_linear_forecast(cs, qkind, mode, Y, em, S0, groups=[g], return_tracks=True)
        np.testing.assert_array_equal(one["m_fc"][0], a["m_fc"][g], err_msg=f"group {g}")
        np.testing.assert_array_equal(one["S_fc"][0], a["S_fc"][g], err_msg=f"group {g}")
    for i in (0, 5, 8):                                                             # an origin alone
        one = run_linear_forecast(cs, qkind, mode, Y, em, S0, origins=[i], return_tracks=True)
        assert one["origins"].tolist() == [i]
        for k in ("m_fc", "S_fc"):
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, i], err_msg=f"{k}, origin {i}")
        for k in POOLED:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=f"{k}, origin {i}")
    for tpp in (1, 2, 4):                                                           # passes of 1, 2 (a ragged last pass) and 4 origins
        p = run_linear_forecast(cs, qkind, mode, Y, em, S0, tracks_per_pass=tpp, **kw)
        for k in FULL_KEYS:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, tracks_per_pass {tpp}")
    some = run_linear_forecast(cs, qkind, mode, Y, em, S0, origins=[0, 4, 8], return_tracks=True)
    strided = run_linear_forecast(cs, qkind, mode, Y, em, S0, stride=4, return_tracks=True, tracks_per_pass=2)
    for o in (some, strided):
        assert o["origins"].tolist() == [0, 4, 8]
        for k in ("m_fc", "S_fc"):
            np.testing.assert_array_equal(o[k], a[k][:, [0, 4, 8]], err_msg=k)
        for k in POOLED:
            np.testing.assert_array_equal(o[k], a[k][[0, 4, 8]], err_msg=k)


# ---- 3. tile edges the shared cases do not reach -------------------------------------------------------------------------------------
def test_a_ragged_last_column_tile():
    """M = 300: Mp = 320, three column tiles of the product, the last 64 wide (it takes the register path of the main loop, the others
    the LDS-DMA path), and a second stride of 256 columns in the state kernel.  The fixture of
    tests/test_gpu_filter_linear.py::test_a_second_column_stride: two chains of one model, q slices, a start covariance, six rows
    with a gap; h = 2, origins 0 .. 3."""
    params, _, c, meta = synthetic.make_named("tiny", M=300, T=320, S=2)
    gs = [_group(params, c, meta, params["X"][g]) for g in range(2)]
    T, D, n, h = meta["T"], meta["D"], 6, 2
    call = np.concatenate((c, np.random.default_rng(3).standard_normal((n, meta["C"]))), axis=0)
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    sd = np.exp(np.asarray(lr)[0])
    Y = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(31).standard_normal((n, CC.shape[1]))
    Y[2] = NAN
    S0, qs, origins = start_cov(2, D), [g["orc"]["H"] for g in gs], list(range(n - h))
    ref, e_ref = flr.reference(gs, call[T: T + n], Y, CC, DD, sd, qs, S0, "intent", origins, h, WIDE)
    out = pr.forecast_linear_grouped(gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], qs, [g["X"][-1] for g in gs],
                                     call, T, Y, [g["Q"] for g in gs], CC, DD, lr, h, S0s=S0, q_mode="intent", return_tracks=True)
    assert out["origins"].tolist() == origins and out["m_fc"].shape == (2, len(origins), h, D)
    rule("linearised M=300: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
    rule("linearised M=300: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))


def test_a_row_tile_boundary():
    """The 140-row record of tests/forecast_linear_ref.py (M = 24, D = 2, C = 1, two chains with q slices, "intent", a start
    covariance, row 7 unobserved, h = 2): with q slices a unit of the product is (group, dim) and its rows are the group's 138
    origins, so every unit has two row tiles, the second with 10 live rows -- one of its two wavefront rows is all padding.  The same
    call in passes of 50 origins (50, 50, 38: one row tile each) must give the same bits."""
    r = flr.long_record()
    gs, meta, h = r["gs"], r["meta"], r["h"]
    kern = _kernels(r["params"], meta)
    ref, e_ref = flr.reference(gs, r["ctrl"], r["Y"], r["CC"], r["DD"], r["sd"], r["qs"], r["S0"], r["mode"], r["origins"], h, WIDE)

    def call(**kw):
        return pr.forecast_linear_grouped(gs[0]["orc"]["L"], gs[0]["Z"], kern, [g["orc"]["U"] for g in gs], r["qs"], [g["X"][-1] for g in gs],
                                          r["call"], meta["T"], r["Y"], [g["Q"] for g in gs], r["CC"], r["DD"], r["lr"], h, S0s=r["S0"],
                                          q_mode=r["mode"], return_tracks=True, **kw)
    out = call()
    assert out["origins"].tolist() == r["origins"] and len(r["origins"]) == 138 and out["m_fc"].shape == (2, 138, h, meta["D"])
    rule("linearised long record: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
    rule("linearised long record: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    assert out["n_h"].tolist() == [[137], [137]]
    passes = call(tracks_per_pass=50)
    for k in out:
        np.testing.assert_array_equal(passes[k], out[k], err_msg=k)


# ---- 4. the pooled arrays and the horizon curves -------------------------------------------------------------------------------------
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
        print(f"linearised {shape} J={J}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    n_h = seen.sum(axis=0)
    np.testing.assert_array_equal(out["n_h"], n_h)
    assert out["n_h"].shape == (H, J) and np.issubdtype(out["n_h"].dtype, np.integer)
    assert n_h[:, 0].tolist() == ([6, 5, 4] if J == 3 else [7, 6, 5]) and np.all(n_h > 0)
    for k, src in (("rmse_h", None), ("ll_h", "lpd_mix"), ("ll_gauss_h", "lpd_gauss")):
        w = np.empty((H, J))
        for kk in range(H):
            for j in range(J):
                s = seen[:, kk, j]
                w[kk, j] = np.sqrt(np.mean((Yt[s, kk, j] - out["predict_y"][s, kk, j]) ** 2)) if src is None else np.mean(out[src][s, kk, j])
        tol, err = 1e-9 * (1.0 + float(np.max(np.abs(w)))), float(np.max(np.abs(out[k] - w)))
        print(f"linearised {shape} J={J}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert out[k].shape == (H, J) and np.all(np.isfinite(out[k])) and err <= tol, k
    np.testing.assert_array_equal(out["ll_h_original_units"], out["ll_h"])          # Y_train_std = 1


# ---- 5. fused with the posteriors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_forecast_linear_grouped against collapse_u_mean_grouped followed by forecast_linear_grouped, as
    tests/test_gpu_forecast_grouped.py::test_fused_form_against_the_two_calls: the reference is the restatement on the device's own
    posterior (np.longdouble where that is wider), the yardstick the two-call route.  Whether the bits coincide is printed."""
    mode = "reference"
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = observations(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])          # (data only: any posterior's will do)
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(q_mode=mode, return_tracks=True, return_filter=True)
    fused = pr.posterior_forecast_linear_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, H, **kw)
    assert set(fused) == FULL_KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.forecast_linear_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, meta["T"], Y, Qs, CC, DD, lr, H, **kw)
    print(f"linearised {shape}: fused and two-call routes bit-identical: "
          f"{all(np.array_equal(fused[k], two[k], equal_nan=True) for k in FULL_KEYS)}")
    t = np.longdouble if WIDE else np.float64
    ctrl = call[meta["T"]: meta["T"] + STEPS]
    for i, g in enumerate(gs):
        beta, Gam = mr.posterior_terms(Lm[i if per_model else 0], U[i], Hinv[i], mode, dtype=t)
        f = fr.filter(g["X"][-1], np.zeros((meta["D"],) * 2), Y, CC, DD, sd, g["Q"], lf.ekf_transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t),
                      dtype=t)
        tm, tS = flr.tracks(f, ORIGINS, H, Y.shape[1], CC, DD, sd, g["Q"], ctrl, g["Z"], g["okern"], beta, Gam, dtype=t)
        for k, key, ref in (("m_fc", "mean", tm), ("S_fc", "var", tS)):
            ref = ref.astype(np.float64)
            e_f, e_t = float(np.max(np.abs(fused[k][i] - ref))), float(np.max(np.abs(two[k][i] - ref)))
            bnd = max(4.0 * e_t, floor(key, ref))
            print(f"linearised {shape} group {i}: {k}: fused {e_f:.3e}, two calls {e_t:.3e}, bound {bnd:.3e}")
            assert np.all(np.isfinite(fused[k][i])) and e_f <= bnd, k
    np.testing.assert_array_equal(fused["S_fc"], np.swapaxes(fused["S_fc"], -1, -2))
    plain = pr.posterior_filter_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, q_mode=mode, method="linearised")
    for k in FILTER_KEYS:                                                           # the fused call's own filter is the fused filter's
        np.testing.assert_array_equal(fused[k], plain[k], err_msg=k)
    again = pr.posterior_forecast_linear_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, H, tracks_per_pass=2, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(again[k], fused[k], err_msg=k)


# ---- 6. model level: the actuator fixture with three chains --------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_forecast_heldout_linearised(actuator, U_collapse):
    """the curves of the two rules are printed side by side and not asserted"""
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
    out = mod.forecast_heldout_linearised(Yt, c, h, Y_train_std=1.7, return_tracks=True)
    assert set(out) == KEYS | {"m_fc", "S_fc"}
    assert out["origins"].tolist() == list(range(B)) and out["m_fc"].shape == (S, B, h, D) and out["S_fc"].shape == (S, B, h, D, D)
    assert all(out[k].shape == (B, h, J) for k in POOLED) and all(out[k].shape == (h, J) for k in CURVES)
    assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"])) and np.all(np.isfinite(out["predict_y"]))
    assert np.all(out["n_h"] > 0) and all(np.all(np.isfinite(out[k])) for k in CURVES)
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        direct = pr.posterior_forecast_linear_grouped(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, c, N_TRAIN, Yt, lik.CC,
                                                      lik.DD, lik.log_Rchols, h, Y_train_std=1.7, return_tracks=True)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        direct = pr.forecast_linear_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [mod._X_chains[s][-1] for s in range(S)], c, N_TRAIN, Yt,
                                            mod.Q, lik.CC, lik.DD, lik.log_Rchols, h, Y_train_std=1.7, return_tracks=True)
    again = mod.forecast_heldout_linearised(Yt, c, h, Y_train_std=1.7, return_tracks=True)
    for k in out:
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    mm = mod.forecast_heldout(Yt, c, h, Y_train_std=1.7, return_tracks=True)
    assert float(np.max(np.abs(mm["m_fc"] - out["m_fc"]))) > 0.0
    print(f"U_collapse={U_collapse}: horizons 1 .. {h}: linearised rmse_h {np.round(out['rmse_h'][:, 0], 6).tolist()}, "
          f"ll_h {np.round(out['ll_h'][:, 0], 6).tolist()}; moment matching rmse_h {np.round(mm['rmse_h'][:, 0], 6).tolist()}, "
          f"ll_h {np.round(mm['ll_h'][:, 0], 6).tolist()}; n_h {out['n_h'][:, 0].tolist()}")


# ---- 7. the moment fan is what it was ------------------------------------------------------------------------------------------------
def test_the_moment_forecasts_keep_their_default_and_still_refuse_the_linearised_method():
    args = CASES[1]
    cs = case(*args[:3])
    Y, em, S0 = observations(*args)[0], emission(cs, args[5]), _S0(cs, True)
    kw = dict(return_tracks=True, return_filter=True)
    default, moment = run_forecast(cs, args[3], args[4], Y, em, S0, **kw), run_forecast(cs, args[3], args[4], Y, em, S0, method="moment", **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(default[k], moment[k], err_msg=k)
    with pytest.raises(ValueError, match="method"):
        run_forecast(cs, args[3], args[4], Y, em, S0, method="linearised")
    lin = device(*args)
    diff = float(np.max(np.abs(lin["m_fc"] - default["m_fc"])))
    print(f"largest |m_fc(linearised) - m_fc(moment)| {diff:.3e}")
    assert diff > floor("mean", default["m_fc"])
