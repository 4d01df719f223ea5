"""Rolling-origin multi-step forecasts under the third-degree spherical cubature rule on the device: prediction.forecast_cubature_grouped
(`ffvd_op_forecast_cubature_grouped`), fused with the collapsed posteriors (prediction.posterior_forecast_cubature_grouped,
`ffvd_op_posterior_forecast_cubature_grouped`) and DGPSSM.forecast_heldout_cubature.

Fixtures.  The seven cases, the 12-row record with its gaps, H = 3 and origins 0 .. 8 of tests/test_gpu_forecast_grouped.py, with its
helpers imported: `run_forecast` there takes no rule, `run_cubature_forecast` hands it the cubature function in place of
`pr.forecast_grouped` for the duration of the call (the indirection of tests/test_gpu_forecast_linear.py; should the sibling ever bind
the function at import the patch would do nothing, and the accuracy tests and the comparison with the cubature filter fail then).
Three fixtures reach tile edges that the shared cases do not (tests/test_forecast_cubature_ref.py builds them without a device and
shows that the reference's own S_fc is positive definite on each, which is why positivity is asserted here): M = 300 (a ragged last
column tile of the product, a second stride of the state kernel), D = 3 with 24 origins (6 rows of K per track: track 21 straddles the
128-row tile) in both unit layouts, and the 140-row record of tests/forecast_linear_ref.py (552 rows per unit: five row tiles).

Reference and rule.  tests/forecast_cubature_ref.py (pinned in tests/test_forecast_cubature_ref.py) in fp64 on the oracle's posterior;
e_ref is that reference against the same composition in np.longdouble; the device must satisfy error <= max(4 e_ref, floor) with
`rule` and the floors of tests/test_gpu_moment_grouped.py.  Every measured error is printed; DESIGN.md section 9, "Cubature
forecasts", has the largest."""
import functools
from unittest import mock

import numpy as np
import pytest

import forecast_linear_ref as flr
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_forecast_cubature_ref import cpu_case, cpu_observations, d3_record, m300_record, record_reference, shared_reference
from test_gpu_conditional_grouped import _kernels, floor
from test_gpu_filter_grouped import CASES, POOLED, emission, observations
from test_gpu_forecast_grouped import CURVES, FILTER_KEYS, FULL_KEYS, H, KEYS, ORIGINS, _S0, _posteriors, run_forecast
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, TEST_LEN, WIDE, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

NAN = np.nan
SCALARS = ("ll", "ll_joint", "ll_original_units", "RMSE")


def run_cubature_forecast(*args, **kw):
    """`run_forecast` of tests/test_gpu_forecast_grouped.py with the cubature function under the name it looks up at call time"""
    with mock.patch.object(pr, "forecast_grouped", pr.forecast_cubature_grouped):
        return run_forecast(*args, **kw)


def bound(key, ref, e_ref):
    """the rule's bound for an array: max(4 e_ref, floor), the floor alone where np.longdouble is no wider"""
    return max(4.0 * e_ref, floor(key, ref)) if WIDE else floor(key, ref)


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case (every origin, tracks and the filter's outputs), shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    Y, _ = observations(shape, per_model, G, qkind, mode, J, with_S0)
    return run_cubature_forecast(cs, qkind, mode, Y, emission(cs, J), _S0(cs, with_S0), return_tracks=True, return_filter=True)


@functools.lru_cache(maxsize=None)
def forecast_refs(shape, per_model, G, qkind, mode, J, with_S0):
    """The reference of a case and its own error, on the fixture as tests/test_forecast_cubature_ref.py restates it without a device --
    which must be the fixture the device runs on.  Computed once per case, never modified."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, cpu = case(shape, per_model, G), cpu_case(shape, per_model, G)
    np.testing.assert_array_equal(cpu_observations(*args)[0], observations(*args)[0])
    np.testing.assert_array_equal(cpu[1], cs[1])
    for a, b in zip(cpu[0], cs[0]):
        np.testing.assert_array_equal(a["orc"]["U"], b["orc"]["U"])
        np.testing.assert_array_equal(a["orc"]["H"], b["orc"]["H"])
    return shared_reference(args, WIDE)


def one_record_filter(cs, qkind, mode, Y, em, S0):
    """filter_cubature_records_grouped with R = 1 on the inputs of `run_forecast`"""
    call, meta = cs[1], cs[2]
    idx, sel, post = _posteriors(cs, qkind)
    T = meta["T"]
    ctrl = call[T: T + STEPS][None] if meta["C"] else None
    return pr.filter_cubature_records_grouped(*post, np.stack([g["X"][-1] for g in sel])[:, None, :], ctrl, Y[None], [g["Q"] for g in sel], *em,
                                              S0s=None if S0 is None else S0[idx][:, None], q_mode=mode)


# ---- 1. accuracy, symmetry; 2. the call's own filter, horizon 1 -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Cubature forecasts"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, (ref, e_ref) = case(shape, per_model, G), device(*args), forecast_refs(*args)
    what = f"cubature {shape} q={qkind} {mode} J={J}"
    nG, D = len(cs[0]), cs[2]["D"]
    assert set(out) == FULL_KEYS and out["origins"].tolist() == ORIGINS
    assert out["m_fc"].shape == ref["m"].shape == (nG, len(ORIGINS), H, D) and out["S_fc"].shape == ref["S"].shape
    rule(f"{what}: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
    rule(f"{what}: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    low = float(np.min(np.linalg.eigvalsh(out["S_fc"])))
    print(f"{what}: smallest eigenvalue of S_fc {low:.3e} (the reference's {float(np.min(np.linalg.eigvalsh(ref['S']))):.3e})")
    assert low > 0.0
    # the call's own filter is filter_cubature_records_grouped with R = 1 bit for bit, record axis squeezed
    flt = one_record_filter(cs, qkind, mode, observations(*args)[0], emission(cs, J), _S0(cs, with_S0))
    for k in FILTER_KEYS:
        assert flt[k].shape[1] == 1, k
        np.testing.assert_array_equal(out[k], flt[k][:, 0], err_msg=k)
    for k in SCALARS:
        np.testing.assert_array_equal(out[k], flt[k][0], err_msg=k)
    for k in POOLED:
        np.testing.assert_array_equal(out["filter_" + k], flt[k][0], err_msg=k)
    # horizon 1 against the filter's own prediction of the next row: both lie within the rule's bound of one reference, so they are
    # within twice that bound; two kernels may contract differently, so the bits are reported and not asserted
    rows = [i + 1 for i in ORIGINS]
    dm = float(np.max(np.abs(out["m_fc"][:, :, 0] - out["m_pred"][:, rows])))
    dS = float(np.max(np.abs(out["S_fc"][:, :, 0] - out["S_pred"][:, rows])))
    bm, bS = 2.0 * bound("mean", ref["m"], e_ref["m"]), 2.0 * bound("var", ref["S"], e_ref["S"])
    same = np.array_equal(out["m_fc"][:, :, 0], out["m_pred"][:, rows]) and np.array_equal(out["S_fc"][:, :, 0], out["S_pred"][:, rows])
    print(f"{what}: horizon 1 against the filter's m_pred {dm:.3e} (2 x bound {bm:.3e}), S_pred {dS:.3e} (2 x bound {bS:.3e}), "
          f"bit-identical: {same}")
    assert dm <= bm and dS <= bS


# ---- 3. determinism and independence of the decomposition ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_results_do_not_depend_on_the_call_the_groups_the_origins_or_the_pass_size(shape, per_model, G, qkind, mode, J, with_S0):
    """a track must not depend on the other rows of its tile, on the other groups or on the pass it is in"""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a = case(shape, per_model, G), device(*args)
    Y, em, S0 = observations(*args)[0], emission(cs, J), _S0(cs, with_S0)
    kw = dict(return_tracks=True, return_filter=True)
    b = run_cubature_forecast(cs, qkind, mode, Y, em, S0, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(len(cs[0])):                                                     # a group alone
        one = run_cubature_forecast(cs, qkind, mode, Y, em, S0, groups=[g], return_tracks=True)
        np.testing.assert_array_equal(one["m_fc"][0], a["m_fc"][g], err_msg=f"group {g}")
        np.testing.assert_array_equal(one["S_fc"][0], a["S_fc"][g], err_msg=f"group {g}")
    for i in (0, 5, 8):                                                             # an origin alone
        one = run_cubature_forecast(cs, qkind, mode, Y, em, S0, origins=[i], return_tracks=True)
        assert one["origins"].tolist() == [i]
        for k in ("m_fc", "S_fc"):
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, i], err_msg=f"{k}, origin {i}")
        for k in POOLED:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=f"{k}, origin {i}")
    for tpp in (1, 2, 4):                                                           # passes of 1, 2 (a ragged last pass) and 4 origins
        p = run_cubature_forecast(cs, qkind, mode, Y, em, S0, tracks_per_pass=tpp, **kw)
        for k in FULL_KEYS:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, tracks_per_pass {tpp}")
    some = run_cubature_forecast(cs, qkind, mode, Y, em, S0, origins=[0, 4, 8], return_tracks=True)
    strided = run_cubature_forecast(cs, qkind, mode, Y, em, S0, stride=4, return_tracks=True, tracks_per_pass=2)
    for o in (some, strided):
        assert o["origins"].tolist() == [0, 4, 8]
        for k in ("m_fc", "S_fc"):
            np.testing.assert_array_equal(o[k], a[k][:, [0, 4, 8]], err_msg=k)
        for k in POOLED:
            np.testing.assert_array_equal(o[k], a[k][[0, 4, 8]], err_msg=k)


# ---- 4. tile edges the shared cases do not reach -------------------------------------------------------------------------------------
def _record_call(r, slices=True, groups=(0, 1), **kw):
    """the explicit call on a record of tests/test_forecast_cubature_ref.py (two chains of one model, the oracle's posterior)"""
    gs, meta = [r["gs"][g] for g in groups], r["meta"]
    return pr.forecast_cubature_grouped(gs[0]["orc"]["L"], gs[0]["Z"], _kernels(r["params"], meta), [g["orc"]["U"] for g in gs],
                                        [r["qs"][g] for g in groups] if slices else None, [g["X"][-1] for g in gs], r["call"], meta["T"], r["Y"],
                                        [g["Q"] for g in gs], r["CC"], r["DD"], r["lr"], r["h"], S0s=r["S0"][list(groups)], q_mode=r["mode"],
                                        return_tracks=True, **kw)


def _judge_record(what, out, ref, e_ref):
    rule(f"{what}: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
    rule(f"{what}: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    low = float(np.min(np.linalg.eigvalsh(out["S_fc"])))
    print(f"{what}: smallest eigenvalue of S_fc {low:.3e} (the reference's {float(np.min(np.linalg.eigvalsh(ref['S']))):.3e})")
    assert low > 0.0


def test_a_ragged_last_column_tile():
    """M = 300: Mp = 320, three column tiles of the product, the last 64 wide, and a second stride of 256 columns in the state kernel.
    Two chains of one model, q slices, a start covariance, six rows with a gap; h = 2, origins 0 .. 3."""
    r = m300_record()
    ref, e_ref = record_reference(r, WIDE)
    out = _record_call(r)
    assert out["origins"].tolist() == r["origins"] and out["m_fc"].shape == (2, 4, 2, r["meta"]["D"])
    _judge_record("cubature M=300", out, ref, e_ref)


@pytest.mark.parametrize("slices", [True, False], ids=["q slices", "no q slices"])
def test_a_track_that_straddles_a_row_tile(slices):
    """D = 3 ("ragged": M = 77, C = 2, two chains of one model, "intent"), a 26-row record, h = 2, origins 0 .. 23: a track brings 6
    rows of K, which do not divide 128.  With q slices a unit is (group, dim) with 144 rows: rows 126 .. 131 of track 21 lie in two row
    tiles, the second tile has 16 live rows.  Without them a unit is a dim with the 288 rows of all tracks (three row tiles; track 21
    of group 0 and track 18 of group 1, rows 252 .. 257, straddle).  Passes of 10 origins (10, 10, 4: one row tile per (group, dim)
    unit) and the last origin alone must give the same bits."""
    r = d3_record()
    ref, e_ref = record_reference(r, WIDE, slices)
    out = _record_call(r, slices)
    assert out["origins"].tolist() == list(range(24)) and out["m_fc"].shape == (2, 24, 2, 3)
    _judge_record(f"cubature D=3, 24 origins, q slices {slices}", out, ref, e_ref)
    passes = _record_call(r, slices, tracks_per_pass=10)
    for k in out:
        np.testing.assert_array_equal(passes[k], out[k], err_msg=k)
    alone = _record_call(r, slices, origins=[23])
    for k in ("m_fc", "S_fc"):
        np.testing.assert_array_equal(alone[k][:, 0], out[k][:, 23], err_msg=k)
    for k in POOLED:
        np.testing.assert_array_equal(alone[k][0], out[k][23], err_msg=k)


def test_five_row_tiles():
    """The 140-row record of tests/forecast_linear_ref.py (M = 24, D = 2, C = 1, two chains with q slices, "intent", a start
    covariance, row 7 unobserved, h = 2): 4 rows of K per track and 138 origins give every (group, dim) unit 552 rows, so five row
    tiles, the last with 40 live rows.  Passes of 50 origins (200, 200, 152 rows: two row tiles each) must give the same bits."""
    r = flr.long_record()
    ref, e_ref = record_reference(r, WIDE)
    out = _record_call(r)
    assert out["origins"].tolist() == r["origins"] and len(r["origins"]) == 138 and out["m_fc"].shape == (2, 138, 2, 2)
    _judge_record("cubature long record", out, ref, e_ref)
    assert out["n_h"].tolist() == [[137], [137]]
    passes = _record_call(r, tracks_per_pass=50)
    for k in out:
        np.testing.assert_array_equal(passes[k], out[k], err_msg=k)


# ---- 5. fused with the posteriors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_forecast_cubature_grouped is collapse_u_mean_grouped followed by forecast_cubature_grouped on every key, bit for bit:
    the posterior the fused call forms is the one the two-call route downloads and uploads again."""
    mode = "reference"
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, _ = observations(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])            # (data only: any posterior's will do)
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(q_mode=mode, return_tracks=True, return_filter=True)
    fused = pr.posterior_forecast_cubature_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, H, **kw)
    assert set(fused) == FULL_KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.forecast_cubature_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, meta["T"], Y, Qs, CC, DD, lr, H, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    assert np.all(np.isfinite(fused["m_fc"])) and np.all(np.isfinite(fused["S_fc"]))
    np.testing.assert_array_equal(fused["S_fc"], np.swapaxes(fused["S_fc"], -1, -2))
    again = pr.posterior_forecast_cubature_grouped(Zs, kerns, Xs, Qs, call, meta["T"], Y, CC, DD, lr, H, tracks_per_pass=2, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(again[k], fused[k], err_msg=k)


# ---- 6. model level: the actuator fixture with three chains --------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_forecast_heldout_cubature(actuator, U_collapse):
    """the curves of the three rules are printed side by side and not asserted; the other two model-level calls are still their
    prediction-level calls"""
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
    kw = dict(Y_train_std=1.7, return_tracks=True)
    out = mod.forecast_heldout_cubature(Yt, c, h, **kw)
    assert set(out) == KEYS | {"m_fc", "S_fc"}
    assert out["origins"].tolist() == list(range(B)) and out["m_fc"].shape == (S, B, h, D) and out["S_fc"].shape == (S, B, h, D, D)
    assert all(out[k].shape == (B, h, J) for k in POOLED) and all(out[k].shape == (h, J) for k in CURVES)
    assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"])) and np.all(np.isfinite(out["predict_y"]))
    assert np.all(out["n_h"] > 0) and all(np.all(np.isfinite(out[k])) for k in CURVES)
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        def direct(fn):
            return fn(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, c, N_TRAIN, Yt, lik.CC, lik.DD, lik.log_Rchols, h, **kw)
        rules = (pr.posterior_forecast_cubature_grouped, pr.posterior_forecast_grouped, pr.posterior_forecast_linear_grouped)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)

        def direct(fn):
            return fn(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [mod._X_chains[s][-1] for s in range(S)], c, N_TRAIN, Yt, mod.Q, lik.CC, lik.DD,
                      lik.log_Rchols, h, **kw)
        rules = (pr.forecast_cubature_grouped, pr.forecast_grouped, pr.forecast_linear_grouped)
    mm, lin = mod.forecast_heldout(Yt, c, h, **kw), mod.forecast_heldout_linearised(Yt, c, h, **kw)
    again = mod.forecast_heldout_cubature(Yt, c, h, **kw)
    for got, fn in zip((out, mm, lin), rules):
        want = direct(fn)
        assert set(got) == set(want)
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{fn.__name__}: {k}")
    for k in out:
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    d_c, d_l = float(np.max(np.abs(mm["m_fc"] - out["m_fc"]))), float(np.max(np.abs(mm["m_fc"] - lin["m_fc"])))
    assert d_c > 0.0
    for name, o in (("cubature", out), ("linearised", lin), ("moment matching", mm)):
        print(f"U_collapse={U_collapse}: horizons 1 .. {h}: {name} rmse_h {np.round(o['rmse_h'][:, 0], 6).tolist()}, "
              f"ll_h {np.round(o['ll_h'][:, 0], 6).tolist()}")
    print(f"U_collapse={U_collapse}: n_h {out['n_h'][:, 0].tolist()}; largest |m_fc - m_fc(moment)|: cubature {d_c:.3e}, linearised {d_l:.3e}")
