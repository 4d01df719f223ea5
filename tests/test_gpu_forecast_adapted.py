"""Rolling-origin forecasts on the adapted particle filter's sets on the device: prediction.forecast_adapted_grouped
(`ffvd_particle_adapted_forecast_grouped`), fused with the collapsed posteriors (prediction.posterior_forecast_adapted_grouped,
`ffvd_posterior_particle_adapted_forecast_grouped`) and DGPSSM.forecast_heldout_adapted.

Fixtures (tests/forecast_adapted_fixtures.py): two of the bootstrap fan's cases with one model per group (three groups, N = 48) and
four small ones that cross the state kernel's edges in N (2, 8, 257, 2048) at D = 1, 2 and 4, J = 1 and 2, with and without start
covariances, collapsed and explicit U, both q modes; tests/width_fixtures.py for D = 5, 6, 7, 8, J = 8 and P = 32.

Reference and rule.  tests/forecast_adapted_ref.py (pinned in tests/test_forecast_adapted_ref.py) in fp64 on the oracle's posterior;
e_ref is that reference against the same composition in np.longdouble.  Every fixture satisfies the margin condition of
tests/particle_filter_ref.py on its filter stage (identical ancestors in both precisions and gap >= max(1e-8, 1000 x drift)); a track
itself resamples nothing.  error <= max(4 e_ref, floor) with `rule` and the floors of tests/test_gpu_moment_grouped.py, as
tests/test_gpu_forecast_particle.py applies them to the same quantities: 1e-11 + 1e-9 max|ref| on m_fc and fc_particles, 1e-11 + 1e-8
max|ref| on S_fc and lpd_fc.  The identities with the adapted records filter are bit for bit.  Every measured error is printed;
DESIGN.md section 9, "Adapted particle forecasts", has the largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import adapted_fan_poison_script as script
import adapted_particle_fixtures as afx
import forecast_adapted_fixtures as fax
import forecast_adapted_ref as far
import width_fixtures as wf
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.prediction import forecast_adapted_grouped, posterior_forecast_adapted_grouped  # noqa: F401  (without them nothing here runs)
from test_gpu_filter_grouped import POOLED
from test_gpu_filter_records import judge
from test_gpu_forecast_particle import CURVES, FILTER, FULL_KEYS, KEYS, KIND, SCALARS, TRACKS
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, TEST_LEN, WIDE, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

NAN = np.nan
H = fax.H
NAMES = list(fax.CASES) + sorted(fax.SMALL)
JUDGED = ("m_pred", "S_pred", "m_filt", "S_filt", "lpd", "lpd_joint")


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture, shared by the checks below (never modified)."""
    return fax.call(fax.fixture(name))


def targets(fx):
    return fx["Y"][0][fx["origins"][:, None] + 1 + np.arange(fx["h"])[None, :]]            # (B, h, J)


def against_the_reference(what, out, ref, e_ref, fx):
    for k in TRACKS:
        assert out[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)       # NaN exactly where the reference has it
        ok = ~np.isnan(ref[k])
        rule(f"{what}: {k}", KIND[k], out[k][ok], ref[k][ok], e_ref[k])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    np.testing.assert_array_equal(np.isnan(out["lpd_fc"]), np.broadcast_to(np.isnan(targets(fx))[None], out["lpd_fc"].shape))
    # the filter stage: the reference's arrays with the record axis dropped
    flt = {k: v[:, 0] for k, v in ref["filter"].items()}
    judge(what, out, flt, e_ref, keys=JUDGED)
    n = flt["particles"].shape[-2]
    rule(f"{what}: ess / N", "var", out["ess"] / n, flt["ess"] / n, e_ref["ess"] / n)


# ---- 1: parity with the NumPy reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fax.SMALL))
def test_the_filter_stage_of_every_small_fixture_does_not_hang_on_rounding(name):
    """(the two CASES: tests/test_gpu_filter_adapted.py asserts it on the same record and draws)"""
    gap, drift, same, ok = fax.margin_holds(name)
    print(f"{name}: smallest gap {gap:.3e}, cdf drift between the precisions {drift:.3e}, identical ancestors {same}")
    assert ok


@pytest.mark.parametrize("name", NAMES, ids=str)
def test_tracks_and_filter_against_the_reference(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Adapted particle forecasts"."""
    fx, out = fax.fixture(name), device(name)
    ref, e_ref, _ = fax.reference(name)
    G, D, N, J, B = len(fx["gs"]), fx["x0"].shape[-1], fx["eps"].shape[-2], fx["Y"].shape[-1], len(fx["origins"])
    assert set(out) == FULL_KEYS and out["origins"].tolist() == fx["origins"].tolist()
    assert out["m_fc"].shape == (G, B, H, D) and out["S_fc"].shape == (G, B, H, D, D) and out["lpd_fc"].shape == (G, B, H, J)
    assert out["fc_particles"].shape == (G, B, H, N, D)
    what = f"adapted fan {name}"
    against_the_reference(what, out, ref, e_ref, fx)
    # the ancestors of the filter stage are the reference's (the fan call returns none: the same draws through the records call)
    flt = afx.call(fx)
    assert flt["ancestors"].dtype == np.int32
    np.testing.assert_array_equal(flt["ancestors"], ref["filter"]["ancestors"])
    # lpd_mix of the forecast is the mixture over the groups of the device's own lpd_fc
    lp = out["lpd_fc"]
    with np.errstate(invalid="ignore"):
        mx = np.max(lp, axis=0)
        want = mx + np.log(np.mean(np.exp(lp - mx[None]), axis=0))
    np.testing.assert_array_equal(np.isnan(out["lpd_mix"]), np.isnan(targets(fx)))
    ok = ~np.isnan(want)
    err, tol = float(np.max(np.abs(out["lpd_mix"][ok] - want[ok]))), 1e-9 * (1.0 + float(np.max(np.abs(want[ok]))))
    print(f"{what}: lpd_mix: max error {err:.3e}, tolerance {tol:.3e}; ll_h {np.round(out['ll_h'][:, 0], 5).tolist()}")
    assert err <= tol


# ---- 2: the truncation identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES, ids=str)
def test_a_track_is_the_adapted_records_filter_over_the_cut_record_bit_for_bit(name):
    """m_fc, S_fc, fc_particles of track (g, b) are m_pred, S_pred, particles at rows o + 1 .. o + h of filter_adapted_records_grouped
    over R = B records, record b being rows 0 .. o_b followed by h all-NaN rows with the draws concat(eps[:o + 1], eps_fc[g, b]).  Every
    fixture has its first admissible origin (0), interior ones and its last admissible one (n - h - 1)."""
    fx, out = fax.fixture(name), device(name)
    n = fx["Y"].shape[1]
    assert len(fx["origins"]) >= 3 and fx["origins"][0] == 0 and fx["origins"][-1] == n - H - 1
    flt = afx.call(fax.composed(fx))
    for b, o in enumerate(fx["origins"]):
        rows = slice(int(o) + 1, int(o) + 1 + H)
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("fc_particles", "particles")):
            np.testing.assert_array_equal(out[mine][:, b], flt[theirs][:, b, rows], err_msg=f"{mine}, origin {o}")


# ---- 3: the first row is the filter's own prediction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d2_n8", "d4_n257", fax.CASES[0]], ids=str)
def test_the_first_row_of_every_track_is_the_filters_prediction_of_the_next_row_bit_for_bit(name):
    """Every origin o with o + 1 < n that the fan admits at h = 1 (all but the last row), in one call with return_filter:
    m_fc[:, b, 0], S_fc[:, b, 0], fc_lpd[:, b, 0] against m_pred[:, o + 1], S_pred[:, o + 1], lpd[:, o + 1].  The records have entries
    missing in some outputs and a wholly unobserved row, as a target and as an origin."""
    fx = fax.fixture(name)
    n = fx["Y"].shape[1]
    org = np.arange(n - 1)
    Y = fx["Y"][0]
    assert np.isnan(Y).all(axis=1).any() and (np.isnan(Y).any(axis=1) & ~np.isnan(Y).all(axis=1)).any()
    rng = np.random.default_rng(77)
    efc = rng.standard_normal((1, fx["eps"].shape[-2], fx["x0"].shape[-1]))
    out = fax.call(dict(fx, h=1, origins=org), eps_fc=efc)
    for b, o in enumerate(org):
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("lpd_fc", "lpd")):
            np.testing.assert_array_equal(out[mine][:, b, 0], out[theirs][:, o + 1], err_msg=f"{mine}, origin {o}")
    # and at the fixture's own horizon: the first row of its tracks
    own = device(name)
    for b, o in enumerate(fx["origins"]):
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("lpd_fc", "lpd")):
            np.testing.assert_array_equal(own[mine][:, b, 0], own[theirs][:, int(o) + 1], err_msg=f"{mine}, origin {o}")


# ---- 4: the filter stage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES, ids=str)
def test_the_filter_keys_are_the_adapted_records_call_with_one_record_bit_for_bit(name):
    fx, out = fax.fixture(name), device(name)
    flt = afx.call(fx, return_particles=False)
    for k in FILTER:
        assert flt[k].shape[1] == 1 and out[k].shape == flt[k][:, 0].shape, k
        np.testing.assert_array_equal(out[k], flt[k][:, 0], err_msg=k)
    for k in SCALARS:
        np.testing.assert_array_equal(out[k], flt[k] if k == "ll_all" else flt[k][0], err_msg=k)
    for k in POOLED:
        np.testing.assert_array_equal(out["filter_" + k], flt[k][0], err_msg=k)


# ---- 5: independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d2_n8", "d4_n257", fax.CASES[1]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_origins_or_the_pass(name):
    """d2_n8: explicit U (one shared Gamma: a unit is a dim and its rows are those of all tracks of the pass); d4_n257 and the case:
    q slices (unit = (group, dim))."""
    fx, a = fax.fixture(name), device(name)
    G, B = len(fx["gs"]), len(fx["origins"])
    pick = sorted({0, B // 2, B - 1})
    for g in range(G):                                                              # a group alone
        one = fax.call(fax.subset(fx, groups=[g]))
        for k in TRACKS + FILTER:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for i in pick:                                                                  # an origin alone
        one = fax.call(fax.subset(fx, origins=[i]))
        assert one["origins"].tolist() == [int(fx["origins"][i])]
        for k in TRACKS:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, i], err_msg=f"{k}, origin {fx['origins'][i]}")
        for k in POOLED:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=f"{k}, origin {fx['origins'][i]}")
    # the draws permuted over the origins: the pair (origin, draws) decides a track, not its place in the call
    rev = fax.call(dict(fx, eps_fc=np.ascontiguousarray(fx["eps_fc"][:, ::-1])))
    for i in pick:
        one = fax.call(dict(fax.subset(fx, origins=[i]), eps_fc=np.ascontiguousarray(fx["eps_fc"][:, [B - 1 - i]])))
        for k in TRACKS:
            np.testing.assert_array_equal(one[k][:, 0], rev[k][:, i], err_msg=f"{k}, origin {fx['origins'][i]}, draws of place {B - 1 - i}")
    assert float(np.max(np.abs(rev["fc_particles"] - a["fc_particles"]))) > 0.0
    np.testing.assert_array_equal(rev["m_fc"][:, :, 0], a["m_fc"][:, :, 0])          # (no draw enters the first row)
    for tpp in (1, 2):                                                              # passes of 1 and of 2 origins
        p = fax.call(fx, tracks_per_pass=tpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, tracks_per_pass {tpp}")


@pytest.mark.parametrize("name", ["d2_n8", "d1_n2"])
def test_shared_draws_are_the_same_draws_broadcast(name):
    """eps_fc (h, N, D) and (B, h, N, D), eps (steps, N, D), unif (steps,), xi0 (N, D) -- stride 0 -- against the same draws
    materialised in the full layouts: bit for bit in every key."""
    fx = fax.fixture(name)
    G, B = len(fx["gs"]), len(fx["origins"])
    full = lambda v, lead: None if v is None else np.ascontiguousarray(np.broadcast_to(v, lead + v.shape))
    one = lambda v: None if v is None else v[0, 0]
    eps, unif, xi0 = one(fx["eps"]), one(fx["unif"]), one(fx["xi0"])
    for efc, lead in ((fx["eps_fc"][0, 0], (G, B)), (fx["eps_fc"][0], (G,))):
        small = fax.call(fx, eps=eps, unif=unif, xi0=xi0, eps_fc=efc)
        big = fax.call(fx, eps=full(eps, (G,)), unif=full(unif, (G,)), xi0=full(xi0, (G,)), eps_fc=full(efc, lead))
        for k in small:
            np.testing.assert_array_equal(small[k], big[k], err_msg=k)


# ---- 6: not the bootstrap fan -------------------------------------------------------------------------------------------------------------
def test_the_rows_differ_from_the_bootstrap_fans_on_the_same_draws():
    """d4_n257 (the second output's noise, sd = 0.05, is well below the spread of the prediction: informative observations): the
    adapted rows are the Rao-Blackwellised ones from the adapted filter's sets, the bootstrap fan's are plain particle moments from
    the bootstrap filter's.  Guards against the symbol being wired to the old rule."""
    fx = fax.fixture("d4_n257")
    a, b = device("d4_n257"), fax.call(fx, fn=pr.forecast_particle_grouped)
    assert set(a) == set(b) and all(np.shape(a[k]) == np.shape(b[k]) for k in a)
    d = float(np.max(np.abs(a["m_fc"] - b["m_fc"])))
    print(f"adapted against bootstrap fan: largest |m_fc difference| {d:.3e}; smallest ess {a['ess'].min():.1f} against {b['ess'].min():.1f}")
    assert d > 1e-6
    assert float(np.max(np.abs(a["fc_particles"] - b["fc_particles"]))) > 1e-6


# ---- 7: poisoned scratch -----------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/adapted_fan_poison_script.py in one fresh child process each without and with FFVD_OP_CACHE_POISON: every output bit for
    bit, the reversed pass (each call after a history of the others) as the forward one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"adapted_fan{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, _ in script.CALLS:
        assert set(script.SYMBOLS) == set(clean["called/" + label].tolist()), label
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) > 15 * len(script.CALLS)
    for k in results:
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
        if k.startswith("fwd/"):
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)


# ---- 8: the widths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5", "d6", "d7", "p32"])
def test_widths(name):
    """tests/width_fixtures.py, record 0, origins (0, 1, 2), h = 3, N = 48: D = 5, 6, 7 and 8, J = 8 everywhere, P = 32 at p32 (whose
    margin condition under the adapted filter tests/test_width_fixtures.py asserts without a GPU)."""
    w = wf.fixture(name)
    org = np.arange(wf.STEPS - wf.H)
    cut = lambda x: None if x is None else x[:, :1]
    fx = dict(w, Y=w["Y"][:1], ctrl=None if w["ctrl"] is None else w["ctrl"][:1], x0=cut(w["x0"]), S0=cut(w["S0"]), eps=cut(w["eps"]),
              unif=cut(w["unif"]), xi0=cut(w["xi0"]), lengths=np.array([wf.STEPS]), h=wf.H, origins=org)
    out = fax.call(fx)
    ref, e_ref, _ = fax.reference_of(fx)
    D = fx["x0"].shape[-1]
    assert out["m_fc"].shape == (2, len(org), wf.H, D) and out["lpd_fc"].shape == (2, len(org), wf.H, wf.J)
    against_the_reference(f"adapted fan {name}", out, ref, e_ref, fx)
    for b, o in enumerate(org):                                                     # the first row: the filter's prediction
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("lpd_fc", "lpd")):
            np.testing.assert_array_equal(out[mine][:, b, 0], out[theirs][:, o + 1], err_msg=f"{mine}, origin {o}")


# ---- fused with the posteriors ---------------------------------------------------------------------------------------------------------
def test_fused_form_against_the_two_calls():
    """posterior_forecast_adapted_grouped is collapse_u_mean_grouped followed by forecast_adapted_grouped on every key, bit for bit"""
    args = fax.CASES[1]
    shape, per_model, G = args[:3]
    cs, fx = case(shape, per_model, G), fax.fixture(args)
    gs, call = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    T = cs[2]["T"]
    one = lambda x: None if x is None else x[:, 0]
    kw = dict(xi0=one(fx["xi0"]), origins=fx["origins"], S0s=one(fx["S0"]), q_mode="reference", return_tracks=True, return_filter=True,
              return_particles=True)
    draws = (one(fx["eps"]), one(fx["unif"]), fx["eps_fc"])
    fused = pr.posterior_forecast_adapted_grouped(Zs, kerns, Xs, Qs, call, T, fx["Y"][0], CC, DD, lr, H, *draws, **kw)
    assert set(fused) == FULL_KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.forecast_adapted_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, T, fx["Y"][0], Qs, CC, DD, lr, H,
                                      *draws, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    assert np.all(np.isfinite(fused["m_fc"])) and np.all(np.isfinite(fused["S_fc"]))
    np.testing.assert_array_equal(fused["S_fc"], np.swapaxes(fused["S_fc"], -1, -2))


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
def test_forecast_heldout_adapted(actuator):
    """N = 64: the keys and shapes of forecast_heldout_particle, finite curves, the same seed twice the same bits.  The ll_h curves of
    the five rules are printed side by side and not asserted."""
    params, Y, c = actuator
    m = _regression_model(params, c, True)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = np.array(Y[N_TRAIN:N_TRAIN + TEST_LEN])
    Yt[7] = NAN
    h = 5
    kw = dict(Y_train_std=1.7, return_tracks=True)
    out = mod.forecast_heldout_adapted(Yt, c, h, num_particles=64, seed=7, **kw)
    boot = mod.forecast_heldout_particle(Yt, c, h, num_particles=64, seed=7, **kw)
    assert set(out) == set(boot) == KEYS | {"m_fc", "S_fc"}
    assert all(np.shape(out[k]) == np.shape(boot[k]) for k in out) and out["origins"].tolist() == boot["origins"].tolist()
    assert np.all(np.isfinite(out["ll_h"])) and np.all(np.isfinite(out["rmse_h"])) and np.all(out["n_h"] > 0)
    assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"]))
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    again = mod.forecast_heldout_adapted(Yt, c, h, num_particles=64, seed=7, **kw)
    for k in out:
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    assert float(np.max(np.abs(out["m_fc"] - boot["m_fc"]))) > 0.0
    rules = (("adapted (N = 64)", out), ("particle (N = 64)", boot), ("moment matching", mod.forecast_heldout(Yt, c, h, **kw)),
             ("linearised", mod.forecast_heldout_linearised(Yt, c, h, **kw)), ("cubature", mod.forecast_heldout_cubature(Yt, c, h, **kw)))
    for name, o in rules:
        print(f"horizons 1 .. {h}: {name} ll_h {np.round(o['ll_h'][:, 0], 6).tolist()}, rmse_h {np.round(o['rmse_h'][:, 0], 6).tolist()}")
