"""Rolling-origin forecasts by particles on the device: prediction.forecast_particle_grouped (`ffvd_op_forecast_particle_grouped`),
fused with the collapsed posteriors (prediction.posterior_forecast_particle_grouped, `ffvd_op_posterior_forecast_particle_grouped`)
and DGPSSM.forecast_heldout_particle.

Fixtures (tests/forecast_particle_fixtures.py).  Record 0 of each of the seven cases of the particle filter's tests (12 rows with
gaps), N = 48, h = 3, origins (0, 3, 4, 8): 192 rows per (group, dim) unit, so track 2 straddles the 128-row tile; origin 3 is a row
with nothing observed; among the cases D = 8 and the shared-Gamma layout.  Three more reach tile edges: M = 300 (a ragged last column
tile), N = 130 with two origins (three row tiles, the last with 4 live rows), N = 700 with h = 2 (three strides over the particles).

Reference and rule.  tests/forecast_particle_ref.py (pinned in tests/test_forecast_particle_ref.py) in fp64 on the oracle's posterior;
e_ref is that reference against the same composition in np.longdouble.  Every fixture satisfies the margin condition of
tests/particle_filter_ref.py on the filter over its whole record (identical ancestors in both precisions and gap >= max(1e-8, 1000 x
drift)): every track resamples with a prefix of those rows.  error <= max(4 e_ref, floor) with `rule` and the floors of
tests/test_gpu_moment_grouped.py: 1e-11 + 1e-9 max|ref| on m_fc and fc_particles, 1e-11 + 1e-8 max|ref| on S_fc and lpd_fc.  The
pooled arrays and the curves are compared with NumPy on the device's own stacks at 1e-9 (1 + max|ref|).  Every measured error is
printed; DESIGN.md section 9, "Particle forecasts", has the largest."""
import functools

import numpy as np
import pytest

import forecast_particle_fixtures as ffx
import particle_filter_ref as pf
import particle_fixtures as fxt
import records_ref as rr
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.prediction import forecast_particle_grouped, posterior_forecast_particle_grouped  # noqa: F401  (without them nothing here runs)
from test_gpu_filter_grouped import CASES, POOLED
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, TEST_LEN, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

NAN = np.nan
N, H, ORIGINS = ffx.N, ffx.H, list(ffx.ORIGINS)
B = len(ORIGINS)
CURVES = ("n_h", "rmse_h", "ll_h", "ll_gauss_h", "ll_h_original_units")
TRACKS = ("m_fc", "S_fc", "lpd_fc", "fc_particles")
KIND = dict(m_fc="mean", S_fc="var", lpd_fc="var", fc_particles="mean")
FILTER = ("m_pred", "S_pred", "m_filt", "S_filt", "lpd", "lpd_joint", "ess", "log_evidence")
SCALARS = ("ll", "ll_joint", "ll_original_units", "RMSE", "ll_all")
KEYS = set(POOLED) | set(CURVES) | {"origins", "lpd_fc"}
FULL_KEYS = KEYS | set(TRACKS) | set(FILTER) | set(SCALARS) | {"filter_" + k for k in POOLED}


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture (a case of CASES or a key of ffx.EDGES), shared by the checks below (never modified)."""
    return ffx.call(ffx.fixture(name))


@functools.lru_cache(maxsize=None)
def composed(name):
    """filter_particle_records_grouped on the composed form of a fixture: R = B truncated records with NaN rows, draws concatenated"""
    return fxt.call(ffx.composed(ffx.fixture(name)))


def against_the_reference(what, out, name):
    fx = ffx.fixture(name)
    ref, e_ref = ffx.reference(name)
    for k in TRACKS:
        assert out[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)       # NaN exactly where the reference has it
        ok = ~np.isnan(ref[k])
        rule(f"{what}: {k}", KIND[k], out[k][ok], ref[k][ok], e_ref[k])
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    Yt = fx["Y"][0][fx["origins"][:, None] + 1 + np.arange(fx["h"])[None, :]]              # (B, h, J)
    np.testing.assert_array_equal(np.isnan(out["lpd_fc"]), np.broadcast_to(np.isnan(Yt)[None], out["lpd_fc"].shape))


def against_the_composed_form(out, name):
    """m_fc, S_fc, fc_particles of track (g, b) are m_pred, S_pred, particles at rows o + 1 .. o + h of the records filter on the
    truncated record, bit for bit"""
    fx, flt = ffx.fixture(name), composed(name)
    for b, o in enumerate(fx["origins"]):
        rows = slice(int(o) + 1, int(o) + 1 + fx["h"])
        for mine, theirs in (("m_fc", "m_pred"), ("S_fc", "S_pred"), ("fc_particles", "particles")):
            np.testing.assert_array_equal(out[mine][:, b], flt[theirs][:, b, rows], err_msg=f"{mine}, origin {o}")


# ---- the condition the identical ancestors rest on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + sorted(ffx.EDGES), ids=str)
def test_the_ancestors_of_every_fixture_do_not_hang_on_rounding(name):
    fx = ffx.fixture(name)
    ref, _, wide = ffx.filter_reference(name)
    gap, drift, same = pf.margin(ref, fx["unif"], wide)
    print(f"{name}: smallest gap {gap:.3e}, cdf drift between the precisions {drift:.3e}, identical ancestors {same}")
    assert same
    assert gap >= max(1e-8, 1000.0 * drift)


# ---- accuracy, bit identity with the records filter, pooled arrays and curves ---------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Particle forecasts"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, out = ffx.fixture(args), device(args)
    what = f"particle fan {shape} q={qkind} {mode} J={J}"
    nG, D = len(fx["gs"]), fx["x0"].shape[-1]
    assert set(out) == FULL_KEYS and out["origins"].tolist() == ORIGINS
    assert out["m_fc"].shape == (nG, B, H, D) and out["S_fc"].shape == (nG, B, H, D, D) and out["lpd_fc"].shape == (nG, B, H, J)
    assert out["fc_particles"].shape == (nG, B, H, N, D)
    against_the_reference(what, out, args)
    against_the_composed_form(out, args)
    # the call's own filter is filter_particle_records_grouped with R = 1 bit for bit, record axis dropped
    flt = fxt.call(fx, return_particles=False)
    for k in FILTER:
        assert flt[k].shape[1] == 1 and out[k].shape == flt[k][:, 0].shape, k
        np.testing.assert_array_equal(out[k], flt[k][:, 0], err_msg=k)
    for k in SCALARS:
        np.testing.assert_array_equal(out[k], flt[k] if k == "ll_all" else flt[k][0], err_msg=k)
    for k in POOLED:
        np.testing.assert_array_equal(out["filter_" + k], flt[k][0], err_msg=k)
    # pooled arrays and curves against NumPy on the device's own stacks
    (CC, DD, _), sd = fx["em"], np.asarray(fx["sd"]).reshape(-1)
    Yt = fx["Y"][0][fx["origins"][:, None] + 1 + np.arange(H)[None, :]]
    want = rr.pooled(out["m_fc"], out["S_fc"], CC, DD, sd, Yt)
    lp = out["lpd_fc"]
    with np.errstate(invalid="ignore"):
        mx = np.max(lp, axis=0)
        want["lpd_mix"] = mx + np.log(np.mean(np.exp(lp - mx[None]), axis=0))
    for k in POOLED:
        got, w = out[k], want[k]
        assert got.shape == (B, H, J), k
        nan_at = np.isnan(Yt) if k.startswith("lpd") else np.zeros_like(Yt, dtype=bool)
        np.testing.assert_array_equal(np.isnan(got), nan_at, err_msg=k)
        ok = ~nan_at
        tol, err = 1e-9 * (1.0 + float(np.max(np.abs(w[ok])))), float(np.max(np.abs(got[ok] - w[ok])))
        print(f"{what}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    seen = ~np.isnan(Yt)
    n_h = seen.sum(axis=0)
    np.testing.assert_array_equal(out["n_h"], n_h)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = lambda x: np.where(n_h > 0, np.sum(np.where(seen, x, 0.0), axis=0) / n_h, NAN)
        curves = dict(rmse_h=np.sqrt(over((Yt - out["predict_y"]) ** 2)), ll_h=over(out["lpd_mix"]), ll_gauss_h=over(out["lpd_gauss"]))
    curves["ll_h_original_units"] = curves["ll_h"]
    for k, w in curves.items():
        np.testing.assert_array_equal(np.isnan(out[k]), n_h == 0, err_msg=k)
        ok = n_h > 0
        if ok.any():
            err, tol = float(np.max(np.abs(out[k][ok] - w[ok]))), 1e-9 * (1.0 + float(np.max(np.abs(w[ok]))))
            print(f"{what}: {k}: {np.round(out[k][:, 0], 5).tolist()}, max error {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol, k


# ---- tile edges the shared cases do not reach ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ffx.EDGES))
def test_tile_edges(name):
    """m300: a ragged last column tile of the product and a second stride of the rows kernel; n130: three row tiles per unit, the last
    with 4 live rows, a ragged last slab of the rows kernel; n700: three strides over the particles in every loop of the state kernel,
    eleven row tiles."""
    fx, out = ffx.fixture(name), device(name)
    against_the_reference(f"particle fan {name}", out, name)
    against_the_composed_form(out, name)
    if name == "n130":                                            # passes of one origin, and a group alone
        p = ffx.call(fx, tracks_per_pass=1)
        for k in out:
            np.testing.assert_array_equal(p[k], out[k], err_msg=k)
        one = ffx.call(ffx.subset(fx, groups=[1]))
        for k in TRACKS:
            np.testing.assert_array_equal(one[k][0], out[k][1], err_msg=k)


# ---- independence: the call, the groups, the origins, their content, the pass, the layout of the draws ---------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_origins_or_the_pass(shape, per_model, G, qkind, mode, J, with_S0):
    """CASES[1] and CASES[2] have q slices (unit = (group, dim)), CASES[4] one shared model without them (unit = dim, rows = those of
    all tracks of the pass)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, a = ffx.fixture(args), device(args)
    nG = len(fx["gs"])
    b = ffx.call(fx)                                                                # two calls
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = ffx.call(ffx.subset(fx, groups=[g]))
        for k in TRACKS + FILTER:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for i in range(B):                                                              # an origin alone
        one = ffx.call(ffx.subset(fx, origins=[i]))
        assert one["origins"].tolist() == [ORIGINS[i]]
        for k in TRACKS:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, i], err_msg=f"{k}, origin {ORIGINS[i]}")
        for k in POOLED:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=f"{k}, origin {ORIGINS[i]}")
    # the origins reversed in content: the draws permuted, so that origin b runs with the draws origin B - 1 - b had; each set of draws
    # from each origin is a track of its own, and the pair (origin, draws) decides it, not its place in the call
    rev = ffx.call(dict(fx, eps_fc=np.ascontiguousarray(fx["eps_fc"][:, ::-1])))
    for i in range(B):
        one = ffx.call(dict(ffx.subset(fx, origins=[i]), eps_fc=np.ascontiguousarray(fx["eps_fc"][:, [B - 1 - i]])))
        for k in TRACKS:
            np.testing.assert_array_equal(one[k][:, 0], rev[k][:, i], err_msg=f"{k}, origin {ORIGINS[i]}, draws of {ORIGINS[B - 1 - i]}")
    assert float(np.max(np.abs(rev["m_fc"] - a["m_fc"]))) > 0.0
    for tpp in (1, 2):                                                              # passes of 1 and of 2 origins
        p = ffx.call(fx, tracks_per_pass=tpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, tracks_per_pass {tpp}")


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[4]], ids=str)
def test_shared_draws_are_the_same_draws_broadcast(shape, per_model, G, qkind, mode, J, with_S0):
    """eps_fc (h, N, D) and (B, h, N, D), eps (steps, N, D), unif (steps,), xi0 (N, D) against the same draws broadcast to the full
    layouts: bit for bit in every key."""
    fx = ffx.fixture((shape, per_model, G, qkind, mode, J, with_S0))
    nG = len(fx["gs"])
    full = lambda v, lead: None if v is None else np.ascontiguousarray(np.broadcast_to(v, lead + v.shape))
    one = lambda v: None if v is None else v[0, 0]
    eps, unif, xi0 = one(fx["eps"]), one(fx["unif"]), one(fx["xi0"])
    for efc, lead in ((fx["eps_fc"][0, 0], (nG, B)), (fx["eps_fc"][0], (nG,))):
        small = ffx.call(fx, eps=eps, unif=unif, xi0=xi0, eps_fc=efc)
        big = ffx.call(fx, eps=full(eps, (nG,)), unif=full(unif, (nG,)), xi0=full(xi0, (nG,)), eps_fc=full(efc, lead))
        for k in small:
            np.testing.assert_array_equal(small[k], big[k], err_msg=k)
    assert float(np.max(np.abs(small["m_fc"][:, 1:] - device((shape, per_model, G, qkind, mode, J, with_S0))["m_fc"][:, 1:]))) > 0.0


# ---- an outlier ------------------------------------------------------------------------------------------------------------------------
def test_a_target_forty_deviations_away_keeps_everything_finite():
    """CASES[1] (J = 3, start covariances): rows 2 and 5 moved 40 noise deviations away in every output -- a target of the tracks from
    origins 0, 3 and 4 and an observation of the filter: the densities are formed with the largest exponent subtracted."""
    fx = ffx.fixture(CASES[1])
    Y, sd = np.array(fx["Y"]), np.asarray(fx["sd"]).reshape(-1)
    Y[0, 2] = np.nanmean(Y[0], axis=0) + 40.0 * sd
    Y[0, 5] = np.nanmean(Y[0], axis=0) - 40.0 * sd
    out = ffx.call(dict(fx, Y=Y))
    Yt = Y[0][fx["origins"][:, None] + 1 + np.arange(H)[None, :]]
    for k in ("m_fc", "S_fc", "fc_particles", "m_filt", "S_filt", "ess", "log_evidence", "predict_y", "predict_y_var_total"):
        assert np.all(np.isfinite(out[k])), k
    for k in ("lpd_fc", "lpd_mix", "lpd_gauss"):
        np.testing.assert_array_equal(np.isnan(out[k]), np.broadcast_to(np.isnan(Yt), out[k].shape), err_msg=k)
        assert not np.any(np.isinf(out[k])), k
    assert np.all(np.isfinite(out["ll_h"][out["n_h"] > 0]))
    print(f"outlier: lpd_fc of (origin 0, k = 2) {np.round(out['lpd_fc'][:, 0, 1], 1).tolist()}, ll_h {np.round(out['ll_h'][:, 0], 2).tolist()}")


# ---- a particle count whose kernel rows do not fit a pass ------------------------------------------------------------------------------
def test_a_particle_count_whose_rows_do_not_fit_a_pass_is_refused_with_the_largest_that_fits():
    """the records call's case (G = 64 groups with q slices, D = 8, M = 64: 1920 rows per unit in whole tiles) and its message"""
    from test_filter_grouped_args import _filter_args
    from test_moment_grouped_args import _explicit
    a = _filter_args(_explicit(G=64, M=64, D=8, C=1, steps=2), True)
    a.update(CC=np.ones((8, 1)), DD=np.zeros(1), log_Rchols=np.zeros((1, 1)), horizon=1, eps=np.zeros((2, 2048, 8)), unif=np.full(2, 0.5),
             eps_fc=np.zeros((1, 2048, 8)))
    with pytest.raises(ValueError, match="largest N that fits is 1920"):
        pr.forecast_particle_grouped(**a)


# ---- fused with the posteriors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_forecast_particle_grouped is collapse_u_mean_grouped followed by forecast_particle_grouped on every key, bit for bit"""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), ffx.fixture(args)
    gs, call = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    T = cs[2]["T"]
    one = lambda x: None if x is None else x[:, 0]
    kw = dict(xi0=one(fx["xi0"]), origins=fx["origins"], S0s=one(fx["S0"]), q_mode="reference", return_tracks=True, return_filter=True,
              return_particles=True)
    draws = (one(fx["eps"]), one(fx["unif"]), fx["eps_fc"])
    fused = pr.posterior_forecast_particle_grouped(Zs, kerns, Xs, Qs, call, T, fx["Y"][0], CC, DD, lr, H, *draws, **kw)
    assert set(fused) == FULL_KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.forecast_particle_grouped(Ls, Zs, kerns, list(U), list(Hinv), [g["X"][-1] for g in gs], call, T, fx["Y"][0], Qs, CC, DD, lr, H,
                                       *draws, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    assert np.all(np.isfinite(fused["m_fc"])) and np.all(np.isfinite(fused["S_fc"]))
    np.testing.assert_array_equal(fused["S_fc"], np.swapaxes(fused["S_fc"], -1, -2))
    again = pr.posterior_forecast_particle_grouped(Zs, kerns, Xs, Qs, call, T, fx["Y"][0], CC, DD, lr, H, *draws, tracks_per_pass=2, **kw)
    for k in FULL_KEYS:
        np.testing.assert_array_equal(again[k], fused[k], err_msg=k)


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_forecast_heldout_particle(actuator, U_collapse):
    """the ll_h curves of the four rules are printed side by side and not asserted"""
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = np.array(Y[N_TRAIN:N_TRAIN + TEST_LEN])
    Yt[7] = NAN
    Yt[-5:] = NAN
    J, D, h = Yt.shape[1], 4, 5
    nB = TEST_LEN - h
    kw = dict(Y_train_std=1.7, return_tracks=True)
    out = mod.forecast_heldout_particle(Yt, c, h, num_particles=256, seed=7, **kw)
    assert set(out) == KEYS | {"m_fc", "S_fc"}
    assert out["origins"].tolist() == list(range(nB)) and out["m_fc"].shape == (S, nB, h, D) and out["lpd_fc"].shape == (S, nB, h, J)
    assert all(out[k].shape == (nB, h, J) for k in POOLED) and all(out[k].shape == (h, J) for k in CURVES)
    assert np.all(np.isfinite(out["m_fc"])) and np.all(np.isfinite(out["S_fc"])) and np.all(np.isfinite(out["predict_y"]))
    assert np.all(out["n_h"] > 0) and all(np.all(np.isfinite(out[k])) for k in CURVES)
    np.testing.assert_array_equal(out["S_fc"], np.swapaxes(out["S_fc"], -1, -2))
    again = mod.forecast_heldout_particle(Yt, c, h, num_particles=256, seed=7, **kw)           # a seed: the same result
    for k in out:
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    other = mod.forecast_heldout_particle(Yt, c, h, num_particles=64, seed=8, noise="independent", stride=4, S0=0.01 * np.eye(D),
                                          x0=mod._X_chains[0][-1])
    assert other["origins"].tolist() == list(range(0, nB, 4)) and np.all(np.isfinite(other["ll_h"])) and "m_fc" not in other
    rules = (("particle (N = 256)", out), ("moment matching", mod.forecast_heldout(Yt, c, h, **kw)),
             ("linearised", mod.forecast_heldout_linearised(Yt, c, h, **kw)), ("cubature", mod.forecast_heldout_cubature(Yt, c, h, **kw)))
    for name, o in rules:
        print(f"U_collapse={U_collapse}: horizons 1 .. {h}: {name} ll_h {np.round(o['ll_h'][:, 0], 6).tolist()}, "
              f"rmse_h {np.round(o['rmse_h'][:, 0], 6).tolist()}")
