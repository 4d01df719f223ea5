"""CRPS, PIT and predictive quantiles of mixture forecasts on the device (`ffvd_score_points`, `ffvd_score_moments`;
prediction.rollout_score, particle_score, moment_score, forecast_score; DGPSSM.forecast_scores) against tests/score_ref.py on the
fixtures of tests/score_fixtures.py, whose K walks the component tile of the pair kernel (1, 2, T_c - 1, T_c, T_c + 1, 2 T_c + 3).

Tolerances.  crps and pit: 1e-11 + 1e-9 max|ref|, what tests/test_gpu_rollout_summary.py holds the summaries to.  A quantile q_dev of
level p: |F_ref(q_dev) - p| <= 1e-11 + 1e-9 and |q_dev - q_ref| <= (1e-11 + 1e-9) / f_ref(q_ref) + 4 ulp(q_ref); the second follows
from the first where the density at the quantile is not tiny against the mixture's width, which tests/test_score_fixtures.py checks
for every (target, level).  Everything else here is equality of bits."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import score_fixtures as sf
import score_poison_script as script
import score_ref as sr
from ffvd_amd import prediction as pr
from ffvd_amd.prediction import moment_score, particle_score, rollout_score  # noqa: F401  (without them nothing here runs)
from test_gpu_moment_grouped import N_TRAIN, S, TEST_LEN, _chains, _regression_model

pytestmark = pytest.mark.gpu

TOL = 1e-11
RTOL = 1e-9
ARRAYS = ("crps", "pit", "quantiles")
POINTS = tuple(n for n in sf.NAMES if n.startswith("p_"))
STEPPED = tuple(c[0] for c in sf.CASES if c[3] > 1)


def call(fx, Y="own", levels=None, **kw):
    """the prediction-level call of a fixture (Y "own": the fixture's targets)"""
    name, args = sf.call_args(fx)
    return getattr(pr, name)(*args, fx["Y"] if isinstance(Y, str) else Y, levels=fx["levels"] if levels is None else levels, **kw)


@functools.lru_cache(maxsize=None)
def device(name):
    """one device call per fixture, shared by the checks below (never modified)"""
    return call(sf.fixture(name))


def same_bits(a, b, what=""):
    for k in ARRAYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}{k}")


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sf.NAMES)
def test_parity_with_the_reference(name):
    fx, ref, dev = sf.fixture(name), sf.reference(name), device(name)
    assert dev["crps"].shape == dev["pit"].shape == (fx["n_test"], fx["J"]) and dev["quantiles"].shape == (fx["steps"], fx["J"], fx["Q"])
    np.testing.assert_array_equal(dev["levels"], fx["levels"])
    seen = ~np.isnan(fx["Y"])
    for k in ("crps", "pit"):
        assert np.array_equal(np.isnan(dev[k]), ~seen), k
        err, bound = float(np.max(np.abs(dev[k][seen] - ref[k][seen]))), TOL + RTOL * float(np.max(np.abs(ref[k][seen])))
        print(f"{name}: {k}: largest error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, k
    if fx["Q"]:
        q = dev["quantiles"]
        assert np.all(np.isfinite(q))
        F = np.stack([sr.cdf(fx["mu"], fx["var"], q[..., i]) for i in range(fx["Q"])], axis=-1)
        e_F = float(np.max(np.abs(F - fx["levels"])))
        e_q = np.abs(q - ref["quantiles"])
        bound_q = (TOL + RTOL) / ref["density"] + 4.0 * np.spacing(np.abs(ref["quantiles"]))
        print(f"{name}: quantiles: largest |F_ref(q_dev) - p| {e_F:.3e} (bound {TOL + RTOL:.3e}), largest |q_dev - q_ref| {np.max(e_q):.3e}, "
              f"largest share of its bound {np.max(e_q / bound_q):.3e}")
        assert e_F <= TOL + RTOL
        assert np.all(e_q <= bound_q)
    # the means and the coverage are formed on the host from the arrays
    mean = float(np.mean(dev["crps"][seen]))
    assert dev["crps_mean"] == pytest.approx(mean, rel=1e-14) and dev["crps_mean_original_units"] == pytest.approx(mean, rel=1e-14)
    pairs = pr._coverage_pairs(fx["levels"])
    assert dev["coverage"].shape == dev["coverage_levels"].shape == (len(pairs),)
    for n, (i, k) in enumerate(pairs):
        inside = (dev["pit"][seen] >= fx["levels"][i]) & (dev["pit"][seen] <= fx["levels"][k])
        assert dev["coverage"][n] == pytest.approx(np.sum(inside) / np.sum(seen), rel=1e-14)


def test_original_units_scale_the_mean_only():
    fx = sf.fixture("p_k2")
    a, b = device("p_k2"), call(fx, Y_train_std=1.7)
    same_bits(a, b)
    assert b["crps_mean"] == a["crps_mean"] and b["crps_mean_original_units"] == pytest.approx(1.7 * a["crps_mean"], rel=1e-15)


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sf.NAMES)
def test_two_calls_and_every_pass_size_give_the_same_bits(name):
    fx, dev = sf.fixture(name), device(name)
    same_bits(dev, call(fx), "again: ")
    targets = fx["n_test"] * fx["J"]
    for tpp in (1, 8, targets, targets + 5):                       # 8: three passes for the fixtures with more than 16 targets
        same_bits(dev, call(fx, targets_per_pass=tpp), f"targets_per_pass {tpp}: ")


@pytest.mark.parametrize("name", STEPPED)
def test_a_target_alone_is_the_target_among_the_others(name):
    fx, dev = sf.fixture(name), device(name)
    t, j = min(2, fx["n_test"] - 1), fx["J"] - 1
    one = dict(fx, x=np.ascontiguousarray(fx["x"][:, t:t + 1]), CC=np.ascontiguousarray(fx["CC"][:, j:j + 1]), DD=fx["DD"][j:j + 1],
               lr=fx["lr"][j:j + 1])
    if fx["kind"] == "moments":
        one["S"] = np.ascontiguousarray(fx["S"][:, t:t + 1])
    alone = call(one, Y=fx["Y"][t:t + 1, j:j + 1])
    assert not np.isnan(fx["Y"][t, j])
    for k in ARRAYS:
        np.testing.assert_array_equal(alone[k][0, 0], dev[k][t, j], err_msg=k)
    # the last row (no target beyond n_test): its quantiles alone
    last = dict(one, x=np.ascontiguousarray(fx["x"][:, -1:]))
    if fx["kind"] == "moments":
        last["S"] = np.ascontiguousarray(fx["S"][:, -1:])
    if fx["Q"]:
        np.testing.assert_array_equal(call(last, Y=None)["quantiles"][0, 0], dev["quantiles"][-1, j])


@pytest.mark.parametrize("name", [c[0] for c in sf.CASES if c[6] == 16])
def test_a_level_alone_is_the_level_among_sixteen(name):
    fx, dev = sf.fixture(name), device(name)
    for i in (0, 5, 15):
        alone = call(fx, levels=fx["levels"][i:i + 1])
        np.testing.assert_array_equal(alone["quantiles"][..., 0], dev["quantiles"][..., i])
        np.testing.assert_array_equal(alone["crps"], dev["crps"])
        np.testing.assert_array_equal(alone["pit"], dev["pit"])


@pytest.mark.parametrize("name", POINTS)
def test_the_two_layouts_give_the_same_bits(name):
    fx, dev = sf.fixture(name), device(name)
    G, N = sf.split(fx["K"])
    p = sf.as_particles(fx["x"])
    assert p.shape == (G, fx["steps"], N, fx["D"])
    same_bits(dev, pr.particle_score(p, fx["CC"], fx["DD"], fx["lr"], fx["Y"], levels=fx["levels"]), "[G][T][N][D]: ")
    four = fx["x"].reshape(G, N, fx["steps"], fx["D"])              # (G, R, steps, D) of rollout_score: the same memory
    same_bits(dev, pr.rollout_score(four, fx["CC"], fx["DD"], fx["lr"], fx["Y"], levels=fx["levels"]), "(G, R, steps, D): ")


@pytest.mark.parametrize("name", STEPPED)
def test_nan_targets_touch_their_own_entries_only(name):
    fx, dev = sf.fixture(name), device(name)
    gone = np.isnan(fx["Y"])
    assert np.any(gone) and np.array_equal(np.isnan(dev["crps"]), gone) and np.array_equal(np.isnan(dev["pit"]), gone)
    filled = call(fx, Y=np.nan_to_num(fx["Y"]))
    np.testing.assert_array_equal(filled["quantiles"], dev["quantiles"])
    for k in ("crps", "pit"):
        np.testing.assert_array_equal(filled[k][~gone], dev[k][~gone])
        assert np.all(np.isfinite(filled[k]))
    if fx["Q"]:
        bare = call(fx, Y=None)
        np.testing.assert_array_equal(bare["quantiles"], dev["quantiles"])
        assert bare["crps"] is None and bare["pit"] is None and bare["coverage"] is None
    none = call(fx, Y=fx["Y"][:0])                                   # no held-out row
    assert none["crps"].shape == (0, fx["J"]) and np.isnan(none["crps_mean"])
    np.testing.assert_array_equal(none["quantiles"], dev["quantiles"])


# ---- consistency ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m_k2", "m_tile+1", "m_2tile+3"])
def test_moments_without_covariance_are_the_points(name):
    fx = sf.fixture(name)
    em = (fx["CC"], fx["DD"], fx["lr"], fx["Y"])
    mom = pr.moment_score(fx["x"], np.zeros_like(fx["S"]), *em, levels=fx["levels"])
    pts = pr.particle_score(np.ascontiguousarray(np.transpose(fx["x"], (1, 0, 2)))[None], *em, levels=fx["levels"])     # (1, steps, K, D)
    seen = ~np.isnan(fx["Y"])
    for k in ("crps", "pit"):
        err, bound = float(np.max(np.abs(mom[k][seen] - pts[k][seen]))), TOL + RTOL * float(np.max(np.abs(pts[k][seen])))
        print(f"{name}: S = 0 against the points: {k}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    mu, var = sr.components_points(fx["x"], fx["CC"], fx["DD"], fx["sd"])
    dens = np.stack([sr.pdf(mu, var, pts["quantiles"][..., i]) for i in range(fx["Q"])], axis=-1)
    e_q = np.abs(mom["quantiles"] - pts["quantiles"])
    print(f"{name}: S = 0 against the points: quantiles: {np.max(e_q):.3e}")
    assert np.all(e_q <= (TOL + RTOL) / dens + 4.0 * np.spacing(np.abs(pts["quantiles"])))


def test_one_component_is_the_closed_form():
    rng = np.random.default_rng(8)
    steps, D, J = 7, 4, 3
    x, CC, DD, sd = rng.standard_normal((1, steps, D)), rng.standard_normal((D, J)), rng.standard_normal(J), np.array([0.2, 0.7, 1.3])
    Y = rng.standard_normal((steps, J)) * 2.0
    lv = np.array([0.05, 0.5, 0.95])
    L = 0.4 * rng.standard_normal((1, steps, D, D))
    Sx = L @ np.swapaxes(L, -1, -2)
    Sx = 0.5 * (Sx + np.swapaxes(Sx, -1, -2))
    from scipy.special import ndtri
    for what, out, (mu, var) in (("points", pr.rollout_score(x, CC, DD, np.log(sd), Y, levels=lv), sr.components_points(x, CC, DD, sd)),
                                 ("moments", pr.moment_score(x, Sx, CC, DD, np.log(sd), Y, levels=lv), sr.components_moments(x, Sx, CC, DD, sd))):
        m, s = mu[..., 0], np.sqrt(var[..., 0])
        want = sr.crps_gaussian(m, s, Y)
        err, bound = float(np.max(np.abs(out["crps"] - want))), TOL + RTOL * float(np.max(np.abs(want)))
        print(f"K = 1, {what}: crps against sigma [z (2 Phi - 1) + 2 phi - 1 / sqrt(pi)]: {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        Phi = sr.cdf(mu, var, Y)
        assert float(np.max(np.abs(out["pit"] - Phi))) <= TOL + RTOL
        q = m[..., None] + s[..., None] * ndtri(lv)[None, None, :]
        dens = np.exp(-0.5 * ndtri(lv) ** 2) / np.sqrt(2.0 * np.pi) / s[..., None]
        assert np.all(np.abs(out["quantiles"] - q) <= (TOL + RTOL) / dens + 4.0 * np.spacing(np.abs(q)))
        assert np.all(out["quantiles"][..., 1] == pytest.approx(m, abs=1e-12))


@pytest.mark.parametrize("name", ["p_tile+1", "m_tile+1", "p_k1"])
def test_a_target_thirty_deviations_outside_stays_finite(name):
    fx = sf.fixture(name)
    far = 30.0 * np.sqrt(np.max(fx["var"][:fx["n_test"]], axis=-1))
    for sign, edge in ((1.0, 1.0), (-1.0, 0.0)):
        Y = (np.max(fx["mu"][:fx["n_test"]], axis=-1) + far) if sign > 0 else (np.min(fx["mu"][:fx["n_test"]], axis=-1) - far)
        out = call(fx, Y=Y)
        assert np.all(np.isfinite(out["crps"])) and np.all(out["crps"] > 0.0) and not np.any(np.isnan(out["pit"]))
        assert np.all(np.abs(out["pit"] - edge) <= 1e-15)
        ref = sr.crps(fx["mu"][:fx["n_test"]], fx["var"][:fx["n_test"]], Y)
        assert float(np.max(np.abs(out["crps"] - ref))) <= TOL + RTOL * float(np.max(np.abs(ref)))


@pytest.mark.parametrize("name", ["p_2tile+3", "m_2tile+3"])
def test_one_infinite_entry_poisons_its_own_row_and_the_call_returns(name):
    """Not scanned on the host: the row that holds the entry comes back NaN (every output of it that the entry reaches through CC),
    the other rows keep their bits, and the bisection of that row ends."""
    fx, dev = sf.fixture(name), device(name)
    t = 4
    for value in (np.inf, np.nan):
        bad = dict(fx, x=fx["x"].copy())
        bad["x"][fx["K"] // 2 + 1, t, 0] = value
        out = call(bad)
        rows = np.arange(fx["steps"]) != t
        for k in ARRAYS:
            np.testing.assert_array_equal(out[k][rows[:len(out[k])]], dev[k][rows[:len(dev[k])]], err_msg=k)
            assert np.all(np.isnan(out[k][t])), k
        assert np.isnan(out["crps_mean"])
    if fx["kind"] == "moments":                                      # a covariance that makes a variance negative: the same
        bad = dict(fx, S=fx["S"].copy())
        bad["S"][3, t] = -100.0 * np.eye(fx["D"])
        out = call(bad)
        assert all(np.all(np.isnan(out[k][t])) for k in ARRAYS)
        np.testing.assert_array_equal(out["quantiles"][:t], dev["quantiles"][:t])
        # a diverged covariance: +Inf (1 / sqrt(2 v) = 0 is finite, the variance is not) or NaN on the diagonal of one component
        rows = np.arange(fx["steps"]) != t
        for value in (np.inf, np.nan):
            bad = dict(fx, S=fx["S"].copy())
            bad["S"][fx["K"] - 2, t, 0, 0] = value
            out = call(bad)
            for k in ARRAYS:
                assert np.all(np.isnan(out[k][t])), (k, value)
                np.testing.assert_array_equal(out[k][rows], dev[k][rows], err_msg=k)


def test_an_empty_stack_is_refused_by_python_and_fine_for_the_library():
    from ffvd_amd import _lib
    CC, DD, lr = np.ones((2, 1)), np.zeros(1), np.zeros(1)
    with pytest.raises(ValueError, match="particle_score: at least one group"):
        pr.particle_score(np.zeros((0, 3, 4, 2)), CC, DD, lr)
    with pytest.raises(ValueError, match="rollout_score: at least one rollout"):
        pr.rollout_score(np.zeros((0, 3, 2)), CC, DD, lr)
    with pytest.raises(ValueError, match="moment_score: at least one group"):
        pr.moment_score(np.zeros((0, 3, 2)), np.zeros((0, 3, 2, 2)), CC, DD, lr)
    z = np.zeros(8)
    dp = _lib.dptr
    assert _lib.load().ffvd_score_points(dp(z), 0, 4, 3, 2, 24, 2, 8, dp(z), dp(z), dp(z), 1, None, 0, None, 0, 0, None, None, None) == _lib.FFVD_OK


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(actuator):
    params, Y, c = actuator
    m = _regression_model(params, c, True)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = np.array(Y[N_TRAIN:N_TRAIN + TEST_LEN])
    Yt[7] = np.nan
    return mod, Yt, c


@pytest.mark.parametrize("method", ["moment", "linearised", "cubature", "particle", "adapted"])
def test_forecast_scores_of_the_model(model, method):
    mod, Yt, c = model
    h, lv, J, D, N = 5, (0.05, 0.25, 0.5, 0.75, 0.95), Yt.shape[1], 4, 32
    extra = dict(num_particles=N, seed=7) if method in ("particle", "adapted") else {}
    out = mod.forecast_scores(Yt, c, h, method=method, levels=lv, Y_train_std=1.7, stride=3, **extra)
    B = len(range(0, TEST_LEN - h, 3))
    assert set(out) == {"crps", "pit", "quantiles", "levels", "crps_mean", "crps_mean_original_units", "coverage", "coverage_levels", "n_h",
                        "crps_h", "coverage_h", "origins", "used", "fan"}
    assert out["crps"].shape == out["pit"].shape == (B, h, J) and out["quantiles"].shape == (B, h, J, 5)
    assert out["crps_h"].shape == out["n_h"].shape == (h, J) and out["coverage_h"].shape == (h, J, 2) and out["coverage"].shape == (2,)
    assert out["origins"].tolist() == list(range(0, TEST_LEN - h, 3)) and out["used"] == ("particles" if extra else "moments")
    fan = out["fan"]
    assert fan["m_fc"].shape == (S, B, h, D) and (("fc_particles" in fan) == bool(extra))
    if extra:
        assert fan["fc_particles"].shape == (S, B, h, N, D)
    Ytg = Yt[out["origins"][:, None] + 1 + np.arange(h)[None, :]]
    seen = ~np.isnan(Ytg)
    assert np.array_equal(np.isnan(out["crps"]), ~seen) and np.array_equal(np.isnan(out["pit"]), ~seen) and np.all(np.isfinite(out["quantiles"]))
    assert np.array_equal(out["n_h"], np.sum(seen, axis=0)) and np.array_equal(out["n_h"], fan["n_h"])
    np.testing.assert_allclose(out["crps_h"], np.nansum(out["crps"], axis=0) / out["n_h"], rtol=1e-14, atol=0.0)
    for n, (lo, hi) in enumerate(((0.05, 0.95), (0.25, 0.75))):
        inside = seen & (out["pit"] >= lo) & (out["pit"] <= hi)
        np.testing.assert_allclose(out["coverage_h"][..., n], np.sum(inside, axis=0) / out["n_h"], rtol=1e-14, atol=0.0)
        assert out["coverage"][n] == pytest.approx(np.sum(inside) / np.sum(seen), rel=1e-14)
    assert out["crps_mean"] == pytest.approx(np.nanmean(out["crps"]), rel=1e-13) and out["crps_mean_original_units"] == pytest.approx(
        1.7 * out["crps_mean"], rel=1e-15)
    assert np.all(np.diff(out["quantiles"], axis=-1) > 0.0) and np.all(out["crps"][seen] > 0.0)
    lik = mod.likelihood
    direct = pr.forecast_score(fan, Yt, lik.CC, lik.DD, lik.log_Rchols, levels=lv, Y_train_std=1.7)
    for k in ("crps", "pit", "quantiles", "crps_h", "coverage_h", "n_h"):
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
    if extra:                                                        # the per-chain Gaussians of the same fan
        mom = pr.forecast_score(fan, Yt, lik.CC, lik.DD, lik.log_Rchols, levels=lv, use="moments")
        assert mom["used"] == "moments" and float(np.max(np.abs(mom["crps"][seen] - out["crps"][seen]))) > 0.0
    print(f"{method}: crps_h {np.round(out['crps_h'][:, 0], 6).tolist()}, coverage_h(90%) {np.round(out['coverage_h'][:, 0, 0], 3).tolist()}, "
          f"ll_h {np.round(fan['ll_h'][:, 0], 6).tolist()}")


# ---- poisoned scratch -----------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/score_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output bit for bit, the
    reversed pass as the forward one, both symbols in every call."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"score{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, _ in script.CALLS:
        assert set(script.SYMBOLS) == set(clean["called/" + label].tolist()), label
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) >= 2 * 3 * 8 * len(script.CALLS)
    for k in results:
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
        if k.startswith("fwd/"):
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)
    # and they are the results of this process
    label, _ = script.CALLS[0]
    for form, name in ((0, script.PLAN[0][0]), (2, script.PLAN[0][1])):
        for k in ARRAYS:
            np.testing.assert_array_equal(clean[f"fwd/{label}/{form}/{k}"], device(name)[k], err_msg=k)
