"""Fully adapted particle filtering of many records on the device: prediction.filter_adapted_records_grouped
(`ffvd_particle_adapted_records_grouped`), fused with the collapsed posteriors (prediction.posterior_filter_adapted_records_grouped,
`ffvd_posterior_particle_adapted_records_grouped`) and DGPSSM.filter_records_adapted.

Fixtures (tests/adapted_particle_fixtures.py).  The seven cases (R = 3 records of 12 rows, N = 48) and the three tile edges of the
bootstrap filter's tests with the same draws, plus seven small ones for what is new in the adapted weight kernel: D = 1 and D = 8 with
J = 3, N = 2, N = 2048 with 2 rows, a last row unobserved, rows with only some outputs observed, and one output 1e-6 times sharper
than the others.

Reference and rule.  tests/particle_adapted_ref.py (pinned in tests/test_particle_adapted_ref.py) in fp64 on the oracle's posterior;
e_ref is that reference against the same composition in np.longdouble.  The ancestors must be IDENTICAL: every fixture satisfies the
margin condition (the two precisions draw the same ancestors, and no threshold (unif + i) / N lies within max(1e-8, 1000 x the cdf
drift between the precisions) of a cdf entry) -- checked here for the cases and the edges, which are built on the device's posterior
path, and in tests/test_adapted_fixtures.py for the small ones.  Particles, moments and densities: error <= max(4 e_ref, floor) with
`rule` and `judge` of tests/test_gpu_filter_records.py, as the bootstrap filter's tests; ess / N takes the variance floor.
log_evidence, the pooled arrays and the scalars are compared with NumPy on the device's own stacks at 1e-9 (1 + max|ref|).  Every
measured error is printed; DESIGN.md section 9, "Adapted particle filtering", has the largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import adapted_particle_fixtures as afx
import adapted_poison_script as script
import records_ref as rr
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_filter_grouped import CASES, POOLED, emission
from test_gpu_filter_records import LENGTHS, R, SCALARS, judge, live_rows, records
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

NAN = np.nan
N = afx.N
MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt")
TRACK = MOMENTS + ("lpd", "lpd_joint", "ess", "log_evidence")
DRAWN = ("particles", "ancestors")
KEYS = set(TRACK) | set(POOLED) | set(SCALARS) | {"ll_all"}
JUDGED = MOMENTS + ("lpd", "lpd_joint", "particles")
BUILT_ON_THE_DEVICE = list(CASES) + sorted(afx.EDGES)


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture, shared by the checks below (never modified)."""
    return afx.call(afx.fixture(name))


def against_the_reference(what, out, name):
    """identical ancestors; particles, moments and densities by the rule; ess / N by the variance floor; NaN where the reference has it"""
    ref, e_ref, _ = afx.reference(name)
    n = ref["particles"].shape[3]
    assert out["ancestors"].dtype == np.int32
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judge(what, out, ref, e_ref, keys=JUDGED)
    np.testing.assert_array_equal(np.isnan(out["ess"]), np.isnan(ref["ess"]))
    ok = ~np.isnan(ref["ess"])
    rule(f"{what}: ess / N", "var", out["ess"][ok] / n, ref["ess"][ok] / n, e_ref["ess"] / n)
    for k in ("S_pred", "S_filt"):
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)
    le = np.nansum(out["lpd_joint"], axis=2)
    err, tol = float(np.max(np.abs(out["log_evidence"] - le))), 1e-9 * (1.0 + float(np.max(np.abs(le))))
    print(f"{what}: log_evidence {np.round(out['log_evidence'], 4).tolist()}: max error {err:.3e}, tolerance {tol:.3e}")
    assert out["log_evidence"].shape == le.shape and err <= tol


# ---- the condition the identical ancestors rest on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILT_ON_THE_DEVICE, ids=str)
def test_the_ancestors_of_every_fixture_do_not_hang_on_rounding(name):
    """The margin condition of the cases and the edges (the small fixtures: tests/test_adapted_fixtures.py, without a GPU).  A fixture
    that misses it gets another seed, never another bound."""
    gap, drift, same, _ = afx.margin_holds(name)
    print(f"{name}: smallest gap {gap:.3e}, cdf drift between the precisions {drift:.3e}, identical ancestors {same}")
    assert same
    assert gap >= max(1e-8, 1000.0 * drift)


# ---- accuracy, covariances, pooled arrays and scalars ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Adapted particle filtering"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, rec = case(shape, per_model, G), device(args), records(*args)
    what = f"adapted {shape} q={qkind} {mode} J={J}"
    nG, D = len(cs[0]), cs[2]["D"]
    assert set(out) == KEYS | set(DRAWN)
    assert out["m_pred"].shape == (nG, R, STEPS, D) and out["lpd"].shape == (nG, R, STEPS, J) and out["ess"].shape == (nG, R, STEPS)
    assert out["particles"].shape == (nG, R, STEPS, N, D) and out["ancestors"].shape == (nG, R, STEPS, N)
    against_the_reference(what, out, args)
    live = live_rows(LENGTHS, STEPS)
    assert np.all(out["ancestors"][:, ~live] == -1) and np.all(np.isnan(out["particles"][:, ~live]))
    e = out["ess"][:, live]
    assert np.all(e >= 1.0 - 1e-12) and np.all(e <= N * (1.0 + 1e-12))
    # pooled arrays and scalars against NumPy on the device's own stacks
    (CC, DD, _), Y, sd = emission(cs, J), rec["Y"], np.asarray(rec["sd"]).reshape(-1)
    want = rr.pooled(out["m_pred"], out["S_pred"], CC, DD, sd, Y)
    lp = out["lpd"]
    with np.errstate(invalid="ignore"):
        mx = np.max(lp, axis=0)
        want["lpd_mix"] = mx + np.log(np.mean(np.exp(lp - mx[None]), axis=0))
    dead = np.broadcast_to(~live[:, :, None], Y.shape)
    nan_at = dict(predict_y=dead, predict_y_var_total=dead, lpd_mix=np.isnan(Y), lpd_gauss=np.isnan(Y))
    for k in POOLED:
        got, w = out[k], want[k]
        assert got.shape == (R, STEPS, J), k
        np.testing.assert_array_equal(np.isnan(got), nan_at[k], err_msg=k)
        ok = ~nan_at[k]
        tol, err = 1e-9 * (1.0 + float(np.max(np.abs(w[ok])))), float(np.max(np.abs(got[ok] - w[ok])))
        print(f"{what}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    ws = rr.scalars(Y, out["lpd_mix"], out["lpd_joint"], out["predict_y"])
    for k in SCALARS + ("ll_all",):
        w, got = np.asarray(ws[k]), np.asarray(out[k])
        assert got.shape == w.shape == (() if k == "ll_all" else (R,)) and np.all(np.isfinite(got)), k
        err, tol = float(np.max(np.abs(got - w))), 1e-9 * (1.0 + float(np.max(np.abs(w))))
        print(f"{what}: {k}: {np.round(got, 6).tolist()}, max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k


@pytest.mark.parametrize("name", sorted(afx.EDGES) + sorted(afx.SMALL))
def test_tile_edges_and_small_fixtures(name):
    """The bootstrap tests' edges (m300, n130, n700) and the small fixtures of tests/adapted_particle_fixtures.py."""
    fx, out = afx.fixture(name), device(name)
    against_the_reference(f"adapted {name}", out, name)
    if name == "n130":                                            # a group alone: the same bits from a one-unit-per-dim call
        one = afx.call(afx.subset(fx, groups=[1]))
        for k in TRACK + DRAWN:
            np.testing.assert_array_equal(one[k][0], out[k][1], err_msg=k)
    if name == "last_nan":                                        # the unobserved last row: the bootstrap branch
        np.testing.assert_array_equal(out["m_filt"][:, 0, -1], out["m_pred"][:, 0, -1])
        np.testing.assert_array_equal(out["S_filt"][:, 0, -1], out["S_pred"][:, 0, -1])
        assert np.all(out["ess"][:, 0, -1] == N) and np.all(out["ancestors"][:, 0, -1] == np.arange(N))


# ---- independence: the call, the groups, the records, their order, the pass, the padding, the layout of the draws ---------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    """CASES[1] and CASES[2] have q slices (unit = (group, dim), rows = the N rows of each of the group's records), CASES[4] one shared
    model without them (unit = dim, rows = those of all tracks of the pass)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, a = afx.case_fixture(*args), device(args)
    nG, every = len(fx["gs"]), TRACK + DRAWN
    b = afx.call(fx)                                                                # two calls
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = afx.call(afx.subset(fx, groups=[g]))
        for k in every:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = afx.call(afx.subset(fx, recs=[r]))
        for k in every:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
        for k in POOLED + SCALARS:
            np.testing.assert_array_equal(one[k][0], a[k][r], err_msg=f"{k}, record {r}")
    one = afx.call(afx.subset(fx, groups=[nG - 1], recs=[1]))                       # a track alone: G = 1, R = 1
    for k in every:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = afx.call(afx.subset(fx, recs=list(range(R))[::-1]))                       # the records reversed, the draws with them
    for k in every:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for k in POOLED + SCALARS:
        np.testing.assert_array_equal(rev[k], a[k][::-1], err_msg=k)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = afx.call(fx, records_per_pass=rpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 alone, padded from 12 to 15 rows with NaN (draws padded with zeros, uniforms with 0.5)
    n, C, D = LENGTHS[2], 0 if fx["ctrl"] is None else fx["ctrl"].shape[2], fx["x0"].shape[-1]
    two = afx.subset(fx, recs=[2])
    more = dict(two, Y=np.concatenate((two["Y"], np.full((1, 3, J), NAN)), axis=1),
                ctrl=np.concatenate((two["ctrl"], np.ones((1, 3, C))), axis=1) if C else None,
                eps=np.concatenate((two["eps"], np.zeros((nG, 1, 3, N, D))), axis=2),
                unif=np.concatenate((two["unif"], np.full((nG, 1, 3), 0.5)), axis=2))
    unmasked, padded = afx.call(two, lengths=None), afx.call(more)
    assert padded["m_pred"].shape[2] == STEPS + 3
    for k in every:
        if k == "log_evidence":
            np.testing.assert_array_equal(padded[k][:, 0], a[k][:, 2], err_msg=k)
            np.testing.assert_array_equal(unmasked[k][:, 0], a[k][:, 2], err_msg=k)
            continue
        for o, name in ((unmasked, "unmasked"), (padded, "padded")):
            np.testing.assert_array_equal(o[k][:, 0, :n], a[k][:, 2, :n], err_msg=f"{k}, {name}")
        assert np.all(padded[k][:, 0, n:] == -1) if k == "ancestors" else np.all(np.isnan(padded[k][:, 0, n:])), k
    np.testing.assert_array_equal(unmasked["m_filt"][:, 0, n:], unmasked["m_pred"][:, 0, n:])   # an unobserved step: filtered = predicted


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[4]], ids=str)
def test_shared_draws_are_the_same_draws_broadcast(shape, per_model, G, qkind, mode, J, with_S0):
    """eps (steps, N, D), unif (steps,), xi0 (N, D) and their per-record layouts against the same draws broadcast to the full
    (G, R, ...) layout: bit for bit in every key."""
    fx = afx.case_fixture(shape, per_model, G, qkind, mode, J, with_S0)
    nG = len(fx["gs"])
    x = lambda v, n: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (nG, R) + v.shape[-n:]))
    for pick in (lambda v: v[0, 0], lambda v: v[0]):                                # shared by all tracks; shared by the groups
        eps, unif, xi0 = pick(fx["eps"]), pick(fx["unif"]), None if fx["xi0"] is None else pick(fx["xi0"])
        small = afx.call(dict(fx, eps=eps, unif=unif, xi0=xi0))
        full = afx.call(dict(fx, eps=x(eps, 3), unif=x(unif, 1), xi0=x(xi0, 2)))
        for k in small:
            np.testing.assert_array_equal(small[k], full[k], err_msg=k)
    # (the particles, not m_filt: from a point the moments of row 0 are Rao-Blackwellised and no draw enters them)
    assert float(np.max(np.abs(small["particles"][:, :, 0] - device((shape, per_model, G, qkind, mode, J, with_S0))["particles"][:, :, 0]))) > 0.0


# ---- nothing observed: the bootstrap filter's rollout, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[0], CASES[1]], ids=str)
def test_with_every_observation_missing_the_particles_are_the_bootstrap_call_s(shape, per_model, G, qkind, mode, J, with_S0):
    """All NaN (CASES[0] from a point, CASES[1] from start covariances, so that X_0 is compared too): `particles` is
    filter_particle_records_grouped's on the same draws with array_equal, ancestors are the identity, ess = N, m_filt / S_filt are
    m_pred / S_pred bit for bit, lpd all NaN, log_evidence 0."""
    fx = afx.case_fixture(shape, per_model, G, qkind, mode, J, with_S0)
    blind = dict(fx, Y=np.full_like(fx["Y"], NAN))
    out, boot = afx.call(blind, lengths=None), afx.call(blind, fn=pr.filter_particle_records_grouped, lengths=None)
    np.testing.assert_array_equal(out["particles"], boot["particles"])
    np.testing.assert_array_equal(out["ancestors"], np.broadcast_to(np.arange(N, dtype=np.int32), out["ancestors"].shape))
    np.testing.assert_array_equal(out["ancestors"], boot["ancestors"])
    np.testing.assert_array_equal(out["ess"], np.full(out["ess"].shape, float(N)))
    np.testing.assert_array_equal(out["m_filt"], out["m_pred"])
    np.testing.assert_array_equal(out["S_filt"], out["S_pred"])
    assert np.all(np.isnan(out["lpd"])) and np.all(np.isnan(out["lpd_joint"])) and np.all(np.isnan(out["lpd_mix"]))
    np.testing.assert_array_equal(out["log_evidence"], np.zeros(out["log_evidence"].shape))
    assert np.all(np.isfinite(out["particles"]))


# ---- an outlier ------------------------------------------------------------------------------------------------------------------------
def test_an_outlier_forty_deviations_away_keeps_everything_finite():
    """CASES[1] (J = 3, start covariances), row 3 of record 0 moved 40 noise deviations away in every output: the weights are formed
    with the largest exponent subtracted, so everything stays finite, ess >= 1 and the ancestors stay in range."""
    fx = afx.case_fixture(*CASES[1])
    Y, sd = np.array(fx["Y"]), np.asarray(fx["sd"]).reshape(-1)
    Y[0, 3] = np.nanmean(Y[0], axis=0) + 40.0 * sd
    out = afx.call(dict(fx, Y=Y))
    live = live_rows(LENGTHS, STEPS)
    for k in MOMENTS + ("ess", "particles"):
        assert np.all(np.isfinite(out[k][:, live])), k
    seen = live & ~np.all(np.isnan(Y), axis=2)
    assert np.all(np.isfinite(out["lpd_joint"][:, seen])) and np.all(np.isnan(out["lpd_joint"][:, ~seen]))
    assert np.all(np.isfinite(out["log_evidence"])) and np.isfinite(out["ll_all"])
    a = out["ancestors"][:, live]
    assert a.min() >= 0 and a.max() <= N - 1 and np.all(out["ess"][:, live] >= 1.0 - 1e-12)
    print(f"outlier: ess of the row {np.round(out['ess'][:, 0, 3], 3).tolist()}, lpd_joint {np.round(out['lpd_joint'][:, 0, 3], 2).tolist()}")


# ---- fused with the posteriors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_filter_adapted_records_grouped against collapse_u_mean_grouped followed by filter_adapted_records_grouped: the same
    posterior, the same launches, bit for bit in every key."""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), afx.case_fixture(*args)
    gs, call = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True)
    fused = pr.posterior_filter_adapted_records_grouped(Zs, kerns, Xs, Qs, call, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                        x0s=fx["x0"], **kw)
    assert set(fused) == KEYS | set(DRAWN)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_adapted_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), fx["x0"], fx["ctrl"], fx["Y"], Qs, CC, DD, lr, fx["eps"],
                                            fx["unif"], **kw)
    for k in fused:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    for k in ("S_pred", "S_filt"):
        np.testing.assert_array_equal(fused[k], np.swapaxes(fused[k], -1, -2), err_msg=k)


# ---- poisoned scratch ------------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/adapted_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output bit for bit, the
    reversed pass as the forward one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"adapted{mode}.npz")
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


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
def _actuator_records(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    n = 8
    Yr = np.stack([Y[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    cr = np.stack([c[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    Yr[0, 3] = NAN
    Yr[1, 6:] = NAN
    return mod, Yr, cr, n


@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_records_adapted_of_the_model(actuator, U_collapse):
    mod, Yr, cr, n = _actuator_records(actuator, U_collapse)
    D, lengths, J = 4, [8, 6, 8], Yr.shape[2]
    kw = dict(lengths=lengths, Y_train_std=1.7)
    out = mod.filter_records_adapted(Yr, cr, num_particles=128, seed=7, return_particles=True, **kw)
    assert set(out) == KEYS | set(DRAWN)
    assert out["m_filt"].shape == (S, R, n, D) and out["predict_y"].shape == (R, n, J) and out["ll"].shape == (R,)
    assert out["ess"].shape == (S, R, n) and out["log_evidence"].shape == (S, R) and out["particles"].shape == (S, R, n, 128, D)
    live = live_rows(lengths, n)
    assert all(np.all(np.isfinite(out[k][:, live])) and np.all(np.isnan(out[k][:, ~live])) for k in MOMENTS + ("ess",))
    assert np.all(np.isfinite(out["ll"])) and np.isfinite(out["ll_all"]) and np.all(out["ll_original_units"] == out["ll"] - np.log(1.7))
    again = mod.filter_records_adapted(Yr, cr, num_particles=128, seed=7, return_particles=True, **kw)        # a seed: the same result
    for k in out:
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    other = mod.filter_records_adapted(Yr, cr, num_particles=128, seed=8, **kw)
    assert set(other) == KEYS and float(np.max(np.abs(other["m_filt"][:, live] - out["m_filt"][:, live]))) > 0.0
    per = mod.filter_records_adapted(Yr, cr, num_particles=64, seed=3, noise="per_record", S0=0.01 * np.eye(D), **kw)
    assert np.all(np.isfinite(per["log_evidence"]))


def test_on_the_actuator_fixture_the_smallest_ess_is_not_below_the_bootstrap_filter_s(actuator):
    """The point of the feature, asserted loosely: three chains, three records of 8 rows, N = 256, the same seed and therefore the
    same draws for both filters: the smallest ess of the adapted call is not below the bootstrap call's.  Both, and ll_all of both,
    are printed ("Adapted particle filtering", has them)."""
    mod, Yr, cr, n = _actuator_records(actuator, True)
    lengths = [8, 6, 8]
    kw = dict(lengths=lengths, Y_train_std=1.7, num_particles=256, seed=11)
    ada, boot = mod.filter_records_adapted(Yr, cr, **kw), mod.filter_records_particle(Yr, cr, **kw)
    live = live_rows(lengths, n)
    lo_a, lo_b = float(np.min(ada["ess"][:, live])), float(np.min(boot["ess"][:, live]))
    print(f"actuator, N = 256: smallest ess adapted {lo_a:.2f}, bootstrap {lo_b:.2f}; median ess adapted "
          f"{float(np.median(ada['ess'][:, live])):.1f}, bootstrap {float(np.median(boot['ess'][:, live])):.1f}; "
          f"ll_all adapted {ada['ll_all']:.6f}, bootstrap {boot['ll_all']:.6f}")
    assert lo_a >= lo_b
