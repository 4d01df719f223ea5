"""Particle filtering of many records with adaptive (ESS-triggered) resampling on the device:
prediction.filter_adaptive_records_grouped (`ffvd_particle_adaptive_records_grouped`), fused with the collapsed posteriors
(prediction.posterior_filter_adaptive_records_grouped), with seeded device draws (prediction.adaptive_records_seeded,
prediction.posterior_adaptive_records_seeded) and DGPSSM.filter_records_adaptive.

Fixtures (tests/adaptive_particle_fixtures.py): nine small ones on the oracle's posterior, each with its threshold, all of which
satisfy the three conditions that tests/test_adaptive_fixtures.py checks without a GPU -- fp64 and np.longdouble decide and draw
alike, no threshold of a resampling row hangs on a cdf entry, no ess / N hangs on the ESS threshold.

Reference and rule.  tests/particle_adaptive_ref.py (pinned in tests/test_particle_adaptive_ref.py) in fp64; e_ref is that reference
against the same composition in np.longdouble.  `resampled` and `ancestors` must be IDENTICAL.  Particles, moments, densities and
weights: error <= max(4 e_ref, floor) with `rule` and `judge` of tests/test_gpu_filter_records.py; ess / N takes the variance floor.
Against the bootstrap call (threshold 2, threshold 0 on unobserved records) every comparison is bit for bit.  Every measured error is
printed; DESIGN.md section 9, "Adaptive resampling", has the largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_particle_fixtures as afx
import adaptive_poison_script as script
import particle_fixtures as pfx
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_filter_adapted import _actuator_records
from test_gpu_filter_grouped import CASES, POOLED
from test_gpu_filter_records import R, SCALARS, judge, live_rows
from test_gpu_moment_grouped import S, STEPS, _fused_args, case, rule

pytestmark = pytest.mark.gpu

NAN = np.nan
MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt")
TRACK = MOMENTS + ("lpd", "lpd_joint", "ess", "log_evidence", "resampled")
DRAWN = ("particles", "ancestors", "weights")
KEYS = set(TRACK) | set(POOLED) | set(SCALARS) | {"ll_all"}
BOOTSTRAP_KEYS = (KEYS | {"particles", "ancestors"}) - {"resampled"}
JUDGED = MOMENTS + ("lpd", "lpd_joint", "particles")


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture at its own threshold, shared by the checks below (never modified)."""
    return afx.call(afx.fixture(name))


def same_bits(a, b, keys, what=""):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}{k}")


# ---- against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", afx.NAMES)
def test_every_fixture_against_the_reference(name):
    """Identical decisions and ancestors; particles, moments, densities and weights by the rule; ess / N by the variance floor; NaN
    exactly where the reference has it; exactly symmetric covariances.  Measured on one MI355X: see DESIGN.md section 9, "Adaptive
    resampling"."""
    fx, out = afx.fixture(name), device(name)
    ref, e_ref, _ = afx.reference(name)
    what = f"adaptive {name} thr={fx['thr']}"
    n = ref["particles"].shape[3]
    assert set(out) == KEYS | set(DRAWN)
    assert out["resampled"].dtype == np.int32 and out["ancestors"].dtype == np.int32
    np.testing.assert_array_equal(out["resampled"], ref["resampled"])
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judge(what, out, ref, e_ref, keys=JUDGED)
    np.testing.assert_array_equal(np.isnan(out["weights"]), np.isnan(ref["weights"]))
    ok = ~np.isnan(ref["weights"])
    rule(f"{what}: weights", "var", out["weights"][ok], ref["weights"][ok], e_ref["weights"])
    np.testing.assert_array_equal(np.isnan(out["ess"]), np.isnan(ref["ess"]))
    ok = ~np.isnan(ref["ess"])
    rule(f"{what}: ess / N", "var", out["ess"][ok] / n, ref["ess"][ok] / n, e_ref["ess"] / n)
    for k in ("S_pred", "S_filt"):
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)
    le = np.nansum(out["lpd_joint"], axis=2)
    err, tol = float(np.max(np.abs(out["log_evidence"] - le))), 1e-9 * (1.0 + float(np.max(np.abs(le))))
    print(f"{what}: log_evidence {np.round(out['log_evidence'], 4).tolist()}: max error {err:.3e}, tolerance {tol:.3e}; "
          f"rows resampled {int((out['resampled'] == 1).sum())} of {int((~np.isnan(out['lpd_joint'])).sum())} observed")
    assert out["log_evidence"].shape == le.shape and err <= tol
    live = live_rows(fx["lengths"], fx["Y"].shape[1])
    w = out["weights"][:, live]
    assert np.all(w >= 0.0) and float(np.max(np.abs(w.sum(axis=-1) - 1.0))) <= 1e-12
    assert np.all(out["resampled"][:, ~live] == -1) and np.all(np.isnan(out["weights"][:, ~live]))
    blind = live & np.all(np.isnan(fx["Y"]), axis=2)                                # rows with nothing observed: only the propagation
    np.testing.assert_array_equal(out["m_filt"][:, blind], out["m_pred"][:, blind])
    np.testing.assert_array_equal(out["S_filt"][:, blind], out["S_pred"][:, blind])
    assert np.all(out["resampled"][:, blind] == 0) and np.all(out["ancestors"][:, blind] == np.arange(n))


# ---- the contract: threshold 2 is the bootstrap call, bit for bit ----------------------------------------------------------------------------
def _straddling_case():
    """tests/particle_fixtures.py's CASES[1]: R = 3 records, N = 48, 144 rows per unit: track 2 straddles the 128-row tile"""
    return dict(pfx.case_fixture(*CASES[1]), thr=0.5)


@pytest.mark.parametrize("name", ["mixed", "partial", "n300", "straddle"])
def test_threshold_two_is_the_bootstrap_call_bit_for_bit(name):
    """With ess_threshold = 2.0 every expression of the weight kernel reduces to the bootstrap kernel's (exp(0) = 1, 0 + l = l,
    1 x = x, A = N), the sums are formed in its order: every key the two calls share is equal with array_equal, every observed row
    resamples, and weights sum W = W."""
    fx = _straddling_case() if name == "straddle" else afx.fixture(name)
    out, boot = afx.call(fx, ess_threshold=2.0), afx.call(fx, fn=pr.filter_particle_records_grouped)
    assert set(boot) == BOOTSTRAP_KEYS
    same_bits(out, boot, sorted(BOOTSTRAP_KEYS), f"{name}: ")
    seen = ~np.isnan(out["lpd_joint"])
    assert np.all(out["resampled"][seen] == 1)
    live = live_rows(fx["lengths"], fx["Y"].shape[1])
    assert np.all(out["resampled"][:, live][~seen[:, live]] == 0)
    # weights sum W = W: the weights are W / sum W of the cdf the ancestors were drawn from
    w = out["weights"][seen]
    assert float(np.max(np.abs(w.sum(axis=-1) - 1.0))) <= 1e-12 and np.all(w.max(axis=-1) > 0.0)
    np.testing.assert_allclose(1.0 / np.sum(w * w, axis=-1), out["ess"][seen], rtol=1e-12)


# ---- threshold 0: sequential importance sampling --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "partial"])
def test_threshold_zero_never_resamples_and_the_propagation_does_not_read_weights(name):
    """resampled is 0 on every live row, the ancestors are the identity, and `particles` is, bit for bit, the bootstrap call's on the
    same fixture with every observation NaN: the propagation reads the draws and the particles, never the weights."""
    fx = afx.fixture(name)
    out = afx.call(fx, ess_threshold=0.0)
    live = live_rows(fx["lengths"], fx["Y"].shape[1])
    n = out["ancestors"].shape[-1]
    assert np.all(out["resampled"][:, live] == 0) and np.all(out["ancestors"][:, live] == np.arange(n))
    boot = afx.call(dict(fx, Y=np.full_like(fx["Y"], NAN)), fn=pr.filter_particle_records_grouped)
    np.testing.assert_array_equal(out["particles"], boot["particles"])
    assert np.all(np.isfinite(out["weights"][:, live])) and np.all(out["ess"][:, live] >= 1.0 - 1e-12)


@pytest.mark.parametrize("thr", [0.0, 0.5, 2.0])
def test_an_all_nan_record_is_the_bootstrap_call_bit_for_bit(thr):
    """Record 1 of `mixed` all NaN beside an observed record 0: for any threshold its arrays are the bootstrap call's."""
    fx = afx.fixture("mixed")
    Y = np.array(fx["Y"])
    Y[1] = NAN
    blind = dict(fx, Y=Y)
    out, boot = afx.call(blind, ess_threshold=thr), afx.call(blind, fn=pr.filter_particle_records_grouped)
    for k in MOMENTS + ("lpd", "lpd_joint", "ess", "log_evidence", "particles", "ancestors"):
        np.testing.assert_array_equal(out[k][:, 1], boot[k][:, 1], err_msg=k)
    assert np.all(out["resampled"][:, 1] == 0)
    np.testing.assert_array_equal(out["weights"][:, 1], np.full(out["weights"][:, 1].shape, 1.0 / out["weights"].shape[-1]))


# ---- independence ---------------------------------------------------------------------------------------------------------------------
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding():
    """`mixed` (two groups with q slices, two records, every track takes both decisions): a track alone, among the others, reversed,
    for any records_per_pass and under NaN padding, bit for bit in every key."""
    fx, a = afx.fixture("mixed"), device("mixed")
    every = TRACK + DRAWN
    nG, nR, steps = a["ess"].shape
    N, D = a["particles"].shape[-2:]
    same_bits(afx.call(fx), a, sorted(a), "two calls: ")
    for g in range(nG):
        one = afx.call(afx.subset(fx, groups=[g]))
        for k in every:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(nR):
        one = afx.call(afx.subset(fx, recs=[r]))
        for k in every:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
    one = afx.call(afx.subset(fx, groups=[1], recs=[1]))
    for k in every:
        np.testing.assert_array_equal(one[k][0, 0], a[k][1, 1], err_msg=k)
    rev = afx.call(afx.subset(fx, groups=[1, 0], recs=[1, 0]))
    for k in every:
        np.testing.assert_array_equal(rev[k], a[k][::-1, ::-1], err_msg=k)
    same_bits(afx.call(fx, records_per_pass=1), a, sorted(a), "records_per_pass 1: ")
    # padding: record 1 alone, padded from 12 to 15 rows with NaN (draws padded with zeros, uniforms with 0.5)
    C = fx["ctrl"].shape[2]
    two = afx.subset(fx, recs=[1])
    more = dict(two, Y=np.concatenate((two["Y"], np.full((1, 3, two["Y"].shape[2]), NAN)), axis=1),
                ctrl=np.concatenate((two["ctrl"], np.ones((1, 3, C))), axis=1),
                eps=np.concatenate((two["eps"], np.zeros((nG, 1, 3, N, D))), axis=2),
                unif=np.concatenate((two["unif"], np.full((nG, 1, 3), 0.5)), axis=2))
    unmasked, padded = afx.call(more, lengths=None), afx.call(more)
    for k in every:
        if k == "log_evidence":
            np.testing.assert_array_equal(padded[k][:, 0], a[k][:, 1], err_msg=k)
            np.testing.assert_array_equal(unmasked[k][:, 0], a[k][:, 1], err_msg=k)
            continue
        for o, name in ((unmasked, "unmasked"), (padded, "padded")):
            np.testing.assert_array_equal(o[k][:, 0, :steps], a[k][:, 1, :steps], err_msg=f"{k}, {name}")
        assert np.all(padded[k][:, 0, steps:] == -1) if k in ("ancestors", "resampled") else np.all(np.isnan(padded[k][:, 0, steps:])), k
    # the unmasked padding rows keep the weights they are given: no decision, the same weights row after row
    np.testing.assert_array_equal(unmasked["weights"][:, 0, steps], unmasked["weights"][:, 0, steps + 1])
    assert np.all(unmasked["resampled"][:, 0, steps:] == 0)


def test_shared_draws_are_the_same_draws_broadcast():
    """eps (steps, N, D), unif (steps,), xi0 (N, D) and their per-record layouts against the same draws broadcast to the full
    (G, R, ...) layout: bit for bit in every key."""
    fx = afx.fixture("mixed")
    nG, nR = fx["eps"].shape[:2]
    x = lambda v, n: np.ascontiguousarray(np.broadcast_to(v, (nG, nR) + v.shape[-n:]))
    for pick in (lambda v: v[0, 0], lambda v: v[0]):
        eps, unif, xi0 = pick(fx["eps"]), pick(fx["unif"]), pick(fx["xi0"])
        small = afx.call(dict(fx, eps=eps, unif=unif, xi0=xi0))
        full = afx.call(dict(fx, eps=x(eps, 3), unif=x(unif, 1), xi0=x(xi0, 2)))
        same_bits(small, full, sorted(small))


# ---- fused with the posteriors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("small", True, 3, 1)], ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_filter_adaptive_records_grouped against collapse_u_mean_grouped followed by filter_adaptive_records_grouped: the
    same posterior, the same launches, bit for bit in every key."""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), pfx.case_fixture(*args)
    gs, call = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(ess_threshold=0.3, xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True)
    fused = pr.posterior_filter_adaptive_records_grouped(Zs, kerns, Xs, Qs, call, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                         x0s=fx["x0"], **kw)
    assert set(fused) == KEYS | set(DRAWN)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_adaptive_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), fx["x0"], fx["ctrl"], fx["Y"], Qs, CC, DD, lr, fx["eps"],
                                             fx["unif"], **kw)
    same_bits(fused, two, sorted(fused))
    live = live_rows(fx["lengths"], STEPS)
    seen = live[None] & ~np.isnan(fused["lpd_joint"])
    print(f"fused {shape}: rows resampled {int((fused['resampled'] == 1).sum())} of {int(seen.sum())} observed")


# ---- seeded device draws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", pr.PARTICLE_NOISE)
def test_seeded_form_is_the_caller_drawn_form_on_particle_draws(noise):
    """adaptive_records_seeded against filter_adaptive_records_grouped on prediction.particle_draws(seed, noise, ..): bit for bit in
    every key, for two pass sizes; the fused seeded form against the seeded form."""
    fx = afx.fixture("mixed")
    gs = fx["gs"]
    nG, nR, steps, N, D = fx["eps"].shape
    d = pr.particle_draws(41, noise, nG, nR, steps, N, D, with_xi0=True)
    want = afx.call(dict(fx, eps=d["eps"], unif=d["unif"], xi0=d["xi0"]))
    Ls, Zs, kerns = afx._models(fx, "orc")
    for rpp in (0, 1):
        got = pr.adaptive_records_seeded(Ls, Zs, kerns, [g["orc"]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"],
                                         [g["Q"] for g in gs], *fx["em"], seed=41, num_particles=N, ess_threshold=fx["thr"], noise=noise,
                                         lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], records_per_pass=rpp, return_particles=True)
        assert set(got) == KEYS | set(DRAWN)
        same_bits(got, want, sorted(got), f"{noise}, records_per_pass {rpp}: ")
    assert 0 < int((want["resampled"] == 1).sum()) < int((~np.isnan(want["lpd_joint"])).sum())


def test_fused_seeded_form_against_the_fused_form_on_particle_draws():
    args = CASES[0]
    cs, fx = case(*args[:3]), pfx.case_fixture(*args)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    CC, DD, lr = fx["em"]
    nG, nR, steps, N, D = fx["eps"].shape
    d = pr.particle_draws(43, "per_record", nG, nR, steps, N, D, with_xi0=fx["S0"] is not None)
    kw = dict(ess_threshold=0.3, lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True, x0s=fx["x0"])
    want = pr.posterior_filter_adaptive_records_grouped(Zs, kerns, Xs, Qs, cs[1], fx["ctrl"], fx["Y"], CC, DD, lr, d["eps"], d["unif"],
                                                        xi0=d.get("xi0"), **kw)
    got = pr.posterior_adaptive_records_seeded(Zs, kerns, Xs, Qs, cs[1], fx["ctrl"], fx["Y"], CC, DD, lr, seed=43, num_particles=N,
                                               noise="per_record", **kw)
    same_bits(got, want, sorted(want))


# ---- an outlier ------------------------------------------------------------------------------------------------------------------------
def test_an_outlier_forty_deviations_away_keeps_everything_finite():
    """`mixed`, row 3 of record 0 moved 40 noise deviations away in every output, at thresholds 0 (the weights are carried through it)
    and 0.5: the weights are formed with the largest exponent subtracted, so everything stays finite, ess >= 1 and the ancestors stay
    in range."""
    fx = afx.fixture("mixed")
    Y, sd = np.array(fx["Y"]), np.asarray(fx["sd"]).reshape(-1)
    Y[0, 3] = np.nanmean(Y[0], axis=0) + 40.0 * sd
    n = fx["eps"].shape[3]
    for thr in (0.0, 0.5):
        out = afx.call(dict(fx, Y=Y), ess_threshold=thr)
        for k in MOMENTS + ("ess", "particles", "weights", "lpd_joint", "log_evidence"):
            assert np.all(np.isfinite(out[k])), (k, thr)
        assert np.isfinite(out["ll_all"])
        a = out["ancestors"]
        assert a.min() >= 0 and a.max() <= n - 1 and np.all(out["ess"] >= 1.0 - 1e-12)
        print(f"outlier, thr {thr}: ess of the row {np.round(out['ess'][:, 0, 3], 3).tolist()}, lpd_joint "
              f"{np.round(out['lpd_joint'][:, 0, 3], 2).tolist()}, resampled {out['resampled'][:, 0, 3].tolist()}")


# ---- poisoned scratch ------------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/adaptive_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output bit for bit, the
    reversed pass as the forward one.  The carried log-weights are written by the launch at t = 0 and by nothing else."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"adaptive{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, _ in script.CALLS:
        assert set(script.SYMBOLS) == set(clean["called/" + label].tolist()), label
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) > 60 * len(script.CALLS)
    for k in results:
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
        if k.startswith("fwd/"):
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_records_adaptive_of_the_model(actuator, U_collapse):
    mod, Yr, cr, n = _actuator_records(actuator, U_collapse)
    D, lengths, J = 4, [8, 6, 8], Yr.shape[2]
    kw = dict(lengths=lengths, Y_train_std=1.7, num_particles=128)
    live = live_rows(lengths, n)
    for draws in ("numpy", "device"):
        out = mod.filter_records_adaptive(Yr, cr, seed=7, draws=draws, return_particles=True, **kw)
        assert set(out) == KEYS | set(DRAWN)
        assert out["m_filt"].shape == (S, R, n, D) and out["predict_y"].shape == (R, n, J) and out["ll"].shape == (R,)
        assert out["resampled"].shape == (S, R, n) and out["weights"].shape == (S, R, n, 128) and out["log_evidence"].shape == (S, R)
        assert all(np.all(np.isfinite(out[k][:, live])) and np.all(np.isnan(out[k][:, ~live])) for k in MOMENTS + ("ess", "weights"))
        assert np.all(out["resampled"][:, ~live] == -1) and set(np.unique(out["resampled"][:, live])) <= {0, 1}
        again = mod.filter_records_adaptive(Yr, cr, seed=7, draws=draws, return_particles=True, **kw)
        same_bits(out, again, sorted(out), f"{draws}: ")
        other = mod.filter_records_adaptive(Yr, cr, seed=8, draws=draws, **kw)
        assert set(other) == KEYS and float(np.max(np.abs(other["m_filt"][:, live] - out["m_filt"][:, live]))) > 0.0
        print(f"actuator, draws={draws}: rows resampled {int((out['resampled'] == 1).sum())} of "
              f"{int((~np.isnan(out['lpd_joint'])).sum())} observed, median ess {float(np.nanmedian(out['ess'])):.1f}")
    # the NumPy draws are filter_records_particle's for the same seed: threshold 2 is that method, bit for bit
    always = mod.filter_records_adaptive(Yr, cr, seed=7, ess_threshold=2.0, **kw)
    boot = mod.filter_records_particle(Yr, cr, seed=7, **kw)
    same_bits(always, boot, sorted(boot))
