"""Particle smoothing of many records on the device: prediction.smooth_particle_records_grouped
(`ffvd_particle_smooth_records_grouped`), fused with the collapsed posteriors (prediction.posterior_smooth_particle_records_grouped,
`ffvd_posterior_particle_smooth_records_grouped`) and DGPSSM.smooth_records_particle.

Fixtures: those of tests/particle_fixtures.py, unchanged -- the seven cases with R = 3 records of 12 rows, ragged lengths and N = 48
(most of a 256-slab idle), and the three edges M = 300, N = 130 and N = 700 (LDS chunk and slab boundaries with ragged tails) -- plus
N = 2 and a record of one row on CASES[0].

Reference and rule.  tests/particle_smoother_ref.py (pinned in tests/test_particle_smoother_ref.py).  (1) The recursion on the
device's own downloaded stacks (particles, ancestors, weights, trans_mean, trans_var) in fp64, e_ref against the same in
np.longdouble.  (2) End to end on the oracle's posterior, e_ref from its np.longdouble composition, as tests/test_gpu_filter_particle.py
does for the filter (the identical ancestors rest on the margin condition checked there).  Error <= max(4 e_ref, floor) with `rule`
and `key_of` of the existing tests: the mean floor for m_smooth and trans_mean, the variance floor for the rest, ess_smooth as
ess_smooth / N.  Every measured error is printed; DESIGN.md section 9, "Particle smoothing", has the largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import particle_fixtures as fxt
import particle_smoother_ref as psr
import smooth_poison_script as script
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_filter_grouped import CASES
from test_gpu_filter_records import LENGTHS, R, key_of, live_rows
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, WIDE, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

N = fxt.N
SMOOTH = ("m_smooth", "S_smooth", "ess_smooth")
STACKS = ("w_smooth", "weights", "trans_mean", "trans_var")
NEW = SMOOTH + STACKS
EDGES = sorted(fxt.EDGES)
SMALL = ("n2", "one_row")
ALL = list(CASES) + EDGES + list(SMALL)


def call(fx, src="orc", **kw):
    """prediction.smooth_particle_records_grouped on a fixture (the oracle's posterior): fxt.call with the smoothing function"""
    gs = fx["gs"]
    if fx["per_model"]:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g[src]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    args = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    args.update(kw)
    return pr.smooth_particle_records_grouped(Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"],
                                              [g["Q"] for g in gs], *fx["em"], fx["eps"], fx["unif"], **args)


@functools.lru_cache(maxsize=None)
def fixture(name):
    if isinstance(name, tuple):
        return fxt.case_fixture(*name)
    if name in fxt.EDGES:
        return fxt.EDGES[name]()
    if name == "n2":                                              # two particles: one wavefront with two live lanes
        return fxt._one_record(CASES[0], 6, 2, 841)
    return fxt._one_record(CASES[0], 1, 48, 851)                  # one_row: a record of one row, no backward row at all


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture, shared by the checks below (never modified)."""
    return call(fixture(name))


@functools.lru_cache(maxsize=None)
def end_to_end(name):
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return psr.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                         fx["eps"], fx["unif"], fx["xi0"])


def judge(what, out, ref, e_ref, keys):
    worst = {}
    for k in keys:
        assert out[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        n = out["w_smooth"].shape[-1] if k == "ess_smooth" else 1
        rule(f"{what}: {k}" + (" / N" if n > 1 else ""), key_of(k) if k != "trans_mean" else "mean", out[k][ok] / n,
             np.asarray(ref[k][ok], dtype=np.float64) / n, e_ref[k])
        worst[k] = float(np.max(np.abs(out[k][ok] - ref[k][ok]))) / n
    return worst


# ---- 1. parity on the device's own stacks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_recursion_on_the_devices_own_stacks(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Particle smoothing"."""
    fx, out = fixture(name), device(name)
    ref = psr.on_stacks(out, fx["lengths"])
    wide = psr.on_stacks(out, fx["lengths"], dtype=np.longdouble) if WIDE else ref
    e_ref = {k: float(np.nanmax(np.abs(ref[k] - wide[k]))) / (ref["w_smooth"].shape[-1] if k == "ess_smooth" else 1) for k in psr.SMOOTHED}
    judge(f"own stacks {name}", out, ref, e_ref, psr.SMOOTHED)


# ---- 2. end to end on the oracle's posterior -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_end_to_end_against_the_reference(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Particle smoothing"."""
    out, (ref, e_ref) = device(name), end_to_end(name)
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judge(f"end to end {name}", out, ref, e_ref, psr.SMOOTHED + psr.KEPT)


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_exact_properties(name):
    fx, out = fixture(name), device(name)
    filt = fxt.call(fx)
    assert set(out) == set(filt) | set(NEW)
    for k in filt:                                                # the filter of the new call is the filter, bit for bit
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    G, nR, steps, n, D = out["particles"].shape
    assert out["m_smooth"].shape == (G, nR, steps, D) and out["S_smooth"].shape == (G, nR, steps, D, D)
    assert out["ess_smooth"].shape == (G, nR, steps) and out["w_smooth"].shape == out["weights"].shape == (G, nR, steps, n)
    assert out["trans_mean"].shape == out["trans_var"].shape == (G, nR, steps, n, D)
    np.testing.assert_array_equal(out["S_smooth"], np.swapaxes(out["S_smooth"], -1, -2))
    live = live_rows(fx["lengths"], steps)
    for k in NEW:                                                 # NaN (ancestors -1) at and beyond every length, finite inside
        assert np.all(np.isnan(out[k][:, ~live])) and np.all(np.isfinite(out[k][:, live])), k
    assert np.all(out["ancestors"][:, ~live] == -1)
    w = out["w_smooth"][:, live]
    assert np.all(w >= 0.0)
    err = float(np.max(np.abs(w.sum(axis=-1) - 1.0)))
    print(f"{name}: largest |sum w_smooth - 1| {err:.3e} (bound {1e-12 * steps:.1e}); smallest ess_smooth {np.min(out['ess_smooth'][:, live]):.2f}")
    assert err <= 1e-12 * steps
    e = out["ess_smooth"][:, live]
    assert np.all(e >= 1.0 - 1e-12) and np.all(e <= n * (1.0 + 1e-12))
    assert np.all(out["trans_var"][:, live] > 0.0)
    for g in range(G):
        for r, ln in enumerate(fx["lengths"]):
            for t in range(int(ln) - 1):                          # exactly 0 where a particle has no offspring
                childless = np.ones(n, dtype=bool)
                childless[out["ancestors"][g, r, t]] = False
                assert np.all(out["w_smooth"][g, r, t][childless] == 0.0), (g, r, t)
            last = int(ln) - 1                                    # the last row is the filtered one, at the rule's floors
            rule(f"{name}: last row m_smooth", "mean", out["m_smooth"][g, r, last], out["m_filt"][g, r, last], 0.0)
            rule(f"{name}: last row S_smooth", "var", out["S_smooth"][g, r, last], out["S_filt"][g, r, last], 0.0)
            rule(f"{name}: last row ess_smooth / N", "var", out["ess_smooth"][g, r, last] / n, out["ess"][g, r, last] / n, 0.0)
    # the kept terms compose the filter's X^-: trans_mean + eps sqrt(trans_var), to the rounding of one fused multiply-add
    eps = np.broadcast_to(fx["eps"], out["particles"].shape)
    comp = out["trans_mean"] + eps * np.sqrt(out["trans_var"])
    rule(f"{name}: particles from the kept terms", "mean", comp[:, live], out["particles"][:, live], 0.0)


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, a = fixture(args), device(args)
    nG = len(fx["gs"])
    b = call(fx)                                                                    # two calls
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = call(fxt.subset(fx, groups=[g]))
        for k in NEW:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = call(fxt.subset(fx, recs=[r]))
        for k in NEW:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
    one = call(fxt.subset(fx, groups=[nG - 1], recs=[1]))                           # a track alone: G = 1, R = 1
    for k in NEW:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = call(fxt.subset(fx, recs=list(range(R))[::-1]))                           # the records reversed, the draws with them
    for k in NEW:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = call(fx, records_per_pass=rpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 alone, padded from 12 to 15 rows with NaN (draws padded with zeros, uniforms with 0.5), its length kept
    n, C, D = LENGTHS[2], 0 if fx["ctrl"] is None else fx["ctrl"].shape[2], fx["x0"].shape[-1]
    two = fxt.subset(fx, recs=[2])
    more = dict(two, Y=np.concatenate((two["Y"], np.full((1, 3, J), np.nan)), axis=1),
                ctrl=np.concatenate((two["ctrl"], np.ones((1, 3, C))), axis=1) if C else None,
                eps=np.concatenate((two["eps"], np.zeros((nG, 1, 3, N, D))), axis=2),
                unif=np.concatenate((two["unif"], np.full((nG, 1, 3), 0.5)), axis=2))
    padded = call(more)
    assert padded["m_smooth"].shape[2] == STEPS + 3
    for k in NEW:
        np.testing.assert_array_equal(padded[k][:, 0, :n], a[k][:, 2, :n], err_msg=k)
        assert np.all(np.isnan(padded[k][:, 0, n:])), k


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[4]], ids=str)
def test_shared_draws_are_the_same_draws_broadcast(shape, per_model, G, qkind, mode, J, with_S0):
    fx = fixture((shape, per_model, G, qkind, mode, J, with_S0))
    nG = len(fx["gs"])
    x = lambda v, n: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (nG, R) + v.shape[-n:]))
    for pick in (lambda v: v[0, 0], lambda v: v[0]):                                # shared by all tracks; shared by the groups
        eps, unif, xi0 = pick(fx["eps"]), pick(fx["unif"]), None if fx["xi0"] is None else pick(fx["xi0"])
        small = call(dict(fx, eps=eps, unif=unif, xi0=xi0))
        full = call(dict(fx, eps=x(eps, 3), unif=x(unif, 1), xi0=x(xi0, 2)))
        for k in small:
            np.testing.assert_array_equal(small[k], full[k], err_msg=k)


# ---- 5. fused with the posteriors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_smooth_particle_records_grouped against collapse_u_mean_grouped followed by smooth_particle_records_grouped, and its
    filter keys against posterior_filter_particle_records_grouped: bit for bit in every key."""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), fixture(args)
    gs, ctrl_fit = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True)
    fused = pr.posterior_smooth_particle_records_grouped(Zs, kerns, Xs, Qs, ctrl_fit, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                         x0s=fx["x0"], **kw)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, ctrl_fit, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.smooth_particle_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), fx["x0"], fx["ctrl"], fx["Y"], Qs, CC, DD, lr, fx["eps"],
                                             fx["unif"], **kw)
    assert set(fused) == set(two) and set(NEW) <= set(fused)
    for k in fused:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    filt = pr.posterior_filter_particle_records_grouped(Zs, kerns, Xs, Qs, ctrl_fit, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                        x0s=fx["x0"], **kw)
    for k in filt:
        np.testing.assert_array_equal(fused[k], filt[k], err_msg=k)
    plain = pr.posterior_smooth_particle_records_grouped(Zs, kerns, Xs, Qs, ctrl_fit, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                         x0s=fx["x0"], **dict(kw, return_particles=False))
    assert set(plain) == set(fused) - set(STACKS) - {"particles", "ancestors"}     # without the stacks: the same moments
    for k in plain:
        np.testing.assert_array_equal(plain[k], fused[k], err_msg=k)


# ---- 6. poisoned scratch ---------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/smooth_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output bit for bit, the
    reversed pass as the forward one, finite outside the documented NaN rows."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"smooth{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, _ in script.CALLS:
        assert set(script.SYMBOLS) == set(clean["called/" + label].tolist()), label
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) > 20 * len(script.CALLS)
    for k in results:
        tag, label, form, name = k.split("/", 3)
        if name in NEW:
            lengths = clean["%s/%s/2/lengths" % (tag, label)]
            live = live_rows(lengths, clean[k].shape[2])
            assert np.all(np.isfinite(clean[k][:, live])) and np.all(np.isnan(clean[k][:, ~live])), k
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
        if tag == "fwd":
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)


# ---- 7. model level: the actuator fixture with three chains ----------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_smooth_records_particle_of_the_model(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    n, D, lengths = 8, 4, [8, 6, 8]
    Yr = np.stack([Y[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    cr = np.stack([c[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    Yr[0, 3] = np.nan
    Yr[1, 6:] = np.nan
    kw = dict(lengths=lengths, Y_train_std=1.7, num_particles=128, seed=7, return_particles=True)
    out = mod.smooth_records_particle(Yr, cr, **kw)
    filt = mod.filter_records_particle(Yr, cr, **kw)
    assert set(out) == set(filt) | set(NEW)
    for k in filt:                                                # the same seed gives the same filter
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    assert out["m_smooth"].shape == (S, R, n, D) and out["w_smooth"].shape == (S, R, n, 128)
    live = live_rows(lengths, n)
    assert all(np.all(np.isfinite(out[k][:, live])) and np.all(np.isnan(out[k][:, ~live])) for k in NEW)
    # against the given-posterior call on the model's own arguments, bit for bit
    lay, lik = mod.layers[-1], mod.likelihood
    rng = np.random.default_rng(7)
    eps, unif = rng.standard_normal((n, 128, D)), rng.random((n,))
    X = [mod._X_chains[s] for s in range(S)]
    x0 = np.broadcast_to(np.stack([x[-1] for x in X])[:, None, :], (S, R, D))
    pkw = dict(lengths=lengths, Y_train_std=1.7, return_particles=True)
    if U_collapse:
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, X, mod.control_inputs, mod.Q)
        given = pr.smooth_particle_records_grouped(list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv), x0, cr, Yr, mod.Q, lik.CC, lik.DD,
                                                   lik.log_Rchols, eps, unif, **pkw)
    else:
        given = pr.smooth_particle_records_grouped(cmo.kernel_pre_cal(lay.Z, lay.kernel), lay.Z, lay.kernel, [lay.U] * S, None, x0, cr, Yr, mod.Q,
                                                   lik.CC, lik.DD, lik.log_Rchols, eps, unif, **pkw)
    for k in out:
        np.testing.assert_array_equal(out[k], given[k], err_msg=k)
    rts = mod.filter_records(Yr, cr, lengths=lengths, Y_train_std=1.7, smooth=True)
    print(f"U_collapse={U_collapse}: largest |m_smooth - m_smooth(linearised)| {np.nanmax(np.abs(out['m_smooth'] - rts['m_smooth'])):.4f}; "
          f"ess_smooth smallest {np.min(out['ess_smooth'][:, live]):.1f}, median {np.median(out['ess_smooth'][:, live]):.1f}")
