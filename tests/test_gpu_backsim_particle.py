"""Particle backward simulation of many records on the device: prediction.backsim_particle_records_grouped
(`ffvd_particle_backsim_records_grouped`), fused with the collapsed posteriors (prediction.posterior_backsim_particle_records_grouped,
`ffvd_posterior_particle_backsim_records_grouped`) and DGPSSM.sample_records_particle.

Fixtures: tests/backsim_particle_fixtures.py -- those of tests/particle_fixtures.py with seeded uniforms: N = 2, 13, 48, 130, 700
(three particles per thread) and 2048 (eight), D = 1, 2, 3, 4, 8, B = 1, 3 and 300 (the moments kernel strides), a record of one row,
ragged lengths, a last row unobserved, a record that is all NaN, start covariances, J = 3.

Reference and rule.  tests/particle_backsim_ref.py (pinned in tests/test_particle_backsim_ref.py).  Indices are compared exactly, which
rests on the margin condition checked first: fp64 and np.longdouble draw identical indices and no threshold lies closer to a cdf entry
than max(1e-8, 1000 x the drift of the cdf between the two).  Moments: NumPy on the device's own trajectories, error <=
max(4 e_ref, floor) with `rule` of the existing tests, e_ref the fp64-against-longdouble error of that NumPy.  Every measured error is
printed; DESIGN.md section 9, "Particle backward simulation", has the largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import backsim_particle_fixtures as bfx
import backsim_poison_script as script
import particle_backsim_ref as pb
import particle_fixtures as fxt
import test_gpu_smooth_particle as tsp
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_filter_grouped import CASES
from test_gpu_filter_records import LENGTHS, R, live_rows
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, WIDE, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

N = fxt.N
NEW = pb.DRAWN + pb.MOMENTS
KEPT = ("weights", "trans_mean", "trans_var")
ALL = bfx.NAMES
fixture, call = bfx.fixture, bfx.call


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture, shared by the checks below (never modified)."""
    return call(fixture(name))


# ---- 1. the margin condition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_margin_condition_holds(name):
    """The filter's thresholds and the backward ones, on the oracle's posterior in fp64 and np.longdouble."""
    fx = fixture(name)
    ref, _, wide = bfx.reference(name)
    gap, drift, same = pb.margin(ref, fx["unif"], wide)
    print(f"{name}: gap {gap:.3e} (backward {ref['gap_bs']:.3e}), drift {drift:.3e}")
    assert same and gap >= max(1e-8, 1000.0 * drift)


# ---- 2. the indices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_indices_are_the_references(name):
    """IDENTICAL to the reference run on the device's own downloaded stacks, and to the reference on the oracle's posterior end to end"""
    fx, out = fixture(name), device(name)
    own = pb.on_stacks(out, fx["lengths"], fx["unif_bs"])
    print(f"{name}: gap on the device's own stacks {own['gap_bs']:.3e}")
    assert out["traj_index"].dtype == np.int32 and out["traj_index"].shape == own["traj_index"].shape
    np.testing.assert_array_equal(out["traj_index"], own["traj_index"])
    ref = bfx.reference(name)[0]
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    np.testing.assert_array_equal(out["traj_index"], ref["traj_index"])


# ---- 3. the gather, 4. the moments, the shapes and the NaN rows --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_gather_and_the_moments(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Particle backward simulation"."""
    fx, out = fixture(name), device(name)
    G, nR, steps, n, D = out["particles"].shape
    B = fx["unif_bs"].shape[-1]
    assert out["trajectories"].shape == (G, nR, B, steps, D) and out["traj_index"].shape == (G, nR, steps, B)
    assert out["m_traj"].shape == (G, nR, steps, D) and out["S_traj"].shape == out["lag_cov"].shape == (G, nR, steps, D, D)
    live = live_rows(fx["lengths"], steps)
    assert np.all(out["traj_index"][:, ~live] == -1) and np.all(out["traj_index"][:, live] >= 0) and np.all(out["traj_index"][:, live] < n)
    for g in range(G):
        for r, ln in enumerate(fx["lengths"]):
            ln = int(ln)
            traj = out["trajectories"][g, r]
            assert np.all(np.isnan(traj[:, ln:]))
            for t in range(ln):                                   # the gather, bit for bit
                np.testing.assert_array_equal(traj[:, t], out["particles"][g, r, t][out["traj_index"][g, r, t]], err_msg=f"{(g, r, t)}")
            m, Sm, lag = pb.moments(traj[:, :ln])
            wide = pb.moments(traj[:, :ln], np.longdouble) if WIDE else (m, Sm, lag)
            for k, key, ref, w in (("m_traj", "mean", m, wide[0]), ("S_traj", "var", Sm, wide[1]), ("lag_cov", "var", lag, wide[2])):
                dev = out[k][g, r]
                assert np.all(np.isnan(dev[ln:])), k
                rows = ln - 1 if k == "lag_cov" else ln
                assert k != "lag_cov" or np.all(np.isnan(dev[ln - 1]))
                if rows:
                    e_ref = float(np.max(np.abs(ref[:rows] - w[:rows])))
                    rule(f"{name} track {(g, r)}: {k}", key, dev[:rows], ref[:rows], e_ref)
    np.testing.assert_array_equal(out["S_traj"], np.swapaxes(out["S_traj"], -1, -2))


# ---- 5. the filter's keys and the kept stacks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_filter_is_the_filter_and_the_stacks_are_the_smoothers(name):
    fx, out = fixture(name), device(name)
    filt, sm = fxt.call(fx), tsp.call(fx)
    assert set(out) == set(filt) | set(NEW) | set(KEPT)
    for k in filt:
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    for k in KEPT:
        np.testing.assert_array_equal(out[k], sm[k], err_msg=k)
    plain = call(fx, return_particles=False)                      # without the stacks: the same draws and moments
    assert set(plain) == set(out) - set(KEPT) - {"particles", "ancestors"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], out[k], err_msg=k)


# ---- 6. invariance -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, a = fixture(args), device(args)
    nG = len(fx["gs"])
    b = call(fx)                                                                    # two calls
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    keys = NEW + KEPT
    for g in range(nG):                                                             # a group alone
        one = call(bfx.subset(fx, groups=[g]))
        for k in keys:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = call(bfx.subset(fx, recs=[r]))
        for k in keys:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
    one = call(bfx.subset(fx, groups=[nG - 1], recs=[1]))                           # a track alone: G = 1, R = 1
    for k in keys:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = call(bfx.subset(fx, recs=list(range(R))[::-1]))                           # the records reversed, the draws with them
    for k in keys:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = call(fx, records_per_pass=rpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 alone, padded from 12 to 15 rows with NaN (draws padded with zeros, uniforms with 0.5), its length kept
    n, C, D = LENGTHS[2], 0 if fx["ctrl"] is None else fx["ctrl"].shape[2], fx["x0"].shape[-1]
    two = bfx.subset(fx, recs=[2])
    more = dict(two, Y=np.concatenate((two["Y"], np.full((1, 3, J), np.nan)), axis=1),
                ctrl=np.concatenate((two["ctrl"], np.ones((1, 3, C))), axis=1) if C else None,
                eps=np.concatenate((two["eps"], np.zeros((nG, 1, 3, N, D))), axis=2),
                unif=np.concatenate((two["unif"], np.full((nG, 1, 3), 0.5)), axis=2),
                unif_bs=np.concatenate((two["unif_bs"], np.full((nG, 1, 3, 3), 0.5)), axis=2))
    padded = call(more)
    assert padded["m_traj"].shape[2] == STEPS + 3 and padded["trajectories"].shape[3] == STEPS + 3
    for k in keys:
        rows = (lambda v: np.swapaxes(v, 2, 3)) if k == "trajectories" else (lambda v: v)
        np.testing.assert_array_equal(rows(padded[k])[:, 0, :n], rows(a[k])[:, 2, :n], err_msg=k)
        tail = rows(padded[k])[:, 0, n:]
        assert np.all(tail == -1) if k == "traj_index" else np.all(np.isnan(tail)), k


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[4]], ids=str)
def test_a_trajectory_depends_on_its_own_column_alone_and_shared_uniforms_are_the_same_uniforms_broadcast(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    fx = fixture((shape, per_model, G, qkind, mode, J, with_S0))
    nG = len(fx["gs"])
    wide = np.random.default_rng(77).random((nG, R, STEPS, 37))
    few, many = call(dict(fx, unif_bs=wide[..., :5])), call(dict(fx, unif_bs=wide))        # trajectory b of B = 5 and of B = 37
    np.testing.assert_array_equal(few["traj_index"], many["traj_index"][..., :5])
    np.testing.assert_array_equal(few["trajectories"], many["trajectories"][:, :, :5])
    for k in KEPT:
        np.testing.assert_array_equal(few[k], many[k], err_msg=k)
    for pick in (lambda v: v[0, 0], lambda v: v[0]):                                # shared by all tracks; shared by the groups
        ub = pick(wide[..., :5])
        small = call(dict(fx, unif_bs=ub))
        full = call(dict(fx, unif_bs=np.ascontiguousarray(np.broadcast_to(ub, (nG, R, STEPS, 5)))))
        for k in small:
            np.testing.assert_array_equal(small[k], full[k], err_msg=k)


# ---- fused with the posteriors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("small", True, 3, 1)], ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_backsim_particle_records_grouped against collapse_u_mean_grouped followed by backsim_particle_records_grouped: bit
    for bit in every key."""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), fixture(args)
    gs, ctrl_fit = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True)
    fused = pr.posterior_backsim_particle_records_grouped(Zs, kerns, Xs, Qs, ctrl_fit, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                          fx["unif_bs"], x0s=fx["x0"], **kw)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, ctrl_fit, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.backsim_particle_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), fx["x0"], fx["ctrl"], fx["Y"], Qs, CC, DD, lr, fx["eps"],
                                              fx["unif"], fx["unif_bs"], **kw)
    assert set(fused) == set(two) and set(NEW) <= set(fused)
    for k in fused:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)


# ---- 7. model level: the actuator fixture with three chains --------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_sample_records_particle_of_the_model(actuator, U_collapse):
    """N = 128, B = 512, 8 rows: |m_traj - m_smooth| <= 6 sqrt(diag S_smooth / B) (given the filter's run the trajectories are
    independent draws whose marginals are w_smooth).  Measured on one MI355X: see DESIGN.md section 9."""
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    n, D, B, lengths = 8, 4, 512, [8, 6, 8]
    Yr = np.stack([Y[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    cr = np.stack([c[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    Yr[0, 3] = np.nan
    Yr[1, 6:] = np.nan
    kw = dict(lengths=lengths, Y_train_std=1.7, num_particles=128, seed=7, return_particles=True)
    out = mod.sample_records_particle(Yr, cr, num_trajectories=B, **kw)
    sm = mod.smooth_records_particle(Yr, cr, **kw)
    filt = mod.filter_records_particle(Yr, cr, **kw)
    assert set(out) == set(filt) | set(NEW) | set(KEPT)
    for k in filt:                                                # the same seed gives the same filter
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    for k in KEPT:
        np.testing.assert_array_equal(out[k], sm[k], err_msg=k)
    assert out["trajectories"].shape == (S, R, B, n, D) and out["traj_index"].shape == (S, R, n, B)
    live = live_rows(lengths, n)
    assert np.all(np.isfinite(out["m_traj"][:, live])) and np.all(np.isnan(out["m_traj"][:, ~live]))
    ratio = np.abs(out["m_traj"] - sm["m_smooth"])[:, live] / np.sqrt(np.diagonal(sm["S_smooth"], axis1=-2, axis2=-1)[:, live] / B)
    print(f"U_collapse={U_collapse}: largest |m_traj - m_smooth| / sqrt(diag S_smooth / B) {float(np.max(ratio)):.3f} (bound 6)")
    assert np.all(ratio <= 6.0)
    # against the given-posterior call on the model's own arguments, bit for bit
    lay, lik = mod.layers[-1], mod.likelihood
    rng = np.random.default_rng(7)
    eps, unif = rng.standard_normal((n, 128, D)), rng.random((n,))
    ub = rng.random((n, B))
    X = [mod._X_chains[s] for s in range(S)]
    x0 = np.broadcast_to(np.stack([x[-1] for x in X])[:, None, :], (S, R, D))
    pkw = dict(lengths=lengths, Y_train_std=1.7, return_particles=True)
    if U_collapse:
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, X, mod.control_inputs, mod.Q)
        given = pr.backsim_particle_records_grouped(list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv), x0, cr, Yr, mod.Q, lik.CC, lik.DD,
                                                    lik.log_Rchols, eps, unif, ub, **pkw)
    else:
        given = pr.backsim_particle_records_grouped(cmo.kernel_pre_cal(lay.Z, lay.kernel), lay.Z, lay.kernel, [lay.U] * S, None, x0, cr, Yr, mod.Q,
                                                    lik.CC, lik.DD, lik.log_Rchols, eps, unif, ub, **pkw)
    for k in out:
        np.testing.assert_array_equal(out[k], given[k], err_msg=k)


# ---- 8. poisoned scratch -------------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/backsim_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output bit for bit, the
    reversed pass as the forward one, finite outside the documented NaN rows."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"backsim{mode}.npz")
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
        if name in NEW + KEPT:
            lengths = clean["%s/%s/2/lengths" % (tag, label)]
            v = np.swapaxes(clean[k], 2, 3) if name == "trajectories" else clean[k]
            live = live_rows(lengths, v.shape[2])
            if name == "traj_index":
                assert np.all(v[:, live] >= 0) and np.all(v[:, ~live] == -1), k
            elif name == "lag_cov":
                last = np.arange(v.shape[2])[None, :] == np.asarray(lengths)[:, None] - 1
                assert np.all(np.isfinite(v[:, live & ~last])) and np.all(np.isnan(v[:, ~live | last])), k
            else:
                assert np.all(np.isfinite(v[:, live])) and np.all(np.isnan(v[:, ~live])), k
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
        if tag == "fwd":
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)
