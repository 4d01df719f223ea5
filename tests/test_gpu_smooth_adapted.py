"""Particle smoothing and backward simulation on the adapted filter's sets on the device: prediction.smooth_adapted_records_grouped /
backsim_adapted_records_grouped (`ffvd_particle_adapted_smooth_records_grouped`, `ffvd_particle_adapted_backsim_records_grouped`),
fused with the collapsed posteriors (the two posterior_ forms) and DGPSSM.smooth_records_adapted / sample_records_adapted.

Fixtures (tests/adapted_smooth_fixtures.py): the seven shared cases (R = 3 records of 12 rows, lengths (12, 12, 9), N = 48), N = 130,
300 and 700 (slab and chunk edges), N = 2, N = 2048 with 2 rows, D = 1 and D = 8 with J = 3, a record of one row, two records of 5 and 1
rows, a last row unobserved, rows with only some outputs observed, an all-NaN call, and the width fixtures at D = 7 and P = 32.

Reference and rule.  tests/particle_adapted_smooth_ref.py (pinned in tests/test_particle_adapted_smooth_ref.py) in fp64 on the oracle's
posterior; e_ref is that reference against the same composition in np.longdouble.  `ancestors` and `traj_index` must be IDENTICAL:
every fixture satisfies the forward and the backward margin condition -- checked here for the fixtures built on the device's posterior
path and in tests/test_adapted_smooth_fixtures.py, without a GPU, for the others.  Everything else: error <= max(4 e_ref, floor) with
`rule` and `judge` of the siblings (the mean floor for m_smooth, m_traj and trans_mean, the variance floor for the rest, ess_smooth as
ess_smooth / N).  The recursions are also compared on the device's own downloaded stacks (`on_stacks`), separately from end to end.
Every measured error is printed; DESIGN.md section 9, "Adapted particle smoothing", has the largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import adapted_smooth_fixtures as sfx
import adapted_smooth_poison_script as script
import particle_adapted_smooth_ref as pas
import particle_backsim_ref as pb
import test_gpu_smooth_particle as tsp
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_filter_grouped import CASES
from test_gpu_filter_records import LENGTHS, R, live_rows
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, WIDE, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

N = sfx.N
SMOOTH = ("m_smooth", "S_smooth", "ess_smooth")
KEPT = ("trans_mean", "trans_var")
NEW = {"smooth": SMOOTH + ("w_smooth",) + KEPT, "backsim": pb.DRAWN + pb.MOMENTS + KEPT}
FILTER_JUDGED = ("m_pred", "S_pred", "m_filt", "S_filt", "lpd", "lpd_joint", "particles")
BUILT_ON_THE_DEVICE = list(CASES) + list(sfx.DEVICE_EDGES)
ALL = BUILT_ON_THE_DEVICE + list(sfx.ON_THE_ORACLE)
fixture = sfx.fixture


@functools.lru_cache(maxsize=None)
def device(name, what="smooth"):
    """One device call per fixture and form, shared by the checks below (never modified)."""
    return sfx.call(fixture(name), what)


# ---- the conditions the identical indices rest on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILT_ON_THE_DEVICE, ids=str)
def test_the_indices_of_every_fixture_do_not_hang_on_rounding(name):
    """The forward and the backward margin of the cases and the two edges (the others: tests/test_adapted_smooth_fixtures.py, without a
    GPU).  A fixture that misses one gets another seed, never another bound."""
    gap, back, drift, same, _ = sfx.margins(name)
    print(f"{name}: smallest gap {gap:.3e} (backward {back:.3e}), cdf drift between the precisions {drift:.3e}, identical indices {same}")
    assert same
    assert gap >= max(1e-8, 1000.0 * drift) and back >= max(1e-8, 1000.0 * drift)


# ---- end to end on the oracle's posterior ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_smoother_end_to_end_against_the_reference(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Adapted particle smoothing"."""
    fx, out, (ref, e_ref, _) = fixture(name), device(name), sfx.reference(name)
    filt = sfx.call(fx, "filter")
    assert set(out) == set(filt) | set(NEW["smooth"])
    for k in filt:                                                # the filter of the new call is the adapted filter, bit for bit
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judged = [k for k in FILTER_JUDGED + pas.SMOOTHED + KEPT if not np.all(np.isnan(ref[k]))]
    for k in set(FILTER_JUDGED) - set(judged):                    # (lpd and lpd_joint of a call with nothing observed)
        assert out[k].shape == ref[k].shape and np.all(np.isnan(out[k])), k
    tsp.judge(f"end to end {name}", out, ref, e_ref, judged)
    G, nR, steps, n, D = out["particles"].shape
    assert out["m_smooth"].shape == (G, nR, steps, D) and out["S_smooth"].shape == (G, nR, steps, D, D)
    assert out["ess_smooth"].shape == (G, nR, steps) and out["w_smooth"].shape == (G, nR, steps, n)
    assert out["trans_mean"].shape == out["trans_var"].shape == (G, nR, steps, n, D)
    np.testing.assert_array_equal(out["S_smooth"], np.swapaxes(out["S_smooth"], -1, -2))
    live = live_rows(fx["lengths"], steps)
    for k in NEW["smooth"]:                                       # NaN at and beyond every length, finite inside
        assert np.all(np.isnan(out[k][:, ~live])) and np.all(np.isfinite(out[k][:, live])), k
    w = out["w_smooth"][:, live]
    err = float(np.max(np.abs(w.sum(axis=-1) - 1.0)))
    print(f"{name}: largest |sum w_smooth - 1| {err:.3e} (bound {1e-12 * steps:.1e}); ess_smooth smallest "
          f"{np.min(out['ess_smooth'][:, live]):.2f}, median {np.median(out['ess_smooth'][:, live]):.2f}")
    assert np.all(w >= 0.0) and err <= 1e-12 * steps
    e = out["ess_smooth"][:, live]
    assert np.all(e >= 1.0 - 1e-12) and np.all(e <= n * (1.0 + 1e-12)) and np.all(out["trans_var"][:, live] > 0.0)
    for r, ln in enumerate(fx["lengths"]):                        # the last row is uniform, exactly
        np.testing.assert_array_equal(out["w_smooth"][:, r, int(ln) - 1], np.full((G, n), 1.0 / n))
    plain = sfx.call(fx, "smooth", return_particles=False)        # without the stacks: the same moments
    assert set(plain) == set(out) - {"w_smooth", "particles", "ancestors"} - set(KEPT)
    for k in plain:
        np.testing.assert_array_equal(plain[k], out[k], err_msg=k)


@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_backward_simulation_end_to_end_against_the_reference(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Adapted particle smoothing"."""
    fx, out, sm, (ref, e_ref, _) = fixture(name), device(name, "backsim"), device(name), sfx.reference(name)
    filt = sfx.call(fx, "filter")
    assert set(out) == set(filt) | set(NEW["backsim"])
    for k in filt:
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    for k in KEPT:                                                # the kept stacks are the smoothing call's
        np.testing.assert_array_equal(out[k], sm[k], err_msg=k)
    G, nR, steps, n, D = out["particles"].shape
    B = fx["unif_bs"].shape[-1]
    assert out["trajectories"].shape == (G, nR, B, steps, D) and out["traj_index"].shape == (G, nR, steps, B)
    assert out["traj_index"].dtype == np.int32
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    np.testing.assert_array_equal(out["traj_index"], ref["traj_index"])
    live = live_rows(fx["lengths"], steps)
    assert np.all(out["traj_index"][:, ~live] == -1) and np.all(out["traj_index"][:, live] >= 0) and np.all(out["traj_index"][:, live] < n)
    for g in range(G):
        for r, ln in enumerate(fx["lengths"]):
            traj = out["trajectories"][g, r]
            assert np.all(np.isnan(traj[:, int(ln):]))
            for t in range(int(ln)):                              # the gather, bit for bit; no ancestor indirection
                np.testing.assert_array_equal(traj[:, t], out["particles"][g, r, t][out["traj_index"][g, r, t]], err_msg=f"{(g, r, t)}")
    for k, key in (("m_traj", "mean"), ("S_traj", "var"), ("lag_cov", "var")):
        assert out[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        if ok.any():
            rule(f"end to end {name}: {k}", key, out[k][ok], ref[k][ok], e_ref[k])
    np.testing.assert_array_equal(out["S_traj"], np.swapaxes(out["S_traj"], -1, -2))
    plain = sfx.call(fx, "backsim", return_particles=False)
    assert set(plain) == set(out) - {"particles", "ancestors"} - set(KEPT)
    for k in plain:
        np.testing.assert_array_equal(plain[k], out[k], err_msg=k)


# ---- the recursions on the device's own stacks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL, ids=str)
def test_the_recursions_on_the_devices_own_stacks(name):
    """Measured on one MI355X: see DESIGN.md section 9, "Adapted particle smoothing"."""
    fx, out, bs = fixture(name), device(name), device(name, "backsim")
    ref = pas.on_stacks(out, fx["lengths"])
    wide = pas.on_stacks(out, fx["lengths"], dtype=np.longdouble) if WIDE else ref
    e_ref = {k: float(np.nanmax(np.abs(ref[k] - wide[k]))) / (ref["w_smooth"].shape[-1] if k == "ess_smooth" else 1) for k in pas.SMOOTHED}
    tsp.judge(f"own stacks {name}", out, ref, e_ref, pas.SMOOTHED)
    own = pas.on_stacks(bs, fx["lengths"], fx["unif_bs"])
    print(f"{name}: backward gap on the device's own stacks {own['gap_bs']:.3e}")
    np.testing.assert_array_equal(bs["traj_index"], own["traj_index"])
    np.testing.assert_array_equal(bs["trajectories"], own["trajectories"])


# ---- independence: the call, the groups, the records, their order, the pass, the padding, the layout of the draws ----------------------
@pytest.mark.parametrize("what", ["smooth", "backsim"])
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0, what):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, a = fixture(args), device(args, what)
    nG, keys = len(fx["gs"]), NEW[what] + ("particles", "ancestors", "m_filt", "ess", "log_evidence")
    rows = lambda k, v: np.swapaxes(v, 2, 3) if k == "trajectories" else v
    b = sfx.call(fx, what)                                                          # two calls
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = sfx.call(sfx.subset(fx, groups=[g]), what)
        for k in keys:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = sfx.call(sfx.subset(fx, recs=[r]), what)
        for k in keys:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
    one = sfx.call(sfx.subset(fx, groups=[nG - 1], recs=[1]), what)                 # a track alone: G = 1, R = 1
    for k in keys:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = sfx.call(sfx.subset(fx, recs=list(range(R))[::-1]), what)                 # the records reversed, the draws with them
    for k in keys:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = sfx.call(fx, what, records_per_pass=rpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 alone, padded from 12 to 15 rows with NaN (draws padded with zeros, uniforms with 0.5), its length kept
    n, C, D = LENGTHS[2], 0 if fx["ctrl"] is None else fx["ctrl"].shape[2], fx["x0"].shape[-1]
    two = sfx.subset(fx, recs=[2])
    more = dict(two, Y=np.concatenate((two["Y"], np.full((1, 3, J), np.nan)), axis=1),
                ctrl=np.concatenate((two["ctrl"], np.ones((1, 3, C))), axis=1) if C else None,
                eps=np.concatenate((two["eps"], np.zeros((nG, 1, 3, N, D))), axis=2),
                unif=np.concatenate((two["unif"], np.full((nG, 1, 3), 0.5)), axis=2),
                unif_bs=np.concatenate((two["unif_bs"], np.full((nG, 1, 3, 3), 0.5)), axis=2))
    padded = sfx.call(more, what)
    assert padded["m_pred"].shape[2] == STEPS + 3
    for k in NEW[what]:
        np.testing.assert_array_equal(rows(k, padded[k])[:, 0, :n], rows(k, a[k])[:, 2, :n], err_msg=k)
        tail = rows(k, padded[k])[:, 0, n:]
        assert np.all(tail == -1) if k == "traj_index" else np.all(np.isnan(tail)), k


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[4]], ids=str)
def test_shared_draws_are_the_same_draws_broadcast(shape, per_model, G, qkind, mode, J, with_S0):
    """eps, unif, xi0 and unif_bs in their shared and per-record layouts against the same draws broadcast to the full layout: bit for
    bit in every key; trajectory b depends on column b of unif_bs alone."""
    fx = fixture((shape, per_model, G, qkind, mode, J, with_S0))
    nG = len(fx["gs"])
    x = lambda v, n: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (nG, R) + v.shape[-n:]))
    for pick in (lambda v: v[0, 0], lambda v: v[0]):                                # shared by all tracks; shared by the groups
        eps, unif, xi0, ub = pick(fx["eps"]), pick(fx["unif"]), None if fx["xi0"] is None else pick(fx["xi0"]), pick(fx["unif_bs"])
        for what in ("smooth", "backsim"):
            small = sfx.call(dict(fx, eps=eps, unif=unif, xi0=xi0, unif_bs=ub), what)
            full = sfx.call(dict(fx, eps=x(eps, 3), unif=x(unif, 1), xi0=x(xi0, 2), unif_bs=x(ub, 2)), what)
            for k in small:
                np.testing.assert_array_equal(small[k], full[k], err_msg=k)
    wide = np.random.default_rng(78).random((nG, R, STEPS, 37))
    few, many = sfx.call(dict(fx, unif_bs=wide[..., :5]), "backsim"), sfx.call(dict(fx, unif_bs=wide), "backsim")
    np.testing.assert_array_equal(few["traj_index"], many["traj_index"][..., :5])
    np.testing.assert_array_equal(few["trajectories"], many["trajectories"][:, :, :5])


# ---- fused with the posteriors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_forms_against_the_two_calls(shape, per_model, G, J):
    """posterior_smooth_adapted_records_grouped and posterior_backsim_adapted_records_grouped against collapse_u_mean_grouped followed
    by the given-posterior calls, and their filter keys against posterior_filter_adapted_records_grouped: bit for bit in every key."""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), fixture(args)
    gs, ctrl_fit = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, ctrl_fit, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    filt = pr.posterior_filter_adapted_records_grouped(Zs, kerns, Xs, Qs, ctrl_fit, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                       x0s=fx["x0"], **kw)
    for what, tail in (("smooth", ()), ("backsim", (fx["unif_bs"],))):
        fused = getattr(pr, f"posterior_{what}_adapted_records_grouped")(Zs, kerns, Xs, Qs, ctrl_fit, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"],
                                                                         fx["unif"], *tail, x0s=fx["x0"], **kw)
        two = getattr(pr, f"{what}_adapted_records_grouped")(Ls, Zs, kerns, list(U), list(Hinv), fx["x0"], fx["ctrl"], fx["Y"], Qs, CC, DD, lr,
                                                             fx["eps"], fx["unif"], *tail, **kw)
        assert set(fused) == set(two) == set(filt) | set(NEW[what])
        for k in fused:
            np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
        for k in filt:
            np.testing.assert_array_equal(fused[k], filt[k], err_msg=k)


# ---- nothing observed: the bootstrap recursions, bit for bit -----------------------------------------------------------------------------
def test_with_every_observation_missing_both_recursions_are_the_bootstrap_calls():
    """An all-NaN call: identity ancestors and unit weights, so the two recursions coincide with the bootstrap smoother's and the
    bootstrap backward simulation's on the same draws."""
    fx = fixture("all_nan")
    sm, boot = device("all_nan"), sfx.call(fx, "boot_smooth")
    for k in ("w_smooth", "m_smooth", "S_smooth", "ess_smooth", "trans_mean", "trans_var", "particles", "ancestors"):
        np.testing.assert_array_equal(sm[k], boot[k], err_msg=k)
    np.testing.assert_array_equal(boot["weights"], np.ones(boot["weights"].shape))
    bs, bboot = device("all_nan", "backsim"), sfx.call(fx, "boot_backsim")
    for k in ("traj_index", "trajectories", "m_traj", "S_traj", "lag_cov"):
        np.testing.assert_array_equal(bs[k], bboot[k], err_msg=k)


def test_a_record_of_one_row_is_the_plain_mean_of_its_filtered_set():
    """n = 1: the unweighted particle estimate (not the Rao-Blackwellised m_filt), at the rule's floors"""
    out = device("one_row")
    X = out["particles"][:, 0, 0]
    rule("one_row: m_smooth", "mean", out["m_smooth"][:, 0, 0], X.mean(axis=1), 0.0)
    dx = X - X.mean(axis=1)[:, None, :]
    rule("one_row: S_smooth", "var", out["S_smooth"][:, 0, 0], np.einsum("gni,gnj->gij", dx, dx) / X.shape[1], 0.0)
    np.testing.assert_array_equal(out["ess_smooth"][:, 0, 0], np.full(X.shape[0], float(X.shape[1])))
    assert np.all(np.isnan(device("one_row", "backsim")["lag_cov"]))


# ---- poisoned scratch --------------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/adapted_smooth_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output of the four
    entry points bit for bit, the reversed pass as the forward one, finite outside the documented NaN rows."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"adapted_smooth{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, _ in script.CALLS:
        assert set(script.SYMBOLS) == set(clean["called/" + label].tolist()), label
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) > 80 * len(script.CALLS)
    for k in results:
        tag, label, form, name = k.split("/", 3)
        if name in NEW["smooth"] + NEW["backsim"]:
            lengths = clean["%s/%s/4/lengths" % (tag, label)]
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


# ---- model level: the actuator fixture with three chains ---------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_smooth_and_sample_records_adapted_of_the_model(actuator, U_collapse):
    """N = 128, B = 512, 8 rows: the same seed gives the adapted filter; |m_traj - m_smooth| <= 6 sqrt(diag S_smooth / B) (given the
    filter's run the trajectories are independent draws whose marginals are w_smooth); both calls against the given-posterior calls on
    the model's own arguments, bit for bit.  The smallest and the median ess_smooth are printed beside the bootstrap smoother's on the
    same draws (reported, not asserted)."""
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
    sm = mod.smooth_records_adapted(Yr, cr, **kw)
    out = mod.sample_records_adapted(Yr, cr, num_trajectories=B, **kw)
    filt = mod.filter_records_adapted(Yr, cr, **kw)
    assert set(sm) == set(filt) | set(NEW["smooth"]) and set(out) == set(filt) | set(NEW["backsim"])
    for k in filt:                                                # the same seed gives the same filter
        np.testing.assert_array_equal(sm[k], filt[k], err_msg=k)
        np.testing.assert_array_equal(out[k], filt[k], err_msg=k)
    for k in KEPT:
        np.testing.assert_array_equal(out[k], sm[k], err_msg=k)
    assert sm["m_smooth"].shape == (S, R, n, D) and sm["w_smooth"].shape == (S, R, n, 128)
    assert out["trajectories"].shape == (S, R, B, n, D) and out["traj_index"].shape == (S, R, n, B)
    live = live_rows(lengths, n)
    assert all(np.all(np.isfinite(sm[k][:, live])) and np.all(np.isnan(sm[k][:, ~live])) for k in NEW["smooth"])
    assert np.all(np.isfinite(out["m_traj"][:, live])) and np.all(np.isnan(out["m_traj"][:, ~live]))
    ratio = np.abs(out["m_traj"] - sm["m_smooth"])[:, live] / np.sqrt(np.diagonal(sm["S_smooth"], axis1=-2, axis2=-1)[:, live] / B)
    boot = mod.smooth_records_particle(Yr, cr, **kw)
    print(f"U_collapse={U_collapse}: largest |m_traj - m_smooth| / sqrt(diag S_smooth / B) {float(np.max(ratio)):.3f} (bound 6); ess_smooth "
          f"smallest {np.min(sm['ess_smooth'][:, live]):.1f}, median {np.median(sm['ess_smooth'][:, live]):.1f} (bootstrap smoother on the "
          f"same draws: {np.min(boot['ess_smooth'][:, live]):.1f}, {np.median(boot['ess_smooth'][:, live]):.1f})")
    assert np.all(ratio <= 6.0)
    # against the given-posterior calls on the model's own arguments, bit for bit
    lay, lik = mod.layers[-1], mod.likelihood
    rng = np.random.default_rng(7)
    eps, unif = rng.standard_normal((n, 128, D)), rng.random((n,))
    ub = rng.random((n, B))
    X = [mod._X_chains[s] for s in range(S)]
    x0 = np.broadcast_to(np.stack([x[-1] for x in X])[:, None, :], (S, R, D))
    pkw = dict(lengths=lengths, Y_train_std=1.7, return_particles=True)
    if U_collapse:
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, X, mod.control_inputs, mod.Q)
        head = (list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv))
    else:
        head = (cmo.kernel_pre_cal(lay.Z, lay.kernel), lay.Z, lay.kernel, [lay.U] * S, None)
    given = pr.smooth_adapted_records_grouped(*head, x0, cr, Yr, mod.Q, lik.CC, lik.DD, lik.log_Rchols, eps, unif, **pkw)
    for k in sm:
        np.testing.assert_array_equal(sm[k], given[k], err_msg=k)
    given = pr.backsim_adapted_records_grouped(*head, x0, cr, Yr, mod.Q, lik.CC, lik.DD, lik.log_Rchols, eps, unif, ub, **pkw)
    for k in out:
        np.testing.assert_array_equal(out[k], given[k], err_msg=k)
