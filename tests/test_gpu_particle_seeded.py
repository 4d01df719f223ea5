"""Seeded particle draws generated on the device: prediction.particle_draws (`ffvd_particle_draws`), prediction.particle_records_seeded
(`ffvd_particle_seeded_records_grouped`), posterior_particle_records_seeded (`ffvd_posterior_particle_seeded_records_grouped`) and
DGPSSM.particle_records_seeded.

The draws against tests/particle_draws_ref.py (pinned in tests/test_particle_draws_ref.py): the uniform streams are exact and must be
IDENTICAL; the normal streams by the rule of tests/test_gpu_filter_records.py, error <= max(4 e_ref, 2e-14) per array against the
np.longdouble map, e_ref the fp64 reference's own distance from it.  The floor: the device rounds no argument (sincospi of the exact
2 u2) and log, sqrt, sincospi and the product add a few ulp of a result of at most 8.58 -- 8.58 x 8 x 2^-53 = 7.6e-15.  The shapes
are the smallest with more than one workgroup per block (12 x 48 x 4 = 2304 doubles = 1152 pairs = 4.5 workgroups), blocks of odd length
(65, 15: the last pair is half; the odd blocks after the first start 8 bytes off a 16-byte boundary and take the 8-byte stores) and
single-workgroup blocks (60).

The contract: a seeded call equals, in every key and bit for bit, the existing entry point of its (rule, stage) fed
particle_draws(seed, noise, ..) -- on the R = 3, 12-row, N = 48 and the N = 13 fixtures of tests/cache_poison_script.py (a track
crosses a row tile; the scan chunk is ragged).  Every measured error is printed; DESIGN.md section 9, "Device draws", has the
largest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cache_poison_script as base
import particle_draws_ref as pdr
import particle_fixtures as fxt
import seeded_poison_script as script
from ffvd_amd import prediction as pr
from test_gpu_filter_adapted import _actuator_records
from test_gpu_moment_grouped import S

pytestmark = pytest.mark.gpu

NOISE = ("shared", "per_record", "independent")
SEED = 0xC0FFEE1234567890
B = 5
# (G, R, steps, N, D, B)
SHAPES = [(3, 3, 12, 48, 4, 5), (2, 1, 5, 13, 1, 3), (1, 2, 4, 5, 3, 1)]
SIBLINGS = {("bootstrap", "filter"): "filter_particle_records_grouped", ("bootstrap", "smooth"): "smooth_particle_records_grouped",
            ("bootstrap", "backsim"): "backsim_particle_records_grouped", ("adapted", "filter"): "filter_adapted_records_grouped",
            ("adapted", "smooth"): "smooth_adapted_records_grouped", ("adapted", "backsim"): "backsim_adapted_records_grouped"}


@functools.lru_cache(maxsize=None)
def device_draws(seed, noise, G, R, steps, N, D, nb, with_xi0=True):
    """One device call per shape and mode, shared by the checks below (never modified)."""
    return pr.particle_draws(seed, noise, G, R, steps, N, D, with_xi0=with_xi0, B=nb)


@functools.lru_cache(maxsize=None)
def reference_draws(seed, noise, G, R, steps, N, D, nb):
    return (pdr.draws(seed, noise, G, R, steps, N, D, with_xi0=True, B=nb),
            pdr.draws(seed, noise, G, R, steps, N, D, with_xi0=True, B=nb, dtype=np.longdouble))


# ---- 1. the draws against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_draws_against_the_reference(shape, noise):
    """Measured on one MI355X: see DESIGN.md section 9, "Device draws"."""
    G, R, steps, N, D, nb = shape
    out, (ref, wide) = device_draws(SEED, noise, *shape), reference_draws(SEED, noise, *shape)
    lead = pdr.lead_shape(noise, G, R)
    assert set(out) == {"eps", "unif", "xi0", "unif_bs"}
    assert out["eps"].shape == lead + (steps, N, D) and out["unif"].shape == lead + (steps,)
    assert out["xi0"].shape == lead + (N, D) and out["unif_bs"].shape == lead + (steps, nb)
    for k in ("unif", "unif_bs"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
        assert np.all(out[k] >= 0.0) and np.all(out[k] < 1.0)
    for k in ("eps", "xi0"):
        e_ref = float(np.max(np.abs(ref[k] - wide[k])))
        err = float(np.max(np.abs(out[k] - wide[k])))
        bound = max(4.0 * e_ref, 2e-14)
        print(f"draws {shape} {noise}: {k}: max error {err:.3e}, e_ref {e_ref:.3e}, bound {bound:.3e}, max |z| {float(np.max(np.abs(out[k]))):.3f}")
        assert np.all(np.isfinite(out[k])) and err <= bound, k
    again = pr.particle_draws(SEED, noise, G, R, steps, N, D, with_xi0=True, B=nb)                # a seed: the same arrays
    for k in out:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    other = pr.particle_draws(SEED + 1, noise, G, R, steps, N, D)
    assert set(other) == {"eps", "unif"} and not np.any(other["eps"] == out["eps"])


def test_a_smaller_call_is_a_slice_of_a_larger_one():
    big = device_draws(SEED, "independent", *SHAPES[0])
    small = pr.particle_draws(SEED, "independent", 2, 2, 5, 48, 4, with_xi0=True, B=5)
    np.testing.assert_array_equal(small["eps"], big["eps"][:2, :2, :5])
    np.testing.assert_array_equal(small["unif"], big["unif"][:2, :2, :5])
    np.testing.assert_array_equal(small["xi0"], big["xi0"][:2, :2])
    np.testing.assert_array_equal(small["unif_bs"], big["unif_bs"][:2, :2, :5])
    per, shared = device_draws(SEED, "per_record", *SHAPES[0]), device_draws(SEED, "shared", *SHAPES[0])
    for k in big:                                                                            # the modes zero the group and the record word
        np.testing.assert_array_equal(per[k], big[k][0], err_msg=k)
        np.testing.assert_array_equal(shared[k], big[k][0, 0], err_msg=k)


# ---- 2. the contract -----------------------------------------------------------------------------------------------------------------------
# fixture, N, rule, stage, noise, posterior form: every value of every axis, with a start covariance (m300) and without
CONTRACT = [("ragged", 48, "bootstrap", "filter", "shared", False), ("ragged", 13, "bootstrap", "smooth", "per_record", True),
            ("ragged", 13, "bootstrap", "backsim", "independent", False), ("ragged", 48, "adapted", "filter", "shared", True),
            ("m130", 48, "adapted", "filter", "independent", True), ("m130", 13, "adapted", "smooth", "shared", False),
            ("m130", 13, "adapted", "backsim", "per_record", True), ("d8", 13, "bootstrap", "filter", "per_record", True),
            ("d8", 48, "bootstrap", "smooth", "independent", False), ("d8", 13, "adapted", "backsim", "shared", False),
            ("m300", 48, "bootstrap", "filter", "independent", False), ("m300", 13, "bootstrap", "smooth", "shared", True),
            ("m300", 48, "bootstrap", "backsim", "per_record", True), ("m300", 13, "adapted", "filter", "per_record", False),
            ("m300", 48, "adapted", "smooth", "independent", True), ("m300", 13, "adapted", "backsim", "independent", False)]


def _seeded(fx, posterior, **kw):
    if posterior:
        return pr.posterior_particle_records_seeded(*base._fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"], x0s=fx["x0"], groups_per_pass=1, **kw)
    return pr.particle_records_seeded(*base._models(fx), fx["x0"], fx["ctrl"], fx["Y"], base._Qs(fx), *fx["em"], **kw)


def _sibling(fx, posterior, rule, stage, d, **kw):
    name = SIBLINGS[rule, stage]
    tail = (d["eps"], d["unif"]) + ((d["unif_bs"],) if stage == "backsim" else ())
    kw = dict(kw, xi0=d.get("xi0"))
    if posterior:
        return getattr(pr, "posterior_" + name)(*base._fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"], *tail, x0s=fx["x0"], groups_per_pass=1,
                                                **kw)
    return getattr(pr, name)(*base._models(fx), fx["x0"], fx["ctrl"], fx["Y"], base._Qs(fx), *fx["em"], *tail, **kw)


def _dims(fx):
    return len(fx["gs"]), fx["Y"].shape[0], fx["Y"].shape[1], fx["x0"].shape[-1]


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert np.shape(a[k]) == np.shape(b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, (what, k)
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("name,n,rule,stage,noise,posterior", CONTRACT, ids=str)
def test_a_seeded_call_is_the_existing_entry_point_on_the_returned_draws(name, n, rule, stage, noise, posterior):
    fx = base._fixture(name)
    G, R, steps, D = _dims(fx)
    nb = B if stage == "backsim" else 0
    seed = 2 ** 64 - 1 - n
    common = dict(lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], records_per_pass=base._rpp(fx), return_particles=True)
    got = _seeded(fx, posterior, seed=seed, num_particles=n, rule=rule, stage=stage, noise=noise, num_trajectories=nb, **common)
    d = device_draws(seed, noise, G, R, steps, n, D, nb, fx["S0"] is not None)
    want = _sibling(fx, posterior, rule, stage, d, **common)
    _same(got, want, f"{name} n={n} {rule} {stage} {noise}")
    assert "ess" in got and "log_evidence" in got and "particles" in got
    assert ("m_smooth" in got) == (stage == "smooth") and ("trajectories" in got) == (stage == "backsim")
    assert ("weights" in got) == (stage != "filter" and rule == "bootstrap")
    live = np.arange(steps)[None, :] < np.asarray(fx["lengths"])[:, None]
    assert np.all(np.isfinite(got["m_filt"][:, live])) and np.all(np.isfinite(got["log_evidence"]))


# ---- 3. pass independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,stage", [("bootstrap", "smooth"), ("adapted", "backsim")], ids=str)
def test_records_per_pass_changes_nothing(rule, stage):
    fx = base._fixture("m130")
    kw = dict(seed=77, num_particles=13, rule=rule, stage=stage, noise="independent", num_trajectories=B if stage == "backsim" else 0,
              lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    outs = [_seeded(fx, False, records_per_pass=rpp, **kw) for rpp in (0, 1, 2)]
    for rpp, o in zip((1, 2), outs[1:]):
        _same(o, outs[0], f"records_per_pass {rpp} against 0")


# ---- 4. a track alone --------------------------------------------------------------------------------------------------------------------------
def test_a_track_of_an_independent_call_is_the_existing_call_on_that_track_alone():
    fx = base._fixture("m130")
    G, R, steps, D = _dims(fx)
    assert (G, R) == (3, 3)
    n, seed = 13, 4242
    kw = dict(lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    full = _seeded(fx, False, seed=seed, num_particles=n, rule="bootstrap", stage="backsim", noise="independent", num_trajectories=B, **kw)
    d = device_draws(seed, "independent", G, R, steps, n, D, B, False)
    for g, r in ((2, 1), (1, 2)):
        one = fxt.subset(fx, groups=[g], recs=[r])
        cut = {k: v[g:g + 1, r:r + 1] for k, v in d.items()}
        alone = _sibling(one, False, "bootstrap", "backsim", cut, lengths=one["lengths"], S0s=one["S0"], q_mode=one["mode"], return_particles=True)
        per_track = [k for k in full if np.shape(full[k])[:2] == (G, R) and np.shape(alone[k])[:2] == (1, 1)]
        assert {"m_pred", "S_filt", "lpd", "ess", "log_evidence", "particles", "ancestors", "trajectories", "traj_index", "lag_cov", "weights",
                "trans_var"} <= set(per_track)
        for k in per_track:
            np.testing.assert_array_equal(full[k][g, r], alone[k][0, 0], err_msg=f"track ({g}, {r}): {k}")


# ---- 5. model level: the actuator fixture with three chains ------------------------------------------------------------------------------------
def test_particle_records_seeded_of_the_model(actuator):
    mod, Yr, cr, n = _actuator_records(actuator, True)
    lengths = [8, 6, 8]
    kw = dict(lengths=lengths, Y_train_std=1.7, num_particles=128, return_particles=True)
    out = mod.particle_records_seeded(Yr, cr, seed=7, **kw)
    again = mod.particle_records_seeded(Yr, cr, seed=7, **kw)
    _same(again, out, "the same seed twice")
    assert out["m_filt"].shape == (S, 3, n, 4) and out["particles"].shape == (S, 3, n, 128, 4) and out["log_evidence"].shape == (S, 3)
    live = np.arange(n)[None, :] < np.asarray(lengths)[:, None]
    assert np.all(np.isfinite(out["m_filt"][:, live])) and np.all(np.isnan(out["m_filt"][:, ~live])) and np.all(np.isfinite(out["log_evidence"]))
    lay, lik = mod.layers[-1], mod.likelihood
    direct = pr.posterior_particle_records_seeded(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, mod.control_inputs, cr, Yr,
                                                  lik.CC, lik.DD, lik.log_Rchols, seed=7, **kw)
    _same(direct, out, "the model against the prediction-level call")
    other = mod.particle_records_seeded(Yr, cr, seed=8, **kw)
    assert float(np.max(np.abs(other["m_filt"][:, live] - out["m_filt"][:, live]))) > 0.0
    ind = mod.particle_records_seeded(Yr, cr, seed=7, noise="independent", rule="adapted", stage="backsim", num_trajectories=9, S0=0.01 * np.eye(4),
                                      lengths=lengths, num_particles=64)
    assert ind["trajectories"].shape == (S, 3, 9, n, 4) and np.all(np.isfinite(ind["log_evidence"]))
    drawn = [mod.particle_records_seeded(Yr, cr, lengths=lengths, num_particles=16)["m_filt"] for _ in range(2)]      # seed None: the model's generator
    assert float(np.max(np.abs(drawn[0][:, live] - drawn[1][:, live]))) > 0.0


def test_the_explicit_form_of_the_model(actuator):
    mod, Yr, cr, n = _actuator_records(actuator, False)
    kw = dict(lengths=[8, 6, 8], num_particles=64, seed=7, noise="per_record", stage="smooth")
    out, again = mod.particle_records_seeded(Yr, cr, **kw), mod.particle_records_seeded(Yr, cr, **kw)
    _same(again, out, "explicit U, the same seed twice")
    assert out["m_smooth"].shape == (S, 3, n, 4) and np.all(np.isfinite(out["log_evidence"]))


# ---- 6. poisoned scratch -------------------------------------------------------------------------------------------------------------------------
def test_poisoned_operator_cache_changes_nothing(tmp_path):
    """tests/seeded_poison_script.py in one child process each without and with FFVD_OP_CACHE_POISON: every output bit for bit, the
    reversed pass as the forward one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"seeded{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, _ in script.CALLS:
        assert set(script.SYMBOLS) == set(clean["called/" + label].tolist()), label
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) > 30 * len(script.CALLS)
    for k in results:
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
        if k.startswith("fwd/"):
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)
