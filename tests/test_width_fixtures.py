"""The fixtures of tests/width_fixtures.py checked without a GPU (they carry the oracle's posterior only): the conditions that
tests/test_gpu_widths.py rests on, and that each fixture can show the mistakes it is there for.

Conditions.  The margin condition of tests/test_adapted_fixtures.py for the three particle references (fp64 and np.longdouble draw
identical indices; no threshold within max(1e-8, 1000 x the cdf drift) of a cdf entry); weights that are not degenerate (a median
bootstrap ess of at least 3 over the observed rows: with one surviving particle a weighted covariance tests nothing); positive
definite covariances in the Gaussian references.

Sensitivity, in the manner of tests/test_distinct_hypers.py.  The device tests hold a mean to max(4 e_ref, 1e-11 + 1e-9 max|ref|).  A
kernel that swaps the last two input columns, never loads the last one, stops one output short or reads the noise of output 6 for
output 7 computes the reference of the perturbed fixture instead; each of these must lie at least 1000 bounds away from the
reference the device is compared with."""
import numpy as np
import pytest

import width_fixtures as wf
from test_gpu_conditional_grouped import floor
from test_gpu_moment_grouped import WIDE


def _bound(ref, e_ref):
    """the device tests' bound on a mean (`rule` of tests/test_gpu_moment_grouped.py)"""
    return max(4.0 * e_ref, floor("mean", ref)) if WIDE else floor("mean", ref)


@pytest.mark.parametrize("name", wf.NAMES)
def test_no_drawn_index_hangs_on_rounding(name):
    """the ancestors of the bootstrap and of the adapted filter and the indices of the backward simulation.  A fixture that misses
    this gets another seed (tests/width_fixtures.py), never another bound."""
    for key, (gap, drift, same) in wf.margins(name).items():
        print(f"{name} {key}: smallest gap {gap:.3e}, cdf drift between the precisions {drift:.3e}, identical indices {same}")
        assert same, key
        assert gap >= max(1e-8, 1000.0 * drift), key


@pytest.mark.parametrize("name", wf.NAMES)
def test_the_weights_are_not_degenerate_and_the_gaussian_covariances_are_positive_definite(name):
    fx, ref = wf.fixture(name), wf.bootstrap_reference(name)[0]
    seen = ~np.all(np.isnan(fx["Y"]), axis=2)
    ess = ref["ess"][:, seen]
    print(f"{name}: bootstrap ess over the observed rows: median {np.median(ess):.2f}, smallest {ess.min():.2f}")
    assert np.median(ess) >= 3.0
    live = np.arange(wf.STEPS)[None, :] < fx["lengths"][:, None]
    for what, r in (("linearised records", wf.records_reference(name)[0]), ("cubature records", wf.cubature_reference(name)[0])):
        for k in ("S_pred", "S_filt"):
            low = float(np.min(np.linalg.eigvalsh(r[k][:, live])))
            print(f"{name} {what}: smallest eigenvalue of {k} {low:.3e}")
            assert low > 0.0, (what, k)
    for what, r in (("moment filter", wf.moment_filter_reference(name)[0]), ("linearised filter", wf.linear_filter_reference(name)[0])):
        for k in ("S_pred", "S_filt", "S_smooth"):
            assert float(np.min(np.linalg.eigvalsh(r[k]))) > 0.0, (what, k)
    assert float(np.min(np.linalg.eigvalsh(wf.propagation_reference(name)["S"]))) > 0.0


@pytest.mark.parametrize("name", wf.NAMES)
def test_what_the_fixture_is_there_for(name):
    D, C, slices, _ = wf.SPECS[name]
    fx, (params, c, meta) = wf.fixture(name), wf.model(name)
    P = D + C
    assert (D, P) == {"d5": (5, 6), "d6": (6, 8), "d7": (7, 7), "p32": (8, 32), "p32d3": (3, 32)}[name.split("_")[0]]
    assert meta["M"] == 40 and meta["P"] == P and fx["gs"][0]["Z"].shape == (40, P) and len(fx["gs"]) == 2
    assert (fx["qs"] is not None) == slices and fx["mode"] == "intent" and not fx["per_model"]
    assert fx["ctrl"] is None if C == 0 else fx["ctrl"].shape == (2, 6, C)
    assert fx["Y"].shape == (2, 6, 8) and fx["lengths"].tolist() == [6, 5] and fx["em"][0].shape == (D, 8) and fx["sd"].shape == (8,)
    assert fx["eps"].shape == (2, 2, 6, 48, D) and fx["x0"].shape == (2, 2, D) and fx["S0"].shape == (2, 2, D, D)
    assert fx["unif_bs"].shape == (2, 2, 6, 5) and fx["eps_fc"].shape == (2, 3, 3, 48, D)
    np.testing.assert_array_equal(fx["x0"][:, 0], np.stack([g["X"][-1] for g in fx["gs"]]))
    # every (d, p) has a lengthscale of its own, every dim a variance of its own
    assert len(np.unique(params["loglengthscales"])) == D * P and len(np.unique(params["logvariance"])) == D
    # the gaps: a row with nothing, a row with the odd outputs only, every output observed somewhere, output 7 where output 0 is not
    nan = np.isnan(fx["Y"])
    live = np.arange(6)[None, :] < fx["lengths"][:, None]
    assert nan[0, 2].all() and nan[1, 3].tolist() == [True, False] * 4 and nan[~live].all()
    assert int(nan[live].sum()) == 12 and not nan[live].all(axis=0).any()
    assert np.any(~nan[..., 7] & nan[..., 0])
    # the references have the shapes, and NaN where the gaps are
    ref = wf.bootstrap_reference(name)[0]
    assert ref["particles"].shape == (2, 2, 6, 48, D) and ref["lpd"].shape == (2, 2, 6, 8)
    np.testing.assert_array_equal(np.isnan(ref["lpd"]), np.broadcast_to(nan[None], ref["lpd"].shape))
    assert np.all(np.isnan(ref["lpd_joint"][:, 0, 2])) and np.all(np.isfinite(ref["lpd_joint"][:, 1, 3]))


@pytest.mark.parametrize("name", wf.NAMES)
def test_each_index_mistake_moves_the_references_by_1000_bounds(name):
    fx = wf.fixture(name)
    prop, (boot, e_boot, _) = wf.propagation_reference(name), wf.bootstrap_reference(name)
    b_prop = _bound(prop["m"], prop["e_m"])
    ok = ~np.isnan(boot["m_filt"])
    b_boot = {k: _bound(boot[k][ok], e_boot[k]) for k in ("m_pred", "m_filt")}
    for mistake, fn in wf.INPUT_MISTAKES.items():
        if mistake == "zero_last_control" and fx["ctrl"] is None:
            continue
        bad = fn(fx)
        moved = float(np.max(np.abs(wf.propagation(bad, wide=False)["m"] - prop["m"])))
        print(f"{name} {mistake}: the propagated mean moves by {moved:.2e} = {moved / b_prop:.1e} x the bound {b_prop:.1e}")
        assert moved >= 1000.0 * b_prop, (mistake, moved, b_prop)
        moved = float(np.max(np.abs(wf.bootstrap(bad)[0]["m_pred"][ok] - boot["m_pred"][ok])))
        print(f"{name} {mistake}: the particles' m_pred moves by {moved:.2e} = {moved / b_boot['m_pred']:.1e} x the bound {b_boot['m_pred']:.1e}")
        assert moved >= 1000.0 * b_boot["m_pred"], (mistake, moved)
    for mistake, fn in wf.EMISSION_MISTAKES.items():
        moved = float(np.max(np.abs(wf.bootstrap(fn(fx))[0]["m_filt"][ok] - boot["m_filt"][ok])))
        print(f"{name} {mistake}: the particles' m_filt moves by {moved:.2e} = {moved / b_boot['m_filt']:.1e} x the bound {b_boot['m_filt']:.1e}")
        assert moved >= 1000.0 * b_boot["m_filt"], (mistake, moved)
