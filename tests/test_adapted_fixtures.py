"""The small fixtures of tests/adapted_particle_fixtures.py checked without a GPU (they carry the oracle's posterior only): the margin
condition that tests/test_gpu_filter_adapted.py rests on when it asks the device for identical ancestors, and what each fixture is
there for."""
import numpy as np
import pytest

import adapted_particle_fixtures as afx


@pytest.mark.parametrize("name", sorted(afx.SMALL))
def test_the_ancestors_of_every_small_fixture_do_not_hang_on_rounding(name):
    """fp64 and np.longdouble draw identical ancestors, and no threshold (unif + i) / N lies within max(1e-8, 1000 x the cdf drift
    between the precisions) of a cdf entry."""
    gap, drift, same, ok = afx.margin_holds(name)
    print(f"{name}: smallest gap {gap:.3e}, cdf drift between the precisions {drift:.3e}, identical ancestors {same}")
    assert same
    assert gap >= max(1e-8, 1000.0 * drift)
    assert ok


def test_what_the_small_fixtures_are_there_for():
    shapes = {k: afx.reference(k)[0]["particles"].shape for k in afx.SMALL}
    assert shapes["d1"] == (2, 2, 6, afx.N, 1) and shapes["d8"][-1] == 8 and shapes["n2"][3] == 2 and shapes["n2048"][2:4] == (2, 2048)
    assert all(s[2] <= 12 for s in shapes.values())
    for k in ("d1", "d8"):
        assert afx.fixture(k)["Y"].shape[2] == 3
    last = afx.reference("last_nan")[0]
    assert np.all(np.isnan(last["lpd_joint"][:, 0, -1])) and np.all(last["ess"][:, 0, -1] == afx.N)
    np.testing.assert_array_equal(last["ancestors"][:, 0, -1], np.broadcast_to(np.arange(afx.N), (2, afx.N)))
    part = afx.reference("partial")[0]
    assert np.all(np.isnan(part["lpd"][0, 0, :, 1])) and np.isnan(part["lpd_joint"][0, 0, 5]) and np.all(np.isfinite(part["lpd_joint"][0, 0, :5]))
    assert np.isnan(part["lpd"][0, 0, 2, 0]) and np.isfinite(part["lpd"][0, 0, 2, 2])


def test_the_sharp_fixture_loses_a_direction_and_the_two_precisions_zero_the_same_columns():
    """sd = 1e-6 x the others on one output: the update with that output takes a direction out of P, down to about 1e-12 of P's size,
    and the drawn particles carry the cancellation (e_ref of `particles` is 5e-10 here against 1e-15 elsewhere).  Measured: no pivot of
    the unpivoted factor reaches <= 0 -- what is left of the direction is four orders above the rounding of the update -- and the two
    precisions agree on that (and draw the same ancestors: the test above), so the device can be held to the reference on this
    fixture.  A pivot <= 0 cannot be had from any sd > 0 in a way the two precisions share (P is positive definite in exact
    arithmetic); the convention itself is pinned in tests/test_particle_adapted_ref.py on matrices that are singular by construction."""
    ref, e_ref, wide = afx.reference("sharp")
    n = int(ref["zeroed"].sum())
    print(f"sharp: {n} zeroed columns among {ref['zeroed'].size}; e_ref of the particles {e_ref['particles']:.3e}")
    if wide is not None:
        np.testing.assert_array_equal(ref["zeroed"], wide["zeroed"])
        assert e_ref["particles"] > 1e-12                         # the cancellation is there: the fixture does what it is for
