"""The conditions the device tests of the adaptive particle filter rest on (tests/test_gpu_filter_adaptive.py), checked without a GPU on
the fixtures of tests/adaptive_particle_fixtures.py, which carry the oracle's posterior only.  The decision of a row is a comparison:
it is pinned only where rounding cannot flip it.  A fixture that misses a condition gets another seed there, never another bound here."""
import numpy as np
import pytest

import adaptive_particle_fixtures as afx


@pytest.mark.parametrize("name", afx.NAMES)
def test_no_decision_and_no_ancestor_hangs_on_rounding(name):
    """fp64 and np.longdouble make identical decisions and draw identical ancestors; no threshold of a resampling row lies within
    max(1e-8, 1000 x the cdf drift) of a cdf entry; on every observed row |ess / N - thr| >= max(1e-8, 1000 x the drift of ess / N)."""
    fx, m = afx.fixture(name), afx.conditions(name)
    print(f"{name} (thr {fx['thr']}): cdf gap {m['gap']:.3e}, cdf drift {m['drift']:.3e}, |ess / N - thr| >= {m['ess_gap']:.3e}, "
          f"drift of ess / N {m['ess_drift']:.3e}")
    assert fx["Y"].shape[1] <= 12
    assert m["same"] and m["same_decisions"]
    assert m["gap"] >= max(1e-8, 1000.0 * m["drift"])
    assert m["ess_gap"] >= max(1e-8, 1000.0 * m["ess_drift"])
    assert m["holds"]


def _decisions(name):
    ref = afx.reference(name)[0]
    return ref["resampled"], ~np.isnan(ref["lpd_joint"])


def test_every_track_of_the_mixed_fixture_takes_both_decisions():
    rs, seen = _decisions("mixed")
    assert rs.shape == (2, 2, 12) and seen.all()
    for g in range(2):
        for r in range(2):
            n = int((rs[g, r] == 1).sum())
            print(f"mixed: track ({g}, {r}) resamples {n} of 12 rows")
            assert 0 < n < 12


@pytest.mark.parametrize("name", [n for n in afx.NAMES if n != "mixed"])
def test_every_fixture_has_rows_of_both_kinds(name):
    rs, seen = _decisions(name)
    n, of = int((rs == 1).sum()), int(seen.sum())
    print(f"{name}: {n} of {of} observed rows resample")
    assert 0 < n < of


def test_what_each_fixture_is_there_for():
    shapes = {n: afx.fixture(n)["eps"].shape for n in afx.NAMES}
    assert shapes["d1"][-1] == 1 and shapes["d8"][-1] == 8 and shapes["d7"][-1] == 7 and afx.fixture("d7")["Y"].shape[2] == 8
    assert shapes["n2"][-2] == 2 and afx.fixture("n2")["thr"] == 0.75 and shapes["n300"][-2] == 300
    assert shapes["n2048"][-2] == 2048 and shapes["n2048"][2] == 3 and shapes["d3"][-1] == 3
    rs, _ = _decisions("n2048")
    assert rs[0, 0, 0] == 0 and rs[0, 0, 1] == 1                                    # weights carried into row 1 by eight particles per thread
    rs, _ = _decisions("n300")
    assert np.any((rs[0, 0, :-1] == 0) & (rs[0, 0, 1:] == 1))                       # a resampling row after a carried one
    fx = afx.fixture("partial")
    Y, ln = fx["Y"], fx["lengths"]
    none = np.all(np.isnan(Y), axis=2)
    some = np.any(np.isnan(Y), axis=2) & ~none
    assert ln.tolist() == [9, 7] and none[0, 5] and none[0, 6] and none[1, 0] and some[0].sum() >= 7
    rs, seen = _decisions("partial")
    assert np.all(rs[:, 1, 7:] == -1) and np.all(rs[:, none & (np.arange(9)[None, :] < ln[:, None])] == 0)
    ref = afx.reference("partial")[0]
    assert np.any(ref["logw"][:, 0, 4] != 0.0)                                      # the rows with nothing observed are given weights to keep
    np.testing.assert_array_equal(ref["logw"][:, 0, 5], ref["logw"][:, 0, 4])
    np.testing.assert_array_equal(ref["logw"][:, 0, 6], ref["logw"][:, 0, 4])
