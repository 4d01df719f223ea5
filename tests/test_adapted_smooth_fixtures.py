"""The fixtures of tests/adapted_smooth_fixtures.py that carry the oracle's posterior only, checked without a GPU: the conditions that
tests/test_gpu_smooth_adapted.py rests on when it asks the device for identical ancestors and identical trajectory indices, and what
each fixture is there for.  (The seven shared cases, n130 and n700 are built through the device's posterior path: the GPU file asserts
the same conditions for them.)"""
import numpy as np
import pytest

import adapted_smooth_fixtures as sfx


@pytest.mark.parametrize("name", sfx.ON_THE_ORACLE)
def test_neither_the_ancestors_nor_the_trajectories_hang_on_rounding(name):
    """fp64 and np.longdouble draw identical ancestors and identical traj_index; no forward threshold (unif + i) / N and no backward
    threshold u tot -- the last row's u N included -- lies within max(1e-8, 1000 x the cdf drift between the precisions) of a cdf
    entry."""
    gap, back, drift, same, ok = sfx.margins(name)
    print(f"{name}: smallest gap {gap:.3e} (backward alone {back:.3e}), cdf drift between the precisions {drift:.3e}, identical indices {same}")
    assert same
    assert gap >= max(1e-8, 1000.0 * drift)
    assert back >= max(1e-8, 1000.0 * drift)
    assert ok


def test_what_the_fixtures_are_there_for():
    shapes = {k: sfx.reference(k)[0]["particles"].shape for k in sfx.ON_THE_ORACLE}
    assert shapes["d1"][-1] == 1 and shapes["d8"][-1] == 8 and shapes["d7"][-1] == 7 and shapes["p32"][-1] == 8
    assert shapes["n2"][3] == 2 and shapes["n300"][3] == 300 and shapes["n2048"][2:4] == (2, 2048) and shapes["one_row"][2] == 1
    assert all(s[2] <= 12 for s in shapes.values())
    assert sfx.fixture("p32")["ctrl"].shape[-1] == 24
    for k in ("d1", "d8"):
        assert sfx.fixture(k)["Y"].shape[2] == 3
    assert list(sfx.fixture("ragged")["lengths"]) == [5, 1] and np.all(np.isnan(sfx.fixture("all_nan")["Y"]))
    for k in sfx.ON_THE_ORACLE:
        fx, ref = sfx.fixture(k), sfx.reference(k)[0]
        N = ref["particles"].shape[3]
        for r, n in enumerate(fx["lengths"]):
            n = int(n)
            np.testing.assert_array_equal(ref["w_smooth"][:, r, n - 1], np.full((len(fx["gs"]), N), 1.0 / N))
            assert np.all(np.isnan(ref["w_smooth"][:, r, n:])) and np.all(ref["traj_index"][:, r, n:] == -1)
            u = fx["unif_bs"][:, r, n - 1]
            np.testing.assert_array_equal(ref["traj_index"][:, r, n - 1], np.minimum(np.floor(u * N).astype(np.int64), N - 1))
    last = sfx.reference("last_nan")[0]
    np.testing.assert_array_equal(last["ancestors"][:, 0, -1], np.broadcast_to(np.arange(sfx.N), (2, sfx.N)))
    part = sfx.reference("partial")[0]
    assert np.all(np.isnan(part["lpd"][0, 0, :, 1])) and np.isnan(part["lpd_joint"][0, 0, 5])
    blind = sfx.reference("all_nan")[0]
    np.testing.assert_array_equal(blind["ancestors"][0, 0], np.broadcast_to(np.arange(sfx.N), blind["ancestors"][0, 0].shape))
    for k in ("n2", "n300", "d8"):                                # the smoothing weights are not degenerate: they test a weighted sum
        ess = sfx.reference(k)[0]["ess_smooth"]
        assert np.nanmin(ess) >= 1.0 and np.nanmin(ess[:, :, :-1]) < shapes[k][3]
