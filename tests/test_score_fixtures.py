"""CPU: the fixtures of tests/test_gpu_score.py (tests/score_fixtures.py) meet the conditions its tolerances rest on.  A quantile is
held to |q_dev - q_ref| <= tol / f_ref(q_ref) + 4 ulp, which says something only where the density at the quantile is not tiny
against the mixture's width: f(q_ref) (max mu - min mu + max sigma) >= 1e-3 at every (target, level), the bimodal fixtures'
quantiles between the modes included."""
import numpy as np
import pytest

import score_fixtures as sf
import score_ref as sr


def test_the_cases_walk_every_shape_the_decomposition_has():
    col = lambda i, kind: {c[i] for c in sf.CASES if c[1] == kind}
    T = sf.TILE
    for kind in ("points", "moments"):
        assert col(2, kind) == {1, 2, T - 1, T, T + 1, 2 * T + 3}
        assert col(3, kind) == {1, 7} and col(5, kind) == {1, 3, 8} and col(6, kind) == {0, 1, 3, 16}
        assert any(c[4] < c[3] for c in sf.CASES if c[1] == kind)            # n_test < steps
        assert any(c[4] * c[5] > 2 * 8 for c in sf.CASES if c[1] == kind)   # three passes at targets_per_pass = 8
    assert col(7, "points") == {1, 4, 32} and col(7, "moments") == {1, 8}
    assert len(set(sf.NAMES)) == len(sf.CASES)


@pytest.mark.parametrize("name", sf.NAMES)
def test_every_quantile_is_well_conditioned(name):
    fx, ref = sf.fixture(name), sf.reference(name)
    assert fx["mu"].shape == fx["var"].shape == (fx["steps"], fx["J"], fx["K"]) and np.all(fx["var"] > 0.0)
    assert ref["quantiles"].shape == (fx["steps"], fx["J"], fx["Q"])
    if fx["Q"]:
        cond = ref["density"] * ref["width"][..., None]
        print(f"{name}: smallest f(q_ref) * width = {np.min(cond):.3e}")
        assert np.min(cond) >= sf.CONDITION
        F = np.stack([sr.cdf(fx["mu"], fx["var"], ref["quantiles"][..., i]) for i in range(fx["Q"])], axis=-1)
        assert np.max(np.abs(F - fx["levels"])) <= 1e-13
    if fx["kind"] == "moments":
        assert np.min(np.linalg.eigvalsh(fx["S"])) > -1e-12 and np.array_equal(fx["S"], np.swapaxes(fx["S"], -1, -2))
        assert fx["K"] == 1 or float(np.max(fx["var"][0, 0]) / np.min(fx["var"][0, 0])) > 1.2     # a target's variances really differ


def test_a_bimodal_fixture_has_a_quantile_between_its_modes():
    found = 0
    for name in sf.NAMES:
        fx, ref = sf.fixture(name), sf.reference(name)
        if not fx["bimodal"] or not fx["Q"] or fx["K"] < 8:
            continue
        j = int(np.argmin(fx["sd"] / np.abs(fx["CC"][0])))                    # the output that sees the clusters farthest apart
        mu, q, i = fx["mu"][:, j], ref["quantiles"][:, j], int(np.argmin(np.abs(fx["levels"] - 0.5)))
        low, high = mu[:, 0::2], mu[:, 1::2]                                  # the two clusters (which is which depends on CC's sign)
        if np.mean(low) > np.mean(high):
            low, high = high, low
        inner = (q[:, i] > np.max(low, axis=1)) & (q[:, i] < np.min(high, axis=1))
        # bimodal: the density at the midpoint between the cluster centres is below both densities at the centres
        mid = 0.5 * (np.mean(low, axis=1) + np.mean(high, axis=1))
        dip = sr.pdf(mu, fx["var"][:, j], mid) < 0.5 * np.minimum(sr.pdf(mu, fx["var"][:, j], np.mean(low, axis=1)),
                                                                sr.pdf(mu, fx["var"][:, j], np.mean(high, axis=1)))
        both = inner & dip
        if np.any(both):
            found += 1
            assert np.all(ref["density"][both, j, i] * ref["width"][both, j] >= sf.CONDITION)
    assert found >= 1


@pytest.mark.parametrize("name", sf.NAMES)
def test_nan_targets_are_in_some_rows_and_not_in_others(name):
    fx, ref = sf.fixture(name), sf.reference(name)
    Y = fx["Y"]
    assert Y.shape == (fx["n_test"], fx["J"])
    if fx["n_test"] > 2:
        rows = np.any(np.isnan(Y), axis=1)
        assert np.any(rows) and not np.all(rows) and np.any(np.all(np.isnan(Y), axis=1))
        if fx["J"] > 1:
            assert np.any(rows & ~np.all(np.isnan(Y), axis=1))                # a row with some outputs observed and some not
    assert np.array_equal(np.isnan(ref["crps"]), np.isnan(Y)) and np.array_equal(np.isnan(ref["pit"]), np.isnan(Y))
    seen = ~np.isnan(Y)
    assert np.all(ref["crps"][seen] > 0.0) and np.all((ref["pit"][seen] > 0.0) & (ref["pit"][seen] < 1.0))


def test_the_two_layouts_hold_the_same_components_in_the_same_order():
    for K in (1, 2, sf.TILE - 1, sf.TILE, sf.TILE + 1, 2 * sf.TILE + 3):
        G, N = sf.split(K)
        assert G * N == K and 1 <= G <= 8
    x = np.arange(6 * 2 * 3, dtype=np.float64).reshape(6, 2, 3)
    p = sf.as_particles(x)
    G, N = sf.split(6)
    assert p.shape == (G, 2, N, 3)
    for k in range(6):
        np.testing.assert_array_equal(p[k // N, :, k % N], x[k])
