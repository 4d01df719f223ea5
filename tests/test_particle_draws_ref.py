"""tests/particle_draws_ref.py, the host reference of the seeded particle draws, without a GPU: the published known answers of
Philox4x32-10, the exact uniforms, the normal map at its extremes and against np.longdouble, the prefix property the addressing gives,
distinct streams and seeds, and the first two moments of 10^6 normals.

The fp64 normal map against the long-double map: the argument 2 pi u2 is rounded once (relative 2^-53, absolute up to
2 pi 2^-53) and multiplied by rho <= 8.58, cos / sin / log / sqrt add a few ulp of a result of at most 8.58: 8.58 (2 pi + 4) 2^-53 =
1.0e-14, bound 2e-14.  Measured on 4 10^6 pairs with the extremes included: 5.4e-15."""
import itertools

import numpy as np
import pytest

import particle_draws_ref as pd

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_the_known_answers_of_philox4x32_10(counter, key, want):
    got = pd.philox4x32([np.array([c], np.uint64) for c in counter], [np.uint64(k) for k in key])
    assert tuple(int(w[0]) for w in got) == want
    # vectorised: the same block among others
    many = pd.philox4x32([np.array([1, c, 2], np.uint64) for c in counter], [np.uint64(k) for k in key])
    assert tuple(int(w[1]) for w in many) == want


def test_the_key_is_the_two_words_of_the_seed():
    k1, k2 = pd.pair_integers(0x299f31d0a4093822, 0x03707344, 0x85a308d3, 0x13198a2e, np.array([0x243f6a88]))
    w = KNOWN[2][2]
    assert int(k1[0]) == (w[0] >> 5) * 2 ** 26 + (w[1] >> 6) and int(k2[0]) == (w[2] >> 5) * 2 ** 26 + (w[3] >> 6)


def test_uniforms_are_exact_multiples_of_2_to_minus_53_in_the_unit_interval():
    k1, k2 = pd.pair_integers(SEED, 1, 0, 0, np.arange(100000))
    assert int(k1.max()) < 2 ** 53 and int(k2.max()) < 2 ** 53
    for k, u in zip((k1, k2), pd.uniform_pair(k1, k2)):
        assert np.all(u >= 0.0) and np.all(u < 1.0)
        np.testing.assert_array_equal(u * 2.0 ** 53, k.astype(np.float64))
        np.testing.assert_array_equal((u * 2.0 ** 53).astype(np.uint64), k)
    top = np.array([2 ** 53 - 1], np.uint64)
    a, _ = pd.uniform_pair(top, top)
    assert a[0] == 1.0 - 2.0 ** -53 and a[0] < 1.0
    b = pd.block(SEED, "unif", 2, 1, 7)
    np.testing.assert_array_equal(b, np.stack(pd.uniform_pair(*pd.pair_integers(SEED, 1, 2, 1, np.arange(4))), axis=1).reshape(-1)[:7])


def test_normals_are_finite_at_the_extremes():
    ext = np.array([0, 2 ** 53 - 1], np.uint64)
    k1, k2 = (np.repeat(ext, 2), np.tile(ext, 2))
    for dtype in (np.float64, np.longdouble):
        a, b = pd.normal_pair(k1, k2, dtype)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        assert float(np.max(np.abs(np.concatenate((a, b))))) <= 8.58
    a, b = pd.normal_pair(k1, k2)
    assert abs(float(a[0]) - np.sqrt(106.0 * np.log(2.0))) < 1e-12 and b[0] == 0.0          # k1 = 0: the largest radius, angle 0
    assert a[2] == 0.0 and b[2] == 0.0                                                       # k1 = 2^53 - 1: u1 = 1, radius 0


def test_the_fp64_normal_map_against_the_long_double_map():
    rng = np.random.default_rng(17)                       # (where np.longdouble is no wider the two maps are one and the error is 0)
    n = 4_000_000
    k1, k2 = rng.integers(0, 2 ** 53, n, dtype=np.uint64), rng.integers(0, 2 ** 53, n, dtype=np.uint64)
    ext = np.array([0, 1, 2 ** 52, 2 ** 53 - 2, 2 ** 53 - 1], np.uint64)
    k1[:25], k2[:25] = np.repeat(ext, 5), np.tile(ext, 5)
    a, b = pd.normal_pair(k1, k2)
    la, lb = pd.normal_pair(k1, k2, np.longdouble)
    err = max(float(np.max(np.abs(a - la))), float(np.max(np.abs(b - lb))))
    print(f"fp64 normal map against np.longdouble on {n} pairs: max error {err:.3e}")
    assert err <= 2e-14


def test_a_block_does_not_depend_on_steps_groups_or_records():
    big = pd.draws(SEED, "independent", 3, 3, 12, 6, 3, with_xi0=True, B=5)
    small = pd.draws(SEED, "independent", 2, 2, 5, 6, 3, with_xi0=True, B=5)
    np.testing.assert_array_equal(small["eps"], big["eps"][:2, :2, :5])
    np.testing.assert_array_equal(small["unif"], big["unif"][:2, :2, :5])
    np.testing.assert_array_equal(small["xi0"], big["xi0"][:2, :2])
    np.testing.assert_array_equal(small["unif_bs"], big["unif_bs"][:2, :2, :5])
    per = pd.draws(SEED, "per_record", 3, 3, 12, 6, 3, with_xi0=True, B=5)
    shared = pd.draws(SEED, "shared", 3, 3, 12, 6, 3, with_xi0=True, B=5)
    for k in big:
        assert per[k].shape == big[k].shape[1:] and shared[k].shape == big[k].shape[2:]
        np.testing.assert_array_equal(per[k], big[k][0], err_msg=k)                          # group word 0
        np.testing.assert_array_equal(shared[k], big[k][0, 0], err_msg=k)                    # group and record words 0
        assert not np.array_equal(big[k][1, 0], big[k][0, 1])
    odd = pd.block(SEED, "eps", 1, 2, 65)                                                    # an odd block drops the last element only
    np.testing.assert_array_equal(odd, pd.block(SEED, "eps", 1, 2, 66)[:65])


def test_streams_and_seeds_differ_pairwise():
    p = np.arange(4096)
    got = {(s, st): pd.pair_integers(s, st, 0, 0, p)[0] for s in (SEED, SEED + 1) for st in range(4)}
    for a, b in itertools.combinations(got, 2):
        assert np.mean(got[a] == got[b]) == 0.0, (a, b)
    lo, hi = pd.pair_integers(1, 0, 0, 0, p)[0], pd.pair_integers(1 << 32, 0, 0, 0, p)[0]      # both key words count
    assert np.mean(lo == hi) == 0.0


def test_the_first_two_moments_of_a_million_normals():
    z = pd.block(2024, "eps", 0, 0, 1_000_000)
    mean, std = float(np.mean(z)), float(np.std(z))
    print(f"10^6 normals of seed 2024: mean {mean:.3e}, std - 1 {std - 1.0:.3e}")
    assert abs(mean) < 5e-3 and abs(std - 1.0) < 5e-3
    u = pd.block(2024, "unif", 0, 0, 1_000_000)
    assert abs(float(np.mean(u)) - 0.5) < 2e-3 and abs(float(np.var(u)) - 1.0 / 12.0) < 1e-3
