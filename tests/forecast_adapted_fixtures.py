"""The fixtures of the adapted particle forecasts' device tests (tests/test_gpu_forecast_adapted.py): test infrastructure.

A fixture is the one-record dict of tests/forecast_particle_fixtures.py (Y (1, steps, J), eps (G, 1, steps, N, D), ..., h, origins (B,),
eps_fc (G, B, h, N, D)) with the reference of tests/forecast_adapted_ref.py.

`CASES`: the bootstrap fan's own fixtures of two cases with one model per group (three groups with hyper-parameters, Z and Q of their
own; 12 rows with gaps, N = 48, origins (0, 3, 4, 8), h = 3): their margin condition under the adapted filter is the one
tests/test_gpu_filter_adapted.py asserts on the same record and draws.

`SMALL`: fixtures on tests/adapted_particle_fixtures.py's `_small` (the oracle's posterior only, M = 24, 12 rows, h = 3) that cross the
state kernel's edges in N; row 4 lacks output 0 where J > 1, row 7 is wholly unobserved:
  d1_n2     D = 1, J = 1, two groups, start covariances, N = 2
  d2_n8     D = 2, J = 2, three groups, explicit U (no q slices: one shared Gamma, a unit is a dim), "intent", N = 8: one slab of the rows
            kernel; every admissible origin
  d4_n257   D = 4, J = 2, two groups, start covariances, "intent", N = 257: a second trip of the 256-thread loops, thread 0 alone carries
            two particles
  n2048     D = 2, J = 1, one group, N = 2048, 6 rows, origins (0, 1, 2): eight particles per thread
A fixture that misses the margin condition gets another seed here, never another bound."""
import functools

import numpy as np

import adapted_particle_fixtures as afx
import forecast_adapted_ref as far
import forecast_particle_fixtures as ffx
import particle_adapted_ref as pa
from ffvd_amd import prediction as pr
from forecast_particle_fixtures import composed, subset   # noqa: F401  (reused by the tests)
from test_gpu_filter_grouped import CASES as ALL_CASES
from test_gpu_moment_grouped import WIDE

H = 3
CASES = (ALL_CASES[1], ALL_CASES[3])


def _small(seed, origins, explicit=False, mode="reference", steps=12, **kw):
    fx = afx._small(seed, nR=1, steps=steps, **kw)
    Y = np.array(fx["Y"])
    if Y.shape[2] > 1:
        Y[0, 4, 0] = np.nan
    if steps > 7:
        Y[0, 7] = np.nan
    G, _, _, n, D = fx["eps"].shape
    return dict(fx, Y=Y, mode=mode, qs=None if explicit else fx["qs"], h=H, origins=np.asarray(origins),
                eps_fc=np.random.default_rng(seed + 7).standard_normal((G, len(origins), H, n, D)))


@functools.lru_cache(maxsize=None)
def small_d1_n2():
    return _small(3101, (0, 5, 8), D=1, G=2, J=1, n=2, with_S0=True)


@functools.lru_cache(maxsize=None)
def small_d2_n8():
    return _small(3111, tuple(range(12 - H)), explicit=True, mode="intent", D=2, G=3, J=2, n=8)


@functools.lru_cache(maxsize=None)
def small_d4_n257():
    return _small(3121, (0, 5, 8), mode="intent", D=4, G=2, J=2, n=257, with_S0=True)


@functools.lru_cache(maxsize=None)
def small_n2048():
    # (6 rows: with 2048 thresholds per row the smallest gap shrinks with every row; seeds 3131, 3132, 3136 and 3138 miss the margin,
    # 3137 has the largest gap of 3131 .. 3139: 3.9e-8)
    return _small(3137, (0, 1, 2), steps=6, D=2, G=1, J=1, n=2048)


SMALL = dict(d1_n2=small_d1_n2, d2_n8=small_d2_n8, d4_n257=small_d4_n257, n2048=small_n2048)


def fixture(name):
    """a case of CASES (a tuple) or a key of SMALL"""
    return ffx.case_fixture(*name) if isinstance(name, tuple) else SMALL[name]()


def reference_of(fx):
    """ref (the filter's arrays under "filter"), e_ref and the np.longdouble filter arrays of any fixture dict"""
    CC, DD, _ = fx["em"]
    one = lambda x: None if x is None else x[:, 0]
    return far.reference(fx["gs"], None if fx["ctrl"] is None else fx["ctrl"][0], fx["Y"][0], CC, DD, fx["sd"], fx["qs"], one(fx["x0"]),
                         one(fx["S0"]), fx["mode"], fx["origins"], fx["h"], WIDE, one(fx["eps"]), one(fx["unif"]), fx["eps_fc"], one(fx["xi0"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once, never modified."""
    return reference_of(fixture(name))


def margin_holds(name):
    """The margin condition of the filter stage of a fixture: (gap, drift, same ancestors, whether it holds)"""
    ref, _, wide = reference(name)
    gap, drift, same = pa.margin(ref["filter"], fixture(name)["unif"], wide)
    return gap, drift, same, bool(same and gap >= max(1e-8, 1000.0 * drift))


def call(fx, src="orc", fn=None, **kw):
    """prediction.forecast_adapted_grouped (or `fn`: the bootstrap fan) on a fixture (the oracle's posterior), everything returned"""
    gs = fx["gs"]
    Ls, Zs, kerns = afx._models(fx, src)
    one = lambda x: None if x is None else x[:, 0]
    args = dict(xi0=one(fx["xi0"]), origins=fx["origins"], S0s=one(fx["S0"]), q_mode=fx["mode"], return_tracks=True, return_filter=True,
                return_particles=True)
    args.update(kw)
    eps, unif, eps_fc = args.pop("eps", one(fx["eps"])), args.pop("unif", one(fx["unif"])), args.pop("eps_fc", fx["eps_fc"])
    return (fn or pr.forecast_adapted_grouped)(Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"][:, 0],
                                               None if fx["ctrl"] is None else fx["ctrl"][0], 0, fx["Y"][0], [g["Q"] for g in gs], *fx["em"],
                                               fx["h"], eps, unif, eps_fc, **args)
