"""The fixtures of the device tests of particle smoothing and backward simulation on the adapted sets
(tests/test_gpu_smooth_adapted.py): test infrastructure.

A fixture is the dict of tests/particle_fixtures.py plus unif_bs (G, R, steps, B), seeded per fixture and held in the full layout.
  the seven cases and n130 / n700 of tests/adapted_particle_fixtures.py (R = 3 records of 12 rows with lengths (12, 12, 9), N = 48;
    N = 130 and N = 700: slab and chunk edges), B = 3 (n130: B = 300, the moments kernel strides twice).  They are built through the
    device's posterior path, so their conditions are asserted in the GPU file.
The others carry the oracle's posterior only (no device call builds them), so tests/test_adapted_smooth_fixtures.py checks their
conditions without a GPU:
  d1, d8, n2, n2048, last_nan, partial   the small fixtures of tests/adapted_particle_fixtures.py (D = 1 and D = 8 with J = 3, N = 2,
                                         N = 2048 with 2 rows, a last row unobserved, rows with only some outputs observed)
  n300                                   N = 300: a second chunk of 44 columns, a second slab of 44 particles
  one_row                                a record of one row: no backward row at all
  ragged                                 two records of 5 and 1 rows in one call: the last-row launch of a track differs per record
  all_nan                                nothing observed: the bootstrap smoother's and backward simulation's recursions coincide
  d7, p32                                tests/width_fixtures.py at D = 7 (P = 7) and D = 8 with P = 32 (their own unif_bs, B = 5)
The conditions: fp64 and np.longdouble draw identical ancestors; the forward margin of tests/test_adapted_fixtures.py (no threshold
(unif + i) / N within max(1e-8, 1000 x the cdf drift between the precisions) of a cdf entry); the backward margin of
particle_backsim_ref.margin with the same bound, the last row included, where u N must stay clear of the integers.  A fixture that
misses one gets another seed here, never another bound."""
import functools

import numpy as np

import adapted_particle_fixtures as afx
import particle_adapted_smooth_ref as pas
import particle_fixtures as fxt
import width_fixtures as wfx
from ffvd_amd import prediction as pr
from test_gpu_moment_grouped import WIDE

N = afx.N
WIDTHS = ("d7", "p32")
REUSED = ("d1", "d8", "n2", "n2048", "last_nan", "partial")
OWN = ("n300", "one_row", "ragged", "all_nan")
ON_THE_ORACLE = REUSED + OWN + WIDTHS
DEVICE_EDGES = ("n130", "n700")
B_OF = {"n130": 300, "last_nan": 300}
SEEDS = {name: 3100 + i for i, name in enumerate(ON_THE_ORACLE + DEVICE_EDGES)}


def with_uniforms(fx, B, seed):
    G, R, steps = fx["unif"].shape
    return dict(fx, unif_bs=np.random.default_rng(seed).random((G, R, steps, B)))


def _base(name):
    if isinstance(name, tuple) or name in DEVICE_EDGES or name in REUSED:
        return afx.fixture(name)
    if name == "n300":
        return afx._small(971, n=300, steps=4, G=2)
    if name == "one_row":
        return afx._small(973, steps=1, with_S0=True)
    if name == "ragged":
        fx = afx._small(975, D=3, nR=2, steps=5, G=2)
        fx["Y"][1, 1:] = np.nan
        return dict(fx, lengths=np.array([5, 1]))
    fx = afx._small(977, G=2, nR=2, steps=6, with_S0=True)                              # all_nan
    return dict(fx, Y=np.full_like(fx["Y"], np.nan))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """a case of CASES (a tuple) or a name above.  Shared, never modified."""
    if name in WIDTHS:
        return wfx.fixture(name)
    return with_uniforms(_base(name), B_OF.get(name, 3), _case_seed(name) if isinstance(name, tuple) else SEEDS[name])


def _case_seed(name):
    from test_gpu_filter_grouped import CASES
    return 3000 + list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref, e_ref and the np.longdouble composition of a fixture by tests/particle_adapted_smooth_ref.py (the filter, the kept
    moments, the smoother and the backward simulation).  Computed once, never modified."""
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return pas.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                         fx["eps"], fx["unif"], fx["xi0"], fx["unif_bs"])


def margins(name):
    """(the smallest gap, forward and backward; the backward gap alone; drift; identical ancestors and indices; whether the conditions
    hold)"""
    ref, _, wide = reference(name)
    gap, drift, same = pas.margin(ref, fixture(name)["unif"], wide)
    back = float(ref["gap_bs"])
    if wide is not None:
        same = same and bool(np.array_equal(ref["ancestors"], wide["ancestors"]))
    return gap, back, drift, same, bool(same and min(gap, back) >= max(1e-8, 1000.0 * drift))


def subset(fx, groups=None, recs=None):
    """the fixture of some groups and some records, the draws sliced with them"""
    gi = list(range(len(fx["gs"]))) if groups is None else groups
    ri = list(range(fx["Y"].shape[0])) if recs is None else recs
    return dict(fxt.subset(fx, groups, recs), unif_bs=fx["unif_bs"][gi][:, ri])


FUNCTIONS = dict(smooth=pr.smooth_adapted_records_grouped, backsim=pr.backsim_adapted_records_grouped, filter=pr.filter_adapted_records_grouped,
                 boot_smooth=pr.smooth_particle_records_grouped, boot_backsim=pr.backsim_particle_records_grouped)


def call(fx, what="smooth", src="orc", **kw):
    """prediction.smooth_adapted_records_grouped (`what` = "backsim": backsim_adapted_records_grouped with the fixture's unif_bs;
    "filter", "boot_smooth", "boot_backsim": the siblings) on a fixture (the oracle's posterior)"""
    gs = fx["gs"]
    Ls, Zs, kerns = afx._models(fx, src)
    args = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    args.update(kw)
    tail = (fx["unif_bs"],) if what.endswith("backsim") else ()
    return FUNCTIONS[what](Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"], [g["Q"] for g in gs], *fx["em"],
                           fx["eps"], fx["unif"], *tail, **args)
