"""The fixtures of the adaptive particle filter's device tests (tests/test_gpu_filter_adaptive.py): test infrastructure.

Every fixture is the dict of tests/particle_fixtures.py plus `thr`, the ESS threshold it is run at.  They carry the oracle's posterior
only (`_small` of tests/adapted_particle_fixtures.py; `d7` is tests/width_fixtures.py's), so tests/test_adaptive_fixtures.py checks
without a GPU the three conditions the device tests rest on.  The decision of a row is a comparison and is pinned only where rounding
cannot flip it:
  - fp64 and np.longdouble make identical decisions and draw identical ancestors;
  - no threshold of a resampling row lies within max(1e-8, 1000 x the cdf drift) of a cdf entry (the bootstrap fixtures' condition);
  - on every observed row |ess / N - thr| >= max(1e-8, 1000 x the fp64-longdouble drift of ess / N).
A fixture that misses a condition gets another seed here, never another bound.  The existing small fixtures have an output with
sd = 0.05 and resample on every row at 0.5; these have sd = (0.8, 0.3, 1.3) or wider so that rows of both kinds occur.  All have
<= 12 rows, M = 24 and N = 48 unless said otherwise.
  mixed    D = 2, two groups, two records of 12 rows with start covariances: every track takes both decisions
  d1       D = 1, narrower outputs (at SD a one-dimensional state never falls below 0.5 N in 8 rows)
  d3       D = 3, wide outputs
  d8       D = 8 (36 entries in the triangle), outputs wide enough that rows are carried
  n2       N = 2 at thr = 0.75 (ess = 1 is exactly 0.5 N there)
  n2048    N = 2048, 3 rows, the first of which does not resample: eight particles per thread carry weights into row 1
  n300     N = 300: several particles per thread after a carried row
  partial  rows with some outputs, rows with none (which keep the weights they are given), records of 9 and 7 rows
  d7       tests/width_fixtures.py's d7: D = 7, J = 8, "intent", records of 6 and 5 rows, at thr = 0.2 (eight outputs: every row falls below 0.5 N)"""
import functools

import numpy as np

import particle_adaptive_ref as pe
import width_fixtures as wf
from adapted_particle_fixtures import _models, _small
from ffvd_amd import prediction as pr
from particle_fixtures import subset   # noqa: F401  (reused by the tests)
from test_gpu_moment_grouped import WIDE

SD = (0.8, 0.3, 1.3)


def _with(fx, thr):
    fx["thr"] = thr
    return fx


@functools.lru_cache(maxsize=None)
def small_mixed():
    return _with(_small(971, D=2, G=2, nR=2, steps=12, sd=SD, with_S0=True), 0.5)


@functools.lru_cache(maxsize=None)
def small_d1():
    return _with(_small(979, D=1, G=2, steps=8, sd=(0.4, 0.15, 0.8), with_S0=True), 0.5)


@functools.lru_cache(maxsize=None)
def small_d3():
    return _with(_small(972, D=3, nR=2, steps=12, sd=(1.5, 0.6, 2.0)), 0.5)


@functools.lru_cache(maxsize=None)
def small_d8():
    return _with(_small(975, D=8, steps=6, sd=(4.0, 3.0, 6.0)), 0.5)


@functools.lru_cache(maxsize=None)
def small_n2():
    return _with(_small(976, n=2, steps=10, sd=SD, with_S0=True), 0.75)


@functools.lru_cache(maxsize=None)
def small_n2048():
    return _with(_small(977, n=2048, steps=3, sd=(1.0, 0.45, 1.5)), 0.5)


@functools.lru_cache(maxsize=None)
def small_n300():
    return _with(_small(973, n=300, steps=8, sd=SD), 0.5)


@functools.lru_cache(maxsize=None)
def small_partial():
    fx = _small(978, D=3, G=2, nR=2, steps=9, sd=SD, with_S0=True)
    fx["Y"][0, :, 1] = np.nan                                     # the middle output of record 0 is never observed
    fx["Y"][0, 2, 0] = fx["Y"][0, 4, 2] = np.nan                  # rows with one output, with another
    fx["Y"][0, 5] = fx["Y"][0, 6] = np.nan                        # two rows with none in a row, then observed ones
    fx["Y"][1, 0] = np.nan                                        # a first row with none
    fx["Y"][1, 7:] = np.nan
    fx["lengths"] = np.array([9, 7])
    return _with(fx, 0.5)


@functools.lru_cache(maxsize=None)
def width_d7():
    return _with(dict(wf.fixture("d7")), 0.2)


SMALL = dict(mixed=small_mixed, d1=small_d1, d3=small_d3, d8=small_d8, n2=small_n2, n2048=small_n2048, n300=small_n300,
             partial=small_partial, d7=width_d7)
NAMES = tuple(SMALL)


def fixture(name):
    return SMALL[name]()


@functools.lru_cache(maxsize=None)
def reference(name, thr=None):
    """ref, e_ref and the np.longdouble composition of a fixture by tests/particle_adaptive_ref.py at the fixture's threshold (or
    `thr`).  Computed once, never modified."""
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return pe.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                        fx["eps"], fx["unif"], fx["xi0"], fx["thr"] if thr is None else thr)


def conditions(name):
    """particle_adaptive_ref.margin of a fixture plus `holds`: the three conditions of the module's docstring"""
    fx = fixture(name)
    ref, _, wide = reference(name)
    m = pe.margin(ref, fx["unif"], fx["thr"], wide)
    m["holds"] = bool(m["same"] and m["same_decisions"] and m["gap"] >= max(1e-8, 1000.0 * m["drift"]) and
                      m["ess_gap"] >= max(1e-8, 1000.0 * m["ess_drift"]))
    return m


def call(fx, fn=None, **kw):
    """prediction.filter_adaptive_records_grouped at the fixture's threshold (or `fn`: the bootstrap call, which takes none) on the
    oracle's posterior"""
    gs = fx["gs"]
    Ls, Zs, kerns = _models(fx, "orc")
    args = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    if fn is None:
        args["ess_threshold"] = fx["thr"]
    args.update(kw)
    return (fn or pr.filter_adaptive_records_grouped)(Ls, Zs, kerns, [g["orc"]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"],
                                                      [g["Q"] for g in gs], *fx["em"], fx["eps"], fx["unif"], **args)
