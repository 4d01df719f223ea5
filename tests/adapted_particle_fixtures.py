"""The fixtures of the adapted particle filter's device tests (tests/test_gpu_filter_adapted.py): test infrastructure.

The seven cases and the three edges are tests/particle_fixtures.py's (`case_fixture`, `EDGES`, `subset`, the same draws), with the
reference of tests/particle_adapted_ref.py.  They are built through the device's posterior path, so their margin condition is asserted
in the GPU file.

`SMALL` adds fixtures for what is new in the adapted weight kernel -- the per-particle factor and the bookkeeping of the triangle.  They
carry the oracle's posterior only (no device call builds them), so tests/test_adapted_fixtures.py checks their margin condition
without a GPU: fp64 and np.longdouble draw identical ancestors, and no threshold lies within max(1e-8, 1000 x the cdf drift) of a cdf
entry.  A fixture that misses it gets another seed here, never another bound.  All have <= 12 rows.
  d1          D = 1, J = 3, two groups, two records with start covariances (a 1 x 1 triangle; the second and third output of a row
              meet a P that the first has already shrunk)
  d8          D = 8, J = 3 (36 entries in the triangle, eight columns in the factor)
  n2          N = 2
  n2048       N = 2048 with 2 rows (eight particles per thread in every pass, the scan and the gather)
  last_nan    a record whose last row is unobserved: the last launch takes the bootstrap branch
  partial     rows with only some outputs observed: the ascending updates skip them
  sharp       one output with sd = 1e-6 x the others: P loses a direction down to 1e-12 of its size and the factor's last pivot is
              what cancellation leaves of it.  It stays positive: the pivot is about 1e-12 relative, the rounding of the update about
              1e-16 (tests/test_adapted_fixtures.py measures it and checks that the two precisions zero the same columns -- none).
              In exact arithmetic P is positive definite for every sd > 0, so a pivot <= 0 can only be rounding's, and then the two
              precisions do not share it: the zero-column convention is pinned on the reference's `factors` instead."""
import functools

import numpy as np

import particle_adapted_ref as pa
import particle_fixtures as fxt
from ffvd_amd import prediction as pr, synthetic
from oracle import ffvd_oracle as orc
from particle_fixtures import EDGES, case_fixture, draws, subset   # noqa: F401  (reused by the tests)
from test_gpu_conditional_grouped import _kernels
from test_gpu_moment_grouped import WIDE, start_cov

N = fxt.N


def _orc_group(p, c, meta, X):
    """test_gpu_conditional_grouped._group without the device's posterior: the oracle's alone"""
    T = meta["T"]
    okern, kern, Q = orc.make_kernels(p, kernel_type=meta["kernel_type"]), _kernels(p, meta), np.exp(p["log_Q"])
    Lo = orc.kernel_pre_cal(p["Z"], okern)
    Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, np.concatenate((X[:T], c[:T]), axis=1), X, p["Z"], okern, Q)
    return dict(Z=p["Z"], kern=kern, okern=okern, X=X, Q=Q, orc=dict(L=list(Lo), U=Uo, H=np.asarray(Ho)))


def _small(seed, D=2, G=1, nR=1, steps=6, n=N, J=3, sd=(0.4, 0.05, 1.3), with_S0=False, M=24, T=64):
    """`G` chains of one model of the "tiny" configuration with D latent dims, `nR` records of `steps` rows around the chains' last
    states, a seeded emission with J outputs and the draws of `seed`"""
    params, _, c, meta = synthetic.make_named("tiny", D=D, M=M, T=T, S=G)
    gs = [_orc_group(params, c, meta, params["X"][g]) for g in range(G)]
    rng = np.random.default_rng(seed)
    CC, DD, sd = rng.standard_normal((D, J)), rng.standard_normal(J), np.asarray(sd, dtype=np.float64)[:J]
    ctrl = rng.standard_normal((nR, steps, meta["C"]))
    last = np.stack([g["X"][-1] for g in gs])
    Y = last.mean(axis=0) @ CC + DD + 0.3 * rng.standard_normal((nR, steps, J))
    x0 = last[:, None, :] + 0.2 * rng.standard_normal((G, nR, D))
    fx = dict(gs=gs, per_model=False, ctrl=ctrl, Y=Y, em=(CC, DD, np.log(sd)), sd=sd, qs=[g["orc"]["H"] for g in gs], x0=x0,
              S0=np.stack([start_cov(G, D, seed=seed + r) for r in range(nR)], axis=1) if with_S0 else None, mode="reference",
              lengths=np.full(nR, steps))
    fx.update(draws(seed + 1, G, nR, steps, n, D, with_S0))
    return fx


@functools.lru_cache(maxsize=None)
def small_d1():
    fx = _small(901, D=1, G=2, nR=2, steps=6, with_S0=True)
    fx["Y"][1, 2] = np.nan
    return fx


@functools.lru_cache(maxsize=None)
def small_d8():
    return _small(911, D=8, steps=5)


@functools.lru_cache(maxsize=None)
def small_n2():
    return _small(921, n=2, steps=8, with_S0=True)


@functools.lru_cache(maxsize=None)
def small_n2048():
    return _small(935, n=2048, steps=2)                           # (931 and 932 miss the margin: gaps of 7.6e-9 and 2.5e-9)


@functools.lru_cache(maxsize=None)
def small_last_nan():
    fx = _small(941, G=2, steps=6)
    fx["Y"][0, -1] = np.nan
    return fx


@functools.lru_cache(maxsize=None)
def small_partial():
    fx = _small(951, D=3, steps=7)
    fx["Y"][0, :, 1] = np.nan                                     # the middle output is never observed
    fx["Y"][0, 2, 0] = fx["Y"][0, 4, 2] = np.nan                  # rows with one output, with another
    fx["Y"][0, 5] = np.nan                                        # and a row with none
    return fx


@functools.lru_cache(maxsize=None)
def small_sharp():
    return _small(961, D=3, steps=6, sd=(0.4, 0.4e-6, 1.3))


SMALL = dict(d1=small_d1, d8=small_d8, n2=small_n2, n2048=small_n2048, last_nan=small_last_nan, partial=small_partial, sharp=small_sharp)


def fixture(name):
    """a case of CASES (a tuple), a key of EDGES or a key of SMALL"""
    return case_fixture(*name) if isinstance(name, tuple) else EDGES[name]() if name in EDGES else SMALL[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref, e_ref and the np.longdouble composition of a fixture by tests/particle_adapted_ref.py.  Computed once, never modified."""
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return pa.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                        fx["eps"], fx["unif"], fx["xi0"])


def margin_holds(name):
    """The margin condition of a fixture: (gap, drift, same ancestors, whether it holds)"""
    ref, _, wide = reference(name)
    gap, drift, same = pa.margin(ref, fixture(name)["unif"], wide)
    return gap, drift, same, bool(same and gap >= max(1e-8, 1000.0 * drift))


def _models(fx, src="orc"):
    gs = fx["gs"]
    if fx["per_model"]:
        return [g[src]["L"] for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs]
    return gs[0][src]["L"], gs[0]["Z"], gs[0]["kern"]


def call(fx, src="orc", fn=None, **kw):
    """prediction.filter_adapted_records_grouped (or `fn`: the bootstrap call) on a fixture (the oracle's posterior)"""
    gs = fx["gs"]
    Ls, Zs, kerns = _models(fx, src)
    args = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    args.update(kw)
    return (fn or pr.filter_adapted_records_grouped)(Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"],
                                                     [g["Q"] for g in gs], *fx["em"], fx["eps"], fx["unif"], **args)
