"""The fixtures of the particle forecasts' device tests (tests/test_gpu_forecast_particle.py): test infrastructure, built on
tests/particle_fixtures.py.

A fixture is a particle fixture with ONE record (`subset(fx, recs=[0])`: Y (1, steps, J), ctrl (1, steps, C) or None, x0 (G, 1, D),
eps (G, 1, steps, N, D), unif (G, 1, steps), xi0 (G, 1, N, D) or None) plus h, origins (B,) and eps_fc (G, B, h, N, D), seeded per
fixture in the full layout.  The filter's draws are those of the particle filter's fixtures, which satisfy the margin condition; a
fixture that misses it gets another seed here or there, never another bound.

`case_fixture`: record 0 of each of the seven cases, 12 rows (row 3 and rows 9 .. 11 unobserved, entries of rows 5 and 6 where J = 3),
N = 48, h = 3, origins (0, 3, 4, 8): 192 rows per (group, dim) unit, so track 2 straddles the 128-row tile, and origin 3 is a row
with nothing observed.  `EDGES`: M = 300 (a ragged last column tile; origin 2 is unobserved), N = 130 with two origins (260 rows per
unit: three row tiles, the last with 4 live rows), N = 700 with h = 2 (three strides in every loop over the particles)."""
import functools

import numpy as np

import forecast_particle_ref as fpr
import particle_filter_ref as pf
import particle_fixtures as fxt
from ffvd_amd import prediction as pr
from test_gpu_filter_grouped import CASES
from test_gpu_moment_grouped import WIDE

N, H, ORIGINS = fxt.N, 3, (0, 3, 4, 8)
SEEDS = {c: 900 + i for i, c in enumerate(CASES)}


def _with_forecast(fx, h, origins, seed):
    G, _, _, n, D = fx["eps"].shape
    return dict(fx, h=h, origins=np.asarray(origins), eps_fc=np.random.default_rng(seed).standard_normal((G, len(origins), h, n, D)))


@functools.lru_cache(maxsize=None)
def case_fixture(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    return _with_forecast(fxt.subset(fxt.case_fixture(*args), recs=[0]), H, ORIGINS, SEEDS[args])


@functools.lru_cache(maxsize=None)
def edge_m300():
    """record 0 of particle_fixtures.edge_m300 (6 rows, row 2 unobserved), h = 2, origins (0, 2, 3)"""
    return _with_forecast(fxt.subset(fxt.edge_m300(), recs=[0]), 2, (0, 2, 3), 911)


@functools.lru_cache(maxsize=None)
def edge_n130():
    """particle_fixtures.edge_n130 (6 rows, N = 130), h = 2, two origins"""
    return _with_forecast(fxt.edge_n130(), 2, (1, 3), 921)


@functools.lru_cache(maxsize=None)
def edge_n700():
    """particle_fixtures.edge_n700 (4 rows, N = 700, one chain without q slices, a start covariance), h = 2, origins (0, 1)"""
    return _with_forecast(fxt.edge_n700(), 2, (0, 1), 931)


EDGES = dict(m300=edge_m300, n130=edge_n130, n700=edge_n700)


def fixture(name):
    return case_fixture(*name) if isinstance(name, tuple) else EDGES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref and e_ref of the tracks of a fixture (tests/forecast_particle_ref.py).  Computed once, never modified."""
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return fpr.reference(fx["gs"], None if fx["ctrl"] is None else fx["ctrl"][0], fx["Y"][0], CC, DD, fx["sd"], fx["qs"], fx["x0"][:, 0],
                         None if fx["S0"] is None else fx["S0"][:, 0], fx["mode"], fx["origins"], fx["h"], WIDE, fx["eps"][:, 0],
                         fx["unif"][:, 0], fx["eps_fc"], None if fx["xi0"] is None else fx["xi0"][:, 0])


@functools.lru_cache(maxsize=None)
def filter_reference(name):
    """ref, e_ref and the np.longdouble composition of the filter over the whole record (particle_filter_ref.reference): what
    `margin` is measured on -- every track resamples with a prefix of these rows."""
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return pf.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                        fx["eps"], fx["unif"], fx["xi0"])


def subset(fx, groups=None, origins=None):
    """the fixture of some groups and some origins (positions in fx["origins"], any order), the draws sliced with them"""
    gi = list(range(len(fx["gs"]))) if groups is None else groups
    bi = list(range(len(fx["origins"]))) if origins is None else origins
    return dict(fxt.subset(fx, groups=gi), h=fx["h"], origins=fx["origins"][bi], eps_fc=fx["eps_fc"][gi][:, bi])


def composed(fx):
    """The composed form: the particle fixture of R = B records, record b being rows 0 .. o_b of the record followed by h all-NaN
    rows (padded to a common length; `lengths` says where each ends), the filter's draws and the forecast draws of (g, b)
    concatenated.  particle_fixtures.call on it gives the same tracks."""
    G, _, steps, n, D = fx["eps"].shape
    org, h = fx["origins"], fx["h"]
    B, J = len(org), fx["Y"].shape[2]
    ln = np.array([int(o) + 1 + h for o in org])
    L = int(ln.max())
    Y, eps, unif = np.full((B, L, J), np.nan), np.zeros((G, B, L, n, D)), np.full((G, B, L), 0.5)
    for b, o in enumerate(org):
        o = int(o)
        Y[b, :o + 1] = fx["Y"][0, :o + 1]
        eps[:, b, :o + 1], eps[:, b, o + 1:o + 1 + h] = fx["eps"][:, 0, :o + 1], fx["eps_fc"][:, b]
        unif[:, b, :o + 1] = fx["unif"][:, 0, :o + 1]
    rep = lambda x: None if x is None else np.ascontiguousarray(np.repeat(x, B, axis=1))
    return dict(fx, Y=Y, ctrl=None if fx["ctrl"] is None else np.ascontiguousarray(np.repeat(fx["ctrl"][:, :L], B, axis=0)), x0=rep(fx["x0"]),
                S0=rep(fx["S0"]), xi0=rep(fx["xi0"]), eps=eps, unif=unif, lengths=ln)


def call(fx, src="orc", **kw):
    """prediction.forecast_particle_grouped on a fixture (the oracle's posterior), everything returned"""
    gs = fx["gs"]
    if fx["per_model"]:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g[src]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    one = lambda x: None if x is None else x[:, 0]
    args = dict(xi0=one(fx["xi0"]), origins=fx["origins"], S0s=one(fx["S0"]), q_mode=fx["mode"], return_tracks=True, return_filter=True,
                return_particles=True)
    args.update(kw)
    eps, unif, eps_fc = args.pop("eps", one(fx["eps"])), args.pop("unif", one(fx["unif"])), args.pop("eps_fc", fx["eps_fc"])
    return pr.forecast_particle_grouped(Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"][:, 0],
                                        None if fx["ctrl"] is None else fx["ctrl"][0], 0, fx["Y"][0], [g["Q"] for g in gs], *fx["em"], fx["h"],
                                        eps, unif, eps_fc, **args)
