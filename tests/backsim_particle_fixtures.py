"""The fixtures of the particle backward simulation's device tests (tests/test_gpu_backsim_particle.py), kept apart from them so that
the margin condition those tests rest on can be checked without a GPU: test infrastructure.

A fixture is one of tests/particle_fixtures.py plus unif_bs (G, R, steps, B), seeded per fixture and held in the full layout; a
fixture that misses the margin condition gets another seed here, never another bound there.

  the seven cases of tests/test_gpu_filter_grouped.py (R = 3 records, lengths (12, 12, 9), N = 48, D = 2, 3, 4, 1, 8; J = 3; start
  covariances; one model per group), B = 3;
  m300 (M = 300), B = 3;  n130 (N = 130), B = 300 -- the moments kernel strides twice;  n700 (PT = 3), B = 3;
  n2 (N = 2, B = 1), n13 (N = 13), n2048 (PT = 8, the smallest M, one group, 3 rows), one_row (a record of one row), last_unobserved
  (B = 300), all_nan (a record with no observation at all: no resampling anywhere)."""
import functools

import numpy as np

import particle_backsim_ref as pb
import particle_fixtures as fxt
from ffvd_amd import prediction as pr
from test_gpu_filter_grouped import CASES
from test_gpu_moment_grouped import WIDE

SMALL = ("n2", "n13", "n2048", "one_row", "last_unobserved", "all_nan")
NAMES = list(CASES) + sorted(fxt.EDGES) + list(SMALL)
B_OF = {"n130": 300, "n2": 1, "last_unobserved": 300}
SEEDS = {name: 1900 + i for i, name in enumerate(NAMES)}


def with_uniforms(fx, B, seed):
    G, R, steps = fx["unif"].shape
    return dict(fx, unif_bs=np.random.default_rng(seed).random((G, R, steps, B)))


def _base(name):
    if isinstance(name, tuple):
        return fxt.case_fixture(*name)
    if name in fxt.EDGES:
        return fxt.EDGES[name]()
    if name == "n2":                                              # two particles: one wavefront with two live lanes
        return fxt._one_record(CASES[0], 6, 2, 841)
    if name == "n13":
        return fxt._one_record(CASES[0], 6, 13, 843)
    if name == "n2048":                                           # eight particles per thread in the scan; M = 24
        return fxt._one_record(CASES[0], 3, 2048, 845, groups=[0])
    if name == "one_row":                                         # no backward row at all
        return fxt._one_record(CASES[0], 1, 48, 851)
    fx = fxt._one_record(CASES[0], 6, 48, 853)
    Y = fx["Y"].copy()
    if name == "last_unobserved":
        Y[0, 5] = np.nan
    else:
        Y[:] = np.nan
    return dict(fx, Y=Y)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return with_uniforms(_base(name), B_OF.get(name, 3), SEEDS[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref, e_ref and the np.longdouble composition of a fixture.  Computed once, never modified."""
    fx = fixture(name)
    CC, DD, _ = fx["em"]
    return pb.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                        fx["eps"], fx["unif"], fx["unif_bs"], fx["xi0"])


def subset(fx, groups=None, recs=None):
    """the fixture of some groups and some records, the draws sliced with them"""
    gi = list(range(len(fx["gs"]))) if groups is None else groups
    ri = list(range(fx["Y"].shape[0])) if recs is None else recs
    return dict(fxt.subset(fx, groups, recs), unif_bs=fx["unif_bs"][gi][:, ri])


def call(fx, src="orc", **kw):
    """prediction.backsim_particle_records_grouped on a fixture (the oracle's posterior)"""
    gs = fx["gs"]
    if fx["per_model"]:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g[src]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    args = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    args.update(kw)
    return pr.backsim_particle_records_grouped(Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"],
                                               [g["Q"] for g in gs], *fx["em"], fx["eps"], fx["unif"], fx["unif_bs"], **args)
