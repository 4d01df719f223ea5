"""The fixtures of the particle filter's device tests (tests/test_gpu_filter_particle.py), kept apart from them so that
tests/test_particle_filter_ref.py can check, without a GPU, the margin condition those tests rest on: test infrastructure.

A fixture is a dict: gs (per group: Z, kern, okern, Q, X, orc), per_model, ctrl (R, steps, C) or None, Y (R, steps, J), em = (CC, DD,
log_Rchols), sd, qs (per group or None), x0 (G, R, D), S0 (G, R, D, D) or None, mode, lengths (R,), eps (G, R, steps, N, D), unif
(G, R, steps), xi0 (G, R, N, D) or None.  The draws are seeded per fixture and held in the full layout; a fixture that misses the
margin condition gets another seed here, never another bound there.

`case_fixture`: the seven cases and the R = 3 records of tests/test_gpu_filter_records.py with N = 48 particles (not a multiple of 64;
144 rows per (group, dim) unit: track 2 straddles the 128-row tile).  `EDGES`: M = 300 (a ragged last column tile), N = 130 with one
record (two row tiles, the second with 2 live rows), N = 700 (several particles per thread in the scan and the gather)."""
import functools

import numpy as np

import particle_filter_ref as pf
from ffvd_amd import prediction as pr, synthetic
from test_gpu_conditional_grouped import _group
from test_gpu_filter_grouped import CASES, emission
from test_gpu_filter_records import R, records
from test_gpu_moment_grouped import STEPS, WIDE, _q, case, start_cov

N = 48
SEEDS = {c: 700 + i for i, c in enumerate(CASES)}


def draws(seed, G, nR, steps, n, D, with_xi0):
    rng = np.random.default_rng(seed)
    return dict(eps=rng.standard_normal((G, nR, steps, n, D)), unif=rng.random((G, nR, steps)),
                xi0=rng.standard_normal((G, nR, n, D)) if with_xi0 else None)


@functools.lru_cache(maxsize=None)
def case_fixture(shape, per_model, G, qkind, mode, J, with_S0):
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, rec = case(shape, per_model, G), records(*args)
    gs, D = cs[0], cs[2]["D"]
    fx = dict(gs=gs, per_model=per_model, ctrl=rec["ctrl"], Y=rec["Y"], em=emission(cs, J), sd=rec["sd"], qs=_q(cs, qkind), x0=rec["x0"],
              S0=rec["S0"], mode=mode, lengths=rec["lengths"])
    fx.update(draws(SEEDS[args], len(gs), R, STEPS, N, D, with_S0))
    return fx


@functools.lru_cache(maxsize=None)
def edge_m300():
    """tests/test_gpu_filter_cubature.py::test_a_ragged_last_column_tile's model and records: M = 300, Mp = 320, three column tiles of
    the product, the last 64 wide, and a second stride of 256 columns in the rows kernel."""
    params, _, c, meta = synthetic.make_named("tiny", M=300, T=320, S=2)
    gs = [_group(params, c, meta, params["X"][g]) for g in range(2)]
    D, n = meta["D"], 6
    rng = np.random.default_rng(3)
    ctrl = rng.standard_normal((2, n, meta["C"]))
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    Y = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(31).standard_normal((2, n, CC.shape[1]))
    Y[0, 2] = np.nan
    Y[1, 5] = np.nan
    x0 = np.stack([g["X"][-1] for g in gs])[:, None, :] + 0.2 * rng.standard_normal((2, 2, D))
    fx = dict(gs=gs, per_model=False, ctrl=ctrl, Y=Y, em=(CC, DD, lr), sd=np.exp(np.asarray(lr)[0]), qs=[g["orc"]["H"] for g in gs], x0=x0,
              S0=np.stack([start_cov(2, D, seed=5 + r) for r in range(2)], axis=1), mode="intent", lengths=np.array([n, 5]))
    fx.update(draws(811, 2, 2, n, N, D, True))
    return fx


def _one_record(args, steps, n, seed, groups=None):
    """record 0 of a case cut to `steps` rows, with n particles"""
    fx = case_fixture(*args)
    idx = list(range(len(fx["gs"]))) if groups is None else groups
    out = dict(fx, gs=[fx["gs"][g] for g in idx], qs=None if fx["qs"] is None else [fx["qs"][g] for g in idx],
               ctrl=None if fx["ctrl"] is None else fx["ctrl"][:1, :steps], Y=fx["Y"][:1, :steps], x0=fx["x0"][idx][:, :1],
               S0=None if fx["S0"] is None else fx["S0"][idx][:, :1], lengths=np.array([steps]))
    out.update(draws(seed, len(idx), 1, steps, n, fx["x0"].shape[-1], fx["S0"] is not None))
    return out


@functools.lru_cache(maxsize=None)
def edge_n130():
    """CASES[0] (two chains of one model, q slices), one record of 6 rows, N = 130: every (group, dim) unit has two row tiles, the
    second with 2 live rows."""
    return _one_record(CASES[0], 6, 130, 821)


@functools.lru_cache(maxsize=None)
def edge_n700():
    """CASES[6] (one chain, no q slices, a start covariance), one record of 4 rows, N = 700: three particles per thread in the scan,
    three strides in the gather, six row tiles."""
    return _one_record(CASES[6], 4, 700, 831)


EDGES = dict(m300=edge_m300, n130=edge_n130, n700=edge_n700)


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref, e_ref and the np.longdouble composition of a fixture: a case of CASES or a key of EDGES.  Computed once, never modified."""
    fx = case_fixture(*name) if isinstance(name, tuple) else EDGES[name]()
    CC, DD, _ = fx["em"]
    return pf.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                        fx["eps"], fx["unif"], fx["xi0"])


def subset(fx, groups=None, recs=None):
    """the fixture of some groups and some records, the draws sliced with them"""
    gi = list(range(len(fx["gs"]))) if groups is None else groups
    ri = list(range(fx["Y"].shape[0])) if recs is None else recs
    cut = lambda x: None if x is None else x[gi][:, ri]
    return dict(fx, gs=[fx["gs"][g] for g in gi], qs=None if fx["qs"] is None else [fx["qs"][g] for g in gi],
                ctrl=None if fx["ctrl"] is None else fx["ctrl"][ri], Y=fx["Y"][ri], x0=cut(fx["x0"]), S0=cut(fx["S0"]),
                lengths=np.asarray(fx["lengths"])[ri], eps=cut(fx["eps"]), unif=cut(fx["unif"]), xi0=cut(fx["xi0"]))


def call(fx, src="orc", **kw):
    """prediction.filter_particle_records_grouped on a fixture (the oracle's posterior)"""
    gs = fx["gs"]
    if fx["per_model"]:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g[src]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    args = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], return_particles=True)
    args.update(kw)
    return pr.filter_particle_records_grouped(Ls, Zs, kerns, [g[src]["U"] for g in gs], fx["qs"], fx["x0"], fx["ctrl"], fx["Y"],
                                              [g["Q"] for g in gs], *fx["em"], fx["eps"], fx["unif"], **args)
