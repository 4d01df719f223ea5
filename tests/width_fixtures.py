"""Fixtures at the widths the filtering family is compiled for but the shared shapes never reach (tests/test_gpu_widths.py): test
infrastructure.  The shared shapes have D in {1, 2, 3, 4, 8}, J in {1, 3} and P = D + C <= 9; the kernels are instantiated for every
D = 1 .. 8 (MG_DISPATCH_D), stage J <= 8 outputs and accept P <= 32 input columns.

A fixture is the dict of tests/particle_fixtures.py (gs, per_model, ctrl, Y, em, sd, qs, x0, S0, mode, lengths, eps, unif, xi0).  It
carries the oracle's posterior only (no device call builds it), so tests/test_width_fixtures.py checks without a GPU what the device
tests rest on: the margin conditions of the three particle references, weights that are not degenerate, and that an index mistake in
the last input columns or the last outputs moves the references by at least 1000 x the device tests' bound.  A fixture that misses a
margin gets another seed here, never another bound.

  d5      D = 5, C = 1, P = 6    15 pairs in the triangle
  d6      D = 6, C = 2, P = 8    the upper edge of the 8-column conditional-gradient kernel
  d7      D = 7, C = 0, P = 7    no control input; 28 pairs; J D = 56 staging threads
  p32     D = 8, C = 24, P = 32  every limit at once
  p32d3   D = 3, C = 29, P = 32  the widest input with few state columns
  d7_shared, p32_shared          the same without q slices: one shared Gamma, a unit is a dim and its rows are all tracks of the pass

Common: synthetic.make_named("tiny", D, C, M = 40, T = 64, S = 2) (a ragged last slab of 8 rows, Mp = 64), two chains of one model,
"intent", R = 2 records of 6 and 5 rows, start covariances, N = 48 particles, J = 8 outputs with sd = SD.

Hyper-parameters.  `make_workload` gives every input column of a dim one lengthscale, so a wrong column index changes nothing there.
Here every (d, p) has its own:  loglengthscales + 0.5 log(max(P, 3) / 3) + 0.05 N(0, 1), and logvariance + 0.05 N(0, 1) per dim.  The
widening keeps the GP alive at P = 32: squared distances between random points grow with P, and at the workload's lengthscales the
kernel between them is about 1e-4 there, the transition a constant.

Observations: the chains' mean last state through the seeded emission plus 0.3 N(0, 1); record 0 row 2 is unobserved, record 1
row 3 lacks outputs 0, 2, 4 and 6 (output 7 is observed where output 0 is not), record 1 ends after 5 rows."""
import functools

import numpy as np

import cubature_filter_ref as cf
import filter_ref as fr
import linear_filter_ref as lf
import moment_ref as mr
import particle_adapted_ref as pa
import particle_backsim_ref as pb
import particle_filter_ref as pf
import records_ref as rr
from adapted_particle_fixtures import _orc_group
from ffvd_amd import synthetic
from particle_fixtures import draws
from test_gpu_moment_grouped import WIDE, start_cov

N, J, R, STEPS, M, B, H = 48, 8, 2, 6, 40, 5, 3
LENGTHS = (6, 5)
SD = (0.8, 1.6, 2.6, 1.4, 1.0, 1.8, 2.2, 1.2)
#            D, C, q slices, seed
#            (seed 2131 gives p32 a median bootstrap ess of 2.5: below the 3 that tests/test_width_fixtures.py asks for)
SPECS = dict(d5=(5, 1, True, 2101), d6=(6, 2, True, 2111), d7=(7, 0, True, 2121), p32=(8, 24, True, 2151), p32d3=(3, 29, True, 2141),
             d7_shared=(7, 0, False, 2121), p32_shared=(8, 24, False, 2151))
NAMES = tuple(SPECS)


def widened(params, meta, seed):
    """a copy of `params` with a lengthscale of its own in every (d, p) and a variance of its own per dim"""
    rng = np.random.default_rng(seed)
    D, P = meta["D"], meta["P"]
    p = dict(params)
    p["loglengthscales"] = params["loglengthscales"] + 0.5 * np.log(max(P, 3) / 3.0) + 0.05 * rng.standard_normal((D, P))
    p["logvariance"] = params["logvariance"] + 0.05 * rng.standard_normal(D)
    return p


@functools.lru_cache(maxsize=None)
def model(name):
    """(params, control rows of the posterior, meta) of a fixture: shared, never modified"""
    D, C, _, seed = SPECS[name]
    params, _, c, meta = synthetic.make_named("tiny", D=D, C=C, M=M, T=64, S=2)
    return widened(params, meta, seed), c, meta


def build(name):
    D, C, slices, seed = SPECS[name]
    p, c, meta = model(name)
    gs = [_orc_group(p, c, meta, p["X"][g]) for g in range(2)]
    rng = np.random.default_rng(seed + 1)
    CC, DD, sd = rng.standard_normal((D, J)), rng.standard_normal(J), np.asarray(SD, dtype=np.float64)
    ctrl = rng.standard_normal((R, STEPS, C)) if C else None
    last = np.stack([g["X"][-1] for g in gs])
    Y = last.mean(axis=0) @ CC + DD + 0.3 * rng.standard_normal((R, STEPS, J))
    Y[0, 2] = np.nan
    Y[1, 3, 0::2] = np.nan
    Y[1, LENGTHS[1]:] = np.nan
    x0 = last[:, None, :] + 0.2 * rng.standard_normal((2, R, D)) * (np.arange(R) > 0)[None, :, None]   # record 0 starts at the chains' last states
    fx = dict(gs=gs, per_model=False, ctrl=ctrl, Y=Y, em=(CC, DD, np.log(sd)), sd=sd, qs=[g["orc"]["H"] for g in gs] if slices else None,
              x0=x0, S0=np.stack([start_cov(2, D, seed=seed + 2 + r) for r in range(R)], axis=1), mode="intent", lengths=np.array(LENGTHS))
    fx.update(draws(seed + 4, 2, R, STEPS, N, D, True))
    fx["unif_bs"] = np.random.default_rng(seed + 5).random((2, R, STEPS, B))
    fx["eps_fc"] = np.random.default_rng(seed + 6).standard_normal((2, STEPS - H, H, N, D))      # the particle fan of record 0
    return fx


@functools.lru_cache(maxsize=None)
def fixture(name):
    """Shared, never modified"""
    return build(name)


def _args(fx):
    CC, DD, _ = fx["em"]
    return fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE


@functools.lru_cache(maxsize=None)
def bootstrap_reference(name):
    """ref, e_ref and the np.longdouble composition by tests/particle_filter_ref.py.  Computed once, never modified."""
    fx = fixture(name)
    return pf.reference(*_args(fx), fx["eps"], fx["unif"], fx["xi0"])


@functools.lru_cache(maxsize=None)
def adapted_reference(name):
    """the same by tests/particle_adapted_ref.py"""
    fx = fixture(name)
    return pa.reference(*_args(fx), fx["eps"], fx["unif"], fx["xi0"])


@functools.lru_cache(maxsize=None)
def backsim_reference(name):
    """the same by tests/particle_backsim_ref.py with B trajectories"""
    fx = fixture(name)
    return pb.reference(*_args(fx), fx["eps"], fx["unif"], fx["unif_bs"], fx["xi0"])


def propagation(fx, wide=WIDE):
    """moment_ref.propagate over the rows of record 0 from its start, per group: m (G, STEPS, D), S (G, STEPS, D, D) in fp64 and their
    largest error against np.longdouble (e_m, e_S; zeros when `wide` is false)"""
    out = dict(m=[], S=[], e_m=0.0, e_S=0.0)
    for i, g in enumerate(fx["gs"]):
        res = {}
        for t in (np.float64, np.longdouble) if wide else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if fx["qs"] is None else fx["qs"][i], fx["mode"], dtype=t)
            res[t] = mr.propagate(fx["x0"][i, 0], fx["S0"][i, 0], None if fx["ctrl"] is None else fx["ctrl"][0], g["Z"], g["okern"], beta, Gam,
                                  g["Q"], STEPS, dtype=t)
        out["m"].append(res[np.float64][0])
        out["S"].append(res[np.float64][1])
        if wide:
            out["e_m"] = max(out["e_m"], float(np.max(np.abs(res[np.float64][0] - res[np.longdouble][0]))))
            out["e_S"] = max(out["e_S"], float(np.max(np.abs(res[np.float64][1] - res[np.longdouble][1]))))
    out["m"], out["S"] = np.stack(out["m"]), np.stack(out["S"])
    return out


@functools.lru_cache(maxsize=None)
def propagation_reference(name):
    """Computed once, never modified."""
    return propagation(fixture(name))


@functools.lru_cache(maxsize=None)
def records_reference(name):
    """ref, e_ref of the linearised records filter (tests/records_ref.py).  Computed once, never modified."""
    return rr.reference(*_args(fixture(name)))


@functools.lru_cache(maxsize=None)
def cubature_reference(name):
    """ref, e_ref of the cubature records filter (tests/cubature_filter_ref.py)"""
    return cf.reference(*_args(fixture(name)))


def single_record_filter(fx, transition, wide=WIDE):
    """filter_ref.filter and smooth over record 0 per group with `transition` (filter_ref.gp_transition: moment matching;
    linear_filter_ref.ekf_transition): the arrays of tests/test_gpu_filter_grouped.py's MOMENTS stacked over the groups, and e_ref"""
    CC, DD, _ = fx["em"]
    keys = ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "m_smooth", "S_smooth")
    ref, e_ref = {k: [] for k in keys}, {k: 0.0 for k in keys}
    ctrl = None if fx["ctrl"] is None else fx["ctrl"][0]
    for i, g in enumerate(fx["gs"]):
        res = {}
        for t in (np.float64, np.longdouble) if wide else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if fx["qs"] is None else fx["qs"][i], fx["mode"], dtype=t)
            f = fr.filter(fx["x0"][i, 0], fx["S0"][i, 0], fx["Y"][0], CC, DD, fx["sd"], g["Q"], transition(ctrl, g["Z"], g["okern"], beta, Gam, dtype=t),
                          dtype=t)
            f["m_smooth"], f["S_smooth"] = fr.smooth(f, dtype=t)
            res[t] = f
        for k in keys:
            ref[k].append(res[np.float64][k])
            if wide:
                e_ref[k] = max(e_ref[k], float(np.max(np.abs(res[np.float64][k] - res[np.longdouble][k]))))
    return {k: np.stack(v) for k, v in ref.items()}, e_ref


@functools.lru_cache(maxsize=None)
def moment_filter_reference(name):
    """ref, e_ref of the moment-matching filter and smoother over record 0 (tests/filter_ref.py)"""
    return single_record_filter(fixture(name), fr.gp_transition)


@functools.lru_cache(maxsize=None)
def linear_filter_reference(name):
    """the same with the linearised transition (tests/linear_filter_ref.py)"""
    return single_record_filter(fixture(name), lf.ekf_transition)


def bootstrap(fx, wide=False):
    """tests/particle_filter_ref.py on any fixture dict (a perturbed one: tests/test_width_fixtures.py)"""
    return pf.reference(*_args(fx)[:-1], wide, fx["eps"], fx["unif"], fx["xi0"])


# ---- the index mistakes the fixtures are there to show (tests/test_width_fixtures.py measures what each moves) -------------------------
def _swap_last(x):
    x = np.array(x)
    x[..., [-2, -1]] = x[..., [-1, -2]]
    return x


def swap_last_two_inputs(fx):
    """a kernel that reads input column P - 2 for P - 1 and the reverse: with two control columns or more, the last two of the control
    rows; otherwise (d5: one control column; d7: none) the last two columns of Z under the same posterior"""
    if fx["ctrl"] is not None and fx["ctrl"].shape[-1] >= 2:
        return dict(fx, ctrl=_swap_last(fx["ctrl"]))
    return dict(fx, gs=[dict(g, Z=_swap_last(g["Z"])) for g in fx["gs"]])


def zero_last_control(fx):
    """a kernel that never loads input column P - 1"""
    ctrl = np.array(fx["ctrl"])
    ctrl[..., -1] = 0.0
    return dict(fx, ctrl=ctrl)


def drop_output_7(fx):
    """a kernel whose loop over the outputs ends one short"""
    Y = np.array(fx["Y"])
    Y[..., J - 1] = np.nan
    return dict(fx, Y=Y)


def swap_sd_6_and_7(fx):
    """a kernel that reads the noise of output 6 for output 7 and the reverse"""
    return dict(fx, sd=_swap_last(fx["sd"]))


INPUT_MISTAKES = dict(swap_last_two_inputs=swap_last_two_inputs, zero_last_control=zero_last_control)
EMISSION_MISTAKES = dict(drop_output_7=drop_output_7, swap_sd_6_and_7=swap_sd_6_and_7)


def margins(name):
    """per reference (gap, drift, identical indices): the condition of tests/test_adapted_fixtures.py"""
    unif = fixture(name)["unif"]
    out = {}
    for key, (ref, _, wide), fn in (("bootstrap", bootstrap_reference(name), pf.margin), ("adapted", adapted_reference(name), pa.margin),
                                    ("backsim", backsim_reference(name), pb.margin)):
        out[key] = fn(ref, unif, wide)
    return out
