"""The reference of the cubature forecasts, pinned without a device (tests/forecast_cubature_ref.py), and the fixtures the GPU tests
of tests/test_gpu_forecast_cubature.py run on, built here on the oracle's posterior alone so that they can be judged on the CPU.

1. The definition -- one filter_ref.filter with cubature_filter_ref.ckf_transition per origin over the truncated record followed by h
   all-NaN rows -- equals, bit for bit, continuing h unobserved rows from the filtered state of ONE filter over the whole record
   (`tracks`, which the GPU tests use).
2. On the linear-Gaussian model of tests/test_linear_filter_ref.py the tracks of the rule reproduce the exact Kalman prediction
   (filter_ref.linear_transition from the same filtered states) to 7e-15, the level the cubature filter reference reaches on that
   model (measured here: 4.4e-16 over horizons 1 .. 4 from every origin).
3. From S = 0 at an origin and a process noise of 1e-300, horizon 1 is the ORACLE's conditional at [mu, c] within the floors of
   tests/test_transition_grad_ref.py.
4. Every fixture of the GPU tests keeps the fp64 reference's own S_fc positive definite; the smallest eigenvalue is printed.  The GPU
   tests assert positivity of the device's S_fc only because the reference has it.  Measured: the seven shared cases 0.197 .. 0.666,
   M = 300 0.418, D = 3 with 24 origins 0.389 (q slices) and 0.307 (none), the 140-row record 0.419."""
import functools

import numpy as np
import pytest

import cubature_filter_ref as cf
import filter_ref as fr
import forecast_cubature_ref as fcr
import forecast_linear_ref as flr
import moment_ref as mr
from ffvd_amd import synthetic
from oracle import ffvd_oracle as orc
from test_gpu_filter_grouped import CASES, emission, gaps
from test_gpu_forecast_grouped import H, ORIGINS
from test_gpu_moment_grouped import SHAPES, STEPS, _q
from test_transition_grad_ref import MODES, case as point_case, floor
from test_transition_grad_ref import SHAPES as POINT_SHAPES


# ---- the fixtures of the GPU tests, on the oracle's posterior (no device) ------------------------------------------------------------
def orc_group(p, c, meta, X):
    """tests/test_gpu_conditional_grouped.py::_group without the device's posterior (the reference reads the oracle's alone)"""
    T = meta["T"]
    okern, Q = orc.make_kernels(p, kernel_type=meta["kernel_type"]), np.exp(p["log_Q"])
    Lo = orc.kernel_pre_cal(p["Z"], okern)
    Uo, Ho = orc.collapse_u_mean_after_kernel_precalculation(Lo, np.concatenate((X[:T], c[:T]), axis=1), X, p["Z"], okern, Q)
    return dict(Z=p["Z"], okern=okern, X=X, Q=Q, orc=dict(L=list(Lo), U=Uo, H=np.asarray(Ho)))


@functools.lru_cache(maxsize=None)
def cpu_case(shape, per_model=False, G=None):
    """tests/test_gpu_moment_grouped.py::case on `orc_group` (the GPU tests compare the two)"""
    name, ov = SHAPES[shape]
    if G is not None:
        ov = dict(ov, S=G)
    params, _, c, meta = synthetic.make_named(name, **ov)
    gs = []
    for g in range(meta["S"]):
        q, X = dict(params), params["X"][g]
        if per_model:
            rng = np.random.default_rng(1000 + g)
            q["logvariance"] = params["logvariance"] + 0.05 * rng.standard_normal(params["logvariance"].shape)
            q["loglengthscales"] = params["loglengthscales"] + 0.05 * rng.standard_normal(params["loglengthscales"].shape)
            q["Z"] = params["Z"] + 0.01 * rng.standard_normal(params["Z"].shape)
            q["log_Q"] = params["log_Q"] + 0.05 * rng.standard_normal(params["log_Q"].shape)
            X = X + 0.1 * rng.standard_normal(X.shape)
        gs.append(orc_group(q, c, meta, X))
    call = np.concatenate((c, np.random.default_rng(3).standard_normal((STEPS, meta["C"]))), axis=0)
    return gs, call, meta, per_model, params


def _start_covs(cs, with_S0):
    n, D = len(cs[0]), cs[2]["D"]
    return flr.start_cov(n, D) if with_S0 else np.zeros((n, D, D))


@functools.lru_cache(maxsize=None)
def cpu_observations(shape, per_model, G, qkind, mode, J, with_S0):
    """tests/test_gpu_filter_grouped.py::observations on `cpu_case`: the 12-row record with its gaps, and sd"""
    cs = cpu_case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    qs, S0 = _q(cs, qkind), _start_covs(cs, with_S0)
    ms, Ss = [], []
    for i, g in enumerate(gs):
        beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode)
        m, S = mr.propagate(g["X"][-1], S0[i], call[meta["T"]: meta["T"] + STEPS], g["Z"], g["okern"], beta, Gam, g["Q"], STEPS)
        ms.append(m)
        Ss.append(S)
    CC, DD, lr = emission(cs, J)
    sd = np.exp(np.asarray(lr).reshape(-1)[:J]) if J > 1 else np.exp(np.asarray(lr)[0])
    m = np.mean(np.einsum("gtk,kj->gtj", np.stack(ms), CC) + DD, axis=0)
    s2 = np.mean(np.einsum("kj,gtkl,lj->gtj", CC, np.stack(Ss), CC) + sd ** 2, axis=0)
    return gaps(m + 0.5 * np.sqrt(s2) * np.random.default_rng(29).standard_normal(m.shape)), sd


def shared_reference(args, wide):
    """the reference of one of the seven CASES: the 12-row record, H = 3, origins 0 .. 8"""
    shape, per_model, G, qkind, mode, J, with_S0 = args
    cs = cpu_case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    Y, sd = cpu_observations(*args)
    CC, DD, _ = emission(cs, J)
    return fcr.reference(gs, call[meta["T"]: meta["T"] + STEPS], Y, CC, DD, sd, _q(cs, qkind), _start_covs(cs, with_S0), mode, ORIGINS, H, wide)


def _record(params, c, meta, n, h, seed, gap, **kw):
    """two chains of one model with q slices, "intent", a start covariance: n rows of noise 0.3 around the emission of the chains' last
    states (default_rng(seed)), row `gap` unobserved, default_rng(3) controls, origins 0 .. n - h - 1"""
    gs = [orc_group(params, c, meta, params["X"][g]) for g in range(2)]
    T, D = meta["T"], meta["D"]
    call = np.concatenate((c, np.random.default_rng(3).standard_normal((n, meta["C"]))), axis=0)
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    Y = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(seed).standard_normal((n, CC.shape[1]))
    Y[gap] = np.nan
    return dict(params=params, c=c, meta=meta, gs=gs, call=call, ctrl=call[T: T + n], Y=Y, CC=CC, DD=DD, lr=lr, sd=np.exp(np.asarray(lr)[0]),
                S0=flr.start_cov(2, D), qs=[g["orc"]["H"] for g in gs], mode="intent", origins=list(range(n - h)), h=h, **kw)


@functools.lru_cache(maxsize=None)
def m300_record():
    """synthetic "tiny" with M = 300, T = 320, S = 2: Mp = 320, a ragged last column tile of the product and a second stride of 256
    columns in the state kernel; six rows with a gap, h = 2, origins 0 .. 3.  Shared, never modified."""
    params, _, c, meta = synthetic.make_named("tiny", M=300, T=320, S=2)
    return _record(params, c, meta, 6, 2, 31, 2)


@functools.lru_cache(maxsize=None)
def d3_record():
    """synthetic "ragged" (M = 77, D = 3, C = 2, two chains of one model): a 26-row record, h = 2, origins 0 .. 23, so 24 tracks of 6
    rows = 144 rows per (group, dim) unit: rows 126 .. 131 of track 21 lie in two row tiles, the second tile has 16 live rows.
    Shared, never modified."""
    params, _, c, meta = synthetic.make_named("ragged")
    return _record(params, c, meta, 26, 2, 37, 7)


def record_reference(r, wide, slices=True):
    return fcr.reference(r["gs"], r["ctrl"], r["Y"], r["CC"], r["DD"], r["sd"], r["qs"] if slices else None, r["S0"], r["mode"], r["origins"],
                         r["h"], wide)


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------------
def test_continuing_from_the_filtered_state_is_the_definition():
    r = flr.long_record()
    origins, h, J = [0, 6, 7, 8, 77, 137], r["h"], r["Y"].shape[1]
    for i, g in enumerate(r["gs"]):
        beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], r["qs"][i], r["mode"])
        model = (r["ctrl"], g["Z"], g["okern"], beta, Gam)
        f = fr.filter(g["X"][-1], r["S0"][i], r["Y"], r["CC"], r["DD"], r["sd"], g["Q"], cf.ckf_transition(*model))
        m, S = fcr.tracks(f, origins, h, J, r["CC"], r["DD"], r["sd"], g["Q"], *model)
        mn, Sn = fcr.naive(g["X"][-1], r["S0"][i], r["Y"], origins, h, r["CC"], r["DD"], r["sd"], g["Q"], *model)
        assert m.shape == (len(origins), h, 2) and S.shape == (len(origins), h, 2, 2)
        np.testing.assert_array_equal(m, mn)
        np.testing.assert_array_equal(S, Sn)
        rows = [o + 1 for o in origins]                           # horizon 1 is the filter's own prediction of the next row
        np.testing.assert_array_equal(m[:, 0], f["m_pred"][rows])
        np.testing.assert_array_equal(S[:, 0], f["S_pred"][rows])


# ---- 2. exact on a linear-Gaussian model ----------------------------------------------------------------------------------------------
def test_on_a_linear_gaussian_model_the_tracks_are_the_kalman_prediction():
    rng = np.random.default_rng(41)                               # the model of test_linear_filter_ref.py
    D, J, n, h = 3, 2, 9, 4
    A, b = np.eye(D) + 0.3 * rng.standard_normal((D, D)), rng.standard_normal(D)
    CC, DD, sd, Q = rng.standard_normal((D, J)), rng.standard_normal(J), np.asarray((0.3, 0.7)), np.asarray((0.05, 0.1, 0.2))
    Y = rng.standard_normal((n, J))
    Y[2, :] = np.nan
    Y[5, 0] = np.nan
    x0, S0 = rng.standard_normal(D), 0.4 * np.eye(D)
    F = A - np.eye(D)
    cond = lambda i, X: (X @ F.T + b[None, :], np.zeros_like(X))
    rule = lambda c, Z, kern, beta, Gam, dtype: cf.cubature_transition(cond, dtype=dtype)
    exact = lambda c, Z, kern, beta, Gam, dtype: fr.linear_transition(A, b)
    origins, none = list(range(n - h)), (None,) * 5
    f = fr.filter(x0, S0, Y, CC, DD, sd, Q, cf.cubature_transition(cond))
    m, S = fcr.tracks(f, origins, h, J, CC, DD, sd, Q, *none, transition=rule)
    mn, Sn = fcr.naive(x0, S0, Y, origins, h, CC, DD, sd, Q, *none, transition=rule)
    np.testing.assert_array_equal(m, mn)
    np.testing.assert_array_equal(S, Sn)
    mk, Sk = fcr.tracks(f, origins, h, J, CC, DD, sd, Q, *none, transition=exact)          # the Kalman prediction from the same states
    worst = max(float(np.max(np.abs(m - mk))), float(np.max(np.abs(S - Sk))))
    print(f"linear-Gaussian model: largest difference of the cubature tracks from the Kalman prediction {worst:.3e}")
    assert worst <= 7e-15


# ---- 3. from a point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(POINT_SHAPES))
def test_horizon_one_from_a_point_is_the_oracle_conditional(shape, mode):
    cs = point_case(shape)
    U, Hq = cs["post"][0]
    D = cs["D"]
    beta, Gam = mr.posterior_terms(cs["L"], U, Hq, mode)
    Q = np.full(D, 1e-300)
    fn = orc.conditional_after_kernel_precalculation
    if mode == "reference":
        om, ov = fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=Hq, white=True)
    else:
        outs = [fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=Hq[d:d + 1], white=True) for d in range(D)]
        om, ov = outs[0][0], np.stack([outs[d][1][:, d] for d in range(D)], axis=1)
    for n in (1, 3, 10):                                          # the track from origin n - 1 reads control row n
        mu, ctrl = cs["Xnew"][n, :D], cs["Xnew"][:, D:]
        f = dict(m_filt=np.broadcast_to(mu, (n, D)), S_filt=np.zeros((n, D, D)))
        m, S = fcr.tracks(f, [n - 1], 1, 1, np.ones((D, 1)), np.zeros(1), np.ones(1), Q, ctrl, cs["Z"], cs["kern"], beta, Gam)
        em, ev = float(np.max(np.abs(m[0, 0] - mu - om[n]))), float(np.max(np.abs(np.diag(S[0, 0]) - ov[n])))
        off = float(np.max(np.abs(S[0, 0] - np.diag(np.diag(S[0, 0])))))
        print(f"{shape} {mode} row {n}: mean {em:.3e} (floor {floor('mean', om):.3e}), var {ev:.3e}, off-diagonal {off:.3e} "
              f"(floor {floor('var', ov):.3e})")
        assert em <= floor("mean", om) and ev <= floor("var", ov) and off <= floor("var", ov)


# ---- 4. the reference's own S_fc is positive definite on every fixture of the GPU tests -----------------------------------------------
def _positive(what, ref):
    assert np.all(np.isfinite(ref["m"])) and np.all(np.isfinite(ref["S"]))
    np.testing.assert_array_equal(ref["S"], np.swapaxes(ref["S"], -1, -2))
    low = float(np.min(np.linalg.eigvalsh(ref["S"])))
    print(f"{what}: smallest eigenvalue of the reference's S_fc {low:.3e}, max|m_fc| {float(np.max(np.abs(ref['m']))):.3e}")
    assert low > 0.0


@pytest.mark.parametrize("args", CASES, ids=str)
def test_the_reference_is_positive_definite_on_the_shared_cases(args):
    ref, _ = shared_reference(args, False)
    cs = cpu_case(*args[:3])
    assert ref["m"].shape == (len(cs[0]), len(ORIGINS), H, cs[2]["D"])
    _positive(f"{args}", ref)


def test_the_reference_is_positive_definite_on_the_tile_edge_fixtures():
    r = m300_record()
    assert r["meta"]["M"] == 300 and len(r["origins"]) == 4
    _positive("M = 300", record_reference(r, False)[0])
    r = d3_record()
    assert (r["meta"]["M"], r["meta"]["D"], r["meta"]["C"]) == (77, 3, 2) and r["Y"].shape[0] == 26 and len(r["origins"]) == 24
    for slices in (True, False):
        ref, _ = record_reference(r, False, slices)
        assert ref["m"].shape == (2, 24, 2, 3)
        _positive(f"D = 3, 24 origins, q slices {slices}", ref)
    r = flr.long_record()
    ref, _ = record_reference(r, False)
    assert ref["m"].shape == (2, 138, 2, 2)
    _positive("140-row record", ref)
