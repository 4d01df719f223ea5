"""Moment-matched prediction on the device: `ffvd_op_moment_grouped` (prediction.moment_grouped), fused with the collapsed posteriors
(`ffvd_op_posterior_moment_grouped`, prediction.posterior_moment_grouped), the summaries and DGPSSM.predict_moments /
evaluate_heldout(method="moment") / fit(eval_method="moment").

Reference and rule.  The reference is tests/moment_ref.py, the NumPy fp64 restatement of DESIGN.md section 9 (pinned against
Gauss-Hermite quadrature of the oracle's conditional in tests/test_moment_ref.py).  Its own error e_ref is measured against the same
restatement run in np.longdouble, never on the device; the device must satisfy, per array,  error <= max(4 e_ref, floor)  with the
floors of tests/test_gpu_conditional_grouped.py (1e-11 + 1e-9 max|ref| on means, 1e-11 + 1e-8 max|ref| on variances and covariances).
Where np.longdouble is no wider than 1e-18 the floor alone is used (printed).  Every measured error is printed.

Shapes: tiny (M = 24, D = 2, C = 1), ragged (M = 77, D = 3, C = 2), small (M = 96, D = 4, C = 1), M = 130 past one 128 tile with D = 1
and no control input, and D = 8 at M = 40: padding, slab edges (M not a multiple of 16), pair indexing and the D x D elimination.
These have D = 2, 3, 4, 1 and 8, P <= 9 and J <= 3; D = 5, 6 and 7, J = 8 and P up to 32 run in tests/test_gpu_widths.py."""
import functools

import numpy as np
import pytest

import moment_ref as mr
from ffvd_amd import prediction as pr, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from oracle import ffvd_oracle as orc
from test_gpu_conditional_grouped import _group, floor

pytestmark = pytest.mark.gpu

SHAPES = {"tiny": ("tiny", {}), "ragged": ("ragged", {}), "small": ("small", dict(S=3)), "m130": ("tiny", dict(M=130, D=1, C=0, T=160)),
          "d8": ("tiny", dict(M=40, D=8, C=1))}
STEPS = 12
WIDE = np.finfo(np.longdouble).eps < 1e-18
MODES = ("reference", "intent")


def rule(what, key, dev, ref, e_ref):
    """device error <= max(4 x the reference's own error, the project's floor for this array)"""
    e_dev, fl = float(np.max(np.abs(np.asarray(dev) - ref))), floor(key, ref)
    bound = max(4.0 * e_ref, fl) if WIDE else fl
    print(f"{what}: {key}: device {e_dev:.3e}, e_ref {e_ref:.3e}{'' if WIDE else ' (longdouble is not wider: floor alone)'}, "
          f"floor {fl:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(dev)), f"{what}: {key}"
    assert e_dev <= bound, f"{what}: {key}: {e_dev:.3e} > max(4 x {e_ref:.3e}, {fl:.3e})"


@functools.lru_cache(maxsize=None)
def case(shape, per_model=False, G=None):
    """Shared model: the workload's own S chains.  One model per group: seeded perturbations of the hyper-parameters, Z, Q and X
    (those of tests/test_gpu_conditional_grouped.py).  Plus STEPS seeded control rows for the propagation, after the T rows of the
    posterior."""
    name, ov = SHAPES[shape]
    if G is not None:
        ov = dict(ov, S=G)
    params, Y, c, meta = synthetic.make_named(name, **ov)
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
        gs.append(_group(q, c, meta, X))
    call = np.concatenate((c, np.random.default_rng(3).standard_normal((STEPS, meta["C"]))), axis=0)
    return gs, call, meta, per_model, params


def start_cov(G, D, seed=5):
    """random SPD start covariances, scale 0.05 .. 0.5, exactly symmetric"""
    rng = np.random.default_rng(seed)
    out = np.empty((G, D, D))
    for g in range(G):
        A = rng.standard_normal((D, D))
        S = (0.05 + 0.45 * rng.random()) * (A @ A.T / D + 0.1 * np.eye(D))
        out[g] = np.triu(S) + np.triu(S, 1).T
    return out


def _dense(gs, meta):
    rng = np.random.default_rng(21)
    return [g["orc"]["H"] + 0.01 * np.tril(rng.standard_normal((meta["D"], meta["M"], meta["M"])), -1) for g in gs]


def _q(cs, qkind, src="orc"):
    gs, meta = cs[0], cs[2]
    return None if qkind == "none" else _dense(gs, meta) if qkind == "dense" else [g[src]["H"] for g in gs]


@functools.lru_cache(maxsize=None)
def refs(shape, per_model, G, qkind, mode, steps, with_S0):
    """Per group: the restatement's m_x / S_x in fp64 (`ref`) and its error against np.longdouble (`e_ref`), on the oracle's
    posterior.  Computed once per case, shared by the tests, never modified."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    qs, S0 = _q(cs, qkind), start_cov(len(gs), meta["D"]) if with_S0 else np.zeros((len(gs), meta["D"], meta["D"]))
    ctrl = call[meta["T"]: meta["T"] + steps]
    out = dict(m=[], S=[], e_m=0.0, e_S=0.0)
    for i, g in enumerate(gs):
        res = {}
        for t in (np.float64, np.longdouble) if WIDE else (np.float64,):
            beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
            res[t] = mr.propagate(g["X"][-1], S0[i], ctrl, g["Z"], g["okern"], beta, Gam, g["Q"], steps, dtype=t)
        out["m"].append(res[np.float64][0])
        out["S"].append(res[np.float64][1])
        if WIDE:
            out["e_m"] = max(out["e_m"], float(np.max(np.abs(res[np.float64][0] - res[np.longdouble][0]))))
            out["e_S"] = max(out["e_S"], float(np.max(np.abs(res[np.float64][1] - res[np.longdouble][1]))))
    out["m"], out["S"] = np.stack(out["m"]), np.stack(out["S"])
    return out


def run_explicit(cs, qkind, mode, steps, S0=None, src="orc", groups=None):
    gs, call, meta, per_model = cs[0], cs[1], cs[2], cs[3]
    idx = list(range(len(gs))) if groups is None else groups
    sel, qs = [gs[i] for i in idx], _q(cs, qkind, src)
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in sel], [g["kern"] for g in sel], [g[src]["L"] for g in sel]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    return pr.moment_grouped(Ls, Zs, kerns, [g[src]["U"] for g in sel], None if qs is None else [qs[i] for i in idx],
                             [g["X"][-1] for g in sel], call, meta["T"], steps, [g["Q"] for g in sel],
                             S0s=None if S0 is None else S0[idx], q_mode=mode)


def _fused_args(cs, steps):
    gs, call, meta, per_model = cs[0], cs[1], cs[2], cs[3]
    Zs, kerns = ([g["Z"] for g in gs], [g["kern"] for g in gs]) if per_model else (gs[0]["Z"], gs[0]["kern"])
    return Zs, kerns, [g["X"] for g in gs], [g["Q"] for g in gs], call, meta["T"], steps


def check(what, r, m_x, S_x):
    assert m_x.shape == r["m"].shape and S_x.shape == r["S"].shape
    rule(what, "mean", m_x, r["m"], r["e_m"])
    rule(what, "var", S_x, r["S"], r["e_S"])
    np.testing.assert_array_equal(S_x, np.swapaxes(S_x, -1, -2))


# ---- 1. one step from zero covariance: the existing conditional ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_step_from_a_point_is_the_conditional(shape):
    """Sigma = 0: m_x - x_last = f_mu and diag(S_x) - Q = f_var of the oracle's conditional at [x_last, c]; the yardstick is
    conditional_grouped on the same inputs; the off-diagonal of S_x is a covariance of independent GPs at a point: zero.

    Measured on one MI355X: the closest case is small, var 1.9e-13 against 4.1e-10.  m130 (130 inducing points on a line: K_uu at
    the jitter's condition number) is what decided how Gamma is formed: as W W^T - (W q)(W q)^T, a difference of products with
    entries near 1e5, its variance missed this bound (2.1e-11 / 5.5e-11 against 3.5e-11 / 3.1e-11); as (W E) W^T with
    E = (N + N^T) - N N^T, N = I - q, it is at 4.1e-15 / 6.2e-15 / 1.7e-15."""
    cs = case(shape)
    gs, call, meta = cs[0], cs[1], cs[2]
    T, D = meta["T"], meta["D"]
    m_x, S_x = run_explicit(cs, "upper", "reference", 1)
    assert m_x.shape == (len(gs), 1, D) and S_x.shape == (len(gs), 1, D, D)
    for i, g in enumerate(gs):
        xc = np.concatenate((g["X"][-1], call[T]))[None, :]
        fm, fv = orc.conditional_after_kernel_precalculation(g["orc"]["L"], xc, g["Z"], g["okern"], g["orc"]["U"], q_sqrt=g["orc"]["H"],
                                                             white=True)
        dm, dv, _, _ = cmo.conditional_grouped(g["orc"]["L"], g["Z"], g["kern"], [g["orc"]["U"]], [g["orc"]["H"]], xc)
        got_m, got_v = m_x[i, 0] - g["X"][-1], np.diag(S_x[i, 0]) - g["Q"]
        for key, got, dev, ref in (("mean", got_m, dm[0, 0], fm[0]), ("var", got_v, dv[0, 0], fv[0])):
            e_new, e_cond = float(np.max(np.abs(got - ref))), float(np.max(np.abs(dev - ref)))
            bound = max(4.0 * e_cond, floor(key, ref))
            print(f"{shape} group {i}: {key}: moment step {e_new:.3e}, conditional_grouped {e_cond:.3e}, bound {bound:.3e}")
            assert e_new <= bound
        off = S_x[i, 0] - np.diag(np.diag(S_x[i, 0]))
        print(f"{shape} group {i}: largest off-diagonal entry {np.max(np.abs(off)):.3e}")
        assert np.max(np.abs(off)) <= floor("var", fv[0])


# ---- 2. one step from a non-zero start covariance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("qkind", ["none", "upper", "dense"])
@pytest.mark.parametrize("shape,per_model,G", [("tiny", False, 1), ("tiny", False, 3), ("tiny", True, 3), ("ragged", False, None),
                                               ("small", True, 3), ("m130", False, 3), ("d8", False, 1)], ids=str)
def test_one_step_from_a_start_covariance(shape, per_model, G, qkind, mode):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, qkind, mode, 1, True)
    S0 = start_cov(len(cs[0]), cs[2]["D"])
    m_x, S_x = run_explicit(cs, qkind, mode, 1, S0)
    check(f"{shape} per_model={per_model} G={G} q={qkind} {mode}: one step", r, m_x, S_x)


def test_the_two_q_modes_differ_on_dim_1():
    """dim 0 takes slice 0 in both modes; dim 1 takes slice 1 under "intent": its variance differs, the means of one step do not"""
    cs, S0 = case("tiny"), start_cov(3, 2)
    (ma, Sa), (mb, Sb) = run_explicit(cs, "upper", "reference", 1, S0), run_explicit(cs, "upper", "intent", 1, S0)
    np.testing.assert_array_equal(ma, mb)
    np.testing.assert_array_equal(Sa[:, :, 0, 0], Sb[:, :, 0, 0])
    assert np.max(np.abs(Sa[:, :, 1, 1] - Sb[:, :, 1, 1])) > 1e-4


# ---- 3. twelve steps with controls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode", [("tiny", False, None, "upper", "reference"), ("ragged", False, None, "upper", "intent"),
                                                          ("small", True, 3, "upper", "reference"), ("m130", False, 3, "none", "reference"),
                                                          ("d8", False, 1, "dense", "reference")], ids=str)
def test_twelve_steps(shape, per_model, G, qkind, mode):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, qkind, mode, STEPS, False)
    m_x, S_x = run_explicit(cs, qkind, mode, STEPS)
    check(f"{shape} q={qkind} {mode}: {STEPS} steps", r, m_x, S_x)
    low = float(np.min(np.linalg.eigvalsh(S_x)))
    print(f"{shape}: smallest eigenvalue of S_x {low:.3e}")
    assert low >= -floor("var", r["S"])


def test_no_steps_returns_empty_arrays():
    cs = case("tiny")
    m_x, S_x = run_explicit(cs, "upper", "reference", 0)
    assert m_x.shape == (3, 0, 2) and S_x.shape == (3, 0, 2, 2)
    m_x, S_x = pr.posterior_moment_grouped(*_fused_args(cs, 0))
    assert m_x.shape == (3, 0, 2) and S_x.shape == (3, 0, 2, 2)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,qkind", [("tiny", True, "upper"), ("ragged", False, "dense"), ("small", False, "none")], ids=str)
def test_two_calls_are_equal_and_a_group_alone_equals_the_group_among_the_others(shape, per_model, qkind):
    cs = case(shape, per_model, 3)
    S0 = start_cov(3, cs[2]["D"])
    for mode in MODES:
        a, b = run_explicit(cs, qkind, mode, 5, S0), run_explicit(cs, qkind, mode, 5, S0)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        for g in range(3):
            m1, S1 = run_explicit(cs, qkind, mode, 5, S0, groups=[g])
            np.testing.assert_array_equal(m1[0], a[0][g])
            np.testing.assert_array_equal(S1[0], a[1][g])


# ---- 5. fused with the posteriors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G", [("tiny", False, None), ("ragged", False, None), ("small", True, 3), ("m130", False, 3)], ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, mode):
    """posterior_moment_grouped against collapse_u_mean_grouped followed by moment_grouped.  The two routes do not hand the step
    kernel the same bits by construction (the fused packing writes exact zeros below the diagonal of L^-T and L_H^-T, the explicit
    route takes the downloaded matrices as they are), so the tolerance rule applies: the reference is the restatement on the
    device's own posterior -- in np.longdouble where that is wider -- and the yardstick is the two-call route on the same posterior.
    Whether the bits do coincide is printed."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    args = _fused_args(cs, 5)
    m_f, S_f, U_f = pr.posterior_moment_grouped(*args, q_mode=mode, return_U=True)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(*args[:3], call, args[3])
    np.testing.assert_array_equal(U_f, U)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    m_e, S_e = pr.moment_grouped(Ls, args[0], args[1], list(U), list(Hinv), [g["X"][-1] for g in gs], call, meta["T"], 5, args[3], q_mode=mode)
    print(f"{shape} {mode}: fused and two-call routes bit-identical: {np.array_equal(m_f, m_e) and np.array_equal(S_f, S_e)}")
    t = np.longdouble if WIDE else np.float64
    ctrl = call[meta["T"]: meta["T"] + 5]
    for i, g in enumerate(gs):
        beta, Gam = mr.posterior_terms(Lm[i if per_model else 0], U[i], Hinv[i], mode, dtype=t)
        rm, rS = mr.propagate(g["X"][-1], np.zeros((meta["D"],) * 2), ctrl, g["Z"], g["okern"], beta, Gam, g["Q"], 5, dtype=t)
        rm, rS = rm.astype(np.float64), rS.astype(np.float64)
        for key, f, e, ref in (("mean", m_f[i], m_e[i], rm), ("var", S_f[i], S_e[i], rS)):
            e_f, e_e = float(np.max(np.abs(f - ref))), float(np.max(np.abs(e - ref)))
            bound = max(4.0 * e_e, floor(key, ref))
            print(f"{shape} {mode} group {i}: {key}: fused {e_f:.3e}, two calls {e_e:.3e}, bound {bound:.3e}")
            assert e_f <= bound
    np.testing.assert_array_equal(S_f, np.swapaxes(S_f, -1, -2))
    again = pr.posterior_moment_grouped(*args, q_mode=mode)
    np.testing.assert_array_equal(again[0], m_f)
    np.testing.assert_array_equal(again[1], S_f)


# ---- 6. summaries --------------------------------------------------------------------------------------------------------------------
SUMMARY_KEYS = ("predict_y", "predict_y_var", "predict_y_var_total", "lpd", "lpd_gauss")


def _check_summary(what, out, m_x, S_x, CC, DD, lr, Y):
    sd = np.exp(lr[0])
    ref = mr.summary(m_x, S_x, CC, DD, sd, Y)
    want = dict(predict_y=ref["y_mean"], predict_y_var=ref["y_var_total"], predict_y_var_total=ref["y_var_total"], lpd=ref["lpd"],
                lpd_gauss=ref["lpd_gauss"])
    assert set(out) == set(SUMMARY_KEYS) | {"RMSE", "ll", "ll_original_units"}
    m = np.einsum("gtk,kj->gtj", m_x, CC) + DD
    scale = dict(predict_y=np.max(np.abs(want["predict_y"])), predict_y_var=np.max(np.mean(m * m, axis=0) + want["predict_y_var"]))
    scale["predict_y_var_total"] = scale["predict_y_var"]
    for k in SUMMARY_KEYS:
        got = out[k].reshape(want[k].shape)
        tol = 1e-9 * (1.0 + np.max(np.abs(want[k]))) if k.startswith("lpd") else 1e-11 + 1e-9 * scale[k]
        err = float(np.max(np.abs(got - want[k])))
        print(f"{what}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert np.all(np.isfinite(got)) and err <= tol
    assert out["ll"] == pytest.approx(float(np.mean(want["lpd"])), abs=1e-9 * (1.0 + np.max(np.abs(want["lpd"]))))


@pytest.mark.parametrize("J", [1, 3])
def test_summaries(J):
    cs = case("ragged")
    gs, call, meta = cs[0], cs[1], cs[2]
    D, rng = meta["D"], np.random.default_rng(17)
    CC, DD, lr = rng.standard_normal((D, J)), rng.standard_normal(J), np.log(0.2 + 0.3 * rng.random((J, J)))
    args = _fused_args(cs, STEPS)
    m_x, S_x = pr.posterior_moment_grouped(*args)
    m = np.einsum("gtk,kj->gtj", m_x, CC) + DD
    Y = (m.mean(axis=0) + 0.3 * rng.standard_normal((STEPS, J)))[:9]
    alone = pr.moment_summary(m_x, S_x, CC, DD, lr, Y, 1.7)
    _check_summary(f"J={J}: moment_summary", alone, m_x, S_x, CC, DD, lr, Y)
    fused = pr.posterior_moment_grouped_summary(*args, CC, DD, lr, Y, 1.7, return_moments=True)
    np.testing.assert_array_equal(fused["m_x"], m_x)
    np.testing.assert_array_equal(fused["S_x"], S_x)
    for k in SUMMARY_KEYS:
        np.testing.assert_array_equal(fused[k], alone[k], err_msg=k)
    assert fused["ll"] == alone["ll"] and fused["RMSE"] == alone["RMSE"]
    lean = pr.posterior_moment_grouped_summary(*args, CC, DD, lr, Y, 1.7)
    assert "m_x" not in lean and "S_x" not in lean
    for k in SUMMARY_KEYS:
        np.testing.assert_array_equal(lean[k], alone[k], err_msg=k)
    g0 = gs[0]
    explicit = pr.moment_grouped_summary(g0["orc"]["L"], g0["Z"], g0["kern"], [g["orc"]["U"] for g in gs], [g["orc"]["H"] for g in gs],
                                         [g["X"][-1] for g in gs], call, meta["T"], STEPS, [g["Q"] for g in gs], CC, DD, lr, Y, 1.7,
                                         return_moments=True)
    own = pr.moment_summary(explicit["m_x"], explicit["S_x"], CC, DD, lr, Y, 1.7)
    for k in SUMMARY_KEYS:
        np.testing.assert_array_equal(explicit[k], own[k], err_msg=k)
    # every group at least 40 noise deviations away: every exponent is below -800, an unshifted sum gives -inf
    s2 = np.einsum("kj,gtkl,lj->gtj", CC, S_x, CC) + np.exp(2 * lr[0])
    far = (np.max(m, axis=0) + 40.0 * np.sqrt(np.max(s2, axis=0)))[:9]
    out = pr.moment_summary(m_x, S_x, CC, DD, lr, far)
    assert np.all(np.isfinite(out["lpd"])) and np.all(out["lpd"] < -700)
    _check_summary(f"J={J}: far point", out, m_x, S_x, CC, DD, lr, far)
    no_y = pr.moment_summary(m_x, S_x, CC, DD, lr)
    assert set(no_y) == {"predict_y", "predict_y_var", "predict_y_var_total"}
    np.testing.assert_array_equal(no_y["predict_y"], alone["predict_y"])


# ---- 7. model level: the actuator fixture with three chains --------------------------------------------------------------------------
N_TRAIN, TEST_LEN, S = 400, 40, 3


def _regression_model(params, c, U_collapse=True):
    from ffvd_amd.models import RegressionModel
    m = RegressionModel("normal")
    A = m.ARGS
    A.CC, A.DD = params["CC"], params["DD"]
    A.QQ_chol, A.RR_chol = np.exp(0.5 * params["log_Q"]), np.exp(params["log_Rchols"])
    A.lengthscales, A.variance = np.exp(params["loglengthscales"]), np.exp(params["logvariance"])
    A.UU_ini, A.XX_0_ini, A.x_initialization = params["U"], params["X"][0], params["X"][1:N_TRAIN + 1]
    A.control_inputs, A.num_inducing, A.x_dims, A.ZZ = c, 100, [4], params["Z"]
    A.U_collapse, A.kernel_optimization, A.case_val = U_collapse, True, 4 if U_collapse else 1
    if not U_collapse:
        A.U_optimization, A.Z_optimization = True, True
    return m


def _chains(params):
    X = params["X"][:N_TRAIN + 1]
    return np.stack([X + 0.05 * np.random.default_rng(40 + s).standard_normal(X.shape) * (s > 0) for s in range(S)])


@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_evaluate_heldout_by_moments(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    Yt = Y[N_TRAIN:N_TRAIN + TEST_LEN]
    J = Yt.shape[1]
    ev = mod.evaluate_heldout(Yt, c, 8, Y_train_std=1.7, method="moment")
    assert set(ev) == {"predict_y", "predict_y_var", "predict_y_var_total", "lpd", "lpd_gauss", "ll", "ll_original_units", "RMSE"}
    assert ev["predict_y"].shape == ev["predict_y_var"].shape == ev["predict_y_var_total"].shape == (TEST_LEN * J,)
    assert ev["lpd"].shape == ev["lpd_gauss"].shape == (TEST_LEN, J)
    assert all(np.all(np.isfinite(ev[k])) for k in ev)
    np.testing.assert_array_equal(ev["predict_y_var"], ev["predict_y_var_total"])
    assert np.all(ev["predict_y_var_total"] > np.exp(2 * mod.likelihood.log_Rchols[0, 0]))
    again = mod.evaluate_heldout(Yt, c, 100, Y_train_std=1.7, method="moment", seed=3)      # num_per_chain and seed are ignored
    for k in ev:
        np.testing.assert_array_equal(again[k], ev[k], err_msg=k)
    pm = mod.predict_moments(c, TEST_LEN, Y_test=Yt, Y_train_std=1.7)
    assert pm["m_x"].shape == (S, TEST_LEN, 4) and pm["S_x"].shape == (S, TEST_LEN, 4, 4)
    for k in ev:
        np.testing.assert_array_equal(pm[k], ev[k], err_msg=k)
    _check_summary("model level", ev, pm["m_x"], pm["S_x"], mod.likelihood.CC, mod.likelihood.DD, mod.likelihood.log_Rchols, Yt)
    print(f"U_collapse={U_collapse}: moment method ll {ev['ll']:.6f}, RMSE {ev['RMSE']:.6f}")
    # the default method is what it was: the direct summary call at the same eps
    eps = np.random.default_rng(11).standard_normal((TEST_LEN, S, 8, 4))
    default = mod.evaluate_heldout(Yt, c, 8, Y_train_std=1.7, eps=eps)
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        direct = pr.posterior_rollout_grouped_summary(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, c, N_TRAIN,
                                                      TEST_LEN, eps, lik.CC, lik.DD, lik.log_Rchols, Yt, 1.7)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        direct = pr.rollout_grouped_summary([Lm] * S, [lay.Z] * S, [lay.kernel] * S, [lay.U] * S, None,
                                            [mod._X_chains[s][-1] for s in range(S)], c, N_TRAIN, TEST_LEN, [mod.Q] * S, eps,
                                            lik.CC, lik.DD, lik.log_Rchols, Yt, 1.7)
    assert set(default) == set(direct)
    for k in direct:
        np.testing.assert_array_equal(default[k], direct[k], err_msg=k)


def test_fit_records_held_out_metrics_by_moments(actuator):
    params, Y, c = actuator
    Yt = Y[N_TRAIN:N_TRAIN + TEST_LEN]
    m = _regression_model(params, c)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=2, route="gram", grad=True, num_chains=S, Y_test=Yt, eval_every=1,
          eval_method="moment", Ystd=1.7)
    assert len(m.rmse_seq) == 2 and len(m.ll_seq) == 2 and np.all(np.isfinite(m.rmse_seq)) and np.all(np.isfinite(m.ll_seq))
    ev = m.model.evaluate_heldout(Yt, None, 8, Y_train_std=1.7, method="moment")
    assert ev["ll"] == m.ll_seq[-1] and ev["RMSE"] == m.rmse_seq[-1]                      # deterministic: the last round again
    print("held-out RMSE per round", m.rmse_seq, "log predictive density per round", m.ll_seq)
    with pytest.raises(ValueError, match="eval_method"):
        _regression_model(params, c).fit(Y[:N_TRAIN], iterations=0, eval_method="quadrature")
