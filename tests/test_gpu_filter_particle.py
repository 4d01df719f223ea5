"""Particle filtering of many records on the device: prediction.filter_particle_records_grouped
(`ffvd_op_filter_particle_records_grouped`), fused with the collapsed posteriors (prediction.posterior_filter_particle_records_grouped,
`ffvd_op_posterior_filter_particle_records_grouped`) and DGPSSM.filter_records_particle.

Fixtures (tests/particle_fixtures.py).  The seven cases and the R = 3 records of tests/test_gpu_filter_records.py (record 2 is 9 rows
long, NaN gaps) with N = 48 particles: not a multiple of 64, and 144 rows per (group, dim) unit, so that track 2 straddles the 128-row
tile; among them D = 8 ("d8") and the shared-Gamma layout (CASES[4], CASES[6]: one model, no q slices, all tracks of a pass in one
unit).  Three more reach tile edges: M = 300 (a ragged last column tile), N = 130 with one record (two row tiles, the second with 2
live rows), N = 700 (several particles per thread in the scan and the gather).

Reference and rule.  tests/particle_filter_ref.py (pinned in tests/test_particle_filter_ref.py) in fp64 on the oracle's posterior;
e_ref is that reference against the same composition in np.longdouble.  The ancestors must be IDENTICAL: every fixture satisfies the
margin condition (the two precisions draw the same ancestors, and no threshold (unif + i) / N lies within max(1e-8, 1000 x the cdf
drift between the precisions) of a cdf entry), checked here because the fixtures are built on the device's posterior path.  Particles,
moments and densities: error <= max(4 e_ref, floor) with `rule` and `judge` of tests/test_gpu_filter_records.py; ess / N takes the
variance floor.  log_evidence, the pooled arrays and the scalars are compared with NumPy on the device's own stacks at
1e-9 (1 + max|ref|).  Every measured error is printed; DESIGN.md section 9, "Particle filtering", has the largest."""
import functools

import numpy as np
import pytest

import moment_ref as mr
import particle_filter_ref as pf
import particle_fixtures as fxt
import records_ref as rr
import transition_grad_ref as tg
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_filter_grouped import CASES, POOLED, emission
from test_gpu_filter_records import LENGTHS, R, SCALARS, judge, live_rows, records
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, WIDE, _chains, _fused_args, _regression_model, case, rule

pytestmark = pytest.mark.gpu

NAN = np.nan
N = fxt.N
MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt")
TRACK = MOMENTS + ("lpd", "lpd_joint", "ess", "log_evidence")
DRAWN = ("particles", "ancestors")
KEYS = set(TRACK) | set(POOLED) | set(SCALARS) | {"ll_all"}
JUDGED = MOMENTS + ("lpd", "lpd_joint", "particles")


@functools.lru_cache(maxsize=None)
def device(name):
    """One device call per fixture (a case of CASES or a key of fxt.EDGES), shared by the checks below (never modified)."""
    return fxt.call(fxt.case_fixture(*name) if isinstance(name, tuple) else fxt.EDGES[name]())


def against_the_reference(what, out, name):
    """identical ancestors; particles, moments and densities by the rule; ess / N by the variance floor; NaN where the reference has it"""
    ref, e_ref, _ = fxt.reference(name)
    n = ref["particles"].shape[3]
    assert out["ancestors"].dtype == np.int32
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judge(what, out, ref, e_ref, keys=JUDGED)
    np.testing.assert_array_equal(np.isnan(out["ess"]), np.isnan(ref["ess"]))
    ok = ~np.isnan(ref["ess"])
    rule(f"{what}: ess / N", "var", out["ess"][ok] / n, ref["ess"][ok] / n, e_ref["ess"] / n)
    for k in ("S_pred", "S_filt"):
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)
    le = np.nansum(out["lpd_joint"], axis=2)
    err, tol = float(np.max(np.abs(out["log_evidence"] - le))), 1e-9 * (1.0 + float(np.max(np.abs(le))))
    print(f"{what}: log_evidence {np.round(out['log_evidence'], 4).tolist()}: max error {err:.3e}, tolerance {tol:.3e}")
    assert out["log_evidence"].shape == le.shape and err <= tol


# ---- the condition the identical ancestors rest on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + sorted(fxt.EDGES), ids=str)
def test_the_ancestors_of_every_fixture_do_not_hang_on_rounding(name):
    """The fp64 and the np.longdouble reference draw identical ancestors, and the smallest distance of any threshold (unif + i) / N to
    any cdf_k / tot is at least max(1e-8, 1000 x the largest |cdf / tot| difference between the two precisions).  A fixture that
    misses this gets another seed (tests/particle_fixtures.py), never another bound."""
    fx = fxt.case_fixture(*name) if isinstance(name, tuple) else fxt.EDGES[name]()
    ref, _, wide = fxt.reference(name)
    gap, drift, same = pf.margin(ref, fx["unif"], wide)
    print(f"{name}: smallest gap {gap:.3e}, cdf drift between the precisions {drift:.3e}, identical ancestors {same}")
    assert same
    assert gap >= max(1e-8, 1000.0 * drift)


# ---- accuracy, covariances, pooled arrays and scalars ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Particle filtering"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, rec = case(shape, per_model, G), device(args), records(*args)
    what = f"particle {shape} q={qkind} {mode} J={J}"
    nG, D = len(cs[0]), cs[2]["D"]
    assert set(out) == KEYS | set(DRAWN)
    assert out["m_pred"].shape == (nG, R, STEPS, D) and out["lpd"].shape == (nG, R, STEPS, J) and out["ess"].shape == (nG, R, STEPS)
    assert out["particles"].shape == (nG, R, STEPS, N, D) and out["ancestors"].shape == (nG, R, STEPS, N)
    against_the_reference(what, out, args)
    live = live_rows(LENGTHS, STEPS)
    assert np.all(out["ancestors"][:, ~live] == -1) and np.all(np.isnan(out["particles"][:, ~live]))
    e = out["ess"][:, live]
    assert np.all(e >= 1.0 - 1e-12) and np.all(e <= N * (1.0 + 1e-12))
    # pooled arrays and scalars against NumPy on the device's own stacks
    (CC, DD, _), Y, sd = emission(cs, J), rec["Y"], np.asarray(rec["sd"]).reshape(-1)
    want = rr.pooled(out["m_pred"], out["S_pred"], CC, DD, sd, Y)
    lp = out["lpd"]
    with np.errstate(invalid="ignore"):
        mx = np.max(lp, axis=0)
        want["lpd_mix"] = mx + np.log(np.mean(np.exp(lp - mx[None]), axis=0))
    dead = np.broadcast_to(~live[:, :, None], Y.shape)
    nan_at = dict(predict_y=dead, predict_y_var_total=dead, lpd_mix=np.isnan(Y), lpd_gauss=np.isnan(Y))
    for k in POOLED:
        got, w = out[k], want[k]
        assert got.shape == (R, STEPS, J), k
        np.testing.assert_array_equal(np.isnan(got), nan_at[k], err_msg=k)
        ok = ~nan_at[k]
        tol, err = 1e-9 * (1.0 + float(np.max(np.abs(w[ok])))), float(np.max(np.abs(got[ok] - w[ok])))
        print(f"{what}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k
    ws = rr.scalars(Y, out["lpd_mix"], out["lpd_joint"], out["predict_y"])
    for k in SCALARS + ("ll_all",):
        w, got = np.asarray(ws[k]), np.asarray(out[k])
        assert got.shape == w.shape == (() if k == "ll_all" else (R,)) and np.all(np.isfinite(got)), k
        err, tol = float(np.max(np.abs(got - w))), 1e-9 * (1.0 + float(np.max(np.abs(w))))
        print(f"{what}: {k}: {np.round(got, 6).tolist()}, max error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, k


# ---- tile edges the shared cases do not reach ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fxt.EDGES))
def test_tile_edges(name):
    """m300: a ragged last column tile of the product and a second stride of the rows kernel; n130: two row tiles per unit, the second
    with 2 live rows, a ragged last slab of the rows kernel; n700: three particles per thread in the scan, three strides in the
    gather, six row tiles.  (D = 8 and the shared-Gamma layout are CASES[5] and CASES[4] / CASES[6] above.)"""
    fx, out = fxt.EDGES[name](), device(name)
    against_the_reference(f"particle {name}", out, name)
    if name == "n130":                                            # a group alone: the same bits from a one-unit-per-dim call
        one = fxt.call(fxt.subset(fx, groups=[1]))
        for k in TRACK + DRAWN:
            np.testing.assert_array_equal(one[k][0], out[k][1], err_msg=k)


# ---- independence: the call, the groups, the records, their order, the pass, the padding, the layout of the draws ---------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    """CASES[1] and CASES[2] have q slices (unit = (group, dim), rows = the N rows of each of the group's records), CASES[4] one shared
    model without them (unit = dim, rows = those of all tracks of the pass)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    fx, a = fxt.case_fixture(*args), device(args)
    nG, every = len(fx["gs"]), TRACK + DRAWN
    b = fxt.call(fx)                                                                # two calls
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = fxt.call(fxt.subset(fx, groups=[g]))
        for k in every:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = fxt.call(fxt.subset(fx, recs=[r]))
        for k in every:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
        for k in POOLED + SCALARS:
            np.testing.assert_array_equal(one[k][0], a[k][r], err_msg=f"{k}, record {r}")
    one = fxt.call(fxt.subset(fx, groups=[nG - 1], recs=[1]))                       # a track alone: G = 1, R = 1
    for k in every:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = fxt.call(fxt.subset(fx, recs=list(range(R))[::-1]))                       # the records reversed, the draws with them
    for k in every:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for k in POOLED + SCALARS:
        np.testing.assert_array_equal(rev[k], a[k][::-1], err_msg=k)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = fxt.call(fx, records_per_pass=rpp)
        for k in a:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 alone, padded from 12 to 15 rows with NaN (draws padded with zeros, uniforms with 0.5)
    n, C, D = LENGTHS[2], 0 if fx["ctrl"] is None else fx["ctrl"].shape[2], fx["x0"].shape[-1]
    two = fxt.subset(fx, recs=[2])
    more = dict(two, Y=np.concatenate((two["Y"], np.full((1, 3, J), NAN)), axis=1),
                ctrl=np.concatenate((two["ctrl"], np.ones((1, 3, C))), axis=1) if C else None,
                eps=np.concatenate((two["eps"], np.zeros((nG, 1, 3, N, D))), axis=2),
                unif=np.concatenate((two["unif"], np.full((nG, 1, 3), 0.5)), axis=2))
    unmasked, padded = fxt.call(two, lengths=None), fxt.call(more)
    assert padded["m_pred"].shape[2] == STEPS + 3
    for k in every:
        if k == "log_evidence":
            np.testing.assert_array_equal(padded[k][:, 0], a[k][:, 2], err_msg=k)
            np.testing.assert_array_equal(unmasked[k][:, 0], a[k][:, 2], err_msg=k)
            continue
        for o, name in ((unmasked, "unmasked"), (padded, "padded")):
            np.testing.assert_array_equal(o[k][:, 0, :n], a[k][:, 2, :n], err_msg=f"{k}, {name}")
        assert np.all(padded[k][:, 0, n:] == -1) if k == "ancestors" else np.all(np.isnan(padded[k][:, 0, n:])), k
    np.testing.assert_array_equal(unmasked["m_filt"][:, 0, n:], unmasked["m_pred"][:, 0, n:])   # an unobserved step: filtered = predicted


@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[4]], ids=str)
def test_shared_draws_are_the_same_draws_broadcast(shape, per_model, G, qkind, mode, J, with_S0):
    """eps (steps, N, D), unif (steps,), xi0 (N, D) and their per-record layouts against the same draws broadcast to the full
    (G, R, ...) layout: bit for bit in every key."""
    fx = fxt.case_fixture(shape, per_model, G, qkind, mode, J, with_S0)
    nG = len(fx["gs"])
    x = lambda v, n: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (nG, R) + v.shape[-n:]))
    for pick in (lambda v: v[0, 0], lambda v: v[0]):                                # shared by all tracks; shared by the groups
        eps, unif, xi0 = pick(fx["eps"]), pick(fx["unif"]), None if fx["xi0"] is None else pick(fx["xi0"])
        small = fxt.call(dict(fx, eps=eps, unif=unif, xi0=xi0))
        full = fxt.call(dict(fx, eps=x(eps, 3), unif=x(unif, 1), xi0=x(xi0, 2)))
        for k in small:
            np.testing.assert_array_equal(small[k], full[k], err_msg=k)
    assert float(np.max(np.abs(small["m_filt"][:, :, 0] - device((shape, per_model, G, qkind, mode, J, with_S0))["m_filt"][:, :, 0]))) > 0.0


# ---- nothing observed: a rollout -------------------------------------------------------------------------------------------------------
def test_with_every_observation_missing_the_particles_are_a_rollout():
    """CASES[0], record 0, all NaN: ancestors are the identity, ess = N, m_filt is m_pred bit for bit, lpd all NaN, log_evidence 0; the
    particles agree with prediction.rollout_grouped fed the same draws (rearranged to (steps, G, N, D)) to 1e-8, README's rollout
    tolerance."""
    fx = fxt.subset(fxt.case_fixture(*CASES[0]), recs=[0])
    gs, nG = fx["gs"], len(fx["gs"])
    out = fxt.call(dict(fx, Y=np.full_like(fx["Y"], NAN)), lengths=None)
    np.testing.assert_array_equal(out["ancestors"], np.broadcast_to(np.arange(N, dtype=np.int32), out["ancestors"].shape))
    np.testing.assert_array_equal(out["ess"], np.full((nG, 1, STEPS), float(N)))
    np.testing.assert_array_equal(out["m_filt"], out["m_pred"])
    np.testing.assert_array_equal(out["S_filt"], out["S_pred"])
    assert np.all(np.isnan(out["lpd"])) and np.all(np.isnan(out["lpd_joint"])) and np.all(np.isnan(out["lpd_mix"]))
    np.testing.assert_array_equal(out["log_evidence"], np.zeros((nG, 1)))
    px, _ = pr.rollout_grouped([g["orc"]["L"] for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs], [g["orc"]["U"] for g in gs],
                               fx["qs"], list(fx["x0"][:, 0]), fx["ctrl"][0], 0, STEPS, [g["Q"] for g in gs],
                               np.ascontiguousarray(np.transpose(fx["eps"][:, 0], (1, 0, 2, 3))))
    err = float(np.max(np.abs(out["particles"][:, 0] - np.transpose(px, (0, 2, 1, 3)))))
    print(f"all observations missing: particles against rollout_grouped {err:.3e}")
    assert err <= 1e-8


# ---- from a point the first step is the conditional ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [c for c in CASES if not c[6]], ids=str)
def test_first_step_from_a_point_is_the_conditional(shape, per_model, G, qkind, mode, J, with_S0):
    """S0 = None: every particle of row 0 starts at x0, so X^-_i - x0 - eps_i sqrt(v + Q) is the conditional mean at [x0[g, r], c_0 of
    record r] for every i, and v its variance: both against conditional_grouped by the rule and the floors of
    tests/test_gpu_filter_cubature.py::test_first_step_from_a_point_is_the_conditional (e_ref: transition_grad_ref.linearize at the
    same rows, fp64 against np.longdouble)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, fx = case(shape, per_model, G), device(args), fxt.case_fixture(*args)
    gs, meta, qs = cs[0], cs[2], fx["qs"]
    nG, C = len(gs), meta["C"]
    xc = np.stack([np.concatenate((fx["x0"][g, r], fx["ctrl"][r, 0] if C else np.zeros(0))) for g in range(nG) for r in range(R)])
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g["orc"]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0]["orc"]["L"]
    means, vars_, _, _ = cmo.conditional_grouped(Ls, Zs, kerns, [g["orc"]["U"] for g in gs], qs, xc, q_mode=mode, summary=False)
    own = np.arange(nG * R).reshape(nG, R)
    mean, var = np.stack([means[g, own[g]] for g in range(nG)]), np.stack([vars_[g, own[g]] for g in range(nG)])     # (G, R, D)
    Q = np.stack([g["Q"] for g in gs])[:, None, :]
    # all particles of row 0 share one (m, v): the device's own sqrt(v + Q) is the slope of X^- against eps, taken between the particles
    # with the largest and the smallest draw of each dim (rounding of X^- over a difference of draws of about 4: ~1e-16); with it the
    # mean is read off every particle, and v itself is compared too.  (Subtracting eps sqrt(v + Q) with conditional_grouped's v instead
    # would multiply that call's own variance error by eps / (2 sqrt(v + Q)) and judge it by the floor of the means.)
    X0, e0 = out["particles"][:, :, 0], fx["eps"][:, :, 0]                                                    # (G, R, N, D)
    hi, lo = np.argmax(e0, axis=2)[:, :, None, :], np.argmin(e0, axis=2)[:, :, None, :]
    pick = lambda a, i: np.take_along_axis(a, i, axis=2)[:, :, 0]
    slope = (pick(X0, hi) - pick(X0, lo)) / (pick(e0, hi) - pick(e0, lo))                                     # (G, R, D)
    got = X0 - fx["x0"][:, :, None, :] - e0 * slope[:, :, None, :]
    got_v = slope * slope - Q
    e_m = e_v = 0.0
    if WIDE:
        for i, g in enumerate(gs):
            r = {}
            for t in (np.float64, np.longdouble):
                beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
                r[t] = tg.linearize(xc[own[i]], g["Z"], g["okern"], beta, Gam, dtype=t)
            e_m = max(e_m, float(np.max(np.abs(r[np.float64][0] - r[np.longdouble][0]))))
            e_v = max(e_v, float(np.max(np.abs(r[np.float64][1] - r[np.longdouble][1]))))
    rule(f"particle {shape}: first step against conditional_grouped", "mean", got, np.broadcast_to(mean[:, :, None, :], got.shape), e_m)
    rule(f"particle {shape}: first step against conditional_grouped", "var", got_v, var, e_v)


# ---- an outlier ------------------------------------------------------------------------------------------------------------------------
def test_an_outlier_forty_deviations_away_keeps_everything_finite():
    """CASES[1] (J = 3, start covariances), row 3 of record 0 moved 40 noise deviations away in every output: the weights are formed
    with the largest exponent subtracted, so everything stays finite, ess >= 1 and the ancestors stay in range."""
    fx = fxt.case_fixture(*CASES[1])
    Y, sd = np.array(fx["Y"]), np.asarray(fx["sd"]).reshape(-1)
    Y[0, 3] = np.nanmean(Y[0], axis=0) + 40.0 * sd
    out = fxt.call(dict(fx, Y=Y))
    live = live_rows(LENGTHS, STEPS)
    for k in MOMENTS + ("ess", "particles"):
        assert np.all(np.isfinite(out[k][:, live])), k
    seen = live & ~np.all(np.isnan(Y), axis=2)
    assert np.all(np.isfinite(out["lpd_joint"][:, seen])) and np.all(np.isnan(out["lpd_joint"][:, ~seen]))
    assert np.all(np.isfinite(out["log_evidence"])) and np.isfinite(out["ll_all"])
    a = out["ancestors"][:, live]
    assert a.min() >= 0 and a.max() <= N - 1 and np.all(out["ess"][:, live] >= 1.0 - 1e-12)
    print(f"outlier: ess of the row {np.round(out['ess'][:, 0, 3], 3).tolist()}, lpd_joint {np.round(out['lpd_joint'][:, 0, 3], 2).tolist()}")


# ---- a particle count whose kernel rows do not fit a pass ------------------------------------------------------------------------------
def test_a_particle_count_whose_rows_do_not_fit_a_pass_is_refused_with_the_largest_that_fits():
    """G = 64 groups with q slices, D = 8, M = 64: 512 (group, dim) units of 65 doubles per row of K and its partials, so the 2^26
    doubles of a pass hold 2016 rows per unit, 1920 in whole 128-row tiles: N = 2048 is refused by the library with that number, before
    the filter's buffers are allocated."""
    from test_filter_records_args import _records
    from test_moment_grouped_args import _explicit
    a = _records(_explicit(G=64, M=64, D=8, C=1), True, R=1, steps=1, G=64, D=8)
    a.update(CC=np.ones((8, 1)), DD=np.zeros(1), log_Rchols=np.zeros((1, 1)), eps=np.zeros((1, 2048, 8)), unif=np.array([0.5]))
    with pytest.raises(ValueError, match="largest N that fits is 1920"):
        pr.filter_particle_records_grouped(**a)


# ---- fused with the posteriors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_filter_particle_records_grouped against collapse_u_mean_grouped followed by filter_particle_records_grouped: the same
    posterior, the same launches, bit for bit in every key; the start left to the call (x0s None) is every chain's last training
    state."""
    args = [a for a in CASES if a[:3] == (shape, per_model, G)][0]
    cs, fx = case(shape, per_model, G), fxt.case_fixture(*args)
    gs, call = cs[0], cs[1]
    CC, DD, lr = fx["em"]
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode="reference", return_particles=True)
    fused = pr.posterior_filter_particle_records_grouped(Zs, kerns, Xs, Qs, call, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                         x0s=fx["x0"], **kw)
    assert set(fused) == KEYS | set(DRAWN)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_particle_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), fx["x0"], fx["ctrl"], fx["Y"], Qs, CC, DD, lr, fx["eps"],
                                             fx["unif"], **kw)
    for k in fused:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    last = np.ascontiguousarray(np.broadcast_to(np.stack([g["X"][-1] for g in gs])[:, None, :], fx["x0"].shape))
    own, given = (pr.posterior_filter_particle_records_grouped(Zs, kerns, Xs, Qs, call, fx["ctrl"], fx["Y"], CC, DD, lr, fx["eps"], fx["unif"],
                                                               x0s=x, records_per_pass=2, **kw) for x in (None, last))
    for k in own:
        np.testing.assert_array_equal(own[k], given[k], err_msg=k)
    assert float(np.max(np.abs(own["m_filt"][:, 1, 1] - fused["m_filt"][:, 1, 1]))) > 0.0


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_records_particle_of_the_model(actuator, U_collapse):
    params, Y, c = actuator
    m = _regression_model(params, c, U_collapse)
    m.fit(Y[:N_TRAIN], kernel_type="SquaredExponential", iterations=0, num_chains=S)
    mod = m.model
    mod.set_X(_chains(params))
    n, D, lengths = 8, 4, [8, 6, 8]
    Yr = np.stack([Y[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    cr = np.stack([c[N_TRAIN + 10 * i: N_TRAIN + 10 * i + n] for i in range(R)])
    Yr[0, 3] = NAN
    Yr[1, 6:] = NAN
    J = Yr.shape[2]
    kw = dict(lengths=lengths, Y_train_std=1.7)
    out = mod.filter_records_particle(Yr, cr, num_particles=128, seed=7, return_particles=True, **kw)
    assert set(out) == KEYS | set(DRAWN)
    assert out["m_filt"].shape == (S, R, n, D) and out["predict_y"].shape == (R, n, J) and out["ll"].shape == (R,)
    assert out["ess"].shape == (S, R, n) and out["log_evidence"].shape == (S, R) and out["particles"].shape == (S, R, n, 128, D)
    live = live_rows(lengths, n)
    assert all(np.all(np.isfinite(out[k][:, live])) and np.all(np.isnan(out[k][:, ~live])) for k in MOMENTS + ("ess",))
    assert np.all(np.isfinite(out["ll"])) and np.isfinite(out["ll_all"]) and np.all(out["ll_original_units"] == out["ll"] - np.log(1.7))
    again = mod.filter_records_particle(Yr, cr, num_particles=128, seed=7, return_particles=True, **kw)       # a seed: the same result
    for k in out:
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    other = mod.filter_records_particle(Yr, cr, num_particles=128, seed=8, **kw)
    assert set(other) == KEYS and float(np.max(np.abs(other["m_filt"][:, live] - out["m_filt"][:, live]))) > 0.0
    per = mod.filter_records_particle(Yr, cr, num_particles=64, seed=3, noise="per_record", S0=0.01 * np.eye(D), **kw)
    ind = mod.filter_records_particle(Yr[:1], cr[:1], num_particles=64, seed=3, noise="independent", Y_train_std=1.7)      # R = 1
    assert np.all(np.isfinite(per["log_evidence"])) and ind["m_filt"].shape == (S, 1, n, D) and np.all(np.isfinite(ind["log_evidence"]))
    big = mod.filter_records_particle(Yr, cr, num_particles=1024, seed=11, **kw)
    gauss = dict(linearised=mod.filter_records(Yr, cr, **kw), cubature=mod.filter_records_cubature(Yr, cr, **kw))
    mom = mod.filter_heldout(Yr[0], np.concatenate((c[:N_TRAIN], cr[0])), Y_train_std=1.7)     # (moment matching: one record at a time)
    print(f"U_collapse={U_collapse}: ll_all particle (N = 1024) {big['ll_all']:.6f}, " +
          ", ".join(f"{k} {v['ll_all']:.6f}" for k, v in gauss.items()) +
          f"; ll of record 0: particle {big['ll'][0]:.6f}, moment {mom['ll']:.6f}, " +
          ", ".join(f"{k} {v['ll'][0]:.6f}" for k, v in gauss.items()) +
          f"; log_evidence of chain 0 {np.round(big['log_evidence'][0], 4).tolist()}; smallest ess {np.min(big['ess'][:, live]):.1f}")
    assert np.isfinite(big["ll_all"]) and np.all(np.isfinite(big["log_evidence"]))
