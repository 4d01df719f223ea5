"""Cubature (sigma-point) filtering of many records on the device: prediction.filter_cubature_records_grouped
(`ffvd_op_filter_cubature_records_grouped`), fused with the collapsed posteriors (prediction.posterior_filter_cubature_records_grouped,
`ffvd_op_posterior_filter_cubature_records_grouped`) and DGPSSM.filter_records_cubature.

Fixtures.  The seven cases and the R = 3 records of tests/test_gpu_filter_records.py (record 2 is 9 rows long, NaN gaps, smooth=True,
both q_modes), imported.  Three fixtures reach tile edges the shared cases do not: M = 300 (a ragged last column tile of the product, a
second stride of the state kernel); D = 3 with 23 records (6 rows of K per track: the rows of track 21 straddle the 128-row tile); D = 2
with 33 records (132 rows per (group, dim) unit: a second row tile with 4 live rows; 264 rows per dim where the groups share Gamma: a
third with 8).

Reference and rule.  tests/cubature_filter_ref.py (pinned in tests/test_cubature_filter_ref.py): filter_ref.filter with
`ckf_transition` once per (group, record) in fp64 on the oracle's posterior; e_ref is that reference against the same composition in
np.longdouble; the device must satisfy error <= max(4 e_ref, floor) per array with `rule` and the floors of
tests/test_gpu_moment_grouped.py, as tests/test_gpu_filter_records.py.  The pooled arrays and the scalars are compared with NumPy on
the device's own stacks at 1e-9 (1 + max|ref|).  Every measured error is printed; DESIGN.md section 9, "Cubature filtering", has the
largest."""
import functools

import numpy as np
import pytest

import cubature_filter_ref as cf
import forecast_linear_ref as flr
import moment_ref as mr
import records_ref as rr
import transition_grad_ref as tg
from ffvd_amd import prediction as pr, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_conditional_grouped import _group, _kernels
from test_gpu_filter_grouped import CASES, MOMENTS, POOLED, emission
from test_gpu_filter_records import KEYS, LENGTHS, R, SCALARS, TRACK, judge, live_rows, records, symmetric_and_smoothed_last
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, WIDE, _chains, _fused_args, _q, _regression_model, case, rule, start_cov

pytestmark = pytest.mark.gpu

NAN = np.nan


def run(cs, qkind, mode, rec, em, groups=None, recs=None, smooth=True, Y=None, ctrl=None, lengths="own", **kw):
    """tests/test_gpu_filter_records.py's run_records on the cubature call (the oracle's posterior)"""
    gs, per_model = cs[0], cs[3]
    idx, ridx = list(range(len(gs))) if groups is None else groups, list(range(rec["Y"].shape[0])) if recs is None else recs
    sel, qs = [gs[i] for i in idx], _q(cs, qkind)
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in sel], [g["kern"] for g in sel], [g["orc"]["L"] for g in sel]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0]["orc"]["L"]
    Y = rec["Y"][ridx] if Y is None else Y
    ctrl = (None if rec["ctrl"] is None else rec["ctrl"][ridx]) if ctrl is None else ctrl
    return pr.filter_cubature_records_grouped(Ls, Zs, kerns, [g["orc"]["U"] for g in sel], None if qs is None else [qs[i] for i in idx],
                                              rec["x0"][idx][:, ridx], ctrl, Y, [g["Q"] for g in sel], *em,
                                              lengths=rec["lengths"][ridx] if isinstance(lengths, str) else lengths,
                                              S0s=None if rec["S0"] is None else rec["S0"][idx][:, ridx], q_mode=mode, smooth=smooth, **kw)


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case, shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    return run(cs, qkind, mode, records(shape, per_model, G, qkind, mode, J, with_S0), emission(cs, J))


@functools.lru_cache(maxsize=None)
def refs(shape, per_model, G, qkind, mode, J, with_S0):
    """The reference of a case on the oracle's posterior and its own error.  Computed once per case, never modified."""
    cs = case(shape, per_model, G)
    gs, D = cs[0], cs[2]["D"]
    rec = records(shape, per_model, G, qkind, mode, J, with_S0)
    CC, DD, _ = emission(cs, J)
    S0 = np.zeros((len(gs), R, D, D)) if rec["S0"] is None else rec["S0"]
    return cf.reference(gs, rec["ctrl"], rec["Y"], CC, DD, rec["sd"], _q(cs, qkind), rec["x0"], S0, mode, rec["lengths"], WIDE)


def positive_definite(what, out, lengths):
    live = live_rows(lengths, out["S_pred"].shape[2])
    low = {k: float(np.min(np.linalg.eigvalsh(out[k][:, live]))) for k in ("S_pred", "S_filt", "S_smooth")}
    print(f"{what}: smallest eigenvalues {', '.join(f'{k} {v:.3e}' for k, v in low.items())}")
    assert min(low.values()) > 0.0


# ---- accuracy, covariances, pooled arrays and scalars ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Cubature filtering"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, (ref, e_ref), rec = case(shape, per_model, G), device(*args), refs(*args), records(*args)
    what = f"cubature {shape} q={qkind} {mode} J={J}"
    nG, D = len(cs[0]), cs[2]["D"]
    assert set(out) == KEYS and out["m_pred"].shape == (nG, R, STEPS, D) and out["lpd"].shape == (nG, R, STEPS, J)
    judge(what, out, ref, e_ref)
    symmetric_and_smoothed_last(out, LENGTHS)
    positive_definite(what, out, LENGTHS)
    live = live_rows(LENGTHS, STEPS)
    (CC, DD, _), Y, sd = emission(cs, J), rec["Y"], np.asarray(rec["sd"]).reshape(-1)
    want = rr.pooled(out["m_pred"], out["S_pred"], CC, DD, sd, Y)
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


# ---- from a point the first step is the conditional ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [c for c in CASES if not c[6]], ids=str)
def test_first_step_from_a_point_is_the_conditional(shape, per_model, G, qkind, mode, J, with_S0):
    """S0 = None: all 2D points of step 0 coincide.  m_pred[:, :, 0] - x0 and diag(S_pred[:, :, 0]) - Q against conditional_grouped at
    the rows [x0[g, r], c_0 of record r], by the rule and the floors of
    tests/test_gpu_filter_linear.py::test_first_step_from_a_point_is_the_conditional (e_ref: transition_grad_ref.linearize at the same
    rows, fp64 against np.longdouble); `cross` of row 0 is exact zeros; the off-diagonals of S_pred (products of the rounding residues
    m(x_i) - mbar) are below the variance floor."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, rec = case(shape, per_model, G), device(*args), records(*args)
    gs, meta = cs[0], cs[2]
    nG, D, C, qs = len(gs), meta["D"], meta["C"], _q(cs, qkind)
    xc = np.stack([np.concatenate((rec["x0"][g, r], rec["ctrl"][r, 0] if C else np.zeros(0))) for g in range(nG) for r in range(R)])
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g["orc"]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0]["orc"]["L"]
    means, vars_, _, _ = cmo.conditional_grouped(Ls, Zs, kerns, [g["orc"]["U"] for g in gs], qs, xc, q_mode=mode, summary=False)
    own = np.arange(nG * R).reshape(nG, R)
    mean, var = np.stack([means[g, own[g]] for g in range(nG)]), np.stack([vars_[g, own[g]] for g in range(nG)])     # (G, R, D)
    got_m = out["m_pred"][:, :, 0] - rec["x0"]
    got_v = np.diagonal(out["S_pred"][:, :, 0], axis1=-2, axis2=-1) - np.stack([g["Q"] for g in gs])[:, None, :]
    e_m = e_v = 0.0
    if WIDE:
        for i, g in enumerate(gs):
            r = {}
            for t in (np.float64, np.longdouble):
                beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], None if qs is None else qs[i], mode, dtype=t)
                r[t] = tg.linearize(xc[own[i]], g["Z"], g["okern"], beta, Gam, dtype=t)
            e_m = max(e_m, float(np.max(np.abs(r[np.float64][0] - r[np.longdouble][0]))))
            e_v = max(e_v, float(np.max(np.abs(r[np.float64][1] - r[np.longdouble][1]))))
    rule(f"cubature {shape}: first step against conditional_grouped", "mean", got_m, mean, e_m)
    rule(f"cubature {shape}: first step against conditional_grouped", "var", got_v, var, e_v)
    off = float(np.max(np.abs(out["S_pred"][:, :, 0] * (1.0 - np.eye(D)))))
    fl = 1e-11 + 1e-8 * float(np.max(np.abs(var)))
    print(f"cubature {shape}: first step: largest off-diagonal of S_pred {off:.3e}, variance floor {fl:.3e}")
    assert off <= fl
    np.testing.assert_array_equal(out["cross"][:, :, 0], np.zeros((nG, R, D, D)))


# ---- independence: the call, the groups, the records, their order, the pass, the padding -----------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    """CASES[1] and CASES[2] have q slices (unit = (group, dim), rows = the 2D rows of the group's records), CASES[4] one shared model
    without them (unit = dim, rows = those of all tracks of the pass)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a, rec = case(shape, per_model, G), device(*args), records(*args)
    em, nG = emission(cs, J), len(cs[0])
    b = run(cs, qkind, mode, rec, em)                                               # two calls
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = run(cs, qkind, mode, rec, em, groups=[g])
        for k in TRACK:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = run(cs, qkind, mode, rec, em, recs=[r])
        for k in TRACK:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
        for k in POOLED + SCALARS:
            np.testing.assert_array_equal(one[k][0], a[k][r], err_msg=f"{k}, record {r}")
    one = run(cs, qkind, mode, rec, em, groups=[nG - 1], recs=[1])                  # a track alone: G = 1, R = 1
    for k in TRACK:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = run(cs, qkind, mode, rec, em, recs=list(range(R))[::-1])                  # the records reversed
    for k in TRACK:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for k in POOLED + SCALARS:
        np.testing.assert_array_equal(rev[k], a[k][::-1], err_msg=k)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = run(cs, qkind, mode, rec, em, records_per_pass=rpp)
        for k in KEYS:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 cut to its 9 rows, run over 12 rows without `lengths`, and padded to 15 rows with NaN, gives the bits of its
    # first 9 rows in every array, the smoothed ones included
    n, C = LENGTHS[2], cs[2]["C"]
    cut = run(cs, qkind, mode, rec, em, recs=[2], Y=rec["Y"][2:3, :n], ctrl=rec["ctrl"][2:3, :n] if C else None, lengths=None)
    unmasked = run(cs, qkind, mode, rec, em, recs=[2], lengths=None)
    more = run(cs, qkind, mode, rec, em, recs=[2], Y=np.concatenate((rec["Y"][2:3], np.full((1, 3, J), NAN)), axis=1),
               ctrl=np.concatenate((rec["ctrl"][2:3], np.ones((1, 3, C))), axis=1) if C else None, lengths=[n])
    assert cut["m_pred"].shape[2] == n and more["m_pred"].shape[2] == STEPS + 3 and np.all(np.isfinite(unmasked["m_smooth"]))
    for k in TRACK:
        for o, name in ((cut, "cut"), (unmasked, "unmasked"), (more, "padded")):
            np.testing.assert_array_equal(o[k][:, 0, :n], a[k][:, 2, :n], err_msg=f"{k}, {name}")
        assert np.all(np.isnan(more[k][:, 0, n:])), k
    for k in POOLED:
        for o in (cut, unmasked, more):
            np.testing.assert_array_equal(o[k][0, :n], a[k][2, :n], err_msg=k)
    for k in SCALARS:
        for o in (cut, unmasked, more):
            np.testing.assert_array_equal(o[k][0], a[k][2], err_msg=k)
    np.testing.assert_array_equal(unmasked["m_filt"][:, 0, n:], unmasked["m_pred"][:, 0, n:])   # an unobserved step: filtered = predicted


# ---- tile edges the shared cases do not reach ------------------------------------------------------------------------------------------
def test_a_ragged_last_column_tile():
    """M = 300: Mp = 320, three column tiles of the product, the last 64 wide, and a second stride of 256 columns in the state kernel.
    The fixture of tests/test_gpu_filter_records.py::test_a_ragged_last_column_tile."""
    params, _, c, meta = synthetic.make_named("tiny", M=300, T=320, S=2)
    gs = [_group(params, c, meta, params["X"][g]) for g in range(2)]
    D, n = meta["D"], 6
    rng = np.random.default_rng(3)
    ctrl = rng.standard_normal((2, n, meta["C"]))
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    sd = np.exp(np.asarray(lr)[0])
    Y = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(31).standard_normal((2, n, CC.shape[1]))
    Y[0, 2] = NAN
    Y[1, 5] = NAN
    lengths = [n, 5]
    x0 = np.stack([g["X"][-1] for g in gs])[:, None, :] + 0.2 * rng.standard_normal((2, 2, D))
    S0, qs = np.stack([start_cov(2, D, seed=5 + r) for r in range(2)], axis=1), [g["orc"]["H"] for g in gs]
    ref, e_ref = cf.reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, "intent", lengths, WIDE)
    out = pr.filter_cubature_records_grouped(gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], qs, x0, ctrl, Y,
                                             [g["Q"] for g in gs], CC, DD, lr, lengths=lengths, S0s=S0, q_mode="intent", smooth=True)
    judge("cubature M=300", out, ref, e_ref)
    symmetric_and_smoothed_last(out, lengths)
    positive_definite("cubature M=300", out, lengths)


def _short_records(gs, meta, nR, base, seed):
    """nR records of 4 rows around the observations `base` (>= nR + 3 rows): record i is rows i .. i + 3 with seeded control rows and
    starts, one start covariance per group; every fifth record is 3 rows long."""
    n, D, G = 4, meta["D"], len(gs)
    rng = np.random.default_rng(seed)
    Y = np.stack([base[i: i + n] for i in range(nR)])
    lengths = np.where(np.arange(nR) % 5 == 4, 3, n)
    Y[lengths == 3, 3] = NAN
    ctrl = rng.standard_normal((nR, n, meta["C"]))
    x0 = np.stack([g["X"][-1] for g in gs])[:, None, :] + 0.2 * rng.standard_normal((G, nR, D))
    S0 = np.ascontiguousarray(np.broadcast_to(start_cov(G, D)[:, None], (G, nR, D, D)))
    return dict(Y=Y, ctrl=ctrl, x0=x0, S0=S0, lengths=lengths)


def test_a_track_that_straddles_a_row_tile():
    """D = 3 ("ragged": M = 77, C = 2, two chains of one model, q slices, "intent"): a track brings 6 rows of K, which do not divide
    128, and 23 records give every (group, dim) unit 138 rows: rows 126 .. 131 of track 21 lie in two row tiles, the second tile has
    10 live rows.  The same call in passes of 10 records (10, 10, 3: one row tile each) must give the same bits."""
    cs = case("ragged", False, None)
    gs, meta, params = cs[0], cs[2], cs[4]
    CC, DD, lr = params["CC"], params["DD"], params["log_Rchols"]
    sd, qs = np.exp(np.asarray(lr)[0]), [g["orc"]["H"] for g in gs]
    base = np.stack([g["X"][-1] for g in gs]).mean(axis=0) @ CC + DD + 0.3 * np.random.default_rng(37).standard_normal((26, CC.shape[1]))
    base[7] = NAN
    m = _short_records(gs, meta, 23, base, 67)
    ref, e_ref = cf.reference(gs, m["ctrl"], m["Y"], CC, DD, sd, qs, m["x0"], m["S0"], "intent", m["lengths"], WIDE)

    def call(**kw):
        return pr.filter_cubature_records_grouped(gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], qs, m["x0"], m["ctrl"],
                                                  m["Y"], [g["Q"] for g in gs], CC, DD, lr, lengths=m["lengths"], S0s=m["S0"], q_mode="intent",
                                                  smooth=True, **kw)
    out = call()
    assert out["m_pred"].shape == (2, 23, 4, 3)
    judge("cubature D=3, 23 records", out, ref, e_ref)
    symmetric_and_smoothed_last(out, m["lengths"])
    positive_definite("cubature D=3, 23 records", out, m["lengths"])
    passes = call(records_per_pass=10)
    for k in out:
        np.testing.assert_array_equal(passes[k], out[k], err_msg=k)


@pytest.mark.parametrize("slices", [True, False], ids=["q slices", "no q slices"])
def test_a_nearly_empty_last_row_tile(slices):
    """D = 2, 33 records of 4 rows on the model of forecast_linear_ref.long_record() (M = 24, C = 1, two chains, "intent").  With q
    slices a unit is (group, dim) with 132 rows: a second row tile with 4 live rows.  Without them (one model, Gamma per dim) a unit is
    a dim with the 264 rows of all tracks: a third row tile with 8.  Passes of 12 records (12, 12, 9) must give the same bits."""
    r = flr.long_record()
    gs, meta = r["gs"], r["meta"]
    kern, qs = _kernels(r["params"], meta), r["qs"] if slices else None
    m = _short_records(gs, meta, 33, r["Y"], 61)
    ref, e_ref = cf.reference(gs, m["ctrl"], m["Y"], r["CC"], r["DD"], r["sd"], qs, m["x0"], m["S0"], r["mode"], m["lengths"], WIDE)

    def call(**kw):
        return pr.filter_cubature_records_grouped(gs[0]["orc"]["L"], gs[0]["Z"], kern, [g["orc"]["U"] for g in gs], qs, m["x0"], m["ctrl"], m["Y"],
                                                  [g["Q"] for g in gs], r["CC"], r["DD"], r["lr"], lengths=m["lengths"], S0s=m["S0"],
                                                  q_mode=r["mode"], smooth=True, **kw)
    out = call()
    assert out["m_pred"].shape == (2, 33, 4, meta["D"]) and out["ll"].shape == (33,)
    judge(f"cubature 33 records, q slices {slices}", out, ref, e_ref)
    symmetric_and_smoothed_last(out, m["lengths"])
    positive_definite(f"cubature 33 records, q slices {slices}", out, m["lengths"])
    passes = call(records_per_pass=12)
    for k in out:
        np.testing.assert_array_equal(passes[k], out[k], err_msg=k)
    alone = pr.filter_cubature_records_grouped(gs[0]["orc"]["L"], gs[0]["Z"], kern, [gs[1]["orc"]["U"]], None if qs is None else [qs[1]],
                                               m["x0"][1:, 32:], m["ctrl"][32:], m["Y"][32:], [gs[1]["Q"]], r["CC"], r["DD"], r["lr"],
                                               lengths=m["lengths"][32:], S0s=m["S0"][1:, 32:], q_mode=r["mode"], smooth=True)
    for k in TRACK:                                               # the last track (alone in the last row tile) against a G = 1, R = 1 call
        np.testing.assert_array_equal(alone[k][0, 0], out[k][1, 32], err_msg=k)


# ---- fused with the posteriors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_filter_cubature_records_grouped against collapse_u_mean_grouped followed by filter_cubature_records_grouped: the
    same posterior, the same launches, bit for bit in every key; the start left to the call (x0s None) is every chain's last training
    state."""
    mode = "reference"
    cs = case(shape, per_model, G)
    gs, call = cs[0], cs[1]
    rec = records(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])          # (data only: any posterior's will do)
    assert rec["Y"].shape[2] == J
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(lengths=rec["lengths"], S0s=rec["S0"], q_mode=mode, smooth=True)
    fused = pr.posterior_filter_cubature_records_grouped(Zs, kerns, Xs, Qs, call, rec["ctrl"], rec["Y"], CC, DD, lr, x0s=rec["x0"], **kw)
    assert set(fused) == KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_cubature_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), rec["x0"], rec["ctrl"], rec["Y"], Qs, CC, DD, lr, **kw)
    for k in KEYS:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    symmetric_and_smoothed_last(fused, LENGTHS)
    last = np.ascontiguousarray(np.broadcast_to(np.stack([g["X"][-1] for g in gs])[:, None, :], rec["x0"].shape))
    own, given = (pr.posterior_filter_cubature_records_grouped(Zs, kerns, Xs, Qs, call, rec["ctrl"], rec["Y"], CC, DD, lr, x0s=x,
                                                                records_per_pass=2, **kw) for x in (None, last))
    for k in KEYS:
        np.testing.assert_array_equal(own[k], given[k], err_msg=k)
    assert float(np.max(np.abs(own["m_filt"][:, 1, 1] - fused["m_filt"][:, 1, 1]))) > 0.0


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_records_cubature_of_the_model(actuator, U_collapse):
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
    kw = dict(lengths=lengths, smooth=True, Y_train_std=1.7)
    out = mod.filter_records_cubature(Yr, cr, **kw)
    assert set(out) == KEYS and out["m_filt"].shape == (S, R, n, D) and out["predict_y"].shape == (R, n, J) and out["ll"].shape == (R,)
    live = live_rows(lengths, n)
    assert all(np.all(np.isfinite(out[k][:, live])) and np.all(np.isnan(out[k][:, ~live])) for k in MOMENTS)
    assert np.all(np.isfinite(out["ll"])) and np.isfinite(out["ll_all"]) and np.all(out["ll_original_units"] == out["ll"] - np.log(1.7))
    lay, lik = mod.layers[-1], mod.likelihood
    if U_collapse:
        direct = pr.posterior_filter_cubature_records_grouped(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, mod.control_inputs,
                                                              cr, Yr, lik.CC, lik.DD, lik.log_Rchols, **kw)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        x0 = np.broadcast_to(np.stack([mod._X_chains[s][-1] for s in range(S)])[:, None, :], (S, R, D))
        direct = pr.filter_cubature_records_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, x0, cr, Yr, mod.Q, lik.CC, lik.DD, lik.log_Rchols,
                                                    **kw)
    for k in KEYS:
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
    single = mod.filter_records_cubature(Yr[:1], cr[:1], smooth=True, Y_train_std=1.7)        # R = 1: a valid single-record call
    for k in TRACK:
        np.testing.assert_array_equal(single[k][:, 0], out[k][:, 0], err_msg=k)
    # the three rules on record 0 (printed, not asserted): the latent states against moment matching's
    ci = np.concatenate((c[:N_TRAIN], cr[0]))
    mom, lin = mod.filter_heldout(Yr[0], ci, smooth=True, Y_train_std=1.7), mod.filter_records(Yr, cr, **kw)
    dc, dl = (float(np.max(np.abs(o["m_filt"][:, 0] - mom["m_filt"]))) for o in (out, lin))
    print(f"U_collapse={U_collapse}: record 0: max|m_filt - m_filt(moment)| cubature {dc:.3e}, linearised {dl:.3e}; ll cubature "
          f"{out['ll'][0]:.6f}, linearised {lin['ll'][0]:.6f}, moment {mom['ll']:.6f}")
    np.testing.assert_array_equal(out["S_pred"], np.swapaxes(out["S_pred"], -1, -2))
