"""Linearised filtering of many records on the device: prediction.filter_records_grouped (`ffvd_op_filter_records_grouped`), fused
with the collapsed posteriors (prediction.posterior_filter_records_grouped, `ffvd_op_posterior_filter_records_grouped`) and
DGPSSM.filter_records.

Fixtures.  The seven cases, the emissions and the 12-row record with its gaps of tests/test_gpu_filter_grouped.py, imported, with
R = 3 records: record 0 is the case's own (its observations, control rows and start); records 1 and 2 have seeded observations with
gaps of their own, seeded control rows and starts, and record 2 is 9 rows long (`lengths`).  Two fixtures reach tile edges of the
product kernel that the shared cases do not: M = 300 (a ragged last column tile, a second stride of the state kernel) and 130 records
on the model of tests/forecast_linear_ref.long_record() (a second row tile).

Reference and rule.  tests/records_ref.py (pinned in tests/test_records_ref.py): filter_ref.filter with
linear_filter_ref.ekf_transition once per (group, record) in fp64 on the oracle's posterior; e_ref is that reference against the same
composition in np.longdouble; the device must satisfy error <= max(4 e_ref, floor) per array with `rule` and the floors of
tests/test_gpu_moment_grouped.py (1e-11 + 1e-9 max|ref| on means, 1e-11 + 1e-8 max|ref| on covariances; the per-track densities lpd
and lpd_joint are functions of the predicted covariances and take the covariances' floor).  The pooled arrays and the scalars are
compared with NumPy on the device's own stacks at 1e-9 (1 + max|ref|).  Every measured error is printed; DESIGN.md section 9,
"Filtering many records", has the largest."""
import functools

import numpy as np
import pytest

import forecast_linear_ref as flr
import records_ref as rr
from ffvd_amd import prediction as pr, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from test_gpu_conditional_grouped import _group, _kernels, floor
from test_gpu_filter_grouped import CASES, COVS, MOMENTS, POOLED, emission, observations
from test_gpu_moment_grouped import N_TRAIN, S, STEPS, WIDE, _chains, _fused_args, _q, _regression_model, case, rule, start_cov

pytestmark = pytest.mark.gpu

NAN = np.nan
R = 3
LENGTHS = (STEPS, STEPS, 9)
TRACK = MOMENTS + ("lpd", "lpd_joint")
SCALARS = ("ll", "ll_joint", "ll_original_units", "RMSE")
KEYS = set(TRACK) | set(POOLED) | set(SCALARS) | {"ll_all"}


def key_of(k):
    return "mean" if k.startswith("m_") else "var"


def bound(k, ref, e_ref):
    """the rule's bound for an array: max(4 e_ref, floor), the floor alone where np.longdouble is no wider"""
    return max(4.0 * e_ref, floor(key_of(k), ref)) if WIDE else floor(key_of(k), ref)


@functools.lru_cache(maxsize=None)
def records(shape, per_model, G, qkind, mode, J, with_S0):
    """The three records of a case.  Shared, never modified."""
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    nG, D, C, T = len(gs), meta["D"], meta["C"], meta["T"]
    Y0, sd = observations(shape, per_model, G, qkind, mode, J, with_S0)
    rng = np.random.default_rng(53)
    base = np.where(np.isnan(Y0), np.nanmean(Y0, axis=0)[None, :], Y0)
    Y = np.stack([Y0] + [base + 0.3 * np.asarray(sd).reshape(-1)[None, :] * rng.standard_normal(Y0.shape) for _ in range(R - 1)])
    Y[1, 0] = NAN                                                  # a record that starts with a prediction step
    Y[1, 6] = NAN
    Y[2, 4] = NAN
    Y[2, LENGTHS[2]:] = NAN
    if J > 1:
        Y[1, 2, 0] = NAN
        Y[2, 7, 1:] = NAN
    ctrl = np.stack([call[T: T + STEPS]] + [rng.standard_normal((STEPS, C)) for _ in range(R - 1)]) if C else None
    x0 = np.stack([g["X"][-1] for g in gs])[:, None, :] + 0.3 * rng.standard_normal((nG, R, D)) * (np.arange(R) > 0)[None, :, None]
    S0 = np.stack([start_cov(nG, D, seed=5 + r) for r in range(R)], axis=1) if with_S0 else None
    return dict(Y=Y, ctrl=ctrl, x0=x0, S0=S0, sd=sd, lengths=np.array(LENGTHS))


def run_records(cs, qkind, mode, rec, em, groups=None, recs=None, src="orc", smooth=True, Y=None, ctrl=None, lengths="own", **kw):
    gs, per_model = cs[0], cs[3]
    idx, ridx = list(range(len(gs))) if groups is None else groups, list(range(rec["Y"].shape[0])) if recs is None else recs
    sel, qs = [gs[i] for i in idx], _q(cs, qkind, src)
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in sel], [g["kern"] for g in sel], [g[src]["L"] for g in sel]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0][src]["L"]
    Y = rec["Y"][ridx] if Y is None else Y
    ctrl = (None if rec["ctrl"] is None else rec["ctrl"][ridx]) if ctrl is None else ctrl
    return pr.filter_records_grouped(Ls, Zs, kerns, [g[src]["U"] for g in sel], None if qs is None else [qs[i] for i in idx],
                                     rec["x0"][idx][:, ridx], ctrl, Y, [g["Q"] for g in sel], *em,
                                     lengths=rec["lengths"][ridx] if isinstance(lengths, str) else lengths,
                                     S0s=None if rec["S0"] is None else rec["S0"][idx][:, ridx], q_mode=mode, smooth=smooth, **kw)


@functools.lru_cache(maxsize=None)
def device(shape, per_model, G, qkind, mode, J, with_S0):
    """One device call per case, shared by the checks below (never modified)."""
    cs = case(shape, per_model, G)
    return run_records(cs, qkind, mode, records(shape, per_model, G, qkind, mode, J, with_S0), emission(cs, J))


@functools.lru_cache(maxsize=None)
def record_refs(shape, per_model, G, qkind, mode, J, with_S0):
    """The reference of a case on the oracle's posterior and its own error.  Computed once per case, never modified."""
    cs = case(shape, per_model, G)
    gs, D = cs[0], cs[2]["D"]
    rec = records(shape, per_model, G, qkind, mode, J, with_S0)
    CC, DD, _ = emission(cs, J)
    S0 = np.zeros((len(gs), R, D, D)) if rec["S0"] is None else rec["S0"]
    return rr.reference(gs, rec["ctrl"], rec["Y"], CC, DD, rec["sd"], _q(cs, qkind), rec["x0"], S0, mode, rec["lengths"], WIDE)


def judge(what, out, ref, e_ref, keys=TRACK):
    """the rule per array over the entries the reference has; NaN exactly where the reference is NaN"""
    for k in keys:
        assert out[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        rule(f"{what}: {k}", key_of(k), out[k][ok], ref[k][ok], e_ref[k])


def live_rows(lengths, steps):
    return np.arange(steps)[None, :] < np.asarray(lengths)[:, None]


def symmetric_and_smoothed_last(out, lengths):
    for k in COVS:
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)      # (NaN rows compare equal to themselves here)
    for r, n in enumerate(lengths):                                                          # the last row of the smoother is the filtered one
        np.testing.assert_array_equal(out["m_smooth"][:, r, n - 1], out["m_filt"][:, r, n - 1])
        np.testing.assert_array_equal(out["S_smooth"][:, r, n - 1], out["S_filt"][:, r, n - 1])


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_tracks_against_the_reference(shape, per_model, G, qkind, mode, J, with_S0):
    """Measured on one MI355X: see DESIGN.md section 9, "Filtering many records"."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, (ref, e_ref), rec = case(shape, per_model, G), device(*args), record_refs(*args), records(*args)
    what = f"records {shape} q={qkind} {mode} J={J}"
    nG, D = len(cs[0]), cs[2]["D"]
    assert set(out) == KEYS and out["m_pred"].shape == (nG, R, STEPS, D) and out["lpd"].shape == (nG, R, STEPS, J)
    judge(what, out, ref, e_ref)
    symmetric_and_smoothed_last(out, LENGTHS)
    live = live_rows(LENGTHS, STEPS)
    low = float(np.min(np.linalg.eigvalsh(out["S_filt"][:, live])))
    print(f"{what}: smallest eigenvalue of S_filt {low:.3e}")
    assert low > 0.0
    # pooled arrays and scalars against NumPy on the device's own stacks
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


# ---- guarantee 4: against the single-record filter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", CASES, ids=str)
def test_against_the_single_record_filter(shape, per_model, G, qkind, mode, J, with_S0):
    """filter_grouped(method="linearised") record by record: not bit for bit (the quadratic form is summed in column tiles here and in
    16-row slabs there, the mean sums per wavefront here and per slab there); both lie within the rule's bound of one reference, so
    they are within twice that bound of each other."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, out, (ref, e_ref), rec = case(shape, per_model, G), device(*args), record_refs(*args), records(*args)
    gs, em, qs = cs[0], emission(cs, J), _q(cs, qkind)
    if per_model:
        Zs, kerns, Ls = [g["Z"] for g in gs], [g["kern"] for g in gs], [g["orc"]["L"] for g in gs]
    else:
        Zs, kerns, Ls = gs[0]["Z"], gs[0]["kern"], gs[0]["orc"]["L"]
    same = True
    for r, n in enumerate(LENGTHS):
        one = pr.filter_grouped(Ls, Zs, kerns, [g["orc"]["U"] for g in gs], qs, list(rec["x0"][:, r]), None if rec["ctrl"] is None else rec["ctrl"][r][:n],
                                0, rec["Y"][r][:n], [g["Q"] for g in gs], *em, S0s=None if rec["S0"] is None else rec["S0"][:, r], q_mode=mode,
                                smooth=True, method="linearised")
        for k in TRACK:
            a, b, w = out[k][:, r, :n], one[k], ref[k][:, r, :n]
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=k)
            ok = ~np.isnan(w)
            d, bd = float(np.max(np.abs(a[ok] - b[ok]))), 2.0 * bound(k, w[ok], e_ref[k])
            same = same and np.array_equal(a, b, equal_nan=True)
            print(f"records {shape} J={J} record {r}: {k}: against filter_grouped {d:.3e}, 2 x bound {bd:.3e}")
            assert d <= bd, k
    print(f"records {shape} J={J}: bit-identical to filter_grouped(method=\"linearised\"): {same}")


# ---- guarantees 1 - 3: independence, symmetry and the smoother, ragged records ---------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,qkind,mode,J,with_S0", [CASES[1], CASES[2], CASES[4]], ids=str)
def test_a_track_does_not_depend_on_the_call_the_groups_the_records_their_order_the_pass_or_the_padding(shape, per_model, G, qkind, mode, J,
                                                                                                           with_S0):
    """CASES[1] and CASES[2] have q slices (unit = (group, dim), rows = the group's records), CASES[4] one shared model without
    them (unit = dim, rows = all tracks of the pass)."""
    args = (shape, per_model, G, qkind, mode, J, with_S0)
    cs, a, rec = case(shape, per_model, G), device(*args), records(*args)
    em, nG = emission(cs, J), len(cs[0])
    b = run_records(cs, qkind, mode, rec, em)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g in range(nG):                                                             # a group alone
        one = run_records(cs, qkind, mode, rec, em, groups=[g])
        for k in TRACK:
            np.testing.assert_array_equal(one[k][0], a[k][g], err_msg=f"{k}, group {g}")
    for r in range(R):                                                              # a record alone
        one = run_records(cs, qkind, mode, rec, em, recs=[r])
        for k in TRACK:
            np.testing.assert_array_equal(one[k][:, 0], a[k][:, r], err_msg=f"{k}, record {r}")
        for k in POOLED + SCALARS:
            np.testing.assert_array_equal(one[k][0], a[k][r], err_msg=f"{k}, record {r}")
    one = run_records(cs, qkind, mode, rec, em, groups=[nG - 1], recs=[1])         # a track alone: G = 1, R = 1
    for k in TRACK:
        np.testing.assert_array_equal(one[k][0, 0], a[k][nG - 1, 1], err_msg=k)
    rev = run_records(cs, qkind, mode, rec, em, recs=list(range(R))[::-1])          # the records reversed
    for k in TRACK:
        np.testing.assert_array_equal(rev[k], a[k][:, ::-1], err_msg=k)
    for k in POOLED + SCALARS:
        np.testing.assert_array_equal(rev[k], a[k][::-1], err_msg=k)
    assert rev["ll_all"] == pytest.approx(a["ll_all"], rel=1e-13)
    for rpp in (1, 2):                                                              # passes of 1 and of 2 records (a ragged last pass)
        p = run_records(cs, qkind, mode, rec, em, records_per_pass=rpp)
        for k in KEYS:
            np.testing.assert_array_equal(p[k], a[k], err_msg=f"{k}, records_per_pass {rpp}")
    # padding: record 2 cut to its 9 rows, run over 12 rows without `lengths` (the device runs prediction steps, nothing is masked),
    # and padded to 15 rows, gives the bits of its first 9 rows in every array, the smoothed ones included
    n, C = LENGTHS[2], cs[2]["C"]
    cut = run_records(cs, qkind, mode, rec, em, recs=[2], Y=rec["Y"][2:3, :n], ctrl=rec["ctrl"][2:3, :n] if C else None, lengths=None)
    unmasked = run_records(cs, qkind, mode, rec, em, recs=[2], lengths=None)
    more = run_records(cs, qkind, mode, rec, em, recs=[2], Y=np.concatenate((rec["Y"][2:3], np.full((1, 3, J), NAN)), axis=1),
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
    np.testing.assert_array_equal(unmasked["S_smooth"][:, 0, n:], unmasked["S_pred"][:, 0, n:])


# ---- tile edges the shared cases do not reach ------------------------------------------------------------------------------------------
def test_a_ragged_last_column_tile():
    """M = 300: Mp = 320, three column tiles of the product, the last 64 wide, and a second stride of 256 columns in the state kernel.
    The fixture of tests/test_gpu_forecast_linear.py::test_a_ragged_last_column_tile: two chains of one model, q slices, "intent",
    start covariances; R = 2 records of 6 rows, the first with a gap, the second seeded anew and 5 rows long."""
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
    ref, e_ref = rr.reference(gs, ctrl, Y, CC, DD, sd, qs, x0, S0, "intent", lengths, WIDE)
    out = pr.filter_records_grouped(gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], qs, x0, ctrl, Y, [g["Q"] for g in gs],
                                    CC, DD, lr, lengths=lengths, S0s=S0, q_mode="intent", smooth=True)
    judge("records M=300", out, ref, e_ref)
    symmetric_and_smoothed_last(out, lengths)


@functools.lru_cache(maxsize=None)
def many_records():
    """130 records of 4 rows on the model of forecast_linear_ref.long_record() (M = 24, D = 2, C = 1, two chains with q slices,
    "intent"): record i is rows i .. i + 3 of its 140-row record (row 7 is unobserved there) with seeded control rows and starts, one
    start covariance per chain; every fifth record is 3 rows long.  Shared, never modified."""
    r = flr.long_record()
    nR, n, D = 130, 4, r["meta"]["D"]
    rng = np.random.default_rng(61)
    Y = np.stack([r["Y"][i: i + n] for i in range(nR)])
    lengths = np.where(np.arange(nR) % 5 == 4, 3, n)
    Y[lengths == 3, 3] = NAN
    ctrl = rng.standard_normal((nR, n, r["meta"]["C"]))
    x0 = np.stack([g["X"][-1] for g in r["gs"]])[:, None, :] + 0.2 * rng.standard_normal((2, nR, D))
    S0 = np.ascontiguousarray(np.broadcast_to(r["S0"][:, None], (2, nR, D, D)))
    return dict(r=r, Y=Y, ctrl=ctrl, x0=x0, S0=S0, lengths=lengths)


@pytest.mark.parametrize("slices", [True, False], ids=["q slices", "no q slices"])
def test_a_row_tile_boundary(slices):
    """With q slices a unit of the product is (group, dim) and its rows are the group's 130 records: every unit has two row tiles,
    the second with 2 live rows.  Without them (one model, Gamma per dim) a unit is a dim and its rows are all 260 tracks of the pass:
    three row tiles, the last with 4 live rows.  The same call in passes of 50 records (50, 50, 30: one row tile each) must give the
    same bits."""
    m = many_records()
    r = m["r"]
    gs, meta = r["gs"], r["meta"]
    kern, qs = _kernels(r["params"], meta), r["qs"] if slices else None
    ref, e_ref = rr.reference(gs, m["ctrl"], m["Y"], r["CC"], r["DD"], r["sd"], qs, m["x0"], m["S0"], r["mode"], m["lengths"], WIDE)

    def call(**kw):
        return pr.filter_records_grouped(gs[0]["orc"]["L"], gs[0]["Z"], kern, [g["orc"]["U"] for g in gs], qs, m["x0"], m["ctrl"], m["Y"],
                                         [g["Q"] for g in gs], r["CC"], r["DD"], r["lr"], lengths=m["lengths"], S0s=m["S0"], q_mode=r["mode"],
                                         smooth=True, **kw)
    out = call()
    assert out["m_pred"].shape == (2, 130, 4, meta["D"]) and out["ll"].shape == (130,)
    judge(f"130 records, q slices {slices}", out, ref, e_ref)
    symmetric_and_smoothed_last(out, m["lengths"])
    passes = call(records_per_pass=50)
    for k in out:
        np.testing.assert_array_equal(passes[k], out[k], err_msg=k)


# ---- fused with the posteriors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_model,G,J", [("tiny", False, None, 1), ("ragged", False, None, 3), ("small", True, 3, 1), ("m130", False, 3, 1)],
                         ids=str)
def test_fused_form_against_the_two_calls(shape, per_model, G, J):
    """posterior_filter_records_grouped against collapse_u_mean_grouped followed by filter_records_grouped: the same posterior, the
    same launches, bit for bit; the start left to the call (x0s None) is every chain's last training state."""
    mode = "reference"
    cs = case(shape, per_model, G)
    gs, call, meta = cs[0], cs[1], cs[2]
    rec = records(*[a for a in CASES if a[:3] == (shape, per_model, G)][0])          # (data only: any posterior's will do)
    assert rec["Y"].shape[2] == J
    CC, DD, lr = emission(cs, J)
    Zs, kerns, Xs, Qs = _fused_args(cs, STEPS)[:4]
    kw = dict(lengths=rec["lengths"], S0s=rec["S0"], q_mode=mode, smooth=True)
    fused = pr.posterior_filter_records_grouped(Zs, kerns, Xs, Qs, call, rec["ctrl"], rec["Y"], CC, DD, lr, x0s=rec["x0"], **kw)
    assert set(fused) == KEYS
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, Xs, call, Qs)
    Ls = [list(Lm[i]) for i in range(len(gs))] if per_model else list(Lm[0])
    two = pr.filter_records_grouped(Ls, Zs, kerns, list(U), list(Hinv), rec["x0"], rec["ctrl"], rec["Y"], Qs, CC, DD, lr, **kw)
    for k in sorted(KEYS):
        print(f"records {shape}: {k}: fused and two-call routes bit-identical: {np.array_equal(fused[k], two[k], equal_nan=True)}, largest "
              f"difference {float(np.nanmax(np.abs(np.asarray(fused[k]) - np.asarray(two[k])))):.3e}")
    for k in KEYS:
        np.testing.assert_array_equal(fused[k], two[k], err_msg=k)
    symmetric_and_smoothed_last(fused, LENGTHS)
    last = np.ascontiguousarray(np.broadcast_to(np.stack([g["X"][-1] for g in gs])[:, None, :], rec["x0"].shape))
    own, given = (pr.posterior_filter_records_grouped(Zs, kerns, Xs, Qs, call, rec["ctrl"], rec["Y"], CC, DD, lr, x0s=x, records_per_pass=2, **kw)
                  for x in (None, last))
    for k in KEYS:
        np.testing.assert_array_equal(own[k], given[k], err_msg=k)
    assert float(np.max(np.abs(own["m_filt"][:, 1, 1] - fused["m_filt"][:, 1, 1]))) > 0.0


# ---- model level: the actuator fixture with three chains -------------------------------------------------------------------------------
@pytest.mark.parametrize("U_collapse", [True, False], ids=["collapsed U", "explicit U"])
def test_filter_records_of_the_model(actuator, U_collapse):
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
    out = mod.filter_records(Yr, cr, lengths=lengths, smooth=True, Y_train_std=1.7)
    assert set(out) == KEYS and out["m_filt"].shape == (S, R, n, D) and out["predict_y"].shape == (R, n, J) and out["ll"].shape == (R,)
    live = live_rows(lengths, n)
    assert all(np.all(np.isfinite(out[k][:, live])) and np.all(np.isnan(out[k][:, ~live])) for k in MOMENTS)
    assert np.all(np.isfinite(out["ll"])) and np.isfinite(out["ll_all"]) and np.all(out["ll_original_units"] == out["ll"] - np.log(1.7))
    lay, lik = mod.layers[-1], mod.likelihood
    kw = dict(lengths=lengths, smooth=True, Y_train_std=1.7)
    if U_collapse:
        direct = pr.posterior_filter_records_grouped(lay.Z, lay.kernel, [mod._X_chains[s] for s in range(S)], mod.Q, mod.control_inputs, cr, Yr,
                                                     lik.CC, lik.DD, lik.log_Rchols, **kw)
    else:
        Lm = cmo.kernel_pre_cal(lay.Z, lay.kernel)
        x0 = np.broadcast_to(np.stack([mod._X_chains[s][-1] for s in range(S)])[:, None, :], (S, R, D))
        direct = pr.filter_records_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, x0, cr, Yr, mod.Q, lik.CC, lik.DD, lik.log_Rchols, **kw)
    again = mod.filter_records(Yr, cr, lengths=lengths, smooth=True, Y_train_std=1.7, records_per_pass=1)
    for k in KEYS:
        np.testing.assert_array_equal(out[k], direct[k], err_msg=k)
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
    # record 0 continues the training sequence with the model's own controls: the single-record filter agrees to rounding (printed;
    # test_against_the_single_record_filter has the bound)
    one = mod.filter_heldout_linearised(Yr[0], np.concatenate((c[:N_TRAIN], cr[0])), smooth=True, Y_train_std=1.7)
    d = max(float(np.max(np.abs(out[k][:, 0] - one[k]))) for k in MOMENTS)
    print(f"U_collapse={U_collapse}: per record ll {np.round(out['ll'], 6).tolist()}, RMSE {np.round(out['RMSE'], 6).tolist()}, ll_all "
          f"{out['ll_all']:.6f}; record 0 against filter_heldout_linearised: largest difference {d:.3e}, its ll {one['ll']:.6f}")
    with pytest.raises(ValueError, match="control_records"):
        mod.filter_records(Yr)
    x0 = np.stack([mod._X_chains[s][-1] for s in range(S)]).mean(axis=0)
    fresh = mod.filter_records(Yr, cr, lengths=lengths, x0=x0, S0=0.1 * np.eye(D))
    assert "m_smooth" not in fresh and float(np.max(np.abs(fresh["m_filt"][:, live] - out["m_filt"][:, live]))) > 0.0
    np.testing.assert_array_equal(fresh["S_pred"], np.swapaxes(fresh["S_pred"], -1, -2))
