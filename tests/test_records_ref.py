"""Pins tests/records_ref.py, the reference of the linearised filter over many records, without a GPU: one record is the existing
linearised-filter reference (filter_ref.filter with linear_filter_ref.ekf_transition, then filter_ref.smooth) exactly; a permutation
of the records permutes the outputs; a record padded with all-NaN rows (run as prediction steps) equals its truncated self on its own
rows bit for bit, smoothed arrays included -- an unobserved step leaves the filtered state equal to the predicted one, so the RTS
correction through it is an exact zero; the pooled arrays and the per-record scalars are those of prediction._filter_scalars record
by record.  Fixture: the two chains of forecast_linear_ref.long_record() (M = 24, D = 2, C = 1, q slices, "intent") with three
records of 6 rows cut from its data."""
import functools

import numpy as np

import filter_ref as fr
import forecast_linear_ref as flr
import linear_filter_ref as lf
import moment_ref as mr
import records_ref as rr
from ffvd_amd import prediction as pr

R, N = 3, 6


@functools.lru_cache(maxsize=None)
def fixture():
    """Shared, never modified."""
    r = flr.long_record()
    gs, D = r["gs"], r["meta"]["D"]
    rng = np.random.default_rng(41)
    Y = np.stack([r["Y"][10 * i: 10 * i + N] for i in range(R)]) + 0.1 * rng.standard_normal((R, N, r["Y"].shape[1]))
    Y[0, 2] = np.nan
    Y[2, 4] = np.nan
    ctrl = np.stack([r["ctrl"][20 * i: 20 * i + N] for i in range(R)])
    x0 = np.stack([g["X"][-1] for g in gs])[:, None, :] + 0.2 * rng.standard_normal((len(gs), R, D))
    S0 = np.stack([flr.start_cov(R, D, seed=7 + g) for g in range(len(gs))])
    terms = [mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], r["qs"][i], r["mode"]) for i, g in enumerate(gs)]
    return dict(r=r, gs=gs, Y=Y, ctrl=ctrl, x0=x0, S0=S0, terms=terms)


def run(fx, idx=None, Y=None, ctrl=None, lengths=None):
    idx = list(range(R)) if idx is None else idx
    r = fx["r"]
    Y = fx["Y"][idx] if Y is None else Y
    ctrl = fx["ctrl"][idx] if ctrl is None else ctrl
    return rr.tracks(fx["terms"], fx["gs"], ctrl, Y, r["CC"], r["DD"], r["sd"], fx["x0"][:, idx], fx["S0"][:, idx], lengths)


def test_one_record_is_the_linearised_filter_reference():
    fx = fixture()
    r = fx["r"]
    for i in range(R):
        out = run(fx, [i])
        for g, grp in enumerate(fx["gs"]):
            beta, Gam = fx["terms"][g]
            f = fr.filter(fx["x0"][g, i], fx["S0"][g, i], fx["Y"][i], r["CC"], r["DD"], r["sd"], grp["Q"],
                          lf.ekf_transition(fx["ctrl"][i], grp["Z"], grp["okern"], beta, Gam))
            f["m_smooth"], f["S_smooth"] = fr.smooth(f)
            for k in rr.MOMENTS + rr.DENSITIES:
                np.testing.assert_array_equal(out[k][g, 0], f[k], err_msg=k)
    assert out["m_pred"].shape == (2, 1, N, 2) and out["lpd_joint"].shape == (2, 1, N)


def test_a_permutation_of_the_records_permutes_the_outputs():
    fx = fixture()
    a, order = run(fx), [2, 0, 1]
    b = run(fx, order)
    for k in rr.MOMENTS + rr.DENSITIES:
        np.testing.assert_array_equal(b[k], a[k][:, order], err_msg=k)
    assert not np.array_equal(a["m_filt"][:, 0], a["m_filt"][:, 1])


def test_a_padded_record_equals_its_truncated_self_on_its_own_rows():
    fx = fixture()
    a, n = run(fx), 4
    Y, ctrl = np.array(fx["Y"]), np.array(fx["ctrl"])
    Y[1, n:] = np.nan
    cut = run(fx, Y=Y, lengths=[N, n, N])                         # record 1 truncated to n rows
    ctrl[1, n:] = 0.0
    pad = run(fx, Y=Y, ctrl=ctrl)                                 # ... and run over all N rows, the last two as prediction steps
    for k in rr.MOMENTS + rr.DENSITIES:
        assert np.all(np.isnan(cut[k][:, 1, n:])), k
        np.testing.assert_array_equal(pad[k][:, 1, :n], cut[k][:, 1, :n], err_msg=k)
        np.testing.assert_array_equal(pad[k][:, [0, 2]], cut[k][:, [0, 2]], err_msg=k)
        np.testing.assert_array_equal(cut[k][:, [0, 2]], a[k][:, [0, 2]], err_msg=k)
    for k in ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "lpd", "lpd_joint"):                # the filter is causal
        np.testing.assert_array_equal(cut[k][:, 1, :n], a[k][:, 1, :n], err_msg=k)
    assert np.all(np.isfinite(pad["m_smooth"])) and float(np.max(np.abs(cut["m_smooth"][:, 1, :n - 1] - a["m_smooth"][:, 1, :n - 1]))) > 0.0
    np.testing.assert_array_equal(pad["m_filt"][:, 1, n:], pad["m_pred"][:, 1, n:])
    np.testing.assert_array_equal(pad["S_smooth"][:, 1, n:], pad["S_pred"][:, 1, n:])


def test_the_reference_reports_its_own_error_and_symmetric_covariances():
    fx = fixture()
    r = fx["r"]
    wide = np.finfo(np.longdouble).eps < 1e-18
    ref, e_ref = rr.reference(fx["gs"], fx["ctrl"], fx["Y"], r["CC"], r["DD"], r["sd"], r["qs"], fx["x0"], fx["S0"], r["mode"], [N, 4, N], wide)
    a = run(fx, lengths=[N, 4, N])
    for k in rr.MOMENTS:
        np.testing.assert_array_equal(ref[k], a[k], err_msg=k)
        assert (0.0 < e_ref[k] < 1e-9) if wide else e_ref[k] == 0.0, k
    for k in ("S_pred", "S_filt", "S_smooth"):
        np.testing.assert_array_equal(ref[k], np.swapaxes(ref[k], -1, -2), err_msg=k)


def test_pooled_arrays_and_scalars_are_the_single_record_definitions():
    fx = fixture()
    r, a = fx["r"], run(fx, lengths=[N, 4, N])
    Y = np.array(fx["Y"])
    Y[1, 4:] = np.nan
    p = rr.pooled(a["m_pred"], a["S_pred"], r["CC"], r["DD"], r["sd"], Y)
    s = rr.scalars(Y, p["lpd_mix"], a["lpd_joint"], p["predict_y"], 1.7)
    assert all(p[k].shape == Y.shape for k in p) and all(s[k].shape == (R,) for k in ("ll", "ll_joint", "ll_original_units", "RMSE"))
    for i in range(R):
        n = [N, 4, N][i]
        one = mr.summary(a["m_pred"][:, i, :n], a["S_pred"][:, i, :n], r["CC"], r["DD"], r["sd"], Y[i, :n])
        np.testing.assert_array_equal(p["predict_y"][i, :n], one["y_mean"])
        np.testing.assert_array_equal(p["lpd_mix"][i, :n], one["lpd"])
        w = pr._filter_scalars(Y[i, :n], one["lpd"], a["lpd_joint"][:, i, :n], one["y_mean"], 1.7)
        for k in ("ll", "ll_joint", "ll_original_units", "RMSE"):
            assert s[k][i] == w[k] or abs(s[k][i] - w[k]) <= 1e-12 * (1.0 + abs(w[k])), k
    seen = ~np.isnan(Y)
    assert s["ll_all"] == float(np.mean(p["lpd_mix"][seen])) and np.isfinite(s["ll_all"])
