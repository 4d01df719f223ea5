"""The reference of the linearised forecasts, pinned without a device (tests/forecast_linear_ref.py).

1. The definition -- one filter_ref.filter with linear_filter_ref.ekf_transition per origin over the truncated record followed by h
   all-NaN rows -- equals, bit for bit, continuing h unobserved rows from the filtered state of ONE filter over the whole record
   (`tracks`, which the GPU tests use because it is 50 x cheaper).
2. The long-record fixture (140 rows, 138 origins: the one that crosses a row-tile boundary on the device) keeps every reference value
   finite and every covariance positive definite; n_h is what the gaps give.  Measured on the CPU: smallest eigenvalue 0.335,
   max|m| 2.18, e_ref (fp64 against np.longdouble) 1.2e-12 on the means and 2.1e-12 on the covariances."""
import numpy as np

import filter_ref as fr
import forecast_linear_ref as flr
import linear_filter_ref as lf
import moment_ref as mr
from ffvd_amd import prediction as pr

WIDE = np.finfo(np.longdouble).eps < 1e-18


def test_continuing_from_the_filtered_state_is_the_definition():
    r = flr.long_record()
    origins, h, J = [0, 6, 7, 8, 77, 137], r["h"], r["Y"].shape[1]
    for i, g in enumerate(r["gs"]):
        beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], r["qs"][i], r["mode"])
        model = (r["ctrl"], g["Z"], g["okern"], beta, Gam)
        f = fr.filter(g["X"][-1], r["S0"][i], r["Y"], r["CC"], r["DD"], r["sd"], g["Q"], lf.ekf_transition(*model))
        m, S = flr.tracks(f, origins, h, J, r["CC"], r["DD"], r["sd"], g["Q"], *model)
        mn, Sn = flr.naive(g["X"][-1], r["S0"][i], r["Y"], origins, h, r["CC"], r["DD"], r["sd"], g["Q"], *model)
        assert m.shape == (len(origins), h, 2) and S.shape == (len(origins), h, 2, 2)
        np.testing.assert_array_equal(m, mn)
        np.testing.assert_array_equal(S, Sn)
        # horizon 1 from origin o is the filter's own prediction of row o + 1 wherever the filter saw nothing it did not
        rows = [o + 1 for o in origins]
        np.testing.assert_array_equal(m[:, 0], f["m_pred"][rows])
        np.testing.assert_array_equal(S[:, 0], f["S_pred"][rows])


def test_the_long_record_is_well_conditioned():
    r = flr.long_record()
    assert r["meta"]["M"] == 24 and r["meta"]["D"] == 2 and r["meta"]["C"] == 1 and r["Y"].shape == (140, 1)
    assert len(r["origins"]) == 138 and r["origins"][-1] + r["h"] == 139
    ref, e_ref = flr.reference(r["gs"], r["ctrl"], r["Y"], r["CC"], r["DD"], r["sd"], r["qs"], r["S0"], r["mode"], r["origins"], r["h"], WIDE)
    assert ref["m"].shape == (2, 138, 2, 2) and ref["S"].shape == (2, 138, 2, 2, 2)
    assert np.all(np.isfinite(ref["m"])) and np.all(np.isfinite(ref["S"]))
    np.testing.assert_array_equal(ref["S"], np.swapaxes(ref["S"], -1, -2))
    low, big = float(np.min(np.linalg.eigvalsh(ref["S"]))), float(np.max(np.abs(ref["m"])))
    print(f"long record: smallest eigenvalue {low:.3e}, max|m| {big:.3e}, e_ref m {e_ref['m']:.3e}, S {e_ref['S']:.3e}")
    assert low > 0.0
    # the curves' counts: row 7 is the only gap, so each horizon loses exactly one of its 138 targets
    _, org = pr._pack_forecast("t", 140, r["h"])
    assert org.tolist() == r["origins"]
    seen = ~np.isnan(r["Y"][org[:, None] + 1 + np.arange(r["h"])[None, :]])
    assert seen.sum(axis=0).tolist() == [[137], [137]]
