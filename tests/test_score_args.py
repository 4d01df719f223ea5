"""CPU: rollout_score, particle_score, moment_score, forecast_score and DGPSSM.forecast_scores raise on every shape, level and
limit error before the library is loaded; `ffvd_score_points` / `ffvd_score_moments` return FFVD_EINVAL with a message that names
the limit before any device call, and FFVD_OK for an empty call."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import score_fixtures as sf
from conftest import ROOT
from ffvd_amd import _lib
from ffvd_amd import prediction as pr

SYMBOLS = ("ffvd_score_points", "ffvd_score_moments")


@pytest.fixture
def no_device(monkeypatch):
    def fail():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", fail)


class Reached(Exception):
    pass


@pytest.fixture
def reached(monkeypatch):
    def hit():
        raise Reached()
    monkeypatch.setattr(_lib, "load", hit)


def _em(D=2, J=1):
    return np.ones((D, J)), np.zeros(J), np.zeros((J, J))


def test_the_constants_of_the_python_layer_are_the_headers():
    with open(os.path.join(ROOT, "ffvd_amd", "csrc", "predict_score.h")) as f:
        text = f.read()
    for name, value in (("PSC_TILE", pr.SCORE_TILE), ("PSC_MAXK", pr.SCORE_MAX_K), ("PSC_MAXQ", pr.SCORE_MAX_Q),
                        ("PSC_MAXD_POINTS", pr.SCORE_MAX_D_POINTS), ("PSC_MAXD_MOMENTS", pr.MOMENT_MAX_D), ("PSC_MAXJ", pr.SUMMARY_MAX_OUTPUTS)):
        assert f"constexpr int {name} = {value};" in text, name
    assert sf.TILE == pr.SCORE_TILE


def test_signatures():
    for fn, lead in ((pr.rollout_score, ["predict_x"]), (pr.particle_score, ["particles"]), (pr.moment_score, ["m_x", "S_x"])):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + ["CC", "DD", "log_Rchols", "Y_test", "levels", "Y_train_std", "targets_per_pass"]
        assert p["Y_test"].default is None and p["levels"].default == (0.05, 0.5, 0.95) and p["Y_train_std"].default == 1.0
        assert p["targets_per_pass"].default == 0 and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[-3:])
    p = inspect.signature(pr.forecast_score).parameters
    assert list(p) == ["fan", "Y_obs", "CC", "DD", "log_Rchols", "levels", "use", "Y_train_std"] and p["use"].default == "auto"
    from ffvd_amd.dgp_model import DGPSSM
    p = inspect.signature(DGPSSM.forecast_scores).parameters
    assert list(p)[:6] == ["self", "Y_test", "control_inputs", "horizon", "method", "levels"] and p["method"].default == "moment"
    assert p["horizon"].default == 10 and p["method"].kind is inspect.Parameter.KEYWORD_ONLY


def test_shape_errors_of_the_three_stack_functions(no_device):
    CC, DD, lr = _em()
    x, S = np.zeros((3, 4, 2)), np.zeros((3, 4, 2, 2))
    bad_points = ((np.zeros((4, 2)), "rollout_score: predict_x"), (np.zeros((0, 4, 2)), "at least one rollout"),
                  (np.zeros((3, 4, 33)), "1 <= D <= 32"), (np.zeros((65537, 1, 1)), "K must lie in"))
    for arr, msg in bad_points:
        em = _em(D=arr.shape[-1]) if arr.ndim >= 3 else (CC, DD, lr)
        with pytest.raises(ValueError, match=msg):
            pr.rollout_score(arr, *em)
    for arr, msg in ((np.zeros((3, 4, 2)), "particle_score: particles"), (np.zeros((2, 4, 0, 2)), "at least one group"),
                     (np.zeros((1, 1, 2, 33)), "1 <= D <= 32"), (np.zeros((257, 1, 256, 1)), "K must lie in")):
        with pytest.raises(ValueError, match=msg):
            pr.particle_score(arr, *_em(D=arr.shape[-1]))
    for m_, S_, msg in ((np.zeros((3, 4)), S, "moment_score: expected m_x"), (x, np.zeros((3, 4, 2)), "moment_score: expected m_x"),
                        (np.zeros((3, 4, 9)), np.zeros((3, 4, 9, 9)), "1 <= D <= 8"), (np.zeros((0, 4, 2)), np.zeros((0, 4, 2, 2)), "at least one group")):
        with pytest.raises(ValueError, match=msg):
            pr.moment_score(m_, S_, *_em(D=m_.shape[-1]))
    with pytest.raises(ValueError, match="K must lie in"):
        pr.moment_score(np.zeros((65537, 1, 1)), np.zeros((65537, 1, 1, 1)), *_em(D=1))
    calls = ((pr.rollout_score, (x,)), (pr.particle_score, (np.zeros((3, 4, 5, 2)),)), (pr.moment_score, (x, S)))
    for fn, lead in calls:
        who = fn.__name__
        for em, msg in (((np.ones((3, 1)), DD, lr), f"{who}: CC"), ((np.ones((2, 9)), np.zeros(9), np.zeros(9)), f"{who}: CC"),
                        ((CC, np.zeros(2), lr), "DD"), ((CC, DD, np.zeros((2, 2))), f"{who}: log_Rchols"),
                        ((CC, DD, np.array([np.inf])), "finite and positive")):
            with pytest.raises(ValueError, match=msg):
                fn(*lead, *em)
        for Y in (np.zeros((5, 1)), np.zeros((3, 2)), np.zeros((2, 2, 1))):
            with pytest.raises(ValueError, match=f"{who}: Y_test"):
                fn(*lead, CC, DD, lr, Y)
        for lv, msg in (((0.0, 0.5), "every level"), ((0.5, 1.0), "every level"), ((1e-10,), "every level"), ((0.5, np.nan), "every level"),
                        (np.linspace(0.1, 0.9, 17), "at most 16"), (((0.1, 0.9),), "at most 16"), (0.5, "at most 16"), ("median", "levels")):
            with pytest.raises(ValueError, match=f"{who}: levels.*{msg}" if msg != "levels" else f"{who}: levels"):
                fn(*lead, CC, DD, lr, np.zeros((2, 1)), levels=lv)
        with pytest.raises(ValueError, match=f"{who}: nothing to compute"):
            fn(*lead, CC, DD, lr, levels=())
        for tpp in (-1, 1.5, True):
            with pytest.raises(ValueError, match=f"{who}: targets_per_pass"):
                fn(*lead, CC, DD, lr, np.zeros((2, 1)), targets_per_pass=tpp)


def test_the_two_to_the_31_limits(no_device):
    big = np.broadcast_to(np.zeros(1), (65536, 4097, 8))                    # K * steps * D = 2^31, no memory behind it
    with pytest.raises(ValueError, match="below 2\\^31"):
        pr._score_points("rollout_score", big, 65536, 1, 4097, 8, (4097 * 8, 0, 8), *_em(D=8), None, (0.5,), 1.0, 0)
    ok = np.broadcast_to(np.zeros(1), (65536, 4096, 1))                     # the stack fits, steps * J * K = 2^31 with J = 8 does not
    with pytest.raises(ValueError, match="steps \\* J \\* K"):
        pr._score_points("rollout_score", ok, 65536, 1, 4096, 1, (4096, 0, 1), *_em(D=1, J=8), None, (0.5,), 1.0, 0)


def test_a_correct_call_reaches_the_library_and_not_before(reached):
    CC, DD, lr = _em()
    for fn, lead in ((pr.rollout_score, (np.zeros((3, 4, 2)),)), (pr.rollout_score, (np.zeros((2, 3, 4, 2)),)),
                     (pr.particle_score, (np.zeros((3, 4, 5, 2)),)), (pr.moment_score, (np.zeros((3, 4, 2)), np.zeros((3, 4, 2, 2))))):
        with pytest.raises(Reached):
            fn(*lead, CC, DD, lr, np.zeros((3, 1)), levels=(0.1, 0.9), targets_per_pass=2)
        with pytest.raises(Reached):
            fn(*lead, CC, DD, lr)                                           # quantiles alone
        with pytest.raises(Reached):
            fn(*lead, CC, DD, np.zeros(1), np.zeros(3), levels=())          # scores alone; J = 1: vectors for log_Rchols and Y_test


def _fan(G=2, B=3, h=2, N=4, D=2, particles=True, tracks=True):
    fan = dict(origins=np.array([0, 2, 4]))
    if particles:
        fan["fc_particles"] = np.zeros((G, B, h, N, D))
    if tracks:
        fan.update(m_fc=np.zeros((G, B, h, D)), S_fc=np.zeros((G, B, h, D, D)))
    return fan


def test_forecast_score_errors(no_device):
    CC, DD, lr = _em()
    Y = np.zeros((8, 1))
    for fan, kw, msg in ((_fan(), dict(use="gauss"), "forecast_score: use"), ([1, 2], {}, "forecast_score: fan"), ({"m_fc": 1}, {}, "forecast_score: fan"),
                         (_fan(particles=False), dict(use="particles"), "needs fc_particles"), (_fan(tracks=False), dict(use="moments"), "needs m_fc"),
                         (_fan(particles=False, tracks=False), {}, "neither fc_particles nor m_fc"),
                         (dict(_fan(), origins=np.array([0.5, 1.5, 2.5])), {}, "origins"), (dict(_fan(), origins=np.zeros((3, 1), dtype=int)), {}, "origins"),
                         (dict(_fan(), fc_particles=np.zeros((2, 4, 2, 4, 2))), {}, "fc_particles: expected"),
                         (dict(_fan(), fc_particles=np.zeros((2, 3, 2, 4))), {}, "fc_particles: expected"),
                         (dict(_fan(), S_fc=np.zeros((2, 3, 2, 2))), dict(use="moments"), "expected m_fc"),
                         (dict(_fan(), origins=np.array([0, 2, 6])), {}, "do not fit"), (dict(_fan(), origins=np.array([2, 0, 4])), {}, "do not fit"),
                         (dict(_fan(), origins=np.array([-1, 2, 4])), {}, "do not fit"),
                         (_fan(), dict(levels=(0.5, 2.0)), "every level"), (_fan(), dict(use="moments", levels=(0.0,)), "every level")):
        with pytest.raises(ValueError, match=msg):
            pr.forecast_score(fan, Y, CC, DD, lr, **kw)
    with pytest.raises(ValueError, match="Y_obs"):
        pr.forecast_score(_fan(), np.zeros((8, 1, 1)), CC, DD, lr)
    with pytest.raises(ValueError, match="Y_test"):
        pr.forecast_score(_fan(), np.zeros((8, 2)), CC, DD, lr)             # the record's J against the emission's


def test_forecast_score_picks_the_stack_and_forms_the_targets(monkeypatch):
    CC, DD, lr = _em()
    Y = np.arange(8.0)[:, None]
    Y[3] = np.nan
    seen = {}

    def fake(name):
        def fn(*a, **kw):
            seen[name] = (a, kw)
            n = a[0].shape[1]
            pit = np.linspace(0.0, 1.0, n)[:, None]
            return dict(crps=np.where(np.isnan(a[-1]), np.nan, 1.0 + a[-1]), pit=np.where(np.isnan(a[-1]), np.nan, pit),
                        quantiles=np.zeros((n, 1, 3)), levels=np.array([0.25, 0.5, 0.75]), crps_mean=0.0, crps_mean_original_units=0.0,
                        coverage=np.zeros(1), coverage_levels=np.array([0.25]))
        return fn
    monkeypatch.setattr(pr, "particle_score", fake("particles"))
    monkeypatch.setattr(pr, "moment_score", fake("moments"))
    r = pr.forecast_score(_fan(), Y, CC, DD, lr, levels=(0.25, 0.5, 0.75), Y_train_std=1.7)
    assert r["used"] == "particles" and set(seen) == {"particles"}
    a, kw = seen["particles"]
    assert a[0].shape == (2, 6, 4, 2) and kw == dict(levels=(0.25, 0.5, 0.75), Y_train_std=1.7)
    want = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])                    # Y[origin + k], k = 1, 2
    want[1, 0] = np.nan
    np.testing.assert_array_equal(a[-1].reshape(3, 2), want)
    assert r["crps"].shape == r["pit"].shape == (3, 2, 1) and r["quantiles"].shape == (3, 2, 1, 3) and r["origins"].tolist() == [0, 2, 4]
    assert r["n_h"].tolist() == [[2], [3]]
    np.testing.assert_allclose(r["crps_h"][:, 0], [1.0 + (1.0 + 5.0) / 2, 1.0 + (2.0 + 4.0 + 6.0) / 3])
    pit = r["pit"][:, :, 0]
    inside = (pit >= 0.25) & (pit <= 0.75)
    np.testing.assert_allclose(r["coverage_h"][:, 0, 0], [np.sum(inside[[0, 2], 0]) / 2, np.sum(inside[:, 1]) / 3])
    assert r["coverage_h"].shape == (2, 1, 1)
    seen.clear()
    assert pr.forecast_score(_fan(), Y, CC, DD, lr, use="moments")["used"] == "moments" and set(seen) == {"moments"}
    assert seen["moments"][0][0].shape == (2, 6, 2) and seen["moments"][0][1].shape == (2, 6, 2, 2)
    seen.clear()
    assert pr.forecast_score(_fan(particles=False), Y, CC, DD, lr)["used"] == "moments"


def test_coverage_pairs_and_shares():
    lv = np.array([0.05, 0.25, 0.5, 0.75, 0.9, 0.95])
    assert pr._coverage_pairs(lv) == [(0, 5), (1, 3)]                        # 0.9 has no mirror image; 0.5 is its own
    pit = np.array([[0.01, 0.3], [0.5, np.nan], [0.96, 0.7], [0.06, 0.2]])
    cov, low = pr._coverage(pit, ~np.isnan(pit), lv)
    np.testing.assert_allclose(low, [0.05, 0.25])
    np.testing.assert_allclose(cov, [5 / 7, 3 / 7])
    cov, _ = pr._coverage(pit, ~np.isnan(pit), lv, axis=0)
    np.testing.assert_allclose(cov, [[2 / 4, 1 / 4], [3 / 3, 2 / 3]])
    cov, low = pr._coverage(np.full((2, 2), np.nan), np.zeros((2, 2), dtype=bool), np.array([0.5]))
    assert cov.shape == (0,) and low.shape == (0,)
    cov, _ = pr._coverage(np.full((2, 2), np.nan), np.zeros((2, 2), dtype=bool), lv, axis=0)
    assert cov.shape == (2, 2) and np.all(np.isnan(cov))


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def test_forecast_scores_of_the_model(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from test_forecast_particle_args import _Model
    Y = np.zeros((8, 1))
    for kw, exc, msg in ((dict(method="ekf"), ValueError, "forecast_scores: method"), (dict(use="gauss"), ValueError, "forecast_scores: use"),
                         (dict(method="cubature", use="particles"), ValueError, "needs a particle rule"),
                         (dict(method="moment", num_particles=8), TypeError, "takes the keywords"),
                         (dict(method="particle", return_tracks=True), TypeError, "takes the keywords"),
                         (dict(levels=(0.5, 1.5)), ValueError, "forecast_scores: levels"),
                         (dict(method="adapted", num_particles=1), ValueError, "forecast_scores: num_particles"),
                         (dict(method="particle", noise="none"), ValueError, "forecast_scores: noise"),
                         (dict(method="linearised", q_mode="slice0"), ValueError, "forecast_scores: q_mode"), (dict(method="particle", horizon=8), ValueError, "horizon")):
        with pytest.raises(exc, match=msg):
            DGPSSM.forecast_scores(_Model(), Y, **dict(dict(horizon=2), **kw))
    seen = {}
    names = ("posterior_forecast_grouped", "posterior_forecast_linear_grouped", "posterior_forecast_cubature_grouped",
             "posterior_forecast_particle_grouped", "posterior_forecast_adapted_grouped")
    for name in names:
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or {"name": _n})
    monkeypatch.setattr(pr, "forecast_score", lambda fan, *a, **kw: seen.update(score=(fan, a, kw)) or {"crps": 1})
    for method, name in zip(DGPSSM.FORECAST_SCORE_METHODS, names):
        seen.clear()
        extra = dict(num_particles=16, seed=3) if method in ("particle", "adapted") else {}
        r = DGPSSM.forecast_scores(_Model(), Y, None, 2, method=method, levels=(0.1, 0.9), stride=2, Y_train_std=1.7, **extra)
        assert r == {"crps": 1, "fan": {"name": name}} and set(seen) == {name, "score"}
        k = seen[name][1]
        assert k["return_tracks"] is True and k["Y_train_std"] == 1.7 and k.get("return_particles", False) is bool(extra)
        fan, a, kw = seen["score"]
        assert fan == {"name": name} and kw == dict(levels=(0.1, 0.9), use="auto", Y_train_std=1.7) and a[0].shape == (8, 1)
    seen.clear()
    DGPSSM.forecast_scores(_Model(), Y, None, 2, method="adapted", use="moments", num_particles=16, seed=3)
    assert "return_particles" not in seen["posterior_forecast_adapted_grouped"][1] and seen["score"][2]["use"] == "moments"


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_keep_out_of_the_op_prefix():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        text = f.read()
    for s in SYMBOLS:
        assert _lib._SIGNATURES[s][0] is ctypes.c_int and s in _lib.exported_symbols() and hasattr(_lib.load(), s) and s + "(" in text
        assert not s.startswith("ffvd_op_")


def _abi(symbol, **ov):
    a = dict(K1=3, K2=2, steps=4, D=2, J=1, n_test=3, Q=2, tpp=0, sk1=16, sk2=2, st=4, sd=0.5, levels=(0.1, 0.9), x=True, out=(True, True, True),
             Y=True, lv=True)
    a.update(ov)
    dp, z = _lib.dptr, np.zeros(4096)
    lv, sd = np.array(a["levels"], dtype=np.float64), np.full(8, a["sd"])
    o = [dp(np.zeros(4096)) if f else None for f in a["out"]]
    tail = (dp(z), dp(z), dp(sd), a["J"], dp(z) if a["Y"] else None, a["n_test"], dp(lv) if a["lv"] else None, a["Q"], a["tpp"], *o)
    lib = _lib.load()
    if symbol == "ffvd_score_points":
        rc = lib.ffvd_score_points(dp(z) if a["x"] else None, a["K1"], a["K2"], a["steps"], a["D"], a["sk1"], a["sk2"], a["st"], *tail)
    else:
        rc = lib.ffvd_score_moments(dp(z) if a["x"] else None, dp(z), a["K1"], a["steps"], a["D"], *tail)
    return rc, lib.ffvd_last_error(None).decode()


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_the_abi_names_the_limit_before_any_device_call(symbol):
    moments = symbol == "ffvd_score_moments"
    cases = [(dict(K1=65537, K2=1), "K must lie in [1, 65536]"), (dict(K1=-1), "K must lie in"), (dict(steps=-1), "steps"),
             (dict(D=0), "D must lie in"), (dict(D=9 if moments else 33), f"D must lie in [1, {8 if moments else 32}]"),
             (dict(J=0), "J must lie in [1, 8]"), (dict(J=9), "J must lie in [1, 8]"), (dict(Q=17), "Q must lie in [0, 16]"), (dict(Q=-1), "Q must lie in"),
             (dict(n_test=5), "n_test must lie in [0, steps]"), (dict(n_test=-1), "n_test"), (dict(tpp=-1), "targets_per_pass"),
             (dict(levels=(0.0, 0.5)), "every level must lie in [1e-9, 1 - 1e-9]"), (dict(levels=(0.5, float("nan"))), "every level"),
             (dict(levels=(0.5, 1.0)), "every level"), (dict(sd=0.0), "noise_std must be finite and positive"), (dict(sd=float("inf")), "noise_std"),
             (dict(out=(False, False, False)), "at least one of crps, pit and quantiles"), (dict(Y=False), "need Y_test"), (dict(lv=False), "need levels"),
             (dict(x=False), "needed"), (dict(K1=65536, K2=1, steps=4096, J=8, n_test=0, sk1=0, st=0), "below 2^31")]
    if not moments:
        cases += [(dict(K1=300, K2=300), "K must lie in"), (dict(sk1=-1), "strides"), (dict(sk1=2 ** 31), "below 2^31"),
                  (dict(K1=1024, K2=1, sk1=2 ** 21 + 2100), "below 2^31")]
    for ov, msg in cases:
        rc, err = _abi(symbol, **ov)
        assert rc == _lib.FFVD_EINVAL and err.startswith(symbol + ": bad argument") and msg in err, (ov, err)
    for ov in (dict(K1=0), dict(steps=0, n_test=0), dict(K1=0, x=False, out=(False, False, False))):
        assert _abi(symbol, **ov)[0] == _lib.FFVD_OK, ov
