"""Argument checks of the rolling-origin forecasts, without a GPU: prediction._pack_forecast, forecast_grouped and
posterior_forecast_grouped raise ValueError before the library is loaded for a horizon of 0, a horizon that does not fit the record,
unsorted, duplicate or out-of-range origins, a stride of 0 and LinearK (and for every mismatch the filter's functions reject:
tests/test_filter_grouped_args.py, imported); the default origins are range(0, n - horizon, stride); ffvd_op_forecast_grouped /
ffvd_op_posterior_forecast_grouped return FFVD_EINVAL before any device call for each scalar rejection, a NULL or bad origin table and
no output at all (and FFVD_OK for G = 0 or steps = 0 without touching anything); the symbols are declared and bound;
DGPSSM.forecast_heldout exists with the documented defaults."""
import ctypes
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import BAD_ABI, BAD_FILTER, EMISSION, SKIP, _filter_args
from test_moment_grouped_args import BAD_EXPLICIT, BAD_FUSED, COMMON, _explicit, _fused, _with

E = _lib.FFVD_EINVAL
N = 4                                            # rows of the record the imported argument builders make (steps = 4)


@pytest.fixture
def no_device(monkeypatch):
    def fail():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", fail)


# ---- _pack_forecast ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,stride", [(12, 3, 1), (12, 3, 4), (12, 11, 1), (2, 1, 1), (200, 10, 10), (7, 2, 100)])
def test_default_origins_are_the_documented_range(n, h, stride):
    hh, org = pr._pack_forecast("t", n, h, None, stride)
    assert hh == h and org.dtype == np.int32 and org.flags["C_CONTIGUOUS"]
    assert org.tolist() == list(range(0, n - h, stride)) and len(org) >= 1 and org[-1] + h <= n - 1


def test_given_origins_are_kept():
    for o in ([0], [8], [0, 4, 8], np.arange(9), (1, 2), np.array([3.0, 5.0])):
        h, org = pr._pack_forecast("t", 12, 3, o)
        assert org.dtype == np.int32 and org.tolist() == [int(v) for v in o]


BAD_PACK = {
    "horizon 0": dict(horizon=0),
    "a negative horizon": dict(horizon=-2),
    "horizon = n": dict(horizon=12),
    "horizon > n": dict(horizon=13),
    "a fractional horizon": dict(horizon=2.5),
    "stride 0": dict(stride=0),
    "a negative stride": dict(stride=-1),
    "a fractional stride": dict(stride=1.5),
    "unsorted origins": dict(origins=[0, 5, 4]),
    "duplicate origins": dict(origins=[0, 4, 4]),
    "descending origins": dict(origins=[8, 4, 0]),
    "a negative origin": dict(origins=[-1, 2]),
    "an origin whose track leaves the record": dict(origins=[0, 9]),
    "an origin past the record": dict(origins=[40]),
    "no origins": dict(origins=[]),
    "origins with two axes": dict(origins=[[0, 1]]),
    "fractional origins": dict(origins=[0.5, 2.0]),
}


@pytest.mark.parametrize("what", sorted(BAD_PACK))
def test_pack_forecast_rejects(what):
    kw = dict(dict(horizon=3, origins=None, stride=1), **BAD_PACK[what])
    with pytest.raises(ValueError):
        pr._pack_forecast("t", 12, kw["horizon"], kw["origins"], kw["stride"])


def test_pack_forecast_rejects_linear_kernels_and_limits():
    pr._pack_forecast("t", 12, 3, model=(0, 5, 3, 2))
    with pytest.raises(ValueError, match="LinearK"):
        pr._pack_forecast("t", 12, 3, model=(1, 5, 3, 2))
    with pytest.raises(ValueError):
        pr._pack_forecast("t", 12, 3, model=(0, 5, 9, 9))


# ---- the public functions ------------------------------------------------------------------------------------------------------------
BAD_PUBLIC = {k: v for k, v in BAD_PACK.items()}
BAD_PUBLIC.update({
    "horizon = n": dict(horizon=N), "horizon > n": dict(horizon=N + 1), "unsorted origins": dict(origins=[0, 2, 1]),
    "duplicate origins": dict(origins=[1, 1]), "descending origins": dict(origins=[2, 0]),
    "an origin whose track leaves the record": dict(origins=[0, 3], horizon=1), "negative tracks_per_pass": dict(tracks_per_pass=-1),
})


def _call(explicit, a, **kw):
    kw = dict(dict(horizon=1), **kw)
    return (pr.forecast_grouped if explicit else pr.posterior_forecast_grouped)(**_filter_args(a, explicit), **EMISSION, **kw)


@pytest.mark.parametrize("what", sorted(BAD_PUBLIC))
def test_public_functions_reject_the_forecast_arguments_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError):
            _call(explicit, make(), **BAD_PUBLIC[what])


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP) + sorted(BAD_EXPLICIT))
def test_explicit_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_explicit) if what in COMMON else BAD_EXPLICIT[what]()
    with pytest.raises(ValueError):
        _call(True, a)


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP) + sorted(BAD_FUSED))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_fused) if what in COMMON else BAD_FUSED[what]()
    with pytest.raises(ValueError):
        _call(False, a)


def test_linear_kernels_are_named(no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError, match="LinearK"):
            _call(explicit, COMMON["LinearK"](make))


@pytest.mark.parametrize("what", sorted(BAD_FILTER))
def test_observations_and_emission_are_checked_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        a = _with(_with(_filter_args(make(), explicit), **EMISSION), **BAD_FILTER[what])
        with pytest.raises(ValueError):
            (pr.forecast_grouped if explicit else pr.posterior_forecast_grouped)(**a, horizon=1)


def test_well_formed_arguments_reach_the_library(monkeypatch):
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    for explicit, make in ((True, _explicit), (False, _fused)):
        for kw in (dict(horizon=1), dict(horizon=3), dict(horizon=2, stride=2), dict(horizon=2, origins=[1]), dict(horizon=1, origins=[0, 2]),
                   dict(horizon=1, return_tracks=True, return_filter=True, tracks_per_pass=2)):
            with pytest.raises(Reached):
                _call(explicit, make(), **kw)
        with pytest.raises(Reached):
            _call(explicit, make(C=0), horizon=2)


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
FILTER_OUT = ("mp", "Sp", "mf", "Sf", "X_", "lpd", "lj", "ms", "Ss", "ym", "yt", "lm", "lg")
FC_OUT = ("mfc", "Sfc", "fym", "fyt", "flm", "flg")


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=6, kind=0, gpp=0, q_mode=0, J=1, null=(), sd=1.0, y=0.0, horizon=2,
         origins=(0, 1, 3), n_origins=None, tpp=0):
    """One ABI call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL."""
    P = D + C if P is None else P
    n, nm, st, Pp, Jp = max(G, 1), max(n_models, 1), max(steps, 1), max(P, 1), max(J, 1)
    B = len(origins) if n_origins is None else n_origins
    Bn, hn = max(B, 1), min(max(horizon, 1), 8)              # (a rejected call touches nothing: no buffer of a huge horizon is built)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((n, T + 1, D)),
             cf=np.zeros((max(T, 1), max(C, 1))), cr=np.zeros((st, max(C, 1))), lq=np.zeros((n, D)), f=np.zeros((n, M, D)),
             xl=np.zeros((n, D)), CC=np.ones((D, Jp)), DD=np.zeros(Jp), sd=np.full(Jp, sd), Y=np.full((st, Jp), y))
    vec, mat = (n, st, D), (n, st, D, D)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, X_=mat, lpd=(n, st, Jp), lj=(n, st), ms=vec, Ss=mat, ym=(st, Jp), yt=(st, Jp), lm=(st, Jp),
                  lg=(st, Jp), U=(n, M, D), mfc=(n, Bn, hn, D), Sfc=(n, Bn, hn, D, D), fym=(Bn * hn, Jp), fyt=(Bn * hn, Jp),
                  flm=(Bn * hn, Jp), flg=(Bn * hn, Jp))
    outs = {k: np.full(s, 7.0) for k, s in shapes.items()}
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    org = np.asarray(origins, dtype=np.int32)
    po = None if "origins" in null else org.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"]) + tuple(p[k] for k in FILTER_OUT)
    fc = (horizon, po, B, tpp) + tuple(p[k] for k in FC_OUT)
    if fused:
        rc = lib.ffvd_op_posterior_forecast_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                    1e-5, gpp, q_mode, None, None, p["cr"], steps, *tail, p["U"], *fc)
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_op_forecast_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, q_mode, p["xl"], None,
                                          p["cr"], C, steps, p["lq"], *tail, *fc)
    return rc, outs


ALL_OUT = FILTER_OUT + FC_OUT
BAD_FORECAST_ABI = [dict(horizon=0), dict(horizon=-1), dict(origins=(), n_origins=0), dict(n_origins=-1), dict(null=("origins",)),
                    dict(origins=(0, 3, 1)), dict(origins=(0, 1, 1)), dict(origins=(3, 1, 0)), dict(origins=(-1, 1, 3)),
                    dict(origins=(0, 1, 4)), dict(origins=(0,), horizon=6), dict(origins=(0,), horizon=7), dict(tpp=-1),
                    dict(null=ALL_OUT), dict(G=2, origins=tuple(range(4)), horizon=2 ** 27)]           # (G B h D D = 2^32)
# (the filter's own list, with its "no output" entry replaced by "no output of either kind" above)
BAD_BOTH = [ov for ov in BAD_ABI if len(ov.get("null", ())) <= 1] + BAD_FORECAST_ABI


@pytest.mark.parametrize("ov", BAD_BOTH + [dict(null=("f",)), dict(null=("xl",)), dict(null=("W",))], ids=str)
def test_explicit_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(False, **ov)
    assert rc == E, rc
    assert b"ffvd_op_forecast_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", BAD_BOTH + [dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))], ids=str)
def test_fused_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(True, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_forecast_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_linear_kernels_are_named_in_the_message():
    for fused in (False, True):
        rc, _ = _abi(fused, kind=1)
        assert rc == E and b"SE kernel only" in _lib.load().ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(G=0, n_models=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())


def test_symbols_are_bound():
    for s in ("ffvd_op_forecast_grouped", "ffvd_op_posterior_forecast_grouped"):
        assert s in _lib.exported_symbols() and hasattr(_lib.load(), s)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_forecast_heldout_is_there_with_the_documented_defaults():
    from ffvd_amd.dgp_model import DGPSSM
    sig = inspect.signature(DGPSSM.forecast_heldout).parameters
    assert list(sig) == ["self", "Y_test", "control_inputs", "horizon", "stride", "origins", "x0", "S0", "q_mode", "Y_train_std", "return_tracks"]
    assert sig["control_inputs"].default is None and sig["horizon"].default == 10 and sig["stride"].default == 1
    assert sig["origins"].default is None and sig["x0"].default is None and sig["S0"].default is None
    assert sig["q_mode"].default == "reference" and sig["Y_train_std"].default == 1.0 and sig["return_tracks"].default is False
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("stride", "origins", "x0", "S0", "q_mode", "Y_train_std", "return_tracks"))

    class Stub:
        _host_stale = False
        Y = np.zeros((4, 1))

    with pytest.raises(ValueError, match="q_mode"):              # stopped before any parameter or device is touched
        DGPSSM.forecast_heldout(Stub(), np.zeros((2, 1)), q_mode="slice0")
    with pytest.raises(ValueError, match="Y_test"):
        DGPSSM.forecast_heldout(Stub(), np.zeros((2, 3)))
    for f in (pr.forecast_grouped, pr.posterior_forecast_grouped):
        sig = inspect.signature(f).parameters
        assert sig["origins"].default is None and sig["stride"].default == 1 and sig["S0s"].default is None
        assert sig["q_mode"].default == "reference" and sig["Y_train_std"].default == 1.0 and sig["tracks_per_pass"].default == 0
        assert sig["return_tracks"].default is False and sig["return_filter"].default is False
    assert "not re-weighted" in pr.forecast_grouped.__doc__
