"""Argument checks of the cubature filter over many records, without a GPU: prediction.filter_cubature_records_grouped /
posterior_filter_cubature_records_grouped run the packing stage of the records functions (`_pack_records`): every error of
tests/test_filter_records_args.py raises ValueError before the library is loaded, well-formed arguments reach it; their signatures
are the records functions'; DGPSSM.filter_records_cubature has `filter_records`' parameter list, shares its body and hands the two
forms to the cubature functions; ffvd_op_filter_cubature_records_grouped / ffvd_op_posterior_filter_cubature_records_grouped are
declared in the header with the argument lists of the records entry points, bound in _lib.py, exported where the library is built,
and return FFVD_EINVAL before any device call beyond their limits (FFVD_OK for no groups, records or rows).  What is pinned for the
existing calls stays: no `method` parameter on the records calls, FILTER_METHODS, DGPSSM.filter_records' parameter list."""
import ctypes
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_filter_records_args import BAD, OUT_NAMES, R, SKIP, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import COMMON, _explicit, _fused, _with

SYMBOLS = ("ffvd_op_filter_cubature_records_grouped", "ffvd_op_posterior_filter_cubature_records_grouped")
RECORDS = ("ffvd_op_filter_records_grouped", "ffvd_op_posterior_filter_records_grouped")


def _fn(explicit):
    return pr.filter_cubature_records_grouped if explicit else pr.posterior_filter_cubature_records_grouped


def _call(explicit, **kw):
    return _fn(explicit)(**_with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **kw))


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP))
def test_model_mismatches_are_rejected_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError):
            _fn(explicit)(**_records(COMMON[what](make), explicit), **EMISSION)


def test_linear_kernels_are_rejected_by_the_moment_limits(no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError, match="SquaredExponential"):
            _fn(explicit)(**_records(COMMON["LinearK"](make), explicit), **EMISSION)


@pytest.mark.parametrize("what", sorted(BAD))
def test_every_error_of_the_records_packing_raises_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **BAD[what])


def test_the_messages_name_the_function_and_the_argument(no_device):
    with pytest.raises(ValueError, match="filter_cubature_records_grouped: x0s"):
        _call(True, x0s=None)
    for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                     (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records")):
        for explicit in (True, False):
            who = ("" if explicit else "posterior_") + "filter_cubature_records_grouped"
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call(explicit, **kw)


def test_well_formed_arguments_reach_the_cubature_symbols(monkeypatch):
    class Reached(Exception):
        pass
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                seen.append((name, len(a)))
                raise Reached()
            return f
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    Y = np.zeros((R, STEPS, 1))
    Y[1, 2:] = np.nan
    for kw in (dict(), dict(Y_records=Y, lengths=[STEPS, 2, STEPS]), dict(records_per_pass=2, smooth=True, q_mode="intent", Y_train_std=1.7),
               dict(Y_records=Y[:1], control_records=np.zeros((1, STEPS, 1)), x0s=np.zeros((1, 2)))):          # (R = 1: a single record)
        for explicit in (True, False):
            with pytest.raises(Reached):
                _call(explicit, **kw)
            assert seen[-1] == (SYMBOLS[not explicit], len(_lib._SIGNATURES[SYMBOLS[not explicit]][1]))
    with pytest.raises(Reached):                                  # the fused call may leave the start to the training states
        _call(False, x0s=None)
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_the_signatures_are_the_records_functions(no_device):
    for new, old in ((pr.filter_cubature_records_grouped, pr.filter_records_grouped),
                     (pr.posterior_filter_cubature_records_grouped, pr.posterior_filter_records_grouped)):
        assert inspect.signature(new) == inspect.signature(old)
        assert "method" not in inspect.signature(new).parameters and "method" not in inspect.signature(old).parameters
    assert pr.FILTER_METHODS == ("moment", "linearised")
    doc = pr.filter_cubature_records_grouped.__doc__
    assert "EQUAL weights" in doc and "sqrt(D)" in doc and "second order" in doc


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    old, new = inspect.signature(DGPSSM.filter_records), inspect.signature(DGPSSM.filter_records_cubature)
    assert new == old
    assert list(old.parameters) == ["self", "Y_records", "control_records", "lengths", "x0", "S0", "smooth", "q_mode", "Y_train_std", "records_per_pass"]
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    with pytest.raises(ValueError, match="filter_records_cubature: q_mode"):
        DGPSSM.filter_records_cubature(_Model(), Y, ctrl, q_mode="slice0")
    with pytest.raises(ValueError, match="filter_records_cubature: Y_records"):
        DGPSSM.filter_records_cubature(_Model(), np.zeros((STEPS, 1)), ctrl)
    with pytest.raises(ValueError, match="control_records"):
        DGPSSM.filter_records_cubature(_Model(), Y)
    with pytest.raises(ValueError, match="x0"):
        DGPSSM.filter_records_cubature(_Model(), Y, ctrl, x0=np.zeros(3))
    seen = {}
    for name in ("posterior_filter_records_grouped", "filter_records_grouped", "posterior_filter_cubature_records_grouped",
                 "filter_cubature_records_grouped"):
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    m, e = _Model(), _Model(U_collapse=False)
    kw = dict(lengths=[4, 2, 4], smooth=True, records_per_pass=2, Y_train_std=1.7)
    assert DGPSSM.filter_records_cubature(m, Y, ctrl, **kw) == "posterior_filter_cubature_records_grouped"
    assert DGPSSM.filter_records(m, Y, ctrl, **kw) == "posterior_filter_records_grouped"
    (a, k), (b, l) = seen["posterior_filter_cubature_records_grouped"], seen["posterior_filter_records_grouped"]
    assert k == l == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", smooth=True, Y_train_std=1.7, records_per_pass=2, x0s=None)
    assert len(a) == len(b) and all(x is y or np.array_equal(x, y) for x, y in zip(a, b))
    Y1, c1 = Y[:1], ctrl[:1]                                       # R = 1: a single record
    assert DGPSSM.filter_records_cubature(e, Y1, c1, x0=np.arange(2.0)) == "filter_cubature_records_grouped"
    assert DGPSSM.filter_records(e, Y1, c1, x0=np.arange(2.0)) == "filter_records_grouped"
    (a, k), (b, l) = seen["filter_cubature_records_grouped"], seen["filter_records_grouped"]
    assert k == l and a[0] == "Lm" and a[5].shape == (3, 1, 2) and np.array_equal(a[5], b[5]) and a[6] is b[6]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_beside_the_records_ones_and_bound():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, RECORDS):
        assert _declaration(new) == _declaration(old)
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and _lib._SIGNATURES[new][1] == _lib._SIGNATURES[old][1]
        assert new in _lib.exported_symbols()
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")


def test_the_symbols_are_exported():
    for s in SYMBOLS:
        assert hasattr(_lib.load(), s)


def _abi(fused, *, G=2, R=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=3, kind=0, gpp=0, q_mode=0, J=1, rpp=0, null=(), sd=1.0, y=0.0,
         small=False):
    """tests/test_filter_records_args.py's `_abi` on the cubature symbols: one call on zero inputs with every output buffer filled
    with 7; `null`: the arguments passed as NULL; small: the arrays are not sized by R and steps."""
    P = D + C if P is None else P
    n, nm, nr, st, Pp, Jp = max(G, 1), max(n_models, 1), 1 if small else max(R, 1), 1 if small else max(steps, 1), max(P, 1), max(J, 1)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((n, T + 1, D)), cf=np.zeros((max(T, 1), max(C, 1))),
             cr=np.zeros((nr, st, max(C, 1))), lq=np.zeros((n, D)), f=np.zeros((n, M, D)), xl=np.zeros((n, nr, D)), CC=np.ones((D, Jp)),
             DD=np.zeros(Jp), sd=np.full(Jp, sd), Y=np.full((nr, st, Jp), y))
    vec, mat = (n, nr, st, D), (n, nr, st, D, D)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, X_=mat, lpd=(n, nr, st, Jp), lj=(n, nr, st), ms=vec, Ss=mat, ym=(nr, st, Jp), yt=(nr, st, Jp),
                  lm=(nr, st, Jp), lg=(nr, st, Jp), U=(n, M, D))
    outs = {k: np.full(s, 7.0) for k, s in shapes.items()}
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"], rpp) + tuple(p[k] for k in OUT_NAMES)
    if fused:
        rc = lib.ffvd_op_posterior_filter_cubature_records_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T,
                                                                   p["lq"], 1e-5, gpp, q_mode, R, None, None, p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_op_filter_cubature_records_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, q_mode, R, p["xl"],
                                                         None, p["cr"], C, steps, p["lq"], *tail)
    return rc, outs


BAD_ABI = [dict(kind=1), dict(kind=2), dict(D=9, C=0), dict(D=2, C=31), dict(M=2049), dict(M=0), dict(D=0), dict(J=9), dict(J=0), dict(q_mode=2),
           dict(G=3, n_models=2), dict(G=-1), dict(steps=-1), dict(R=-1), dict(rpp=-1), dict(P=2), dict(null=("Z",)), dict(null=("lv",)),
           dict(null=("ll",)), dict(null=("lq",)), dict(null=("cr",)), dict(null=("CC",)), dict(null=("DD",)), dict(null=("sd",)), dict(null=("Y",)),
           dict(null=OUT_NAMES), dict(sd=0.0), dict(sd=np.nan), dict(y=np.inf), dict(y=-np.inf),
           dict(G=2, R=1 << 20, steps=1 << 8, small=True), dict(G=1 << 12, R=1 << 12, steps=1 << 8, D=1, C=0, small=True)]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused):
    rc, outs = _abi(fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_the_messages_say_why():
    lib = _lib.load()
    for fused in (False, True):
        rc, _ = _abi(fused, kind=1)
        msg = lib.ffvd_last_error(None)
        assert rc == E and b"cubature filter of many records" in msg and b"SE kernel only" in msg
        rc, _ = _abi(fused, G=2, R=1 << 20, steps=1 << 8, small=True)
        assert rc == E and b"G * R * steps * D * D < 2^31" in lib.ffvd_last_error(None)
    for ov in (dict(null=("f",)), dict(null=("xl",)), dict(null=("W",))):
        assert _abi(False, **ov)[0] == E
    for ov in (dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))):
        assert _abi(True, **ov)[0] == E


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())
