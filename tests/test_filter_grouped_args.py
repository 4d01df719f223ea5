"""Argument checks of the filter, without a GPU: prediction.filter_grouped / posterior_filter_grouped raise ValueError on every shape,
count, kernel-kind, limit and q_mode mismatch, on an infinite observation and on J > 8 before the library is loaded (the mismatches
of tests/test_moment_grouped_args.py, imported, plus those of the observations, the emission and the start); ffvd_op_filter_grouped /
ffvd_op_posterior_filter_grouped return FFVD_EINVAL before any device call beyond their limits and for each required null pointer
(and FFVD_OK for G = 0 or steps = 0 without touching anything); DGPSSM.filter_heldout exists with the documented defaults."""
import ctypes
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_moment_grouped_args import BAD_EXPLICIT, BAD_FUSED, COMMON, _explicit, _fused, _with

E = _lib.FFVD_EINVAL
EMISSION = dict(CC=np.ones((2, 1)), DD=np.zeros(1), log_Rchols=np.zeros((1, 1)))
SKIP = {"negative steps"}                        # (steps is len(Y_obs) here)


def _filter_args(a, explicit, J=1):
    """moment_grouped's keyword arguments -> filter_grouped's: Y_obs (steps, J) for steps, x0s for x_lasts"""
    a = dict(a)
    steps = a.pop("steps")
    if explicit:
        a["x0s"] = a.pop("x_lasts")
    a["Y_obs"] = np.zeros((steps, J))
    return a


@pytest.fixture
def no_device(monkeypatch):
    def fail():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", fail)


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP) + sorted(BAD_EXPLICIT))
def test_explicit_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_explicit) if what in COMMON else BAD_EXPLICIT[what]()
    with pytest.raises(ValueError):
        pr.filter_grouped(**_filter_args(a, True), **EMISSION)


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP) + sorted(BAD_FUSED))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_fused) if what in COMMON else BAD_FUSED[what]()
    with pytest.raises(ValueError):
        pr.posterior_filter_grouped(**_filter_args(a, False), **EMISSION)


BAD_FILTER = {
    "CC of another D": dict(CC=np.ones((3, 1))),
    "J = 9": dict(CC=np.ones((2, 9)), DD=np.zeros(9), log_Rchols=np.zeros((9, 9)), Y_obs=np.zeros((4, 9))),
    "DD of another J": dict(DD=np.zeros(2)),
    "log_Rchols of another J": dict(log_Rchols=np.zeros((2, 2))),
    "a noise deviation that is not finite": dict(log_Rchols=np.full((1, 1), np.inf)),
    "observations of another J": dict(Y_obs=np.zeros((4, 2))),
    "observations with three axes": dict(Y_obs=np.zeros((4, 1, 1))),
    "a scalar observation": dict(Y_obs=0.5),
    "an infinite observation": dict(Y_obs=np.array([[0.0], [np.inf], [0.0], [np.nan]])),
    "a minus-infinite observation": dict(Y_obs=np.array([[0.0], [0.0], [-np.inf], [0.0]])),
    "too few control rows for the observations": dict(Y_obs=np.zeros((5, 1))),
    "unknown q_mode": dict(q_mode="slice0"),
}


@pytest.mark.parametrize("what", sorted(BAD_FILTER))
def test_observations_and_emission_are_checked_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        a = _with(_with(_filter_args(make(), explicit), **EMISSION), **BAD_FILTER[what])
        with pytest.raises(ValueError):
            (pr.filter_grouped if explicit else pr.posterior_filter_grouped)(**a)


def test_the_start_is_checked_before_the_library_is_loaded(no_device):
    a = _with(_filter_args(_fused(), False), **EMISSION)
    for x0s in (np.zeros((2, 2)), np.zeros((3, 3)), np.zeros(2)):
        with pytest.raises(ValueError):
            pr.posterior_filter_grouped(**a, x0s=x0s)
    b = _with(_filter_args(_explicit(), True), **EMISSION)
    for x0s in ([np.zeros(2)] * 2, [np.zeros(2), np.zeros(2), np.zeros(3)]):
        with pytest.raises(ValueError):
            pr.filter_grouped(**_with(b, x0s=x0s))


def test_well_formed_arguments_reach_the_library(monkeypatch):
    """The other half of the tests above: what they reject is not everything (NaN observations and empty records included)."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    S0 = np.tile(np.array([[1.0, 0.5], [0.5, 1.0]]), (3, 1, 1))
    for kw in (dict(), dict(n_models=3), dict(n_models=1, G=1), dict(C=0), dict(steps=0)):
        for mode in ("reference", "intent"):
            for smooth in (False, True):
                with pytest.raises(Reached):
                    pr.filter_grouped(q_mode=mode, smooth=smooth, **_filter_args(_explicit(**kw), True), **EMISSION)
                with pytest.raises(Reached):
                    pr.posterior_filter_grouped(q_mode=mode, smooth=smooth, **_filter_args(_fused(**kw), False), **EMISSION)
    Y = np.array([[0.1, np.nan], [np.nan, np.nan], [0.3, 0.2], [np.nan, -1.0]])
    em = dict(CC=np.ones((2, 2)), DD=np.zeros(2), log_Rchols=np.zeros(2))
    with pytest.raises(Reached):
        pr.filter_grouped(**_with(_filter_args(_explicit(q=False), True), Y_obs=Y), **em, S0s=S0)
    with pytest.raises(Reached):
        pr.posterior_filter_grouped(**_with(_filter_args(_fused(), False), Y_obs=Y), **em, S0s=S0, x0s=np.zeros((3, 2)))
    with pytest.raises(Reached):
        pr.filter_grouped(**_with(_filter_args(_explicit(), True), Y_obs=np.zeros(4)), **EMISSION)          # (steps,) is (steps, 1)


OUT_NAMES = ("mp", "Sp", "mf", "Sf", "X", "lpd", "lj", "ms", "Ss", "ym", "yt", "lm", "lg")


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=3, kind=0, gpp=0, q_mode=0, J=1, null=(), q=True, sd=1.0, y=0.0):
    """One ABI call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL."""
    P = D + C if P is None else P
    n, nm, st, Pp, Jp = max(G, 1), max(n_models, 1), max(steps, 1), max(P, 1), max(J, 1)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((n, T + 1, D)),
             cf=np.zeros((max(T, 1), max(C, 1))), cr=np.zeros((st, max(C, 1))), lq=np.zeros((n, D)), f=np.zeros((n, M, D)),
             xl=np.zeros((n, D)), CC=np.ones((D, Jp)), DD=np.zeros(Jp), sd=np.full(Jp, sd), Y=np.full((st, Jp), y))
    vec, mat = (n, st, D), (n, st, D, D)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, X_=mat, lpd=(n, st, Jp), lj=(n, st), ms=vec, Ss=mat, ym=(st, Jp), yt=(st, Jp), lm=(st, Jp),
                  lg=(st, Jp), U=(n, M, D))
    outs = {k: np.full(s, 7.0) for k, s in shapes.items()}
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"]) + tuple(p["X_" if k == "X" else k] for k in OUT_NAMES)
    if fused:
        rc = lib.ffvd_op_posterior_filter_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                  1e-5, gpp, q_mode, None, None, p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        qm = [np.zeros((M, M)) for _ in range(n * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[None if "W0" in null and i == 1 else w.ctypes.data for i, w in enumerate(Wm)])
        qt = None if not q else (ctypes.c_void_p * len(qm))(*[None if "q0" in null and i == 1 else x.ctypes.data for i, x in enumerate(qm)])
        rc = lib.ffvd_op_filter_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], qt, q_mode, p["xl"], None,
                                        p["cr"], C, steps, p["lq"], *tail)
    return rc, outs


ALL_OUTPUTS = ("mp", "Sp", "mf", "Sf", "X_", "lpd", "lj", "ms", "Ss", "ym", "yt", "lm", "lg")
BAD_ABI = [dict(kind=1), dict(kind=2), dict(D=9, C=0), dict(D=2, C=31), dict(M=2049), dict(M=0), dict(D=0), dict(J=9), dict(J=0), dict(J=-1),
           dict(q_mode=2), dict(q_mode=-1), dict(G=3, n_models=2), dict(G=-1), dict(steps=-1), dict(P=2), dict(P=4), dict(null=("Z",)),
           dict(null=("lv",)), dict(null=("ll",)), dict(null=("lq",)), dict(null=("cr",)), dict(null=("CC",)), dict(null=("DD",)),
           dict(null=("sd",)), dict(null=("Y",)), dict(null=ALL_OUTPUTS), dict(sd=0.0), dict(sd=np.nan), dict(y=np.inf), dict(y=-np.inf)]


@pytest.mark.parametrize("ov", BAD_ABI + [dict(null=("f",)), dict(null=("xl",)), dict(null=("W",)), dict(null=("W0",)), dict(null=("q0",))],
                         ids=str)
def test_explicit_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(False, **ov)
    assert rc == E, rc
    assert b"ffvd_op_filter_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", BAD_ABI + [dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))], ids=str)
def test_fused_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(True, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_filter_grouped: bad argument" in _lib.load().ffvd_last_error(None)
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


def test_filter_heldout_is_there_with_the_documented_defaults():
    from ffvd_amd.dgp_model import DGPSSM
    sig = inspect.signature(DGPSSM.filter_heldout).parameters
    assert list(sig) == ["self", "Y_test", "control_inputs", "x0", "S0", "smooth", "q_mode", "Y_train_std"]
    assert sig["control_inputs"].default is None and sig["x0"].default is None and sig["S0"].default is None
    assert sig["smooth"].default is False and sig["q_mode"].default == "reference" and sig["Y_train_std"].default == 1.0
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("x0", "S0", "smooth", "q_mode", "Y_train_std"))

    class Stub:
        _host_stale = False
        Y = np.zeros((4, 1))

    with pytest.raises(ValueError, match="q_mode"):              # stopped before any parameter or device is touched
        DGPSSM.filter_heldout(Stub(), np.zeros((2, 1)), q_mode="slice0")
    with pytest.raises(ValueError, match="Y_test"):
        DGPSSM.filter_heldout(Stub(), np.zeros((2, 3)))
    for f in (pr.filter_grouped, pr.posterior_filter_grouped):
        sig = inspect.signature(f).parameters
        assert sig["S0s"].default is None and sig["q_mode"].default == "reference" and sig["smooth"].default is False
    assert "not re-weighted" in pr.filter_grouped.__doc__
