"""Argument checks of the grouped GP conditionals, without a GPU: conditionals_multi_output.conditional_grouped and
prediction.posterior_conditional_grouped raise ValueError on every shape, count, kernel-kind and q_mode mismatch before the library
is loaded; ffvd_op_conditional_grouped / ffvd_op_posterior_conditional_grouped return FFVD_EINVAL before any device call beyond their
limits and for each required null pointer (and FFVD_OK for G = 0 or N = 0 without touching anything); the symbols are declared,
exported and bound; DGPSSM.predict_transition exists with a keyword-only q_mode."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd.conditionals_multi_output import conditional_grouped
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import posterior_conditional_grouped

E = _lib.FFVD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffvd_op_conditional_grouped", "ffvd_op_posterior_conditional_grouped")


def _kern(D, P):
    return [SquaredExponential(P, variance=0.5, lengthscales=np.full(P, 2.0)) for _ in range(D)]


def _explicit(G=3, n_models=None, M=5, D=2, C=1, N=4, q=True):
    """Arguments of conditional_grouped.  n_models None: one model (an array, one kernel list, one list of D matrices)."""
    P = D + C
    one = n_models is None
    W = [np.eye(M) for _ in range(D)]
    return dict(Lm_inverse_seqs=W if one else [list(W) for _ in range(n_models)],
                Zs=np.zeros((M, P)) if one else [np.zeros((M, P)) for _ in range(n_models)],
                kerns=_kern(D, P) if one else [_kern(D, P) for _ in range(n_models)],
                fs=[np.zeros((M, D)) for _ in range(G)], q_sqrts=[np.zeros((D, M, M)) for _ in range(G)] if q else None,
                Xnew=np.zeros((N, P)))


def _fused(G=3, n_models=None, M=5, D=2, C=1, T=6, N=4):
    P = D + C
    one = n_models is None
    return dict(Zs=np.zeros((M, P)) if one else [np.zeros((M, P)) for _ in range(n_models)],
                kerns=_kern(D, P) if one else [_kern(D, P) for _ in range(n_models)], Xs=[np.zeros((T + 1, D)) for _ in range(G)],
                Qs=[np.ones(D) for _ in range(G)], control_inputs=np.zeros((T, C)), Xnew=np.zeros((N, P)))


def _with(base, **kw):
    a = dict(base)
    a.update(kw)
    return a


def _mixed(make):
    a = make(n_models=3)
    a["kerns"][1] = [LinearK(3, variance=0.1) for _ in range(2)]
    return a


# mismatches both interfaces share
COMMON = {
    "Xnew with the wrong column count": lambda mk: _with(mk(), Xnew=np.zeros((4, 2))),
    "Xnew with one axis": lambda mk: _with(mk(), Xnew=np.zeros(3)),
    "unknown q_mode": lambda mk: _with(mk(), q_mode="slice0"),
    "n_models neither 1 nor G": lambda mk: mk(G=3, n_models=2),
    "mixed kernel kinds": _mixed,
    "mixed D (kernels)": lambda mk: _with(mk(n_models=3), kerns=mk(n_models=3)["kerns"][:2] + [_kern(3, 3)]),
    "mixed M (Z)": lambda mk: _with(mk(n_models=3), Zs=mk(n_models=3)["Zs"][:2] + [np.zeros((6, 3))]),
    "one kernel list with a stack of Z": lambda mk: _with(mk(), Zs=np.zeros((3, 5, 3))),
    "negative rows_per_pass": lambda mk: _with(mk(), rows_per_pass=-1),
    "nothing asked for": lambda mk: _with(mk(), per_group=False, summary=False),
}
BAD_EXPLICIT = {
    "fs of another G (one model per group)": lambda: _with(_explicit(n_models=3), fs=_explicit()["fs"][:2], q_sqrts=None),
    "no groups": lambda: _with(_explicit(), fs=[], q_sqrts=None),
    "fs of another M": lambda: _with(_explicit(), fs=_explicit()["fs"][:2] + [np.zeros((6, 2))]),
    "fs of another D": lambda: _with(_explicit(), fs=_explicit()["fs"][:2] + [np.zeros((5, 3))]),
    "q_sqrts of another G": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2]),
    "a q_sqrts entry of the wrong shape": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2] + [np.zeros((2, 5, 4))]),
    "a q_sqrts entry that is one matrix": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2] + [np.zeros((5, 5))]),
    "too few L^-T matrices": lambda: _with(_explicit(), Lm_inverse_seqs=[np.eye(5)]),
    "an L^-T matrix of another M": lambda: _with(_explicit(), Lm_inverse_seqs=[np.eye(5), np.eye(4)]),
    "Lm_inverse_seqs and kerns of different counts": lambda: _with(_explicit(n_models=3), Lm_inverse_seqs=_explicit(n_models=3)["Lm_inverse_seqs"][:2]),
}
BAD_FUSED = {
    "one X of another T": lambda: _with(_fused(), Xs=_fused()["Xs"][:2] + [np.zeros((8, 2))]),
    "Q of another D": lambda: _with(_fused(), Qs=[np.ones(2), np.ones(3), np.ones(2)]),
    "too few control rows": lambda: _with(_fused(), control_inputs=np.zeros((5, 1))),
    "negative groups_per_pass": lambda: _with(_fused(), groups_per_pass=-1),
}


@pytest.fixture
def no_device(monkeypatch):
    def fail():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", fail)


@pytest.mark.parametrize("what", sorted(COMMON) + sorted(BAD_EXPLICIT))
def test_explicit_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_explicit) if what in COMMON else BAD_EXPLICIT[what]()
    with pytest.raises(ValueError):
        conditional_grouped(**a)


@pytest.mark.parametrize("what", sorted(COMMON) + sorted(BAD_FUSED))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_fused) if what in COMMON else BAD_FUSED[what]()
    with pytest.raises(ValueError):
        posterior_conditional_grouped(**a)


def test_well_formed_arguments_reach_the_library(monkeypatch):
    """The other half of the tests above: what they reject is not everything."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    for kw in (dict(), dict(n_models=3), dict(n_models=1, G=1), dict(C=0), dict(N=0)):
        for mode in ("reference", "intent"):
            with pytest.raises(Reached):
                conditional_grouped(q_mode=mode, **_explicit(**kw))
            with pytest.raises(Reached):
                posterior_conditional_grouped(q_mode=mode, **_fused(**kw))
    with pytest.raises(Reached):
        conditional_grouped(**_explicit(q=False), per_group=False)


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, P=None, T=5, N=3, kind=0, gpp=0, q_mode=0, rpp=0, null=(), q=True):
    """One ABI call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL."""
    P = D + C if P is None else P
    n, nm, Np, Pp = max(G, 1), max(n_models, 1), max(N, 1), max(P, 1)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((n, T + 1, D)),
             cf=np.zeros((max(T, 1), max(C, 1))), lq=np.zeros((n, D)), f=np.zeros((n, M, D)), Xnew=np.zeros((Np, Pp)))
    outs = dict(mean=np.full((n, Np, D), 7.0), var=np.full((n, Np, D), 7.0), mm=np.full((Np, D), 7.0), mv=np.full((Np, D), 7.0),
                U=np.full((n, M, D), 7.0))
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    if fused:
        rc = lib.ffvd_op_posterior_conditional_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                       1e-5, gpp, q_mode, p["Xnew"], N, rpp, p["mean"], p["var"], p["mm"], p["mv"], p["U"])
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        qm = [np.zeros((M, M)) for _ in range(n * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[None if "W0" in null and i == 1 else w.ctypes.data for i, w in enumerate(Wm)])
        qt = None if not q else (ctypes.c_void_p * len(qm))(*[None if "q0" in null and i == 1 else x.ctypes.data for i, x in enumerate(qm)])
        rc = lib.ffvd_op_conditional_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], qt, q_mode, p["Xnew"], N, rpp,
                                             p["mean"], p["var"], p["mm"], p["mv"])
    return rc, outs


# beyond a limit, or a required pointer missing: shared by the two entry points
BAD_ABI = [dict(M=2049), dict(M=0), dict(D=0), dict(D=2, C=31), dict(G=3, n_models=2), dict(G=-1), dict(kind=2), dict(N=-1),
           dict(q_mode=2), dict(q_mode=-1), dict(rpp=-1), dict(null=("Z",)), dict(null=("lv",)), dict(null=("ll",)), dict(null=("Xnew",)),
           dict(null=("mean", "var", "mm", "mv")), dict(null=("mm",)), dict(null=("mv",))]


@pytest.mark.parametrize("ov", BAD_ABI + [dict(P=1), dict(null=("f",)), dict(null=("W",)), dict(null=("W0",)), dict(null=("q0",))], ids=str)
def test_explicit_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(False, **ov)
    assert rc == E, rc
    assert b"ffvd_op_conditional_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", BAD_ABI + [dict(P=2), dict(P=4), dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",)),
                                          dict(null=("lq",))], ids=str)
def test_fused_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(True, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_conditional_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_abi_rejects_stacks_beyond_the_limits():
    """G * D * Mp^2 > 2^29 doubles, G * D > 2^24 and G * N * D >= 2^31: rejected on the scalar arguments alone (no array is read before
    the check)."""
    lib = _lib.load()
    z = np.zeros(1)
    p = _lib.dptr(z)
    t = (ctypes.c_void_p * 1)(z.ctypes.data)
    for G, M, D, N in ((129, 1024, 4, 1), (33, 2048, 4, 1), ((1 << 24) + 1, 1, 1, 1), (2, 1, 1, 1 << 30)):
        rc = lib.ffvd_op_conditional_grouped(0, G, 1, t, p, M, D, D, p, p, p, None, 0, p, N, 0, p, p, None, None)
        assert rc == E, (G, M, D, N, rc)
        assert b"ffvd_op_conditional_grouped: bad argument" in lib.ffvd_last_error(None)
        rc = lib.ffvd_op_posterior_conditional_grouped(0, G, 1, p, M, D, D, p, p, p, None, 0, 4, p, 1e-5, 0, 0, p, N, 0, p, p, None, None, None)
        assert rc == E, (G, M, D, N, rc)
        assert b"ffvd_op_posterior_conditional_grouped: bad argument" in lib.ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(G=0, n_models=0), dict(N=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_rows(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.exported_symbols()
        assert hasattr(_lib.load(), name)


def test_predict_transition_exists_with_a_keyword_only_q_mode():
    from ffvd_amd.dgp_model import DGPSSM
    sig = inspect.signature(DGPSSM.predict_transition).parameters
    assert sig["q_mode"].kind is inspect.Parameter.KEYWORD_ONLY and sig["q_mode"].default == "reference"
    assert sig["per_chain"].kind is inspect.Parameter.KEYWORD_ONLY and sig["per_chain"].default is True
    doc = DGPSSM.predict_transition.__doc__
    assert "x_next" in doc and "NOT y" in doc

    class Stub:
        _host_stale = False

    with pytest.raises(ValueError, match="q_mode"):             # stopped before any parameter or device is touched
        DGPSSM.predict_transition(Stub(), np.zeros((2, 3)), q_mode="slice0")
