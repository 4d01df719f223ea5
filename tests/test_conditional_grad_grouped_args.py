"""Argument checks of the linearisation, without a GPU: conditionals_multi_output.conditional_grad_grouped and
prediction.posterior_conditional_grad_grouped raise ValueError on every shape, count, kernel-kind and q_mode mismatch -- LinearK among
them -- before the library is loaded; ffvd_op_conditional_grad_grouped / ffvd_op_posterior_conditional_grad_grouped return FFVD_EINVAL
before any device call for LinearK, beyond their limits (G * D * N * P >= 2^31 among them) and for inconsistent outputs, and FFVD_OK
for G = 0 or N = 0 without touching anything; the symbols are declared, exported and bound; DGPSSM.linearize exists and says what
its A is."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd.conditionals_multi_output import GRAD_KEYS, conditional_grad_grouped
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import posterior_conditional_grad_grouped

E = _lib.FFVD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffvd_op_conditional_grad_grouped", "ffvd_op_posterior_conditional_grad_grouped")


def _kern(D, P, linear=False):
    if linear:
        return [LinearK(P, variance=0.1) for _ in range(D)]
    return [SquaredExponential(P, variance=0.5, lengthscales=np.full(P, 2.0)) for _ in range(D)]


def _explicit(G=3, n_models=None, M=5, D=2, C=1, N=4, q=True, linear=False):
    """Arguments of conditional_grad_grouped.  n_models None: one model (an array, one kernel list, one list of D matrices)."""
    P = D + C
    one = n_models is None
    W = [np.eye(M) for _ in range(D)]
    return dict(Lm_inverse_seqs=W if one else [list(W) for _ in range(n_models)],
                Zs=np.zeros((M, P)) if one else [np.zeros((M, P)) for _ in range(n_models)],
                kerns=_kern(D, P, linear) if one else [_kern(D, P, linear) for _ in range(n_models)],
                fs=[np.zeros((M, D)) for _ in range(G)], q_sqrts=[np.zeros((D, M, M)) for _ in range(G)] if q else None,
                Xnew=np.zeros((N, P)))


def _fused(G=3, n_models=None, M=5, D=2, C=1, T=6, N=4, linear=False):
    P = D + C
    one = n_models is None
    return dict(Zs=np.zeros((M, P)) if one else [np.zeros((M, P)) for _ in range(n_models)],
                kerns=_kern(D, P, linear) if one else [_kern(D, P, linear) for _ in range(n_models)],
                Xs=[np.zeros((T + 1, D)) for _ in range(G)], Qs=[np.ones(D) for _ in range(G)], control_inputs=np.zeros((T, C)),
                Xnew=np.zeros((N, P)))


def _with(base, **kw):
    a = dict(base)
    a.update(kw)
    return a


COMMON = {
    "Xnew with the wrong column count": lambda mk: _with(mk(), Xnew=np.zeros((4, 2))),
    "Xnew with one axis": lambda mk: _with(mk(), Xnew=np.zeros(3)),
    "unknown q_mode": lambda mk: _with(mk(), q_mode="slice0"),
    "n_models neither 1 nor G": lambda mk: mk(G=3, n_models=2),
    "LinearK": lambda mk: mk(linear=True),
    "LinearK, one model per group": lambda mk: mk(n_models=3, linear=True),
    "mixed M (Z)": lambda mk: _with(mk(n_models=3), Zs=mk(n_models=3)["Zs"][:2] + [np.zeros((6, 3))]),
    "negative rows_per_pass": lambda mk: _with(mk(), rows_per_pass=-1),
    "per_group=False with summary=False": lambda mk: _with(mk(), per_group=False, summary=False),
}
BAD_EXPLICIT = {
    "no groups": lambda: _with(_explicit(), fs=[], q_sqrts=None),
    "fs of another M": lambda: _with(_explicit(), fs=_explicit()["fs"][:2] + [np.zeros((6, 2))]),
    "q_sqrts of another G": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2]),
    "a q_sqrts entry of the wrong shape": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2] + [np.zeros((2, 5, 4))]),
    "too few L^-T matrices": lambda: _with(_explicit(), Lm_inverse_seqs=[np.eye(5)]),
}
BAD_FUSED = {
    "one X of another T": lambda: _with(_fused(), Xs=_fused()["Xs"][:2] + [np.zeros((8, 2))]),
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
        conditional_grad_grouped(**a)


@pytest.mark.parametrize("what", sorted(COMMON) + sorted(BAD_FUSED))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_fused) if what in COMMON else BAD_FUSED[what]()
    with pytest.raises(ValueError):
        posterior_conditional_grad_grouped(**a)


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
                conditional_grad_grouped(q_mode=mode, **_explicit(**kw))
            with pytest.raises(Reached):
                posterior_conditional_grad_grouped(q_mode=mode, **_fused(**kw))
    with pytest.raises(Reached):
        conditional_grad_grouped(**_explicit(q=False), per_group=False, variance=False)


OUT_KEYS = ("mean", "var", "dmean", "dvar", "mm", "mv", "mdm", "mdv")


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, T=5, N=3, kind=0, q_mode=0, rpp=0, null=()):
    """One ABI call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL."""
    P = D + C
    n, nm, Np = max(G, 1), max(n_models, 1), max(N, 1)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, P)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, P)), X=np.zeros((n, T + 1, D)), cf=np.zeros((T, max(C, 1))),
             lq=np.zeros((n, D)), f=np.zeros((n, M, D)), Xnew=np.zeros((Np, P)))
    outs = dict(mean=np.full((n, Np, D), 7.0), var=np.full((n, Np, D), 7.0), dmean=np.full((n, Np, D, P), 7.0),
                dvar=np.full((n, Np, D, P), 7.0), mm=np.full((Np, D), 7.0), mv=np.full((Np, D), 7.0), mdm=np.full((Np, D, P), 7.0),
                mdv=np.full((Np, D, P), 7.0), U=np.full((n, M, D), 7.0))
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    o = [p[k] for k in OUT_KEYS]
    if fused:
        rc = lib.ffvd_op_posterior_conditional_grad_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T,
                                                            p["lq"], 1e-5, 0, q_mode, p["Xnew"], N, rpp, *o, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_op_conditional_grad_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, q_mode, p["Xnew"],
                                                  N, rpp, *o)
    return rc, outs


# LinearK, beyond a limit, a required pointer missing, or outputs that do not go together
BAD_ABI = [dict(kind=1), dict(kind=2), dict(M=2049), dict(M=0), dict(D=0), dict(D=2, C=31), dict(G=3, n_models=2), dict(G=-1), dict(N=-1),
           dict(q_mode=2), dict(rpp=-1), dict(null=("Z",)), dict(null=("lv",)), dict(null=("ll",)), dict(null=("Xnew",)),
           dict(null=OUT_KEYS), dict(null=("mm",)), dict(null=("mv",)), dict(null=("mm", "mv")), dict(null=("mm", "mv", "mdv"))]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == E, rc
    name = SYMBOLS[1] if fused else SYMBOLS[0]
    msg = _lib.load().ffvd_last_error(None)
    assert (name + ": bad argument").encode() in msg
    if ov.get("kind") == 1:
        assert b"SE kernel only" in msg
    assert all(np.all(v == 7.0) for v in outs.values())


def test_abi_rejects_stacks_beyond_the_limits():
    """G * D * N * P >= 2^31 (with G * N * D below its own limit) and ffvd_op_conditional_grouped's limits: rejected on the scalar
    arguments alone (no array is read before the check)."""
    lib = _lib.load()
    z = np.zeros(1)
    p = _lib.dptr(z)
    t = (ctypes.c_void_p * 1)(z.ctypes.data)
    for G, M, D, P, N in ((2, 1, 1, 2, 1 << 29), (1, 1, 2, 32, 1 << 25), (129, 1024, 4, 4, 1), ((1 << 24) + 1, 1, 1, 1, 1), (2, 1, 1, 1, 1 << 30)):
        rc = lib.ffvd_op_conditional_grad_grouped(0, G, 1, t, p, M, P, D, p, p, p, None, 0, p, N, 0, p, p, p, p, None, None, None, None)
        assert rc == E, (G, M, D, P, N, rc)
        assert b"ffvd_op_conditional_grad_grouped: bad argument" in lib.ffvd_last_error(None)
        rc = lib.ffvd_op_posterior_conditional_grad_grouped(0, G, 1, p, M, P, D, p, p, p, p, P - D, 4, p, 1e-5, 0, 0, p, N, 0, p, p, p, p,
                                                            None, None, None, None, None)
        assert rc == E, (G, M, D, P, N, rc)
        assert b"ffvd_op_posterior_conditional_grad_grouped: bad argument" in lib.ffvd_last_error(None)


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
    assert GRAD_KEYS == ("mean", "var", "dmean", "dvar", "mix_mean", "mix_var", "mix_dmean", "mix_dvar")


def test_linearize_exists_and_says_what_its_jacobian_is():
    from ffvd_amd.dgp_model import DGPSSM
    sig = inspect.signature(DGPSSM.linearize).parameters
    assert sig["q_mode"].kind is inspect.Parameter.KEYWORD_ONLY and sig["q_mode"].default == "reference"
    assert sig["per_chain"].kind is inspect.Parameter.KEYWORD_ONLY and sig["per_chain"].default is True
    doc = DGPSSM.linearize.__doc__
    assert "x + f(x, c)" in doc and "not" in doc and "of f" in doc

    class Stub:
        _host_stale = False

    with pytest.raises(ValueError, match="q_mode"):             # stopped before any parameter or device is touched
        DGPSSM.linearize(Stub(), np.zeros((2, 3)), q_mode="slice0")
