"""Argument checks of the moment-matched prediction, without a GPU: prediction.moment_grouped / posterior_moment_grouped /
moment_summary (and the _summary forms) raise ValueError on every shape, count, kernel-kind, limit and q_mode mismatch before the
library is loaded; ffvd_op_moment_grouped / ffvd_op_posterior_moment_grouped / ffvd_op_moment_summary return FFVD_EINVAL before any
device call beyond their limits and for each required null pointer (and FFVD_OK for G = 0 or steps = 0 without touching anything);
the symbols are declared, exported and bound; DGPSSM.predict_moments, evaluate_heldout(method=) and fit(eval_method=) exist with
defaults that keep today's behaviour."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from ffvd_amd.kernels import LinearK, SquaredExponential

E = _lib.FFVD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffvd_op_moment_grouped", "ffvd_op_posterior_moment_grouped", "ffvd_op_moment_summary")


def _kern(D, P):
    return [SquaredExponential(P, variance=0.5, lengthscales=np.full(P, 2.0)) for _ in range(D)]


def _explicit(G=3, n_models=None, M=5, D=2, C=1, steps=4, q=True):
    """Arguments of moment_grouped.  n_models None: one model (an array, one kernel list, one list of D matrices)."""
    P = D + C
    one = n_models is None
    W = [np.eye(M) for _ in range(D)]
    return dict(Lm_inverse_seqs=W if one else [list(W) for _ in range(n_models)],
                Zs=np.zeros((M, P)) if one else [np.zeros((M, P)) for _ in range(n_models)],
                kerns=_kern(D, P) if one else [_kern(D, P) for _ in range(n_models)],
                U_vals=[np.zeros((M, D)) for _ in range(G)], q_sqrts=[np.zeros((D, M, M)) for _ in range(G)] if q else None,
                x_lasts=[np.zeros(D) for _ in range(G)], control_inputs=np.zeros((10 + steps, C)), ctrl_offset=10, steps=steps,
                Qs=[np.ones(D) for _ in range(G)])


def _fused(G=3, n_models=None, M=5, D=2, C=1, T=6, steps=4):
    P = D + C
    one = n_models is None
    return dict(Zs=np.zeros((M, P)) if one else [np.zeros((M, P)) for _ in range(n_models)],
                kerns=_kern(D, P) if one else [_kern(D, P) for _ in range(n_models)], Xs=[np.zeros((T + 1, D)) for _ in range(G)],
                Qs=[np.ones(D) for _ in range(G)], control_inputs=np.zeros((T + steps, C)), ctrl_offset=T, steps=steps)


def _with(base, **kw):
    a = dict(base)
    a.update(kw)
    return a


def _mixed(make):
    a = make(n_models=3)
    a["kerns"][1] = [LinearK(3, variance=0.1) for _ in range(2)]
    return a


def _linear(make):
    a = make()
    a["kerns"] = [LinearK(3, variance=0.1) for _ in range(2)]
    return a


# mismatches both interfaces share
COMMON = {
    "LinearK": _linear,
    "mixed kernel kinds": _mixed,
    "unknown q_mode": lambda mk: _with(mk(), q_mode="slice0"),
    "n_models neither 1 nor G": lambda mk: mk(G=3, n_models=2),
    "D = 9": lambda mk: mk(D=9),
    "P = 33": lambda mk: mk(D=2, C=31),
    "M = 2049": lambda mk: mk(M=2049, **(dict(q=False) if mk is _explicit else {})),
    "mixed D (kernels)": lambda mk: _with(mk(n_models=3), kerns=mk(n_models=3)["kerns"][:2] + [_kern(3, 3)]),
    "mixed M (Z)": lambda mk: _with(mk(n_models=3), Zs=mk(n_models=3)["Zs"][:2] + [np.zeros((6, 3))]),
    "one kernel list with a stack of Z": lambda mk: _with(mk(), Zs=np.zeros((3, 5, 3))),
    "negative steps": lambda mk: _with(mk(), steps=-1),
    "negative ctrl_offset": lambda mk: _with(mk(), ctrl_offset=-1),
    "too few control rows for the steps": lambda mk: _with(mk(), control_inputs=np.zeros((8, 1))),
    "control inputs of another width": lambda mk: _with(mk(), control_inputs=np.zeros((20, 2))),
    "S0s of another G": lambda mk: _with(mk(), S0s=np.zeros((2, 2, 2))),
    "S0s of another D": lambda mk: _with(mk(), S0s=np.zeros((3, 3, 3))),
    "an S0 that is not symmetric": lambda mk: _with(mk(), S0s=np.tile(np.array([[1.0, 0.5], [0.4, 1.0]]), (3, 1, 1))),
    "an S0 that is not finite": lambda mk: _with(mk(), S0s=np.full((3, 2, 2), np.nan)),
    "Q of another D": lambda mk: _with(mk(), Qs=[np.ones(2), np.ones(3), np.ones(2)]),
}
BAD_EXPLICIT = {
    "no groups": lambda: _with(_explicit(), U_vals=[], q_sqrts=None, x_lasts=[]),
    "U_vals of another G (one model per group)": lambda: _with(_explicit(n_models=3), U_vals=_explicit()["U_vals"][:2], q_sqrts=None),
    "U_vals of another M": lambda: _with(_explicit(), U_vals=_explicit()["U_vals"][:2] + [np.zeros((6, 2))]),
    "U_vals of another D": lambda: _with(_explicit(), U_vals=_explicit()["U_vals"][:2] + [np.zeros((5, 3))]),
    "x_lasts of another G": lambda: _with(_explicit(), x_lasts=_explicit()["x_lasts"][:2]),
    "an x_last of another D": lambda: _with(_explicit(), x_lasts=_explicit()["x_lasts"][:2] + [np.zeros(3)]),
    "q_sqrts of another G": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2]),
    "a q_sqrts entry of the wrong shape": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2] + [np.zeros((2, 5, 4))]),
    "a q_sqrts entry that is one matrix": lambda: _with(_explicit(), q_sqrts=_explicit()["q_sqrts"][:2] + [np.zeros((5, 5))]),
    "too few L^-T matrices": lambda: _with(_explicit(), Lm_inverse_seqs=[np.eye(5)]),
    "an L^-T matrix of another M": lambda: _with(_explicit(), Lm_inverse_seqs=[np.eye(5), np.eye(4)]),
    "Lm_inverse_seqs and kerns of different counts": lambda: _with(_explicit(n_models=3), Lm_inverse_seqs=_explicit(n_models=3)["Lm_inverse_seqs"][:2]),
}
BAD_FUSED = {
    "one X of another T": lambda: _with(_fused(), Xs=_fused()["Xs"][:2] + [np.zeros((8, 2))]),
    "negative groups_per_pass": lambda: _with(_fused(), groups_per_pass=-1),
}
EMISSION = dict(CC=np.ones((2, 1)), DD=np.zeros(1), log_Rchols=np.zeros((1, 1)))
BAD_SUMMARY = {
    "CC of another D": dict(CC=np.ones((3, 1))),
    "J = 9": dict(CC=np.ones((2, 9)), DD=np.zeros(9), log_Rchols=np.zeros((9, 9))),
    "DD of another J": dict(DD=np.zeros(2)),
    "log_Rchols of another J": dict(log_Rchols=np.zeros((2, 2))),
    "more held-out rows than steps": dict(Y_test=np.zeros((5, 1))),
    "held-out data of another J": dict(Y_test=np.zeros((2, 2))),
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
        pr.moment_grouped(**a)
    with pytest.raises(ValueError):
        pr.moment_grouped_summary(**a, **EMISSION)


@pytest.mark.parametrize("what", sorted(COMMON) + sorted(BAD_FUSED))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_fused) if what in COMMON else BAD_FUSED[what]()
    with pytest.raises(ValueError):
        pr.posterior_moment_grouped(**a)
    with pytest.raises(ValueError):
        pr.posterior_moment_grouped_summary(**a, **EMISSION)


@pytest.mark.parametrize("what", sorted(BAD_SUMMARY))
def test_summaries_reject_mismatches_before_the_library_is_loaded(what, no_device):
    em = _with(EMISSION, **BAD_SUMMARY[what])
    with pytest.raises(ValueError):
        pr.moment_summary(np.zeros((3, 4, 2)), np.zeros((3, 4, 2, 2)), **em)
    with pytest.raises(ValueError):
        pr.moment_grouped_summary(**_explicit(), **em)
    with pytest.raises(ValueError):
        pr.posterior_moment_grouped_summary(**_fused(), **em)


@pytest.mark.parametrize("m,S", [((3, 4, 2), (3, 4, 2, 3)), ((3, 4, 2), (3, 4, 2)), ((4, 2), (4, 2, 2)), ((3, 4, 9), (3, 4, 9, 9)),
                                 ((0, 4, 2), (0, 4, 2, 2)), ((3, 0, 2), (3, 0, 2, 2))], ids=str)
def test_moment_summary_rejects_stacks_of_the_wrong_shape(m, S, no_device):
    with pytest.raises(ValueError):
        pr.moment_summary(np.zeros(m), np.zeros(S), np.ones((m[-1], 1)), np.zeros(1), np.zeros((1, 1)))


def test_well_formed_arguments_reach_the_library(monkeypatch):
    """The other half of the tests above: what they reject is not everything."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    S0 = np.tile(np.array([[1.0, 0.5], [0.5, 1.0]]), (3, 1, 1))
    for kw in (dict(), dict(n_models=3), dict(n_models=1, G=1), dict(C=0), dict(steps=0), dict(D=8, C=24)):
        for mode in ("reference", "intent"):
            with pytest.raises(Reached):
                pr.moment_grouped(q_mode=mode, **_explicit(**kw))
            with pytest.raises(Reached):
                pr.posterior_moment_grouped(q_mode=mode, **_fused(**kw))
    with pytest.raises(Reached):
        pr.moment_grouped(**_explicit(q=False), S0s=S0)
    with pytest.raises(Reached):
        pr.posterior_moment_grouped_summary(**_fused(), **EMISSION, Y_test=np.zeros((3, 1)), S0s=S0)
    with pytest.raises(Reached):
        pr.moment_summary(np.zeros((3, 4, 2)), np.zeros((3, 4, 2, 2)), **EMISSION, Y_test=np.zeros(4))


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=3, kind=0, gpp=0, q_mode=0, J=0, n_test=0, null=(), q=True):
    """One ABI call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL.  J = 0: no summary."""
    P = D + C if P is None else P
    n, nm, st, Pp, Jp = max(G, 1), max(n_models, 1), max(steps, 1), max(P, 1), max(J, 1)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((n, T + 1, D)),
             cf=np.zeros((max(T, 1), max(C, 1))), cr=np.zeros((st, max(C, 1))), lq=np.zeros((n, D)), f=np.zeros((n, M, D)),
             xl=np.zeros((n, D)), CC=np.ones((D, Jp)), DD=np.zeros(Jp), sd=np.ones(Jp), Y=np.zeros((max(n_test, 1), Jp)))
    outs = dict(m=np.full((n, st, D), 7.0), S=np.full((n, st, D, D), 7.0), U=np.full((n, M, D), 7.0), ym=np.full((st, Jp), 7.0),
                yv=np.full((st, Jp), 7.0), yt=np.full((st, Jp), 7.0), lpd=np.full((max(n_test, 1), Jp), 7.0),
                lg=np.full((max(n_test, 1), Jp), 7.0))
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"] if n_test or "keepY" in null else None, n_test, p["ym"], p["yv"], p["yt"],
            p["lpd"] if n_test else None, p["lg"] if n_test else None) if J else (None, None, None, 0, None, 0) + (None,) * 5
    if fused:
        rc = lib.ffvd_op_posterior_moment_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                  1e-5, gpp, q_mode, None, p["cr"], steps, p["m"], p["S"], p["U"], *tail)
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        qm = [np.zeros((M, M)) for _ in range(n * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[None if "W0" in null and i == 1 else w.ctypes.data for i, w in enumerate(Wm)])
        qt = None if not q else (ctypes.c_void_p * len(qm))(*[None if "q0" in null and i == 1 else x.ctypes.data for i, x in enumerate(qm)])
        rc = lib.ffvd_op_moment_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], qt, q_mode, p["xl"], None,
                                        p["cr"], C, steps, p["lq"], p["m"], p["S"], *tail)
    return rc, outs


# beyond a limit, or a required pointer missing: shared by the two entry points
BAD_ABI = [dict(kind=1), dict(kind=2), dict(D=9, C=0), dict(D=2, C=31), dict(M=2049), dict(M=0), dict(D=0), dict(J=9), dict(q_mode=2),
           dict(q_mode=-1), dict(G=3, n_models=2), dict(G=-1), dict(steps=-1), dict(P=2), dict(P=4), dict(null=("Z",)),
           dict(null=("lv",)), dict(null=("ll",)), dict(null=("lq",)), dict(null=("cr",)), dict(null=("m",)), dict(null=("S",)),
           dict(J=1, null=("CC",)), dict(J=1, null=("DD",)), dict(J=1, null=("sd",)), dict(J=1, n_test=4), dict(J=1, n_test=2, null=("Y",)),
           dict(J=1, null=("ym", "yv", "yt"))]


@pytest.mark.parametrize("ov", BAD_ABI + [dict(null=("f",)), dict(null=("xl",)), dict(null=("W",)), dict(null=("W0",)), dict(null=("q0",))],
                         ids=str)
def test_explicit_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(False, **ov)
    assert rc == E, rc
    assert b"ffvd_op_moment_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", BAD_ABI + [dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))], ids=str)
def test_fused_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(True, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_moment_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_linear_kernels_are_named_in_the_message():
    for fused in (False, True):
        rc, _ = _abi(fused, kind=1)
        assert rc == E and b"SE kernel only" in _lib.load().ffvd_last_error(None)


def test_abi_rejects_stacks_beyond_the_limits():
    """G * D * Mp^2 > 2^29 doubles, G * D > 2^24 and G * steps * D^2 >= 2^31: rejected on the scalar arguments alone (no array is read
    before the check)."""
    lib = _lib.load()
    z = np.zeros(1)
    p = _lib.dptr(z)
    t = (ctypes.c_void_p * 1)(z.ctypes.data)
    none = (None, None, None, 0, None, 0, None, None, None, None, None)
    for G, M, D, steps in ((129, 1024, 4, 1), (33, 2048, 4, 1), ((1 << 24) + 1, 1, 1, 1), (2, 1, 1, 1 << 30), (1 << 22, 1, 8, 8)):
        rc = lib.ffvd_op_moment_grouped(0, G, 1, t, p, M, D, D, p, p, p, None, 0, p, None, None, 0, steps, p, p, p, *none)
        assert rc == E, (G, M, D, steps, rc)
        assert b"ffvd_op_moment_grouped: bad argument" in lib.ffvd_last_error(None)
        rc = lib.ffvd_op_posterior_moment_grouped(0, G, 1, p, M, D, D, p, p, p, None, 0, 4, p, 1e-5, 0, 0, None, None, steps, p, p, None, *none)
        assert rc == E, (G, M, D, steps, rc)
        assert b"ffvd_op_posterior_moment_grouped: bad argument" in lib.ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(G=0, n_models=0), dict(steps=0), dict(steps=0, J=1)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())


def test_summary_abi_rejects_bad_arguments_and_accepts_empty_stacks():
    lib, dp = _lib.load(), _lib.dptr
    m, S, CC, v, out = np.zeros((2, 3, 2)), np.zeros((2, 3, 2, 2)), np.ones((2, 1)), np.ones(1), np.full((3, 1), 7.0)

    def call(G=2, steps=3, D=2, J=1, n_test=0, m_=m, S_=S, CC_=CC, sd=v, Y=None, o=out):
        opt = lambda x: None if x is None else dp(x)
        return lib.ffvd_op_moment_summary(opt(m_), opt(S_), G, steps, D, opt(CC_), dp(v), opt(sd), J, opt(Y), n_test, opt(o), None, None, None, None)
    for kw in (dict(D=9), dict(D=0), dict(J=9), dict(J=0), dict(G=-1), dict(steps=-1), dict(n_test=4), dict(n_test=1), dict(m_=None),
               dict(S_=None), dict(CC_=None), dict(sd=None), dict(sd=np.zeros(1)), dict(o=None), dict(G=1 << 20, steps=1 << 10)):
        assert call(**kw) == E, kw
        assert b"ffvd_op_moment_summary: bad argument" in lib.ffvd_last_error(None)
    assert call(G=0) == _lib.FFVD_OK and call(steps=0) == _lib.FFVD_OK
    assert np.all(out == 7.0)


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.exported_symbols()
        assert hasattr(_lib.load(), name)


def test_the_model_level_keywords_default_to_the_rollouts():
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd.models import Model, RegressionModel
    sig = inspect.signature(DGPSSM.evaluate_heldout).parameters
    assert sig["method"].kind is inspect.Parameter.KEYWORD_ONLY and sig["method"].default == "rollouts"
    sig = inspect.signature(DGPSSM.predict_moments).parameters
    assert sig["q_mode"].kind is inspect.Parameter.KEYWORD_ONLY and sig["q_mode"].default == "reference"
    assert sig["Y_test"].default is None and sig["Y_train_std"].default == 1.0
    assert inspect.signature(RegressionModel.fit).parameters["eval_method"].default == "rollouts"
    assert inspect.signature(Model._fit).parameters["eval_method"].default == "rollouts"

    class Stub:
        _host_stale = False
        Y = np.zeros((4, 1))

    with pytest.raises(ValueError, match="method"):             # stopped before any parameter or device is touched
        DGPSSM.evaluate_heldout(Stub(), np.zeros((2, 1)), None, 8, method="quadrature")
    with pytest.raises(ValueError, match="q_mode"):
        DGPSSM.predict_moments(Stub(), None, 3, q_mode="slice0")
    with pytest.raises(ValueError, match="test_len"):
        DGPSSM.predict_moments(Stub(), None, 0)
    doc = pr.moment_summary.__doc__
    assert "predict_y_var" in doc and "no separate" in doc
