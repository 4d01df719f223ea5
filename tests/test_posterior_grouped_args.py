"""Argument checks of the grouped posteriors, without a GPU: conditionals_multi_output.collapse_u_mean_grouped and
prediction.posterior_rollout_grouped raise ValueError on every shape, model-count or kernel-kind mismatch before the library is
loaded; ffvd_op_posterior_grouped / ffvd_op_posterior_rollout_grouped return FFVD_EINVAL before any device call beyond their limits
(and FFVD_OK for G = 0, or steps = 0 in the fused form, without touching anything); DGPSSM knows "intent-fused" and `fused`; the
symbols are declared, exported and bound."""
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd.conditionals_multi_output import collapse_u_mean_grouped
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import posterior_rollout_grouped

E = _lib.FFVD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffvd_op_posterior_grouped", "ffvd_op_posterior_rollout_grouped")


def _kern(D, P):
    return [SquaredExponential(P, variance=0.5, lengthscales=np.full(P, 2.0)) for _ in range(D)]


def _args(G=3, n_models=None, M=5, D=2, C=1, T=6, R=2, steps=4):
    """n_models None: one model (an array and one kernel list); otherwise sequences of that length."""
    P = D + C
    Zs = np.zeros((M, P)) if n_models is None else [np.zeros((M, P)) for _ in range(n_models)]
    kerns = _kern(D, P) if n_models is None else [_kern(D, P) for _ in range(n_models)]
    return dict(Zs=Zs, kerns=kerns, Xs=[np.zeros((T + 1, D)) for _ in range(G)], Qs=[np.ones(D) for _ in range(G)],
                control_inputs=np.zeros((T + 2 + steps, C)), ctrl_offset=T + 2, steps=steps, eps=np.zeros((steps, G, R, D)))


def _with(base, **kw):
    a = dict(base)
    a.update(kw)
    return a


def _mixed_kinds():
    a = _args(n_models=3)
    a["kerns"][1] = [LinearK(3, variance=0.1) for _ in range(2)]
    return a


BAD = {
    "wrong length for Xs (shared model, Qs of another G)": lambda: _with(_args(), Xs=_args()["Xs"][:2]),
    "wrong length for Xs (one model per group)": lambda: _with(_args(n_models=3), Xs=_args()["Xs"][:2], Qs=_args()["Qs"][:2],
                                                                eps=np.zeros((4, 2, 2, 2))),
    "no groups": lambda: _with(_args(), Xs=[], Qs=[]),
    "one X of another T": lambda: _with(_args(), Xs=_args()["Xs"][:2] + [np.zeros((8, 2))]),
    "one X of another D": lambda: _with(_args(), Xs=_args()["Xs"][:2] + [np.zeros((7, 3))]),
    "eps without the group axis": lambda: _with(_args(), eps=np.zeros((4, 2, 2))),
    "eps of another G": lambda: _with(_args(), eps=np.zeros((4, 2, 2, 2))),
    "eps of another D": lambda: _with(_args(), eps=np.zeros((4, 3, 2, 3))),
    "eps of other steps": lambda: _with(_args(), eps=np.zeros((5, 3, 2, 2))),
    "eps without rollouts": lambda: _with(_args(), eps=np.zeros((4, 3, 0, 2))),
    "too few control rows for the rollouts": lambda: _with(_args(), control_inputs=np.zeros((11, 1))),
    "too few control rows for the posterior": lambda: _with(_args(), control_inputs=np.zeros((5, 1)), ctrl_offset=0, steps=1,
                                                             eps=np.zeros((1, 3, 2, 2))),
    "control columns": lambda: _with(_args(), control_inputs=np.zeros((12, 2))),
    "n_models neither 1 nor G": lambda: _args(G=3, n_models=2),
    "Zs and kerns of different counts": lambda: _with(_args(n_models=3), Zs=_args(n_models=3)["Zs"][:1]),
    "one kernel list with a stack of Z": lambda: _with(_args(), Zs=np.zeros((3, 5, 3))),
    "mixed kernel kinds": _mixed_kinds,
    "mixed D (kernels)": lambda: _with(_args(n_models=3), kerns=_args(n_models=3)["kerns"][:2] + [_kern(3, 3)]),
    "mixed M (Z)": lambda: _with(_args(n_models=3), Zs=_args(n_models=3)["Zs"][:2] + [np.zeros((6, 3))]),
    "Q of another D": lambda: _with(_args(), Qs=[np.ones(2), np.ones(3), np.ones(2)]),
    "negative groups_per_pass": lambda: _with(_args(), groups_per_pass=-1),
}


@pytest.fixture
def no_device(monkeypatch):
    def fail():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", fail)


@pytest.mark.parametrize("what", sorted(BAD))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    with pytest.raises(ValueError):
        posterior_rollout_grouped(**BAD[what]())


@pytest.mark.parametrize("what", sorted(k for k in BAD if not k.startswith("eps") and "rollouts" not in k))
def test_grouped_posterior_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = BAD[what]()
    kw = {k: a[k] for k in ("Zs", "kerns", "Xs", "control_inputs", "Qs", "groups_per_pass") if k in a}
    with pytest.raises(ValueError):
        collapse_u_mean_grouped(**kw)


def test_well_formed_arguments_reach_the_library(monkeypatch):
    """The other half of the tests above: what they reject is not everything."""
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    for a in (_args(), _args(n_models=3), _args(n_models=1), _args(C=0)):
        with pytest.raises(Reached):
            posterior_rollout_grouped(**a)
        with pytest.raises(Reached):
            collapse_u_mean_grouped(a["Zs"], a["kerns"], a["Xs"], a["control_inputs"], a["Qs"])


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, P=None, T=5, R=2, steps=3, kind=0, gpp=0, null=None):
    P = D + C if P is None else P
    n, nm = max(G, 1), max(n_models, 1)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, max(P, 1))), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, max(P, 1))), X=np.zeros((n, T + 1, D)),
             cf=np.zeros((max(T, 1), max(C, 1))), lq=np.zeros((n, D)), cr=np.zeros((max(steps, 1), max(C, 1))),
             eps=np.zeros((max(steps, 1), n, max(R, 1), D)))
    outs = dict(L=np.full((nm, D, M, M), 7.0), U=np.full((n, M, D), 7.0), H=np.full((n, D, M, M), 7.0),
                px=np.full((n, max(R, 1), max(steps, 1), D), 7.0), pv=np.full((n, max(R, 1), max(steps, 1), D), 7.0))
    p = {k: (None if k == null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    if fused:
        rc = lib.ffvd_op_posterior_rollout_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                   1e-5, gpp, R, p["cr"], steps, p["eps"], p["px"], p["pv"], p["U"])
    else:
        rc = lib.ffvd_op_posterior_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"], 1e-5,
                                           gpp, p["L"], p["U"], p["H"])
    return rc, outs


BAD_ABI = [dict(M=2049), dict(P=2), dict(P=4), dict(D=2, C=31), dict(G=3, n_models=2), dict(G=-1), dict(T=0), dict(kind=2), dict(M=0),
           dict(gpp=-1), dict(null="Z"), dict(null="lv"), dict(null="ll"), dict(null="X"), dict(null="cf"), dict(null="lq")]


@pytest.mark.parametrize("ov", BAD_ABI + [dict(null="U")], ids=str)
def test_posterior_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(False, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", BAD_ABI + [dict(null="px"), dict(null="pv"), dict(null="eps"), dict(null="cr"), dict(R=0), dict(steps=-1)],
                         ids=str)
def test_fused_abi_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _abi(True, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_rollout_grouped: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_fused_abi_rejects_operand_stacks_beyond_the_rollout_limits():
    """G * D * Mp16^2 > 2^29 doubles and G * R > 2^20: rejected on the scalar arguments alone (no array is read before the check)."""
    lib = _lib.load()
    z = np.zeros(1)
    p = _lib.dptr(z)
    for G, M, D, R in ((129, 1024, 4, 1), (2048, 16, 1, 1024)):
        rc = lib.ffvd_op_posterior_rollout_grouped(0, G, 1, p, M, D, D, p, p, p, None, 0, 4, p, 1e-5, 0, R, None, 1, p, p, p, None)
        assert rc == E, (G, M, D, R, rc)
        assert b"ffvd_op_posterior_rollout_grouped: bad argument" in lib.ffvd_last_error(None)


@pytest.mark.parametrize("fused,ov", [(False, dict(G=0)), (False, dict(G=0, n_models=0)), (True, dict(G=0)), (True, dict(steps=0))], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())


def test_model_level_switches_exist():
    from ffvd_amd.dgp_model import DGPSSM
    assert "intent-fused" in DGPSSM.ROLLOUT_MODES and {"reference", "intent", "intent-batched"} <= set(DGPSSM.ROLLOUT_MODES)
    par = inspect.signature(DGPSSM.collect_samples_chains).parameters["fused"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False

    class Stub:
        ROLLOUT_MODES = DGPSSM.ROLLOUT_MODES
        vars = ["logvariance"]

    with pytest.raises(ValueError, match="sghmc_var_len"):          # past the mode check, stopped by the next one: no device needed
        DGPSSM.collect_samples_formal(Stub(), 1, 1, None, 1, sghmc_var_len=5, rollout_mode="intent-fused")
    with pytest.raises(ValueError, match="rollout_mode"):
        DGPSSM.collect_samples_formal(Stub(), 1, 1, None, 1, rollout_mode="intent_fused")


def test_fused_chains_need_the_collapsed_branch():
    from ffvd_amd.dgp_model import DGPSSM

    class Stub:
        _host_stale = False
        U_collapse = False
        num_chains, output_dim, X_N = 2, 2, 5

    with pytest.raises(ValueError, match="explicit U"):
        DGPSSM.collect_samples_chains(Stub(), 1, None, 3, fused=True)


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.exported_symbols()
        assert hasattr(_lib.load(), name)
