"""Argument checks of the grouped rollouts, without a GPU: prediction.rollout_grouped raises ValueError on every shape or kernel-kind
mismatch before any device call, ffvd_op_rollout_grouped returns FFVD_EINVAL before any device work beyond its limits (and FFVD_OK
for G = 0 or steps = 0 without touching anything), DGPSSM's mode check accepts "intent-batched", and the symbol is declared."""
import ctypes
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd.kernels import LinearK, SquaredExponential
from ffvd_amd.prediction import rollout_grouped

E = _lib.FFVD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(G=3, M=5, D=2, C=1, R=2, steps=4, q=True):
    P = D + C
    kern = [[SquaredExponential(P, variance=0.5, lengthscales=np.full(P, 2.0)) for _ in range(D)] for _ in range(G)]
    return dict(Lm_inverse_seqs=[[np.eye(M) for _ in range(D)] for _ in range(G)], Zs=[np.zeros((M, P)) for _ in range(G)],
                kerns=kern, U_vals=[np.zeros((M, D)) for _ in range(G)],
                q_sqrts=[np.zeros((D, M, M)) for _ in range(G)] if q else None, x_lasts=[np.zeros(D) for _ in range(G)],
                control_inputs=np.zeros((10 + steps, C)), ctrl_offset=10, steps=steps, Qs=[np.ones(D) for _ in range(G)],
                eps=np.zeros((steps, G, R, D)))


def _break(name, value, index=None):
    a = _args()
    if index is None:
        a[name] = value
    else:
        a[name] = list(a[name])
        a[name][index] = value
    return a


BAD = {
    "no groups": lambda: dict(_args(), kerns=[]),
    "one W stack missing": lambda: _break("Lm_inverse_seqs", _args()["Lm_inverse_seqs"][:2]),
    "one Z missing": lambda: _break("Zs", _args()["Zs"][:2]),
    "one U missing": lambda: _break("U_vals", _args()["U_vals"][:2]),
    "one q_sqrt missing": lambda: _break("q_sqrts", _args()["q_sqrts"][:2]),
    "one x_last missing": lambda: _break("x_lasts", _args()["x_lasts"][:2]),
    "one Q missing": lambda: _break("Qs", _args()["Qs"][:2]),
    "mixed kernel kinds": lambda: _break("kerns", [LinearK(3, variance=0.1) for _ in range(2)], 1),
    "mixed D (kernels)": lambda: _break("kerns", _args(D=3, C=0)["kerns"][0], 1),
    "mixed M (Z)": lambda: _break("Zs", np.zeros((6, 3)), 2),
    "mixed P (Z)": lambda: _break("Zs", np.zeros((5, 4)), 2),
    "mixed M (W)": lambda: _break("Lm_inverse_seqs", [np.eye(6), np.eye(6)], 1),
    "W stack of another D": lambda: _break("Lm_inverse_seqs", [np.eye(5)] * 3, 1),
    "U of another shape": lambda: _break("U_vals", np.zeros((5, 3)), 0),
    "q_sqrt not a stack": lambda: _break("q_sqrts", np.zeros((5, 5)), 0),
    "q_sqrt of another M": lambda: _break("q_sqrts", np.zeros((2, 6, 6)), 2),
    "x_last of another D": lambda: _break("x_lasts", np.zeros(3), 1),
    "Q of another D": lambda: _break("Qs", np.ones(3), 1),
    "eps without the group axis": lambda: _break("eps", np.zeros((4, 2, 2))),
    "eps of another G": lambda: _break("eps", np.zeros((4, 2, 2, 2))),
    "eps of another D": lambda: _break("eps", np.zeros((4, 3, 2, 3))),
    "eps of other steps": lambda: _break("eps", np.zeros((5, 3, 2, 2))),
    "eps without rollouts": lambda: _break("eps", np.zeros((4, 3, 0, 2))),
    "too few control rows": lambda: _break("control_inputs", np.zeros((12, 1))),
    "control columns": lambda: _break("control_inputs", np.zeros((14, 2))),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_rollout_grouped_rejects_mismatched_groups_before_any_device_call(what, monkeypatch):
    def no_device():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(ValueError):
        rollout_grouped(**BAD[what]())


def _abi(*, G=2, M=4, D=2, C=1, P=None, R=2, steps=3, kind=0):
    P = D + C if P is None else P
    n = max(G, 1)
    lib, dp = _lib.load(), _lib.dptr
    W, Z, f, q = np.zeros((n, D, M, M)), np.zeros((n, M, max(P, 1))), np.zeros((n, M, D)), np.zeros((n, M, M))
    lv, ll, lq, xl = np.zeros((n, D)), np.zeros((n, D, max(P, 1))), np.zeros((n, D)), np.zeros((n, D))
    ctrl, eps = np.zeros((max(steps, 1), max(C, 1))), np.zeros((max(steps, 1), n, R, D))
    px, pv = np.full((n, R, max(steps, 1), D), 7.0), np.full((n, R, max(steps, 1), D), 7.0)
    Wt = (ctypes.c_void_p * (n * max(D, 1)))(*[W[g, d].ctypes.data for g in range(n) for d in range(D)])
    qt = (ctypes.c_void_p * n)(*[q[g].ctypes.data for g in range(n)])
    rc = lib.ffvd_op_rollout_grouped(kind, G, Wt, dp(Z), M, P, D, dp(lv), dp(ll), dp(f), qt, dp(xl), R, dp(ctrl), C, steps,
                                     dp(lq), dp(eps), dp(px), dp(pv))
    return rc, px, pv


@pytest.mark.parametrize("ov", [dict(M=2049), dict(D=2, C=31), dict(P=2), dict(P=4), dict(G=-1), dict(R=0), dict(steps=-1),
                                dict(kind=2), dict(M=0), dict(D=0, C=1, P=1)], ids=str)
def test_abi_rejects_bad_arguments_before_any_device_work(ov):
    rc, _, _ = _abi(**ov)
    assert rc == E, rc
    assert b"ffvd_op_rollout_grouped: bad argument" in _lib.load().ffvd_last_error(None)


def test_abi_rejects_operand_stacks_beyond_its_limits():
    """G * D * Mp^2 > 2^29 doubles and G * R > 2^20: rejected on the scalar arguments alone (no array is read before the check)."""
    lib = _lib.load()
    z = np.zeros(1)
    p = _lib.dptr(z)
    tab = (ctypes.c_void_p * 1)(z.ctypes.data)
    for G, M, D, R in ((129, 1024, 4, 1), (2048, 16, 1, 1024)):
        rc = lib.ffvd_op_rollout_grouped(0, G, tab, p, M, D, D, p, p, p, None, p, R, None, 0, 1, p, p, p, p)
        assert rc == E, (G, M, D, R, rc)
        assert b"ffvd_op_rollout_grouped: bad argument" in lib.ffvd_last_error(None)
    assert lib.ffvd_op_rollout_grouped(0, 1, None, None, 4, 2, 2, None, None, None, None, None, 1, None, 0, 1, None, None, None,
                                       None) == E


@pytest.mark.parametrize("ov", [dict(G=0), dict(steps=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(ov):
    rc, px, pv = _abi(**ov)
    assert rc == _lib.FFVD_OK
    assert np.all(px == 7.0) and np.all(pv == 7.0)


def test_mode_check_accepts_intent_batched():
    from ffvd_amd.dgp_model import DGPSSM
    assert "intent-batched" in DGPSSM.ROLLOUT_MODES and {"reference", "intent"} <= set(DGPSSM.ROLLOUT_MODES)
    assert callable(DGPSSM.collect_samples_chains)


def test_collect_samples_formal_rejects_an_unknown_rollout_mode_and_passes_the_batched_one():
    """The check inside the method: a bogus mode raises there; "intent-batched" gets past it (to the next check, which this call is
    built to fail, so that no device is needed)."""
    from ffvd_amd.dgp_model import DGPSSM

    class Stub:
        ROLLOUT_MODES = DGPSSM.ROLLOUT_MODES
        vars = ["logvariance"]

    with pytest.raises(ValueError, match="rollout_mode"):
        DGPSSM.collect_samples_formal(Stub(), 1, 1, None, 1, rollout_mode="intent_batched")
    for mode in DGPSSM.ROLLOUT_MODES:
        with pytest.raises(ValueError, match="sghmc_var_len"):
            DGPSSM.collect_samples_formal(Stub(), 1, 1, None, 1, sghmc_var_len=5, rollout_mode=mode)


def test_symbol_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+ffvd_op_rollout_grouped\s*\(", header)
    assert "ffvd_op_rollout_grouped" in _lib.exported_symbols()
    assert hasattr(_lib.load(), "ffvd_op_rollout_grouped")
