"""Argument checks of the rollout summaries, without a GPU: prediction.rollout_summary, rollout_grouped_summary and
posterior_rollout_grouped_summary raise ValueError on every shape mismatch before the library is loaded; ffvd_op_rollout_summary,
ffvd_op_rollout_grouped_summary and ffvd_op_posterior_rollout_grouped_summary return FFVD_EINVAL before any device call for a bad
shape, J outside 1..8, n_test outside 0..steps, a noise standard deviation that is not finite and positive, missing held-out data
and an element count that overflows (and FFVD_OK without touching anything when there are no rollouts or no steps); DGPSSM knows
`summary` and `evaluate_heldout`, Model._fit knows `eval_every`; the symbols are declared, exported and bound."""
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd.kernels import SquaredExponential
from ffvd_amd.prediction import posterior_rollout_grouped_summary, rollout_grouped_summary, rollout_summary

E = _lib.FFVD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffvd_op_rollout_summary", "ffvd_op_rollout_grouped_summary", "ffvd_op_posterior_rollout_grouped_summary")


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


# ---- Python layer --------------------------------------------------------------------------------------------------------------------
def _emission(D=2, J=1, steps=4, n_test=3):
    return dict(CC=np.ones((D, J)), DD=np.zeros(J), log_Rchols=np.zeros((J, J)), Y_test=None if n_test is None else np.zeros((n_test, J)))


def _standalone(N=5, steps=4, D=2, J=1, n_test=3, **ov):
    a = dict(predict_x=np.zeros((N, steps, D)), predict_x_var=np.ones((N, steps, D)), **_emission(D, J, steps, n_test))
    a.update(ov)
    return a


def _kern(D, P):
    return [SquaredExponential(P, variance=0.5, lengthscales=np.full(P, 2.0)) for _ in range(D)]


def _grouped(G=3, M=5, D=2, C=1, R=2, steps=4, **ov):
    P = D + C
    a = dict(Lm_inverse_seqs=[[np.eye(M) for _ in range(D)] for _ in range(G)], Zs=[np.zeros((M, P)) for _ in range(G)],
             kerns=[_kern(D, P) for _ in range(G)], U_vals=[np.zeros((M, D)) for _ in range(G)], q_sqrts=None,
             x_lasts=[np.zeros(D) for _ in range(G)], control_inputs=np.zeros((10 + steps, C)), ctrl_offset=10, steps=steps,
             Qs=[np.ones(D) for _ in range(G)], eps=np.zeros((steps, G, R, D)), **_emission(D, 1, steps, 3))
    a.update(ov)
    return a


def _fused(G=3, M=5, D=2, C=1, T=6, R=2, steps=4, **ov):
    P = D + C
    a = dict(Zs=np.zeros((M, P)), kerns=_kern(D, P), Xs=[np.zeros((T + 1, D)) for _ in range(G)], Qs=[np.ones(D) for _ in range(G)],
             control_inputs=np.zeros((T + 2 + steps, C)), ctrl_offset=T + 2, steps=steps, eps=np.zeros((steps, G, R, D)),
             **_emission(D, 1, steps, 3))
    a.update(ov)
    return a


BAD_EMISSION = {
    "CC of another D": dict(CC=np.ones((3, 1))),
    "CC not a matrix": dict(CC=np.ones(2)),
    "no outputs": dict(CC=np.ones((2, 0)), DD=np.zeros(0)),
    "nine outputs": dict(CC=np.ones((2, 9)), DD=np.zeros(9), log_Rchols=np.zeros((9, 9)), Y_test=None),
    "DD of another J": dict(DD=np.zeros(2)),
    "log_Rchols of another J": dict(log_Rchols=np.zeros((2, 2))),
    "log_Rchols infinite": dict(log_Rchols=np.full((1, 1), np.inf)),
    "log_Rchols minus infinity": dict(log_Rchols=np.full((1, 1), -np.inf)),
    "log_Rchols NaN": dict(log_Rchols=np.full((1, 1), np.nan)),
    "Y_test of another J": dict(Y_test=np.zeros((3, 2))),
    "Y_test longer than the rollouts": dict(Y_test=np.zeros((5, 1))),
    "Y_test with three axes": dict(Y_test=np.zeros((3, 1, 1))),
}
BAD_STACKS = {
    "stacks of different shapes": dict(predict_x_var=np.ones((5, 4, 3))),
    "stacks with two axes": dict(predict_x=np.zeros((4, 2)), predict_x_var=np.ones((4, 2))),
    "stacks with five axes": dict(predict_x=np.zeros((1, 1, 5, 4, 2)), predict_x_var=np.ones((1, 1, 5, 4, 2))),
    "no rollouts": dict(predict_x=np.zeros((0, 4, 2)), predict_x_var=np.ones((0, 4, 2))),
    "no steps": dict(predict_x=np.zeros((5, 0, 2)), predict_x_var=np.ones((5, 0, 2)), Y_test=None),
}


@pytest.mark.parametrize("what", sorted(BAD_EMISSION) + sorted(BAD_STACKS))
def test_rollout_summary_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    with pytest.raises(ValueError):
        rollout_summary(**_standalone(**{**BAD_EMISSION, **BAD_STACKS}[what]))


@pytest.mark.parametrize("what", sorted(BAD_EMISSION))
def test_grouped_summaries_reject_a_bad_emission_before_the_library_is_loaded(what, no_device):
    with pytest.raises(ValueError):
        rollout_grouped_summary(**_grouped(**BAD_EMISSION[what]))
    with pytest.raises(ValueError):
        posterior_rollout_grouped_summary(**_fused(**BAD_EMISSION[what]))


def test_grouped_summaries_keep_the_checks_of_the_rollout_calls(no_device):
    with pytest.raises(ValueError):
        rollout_grouped_summary(**_grouped(eps=np.zeros((4, 2, 2, 2))))
    with pytest.raises(ValueError):
        rollout_grouped_summary(**_grouped(x_lasts=[np.zeros(2)] * 2))
    with pytest.raises(ValueError):
        posterior_rollout_grouped_summary(**_fused(eps=np.zeros((4, 3, 2, 3))))
    with pytest.raises(ValueError):
        posterior_rollout_grouped_summary(**_fused(control_inputs=np.zeros((11, 1))))


def test_well_formed_arguments_reach_the_library(reached):
    for a in (_standalone(), _standalone(n_test=None), _standalone(J=3, n_test=4), _standalone(log_Rchols=np.zeros(1)),
              dict(_standalone(), predict_x=np.zeros((2, 3, 4, 2)), predict_x_var=np.ones((2, 3, 4, 2))),
              _standalone(Y_test=np.zeros(3))):
        with pytest.raises(Reached):
            rollout_summary(**a)
    with pytest.raises(Reached):
        rollout_grouped_summary(**_grouped(), return_rollouts=True)
    with pytest.raises(Reached):
        posterior_rollout_grouped_summary(**_fused())


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def _summary_arrays(D, J, steps, n_test, sd=None):
    J1, s1, t1 = max(J, 1), max(steps, 1), max(n_test, 1)
    a = dict(CC=np.ones((D, J1)), DD=np.zeros(J1), sd=np.ones(J1) if sd is None else np.full(J1, float(sd)), Y=np.zeros((t1, J1)))
    outs = {k: np.full((s1, J1), 7.0) for k in ("ym", "yv", "yt")}
    outs.update({k: np.full((t1, J1), 7.0) for k in ("lpd", "lg")})
    return a, outs


def _tail(p, J, n_test):
    return (p["CC"], p["DD"], p["sd"], J, p["Y"], n_test, p["ym"], p["yv"], p["yt"], p["lpd"], p["lg"])


def _ptrs(arrays, null):
    null = (null,) if isinstance(null, str) else tuple(null or ())
    return {k: (None if k in null else _lib.dptr(v)) for k, v in arrays.items()}


def _abi_standalone(*, N=5, steps=4, D=2, J=1, n_test=3, sd=None, null=None):
    a, outs = _summary_arrays(max(D, 1), J, steps, n_test, sd)
    a.update(px=np.zeros((max(N, 1), max(steps, 1), max(D, 1))), pv=np.ones((max(N, 1), max(steps, 1), max(D, 1))))
    p = _ptrs({**a, **outs}, null)
    rc = _lib.load().ffvd_op_rollout_summary(p["px"], p["pv"], N, steps, D, *_tail(p, J, n_test))
    return rc, outs


def _abi_grouped(*, G=2, M=4, D=2, C=1, R=2, steps=4, J=1, n_test=3, sd=None, null=None):
    import ctypes
    P, n = D + C, max(G, 1)
    a, outs = _summary_arrays(D, J, steps, n_test, sd)
    W = [np.eye(M) for _ in range(n * D)]
    a.update(Z=np.zeros((n, M, P)), lv=np.zeros((n, D)), ll=np.zeros((n, D, P)), f=np.zeros((n, M, D)), xl=np.zeros((n, D)),
             ctrl=np.zeros((max(steps, 1), max(C, 1))), lq=np.zeros((n, D)), eps=np.zeros((max(steps, 1), n, R, D)))
    outs.update(px=np.full((n, R, max(steps, 1), D), 7.0), pv=np.full((n, R, max(steps, 1), D), 7.0))
    p = _ptrs({**a, **outs}, null)
    Wt = (ctypes.c_void_p * len(W))(*[w.ctypes.data for w in W])
    rc = _lib.load().ffvd_op_rollout_grouped_summary(0, G, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, p["xl"], R, p["ctrl"], C,
                                                     steps, p["lq"], p["eps"], p["px"], p["pv"], *_tail(p, J, n_test))
    return rc, outs


def _abi_fused(*, G=2, M=4, D=2, C=1, T=5, R=2, steps=4, J=1, n_test=3, sd=None, null=None):
    P, n = D + C, max(G, 1)
    a, outs = _summary_arrays(D, J, steps, n_test, sd)
    a.update(Z=np.zeros((1, M, P)), lv=np.zeros((1, D)), ll=np.zeros((1, D, P)), X=np.zeros((n, T + 1, D)), cf=np.zeros((T, max(C, 1))),
             lq=np.zeros((n, D)), cr=np.zeros((max(steps, 1), max(C, 1))), eps=np.zeros((max(steps, 1), n, R, D)))
    outs.update(px=np.full((n, R, max(steps, 1), D), 7.0), pv=np.full((n, R, max(steps, 1), D), 7.0), U=np.full((n, M, D), 7.0))
    p = _ptrs({**a, **outs}, null)
    rc = _lib.load().ffvd_op_posterior_rollout_grouped_summary(0, G, 1, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                               1e-5, 0, R, p["cr"], steps, p["eps"], p["px"], p["pv"], p["U"],
                                                               *_tail(p, J, n_test))
    return rc, outs


ALL_OUTPUTS = ("ym", "yv", "yt", "lpd", "lg")
BAD_SUMMARY = [dict(J=0), dict(J=9), dict(J=-1), dict(n_test=-1), dict(n_test=5), dict(sd=0.0), dict(sd=-1.0), dict(sd=np.nan),
               dict(sd=np.inf), dict(null="Y"), dict(null="Y", n_test=0), dict(null=("Y", "lpd"), n_test=0), dict(null="CC"),
               dict(null="DD"), dict(null="sd"), dict(null=ALL_OUTPUTS)]
ABI = {"standalone": (_abi_standalone, b"ffvd_op_rollout_summary: bad argument"),
       "grouped": (_abi_grouped, b"ffvd_op_rollout_grouped_summary: bad argument"),
       "fused": (_abi_fused, b"ffvd_op_posterior_rollout_grouped_summary: bad argument")}


@pytest.mark.parametrize("ov", BAD_SUMMARY, ids=str)
@pytest.mark.parametrize("which", sorted(ABI))
def test_abi_rejects_a_bad_summary_request_without_a_device(which, ov):
    call, msg = ABI[which]
    rc, outs = call(**ov)
    assert rc == E, rc
    assert msg in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", [dict(N=-1), dict(steps=-1), dict(D=0), dict(D=33), dict(null="px"), dict(null="pv"),
                                dict(N=2 ** 20, steps=2 ** 10, D=2), dict(N=2 ** 31 - 1, steps=2 ** 31 - 1, D=32)], ids=str)
def test_standalone_abi_rejects_bad_shapes_and_overflowing_counts(ov):
    if ov.get("N", 0) > 100:                       # rejected on the scalar arguments alone: no array is read before the check
        z = _lib.dptr(np.zeros(8))
        rc = _lib.load().ffvd_op_rollout_summary(z, z, ov["N"], ov["steps"], ov["D"], z, z, z, 1, None, 0, z, None, None, None, None)
        assert rc == E, rc
        return
    rc, outs = _abi_standalone(**ov)
    assert rc == E, rc
    assert b"ffvd_op_rollout_summary: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("which,ov", [("grouped", dict(R=0)), ("grouped", dict(M=2049)), ("grouped", dict(null="eps")),
                                      ("grouped", dict(null="xl")), ("fused", dict(R=0)), ("fused", dict(T=0)),
                                      ("fused", dict(null="X")), ("fused", dict(null="cr"))], ids=str)
def test_grouped_abi_keeps_the_checks_of_the_rollout_entry_points(which, ov):
    call, msg = ABI[which]
    rc, outs = call(**ov)
    assert rc == E, rc
    assert msg in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("which,ov", [("standalone", dict(N=0)), ("standalone", dict(steps=0, n_test=0)), ("grouped", dict(G=0)),
                                      ("grouped", dict(steps=0, n_test=0)), ("fused", dict(G=0)), ("fused", dict(steps=0, n_test=0))],
                         ids=str)
def test_abi_returns_ok_and_touches_nothing_without_rollouts_or_steps(which, ov):
    rc, outs = ABI[which][0](**ov)
    assert rc == _lib.FFVD_OK, rc
    assert all(np.all(v == 7.0) for v in outs.values())


def test_the_existing_entry_points_still_need_their_output_stacks():
    """predict_x / predict_var may be NULL only where a summary is asked for."""
    import ctypes
    lib, dp = _lib.load(), _lib.dptr
    z, W = np.zeros(64), [np.eye(4) for _ in range(2)]
    Wt = (ctypes.c_void_p * 2)(*[w.ctypes.data for w in W])
    rc = lib.ffvd_op_rollout_grouped(0, 1, Wt, dp(z), 4, 2, 2, dp(z), dp(z), dp(z), None, dp(z), 1, None, 0, 2, dp(z), dp(z), None, None)
    assert rc == E and b"ffvd_op_rollout_grouped: bad argument" in lib.ffvd_last_error(None)
    rc = lib.ffvd_op_posterior_rollout_grouped(0, 1, 1, dp(z), 4, 2, 2, dp(z), dp(z), dp(z), None, 0, 3, dp(z), 1e-5, 0, 1, None, 2, dp(z),
                                               None, None, None)
    assert rc == E and b"ffvd_op_posterior_rollout_grouped: bad argument" in lib.ffvd_last_error(None)


# ---- model level ---------------------------------------------------------------------------------------------------------------------
def test_model_level_switches_exist():
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd.models import Model, RegressionModel
    par = inspect.signature(DGPSSM.collect_samples_chains).parameters["summary"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == "host"
    sig = inspect.signature(DGPSSM.evaluate_heldout).parameters
    assert list(sig)[1:4] == ["Y_test", "control_inputs", "num_per_chain"]
    for k in ("Y_train_std", "eps", "seed"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(Model._fit).parameters["eval_every"].default == 0
    assert inspect.signature(RegressionModel.fit).parameters["eval_every"].default == 0

    class Stub:
        _host_stale = False
        U_collapse = True
        num_chains, output_dim, X_N = 2, 2, 5

    with pytest.raises(ValueError, match="summary"):
        DGPSSM.collect_samples_chains(Stub(), 1, None, 3, summary="gpu")


def test_eval_every_needs_held_out_data():
    from ffvd_amd.models import Model
    m = Model("normal")
    with pytest.raises(ValueError, match="Y_test"):
        m._fit(np.zeros((4, 1)), None, "SquaredExponential", True, iterations=1, eval_every=1)
    with pytest.raises(ValueError, match="eval_every"):
        m._fit(np.zeros((4, 1)), None, "SquaredExponential", True, iterations=1, eval_every=-1, Y_test=np.zeros((2, 1)))


def test_eval_every_takes_one_standard_deviation_for_all_outputs():
    from ffvd_amd.models import RegressionModel
    with pytest.raises(ValueError, match="Ystd"):
        RegressionModel("normal").fit(np.zeros((4, 2)), Y_test=np.zeros((2, 2)), eval_every=1, Ystd=np.array([1.0, 2.0]))


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "ffvd_abi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.exported_symbols()
        assert hasattr(_lib.load(), name)
    i = header.index("ffvd_op_rollout_summary(")
    assert "base_model.py:330-348" in header[:i].rsplit("/*", 1)[1]
