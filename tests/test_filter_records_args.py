"""Argument checks of the linearised filter over many records, without a GPU: prediction.filter_records_grouped /
posterior_filter_records_grouped raise ValueError on every mismatch of the records (shapes, an infinite observation, lengths,
records_per_pass), of the start and of the model (LinearK among them) before the library is loaded; the broadcast forms of x0s / S0s
reach the library; DGPSSM.filter_records checks its arguments through a stand-in model and hands the two forms on;
ffvd_op_filter_records_grouped / ffvd_op_posterior_filter_records_grouped are declared in the header, bound in _lib.py, exported where
the library is built, and return FFVD_EINVAL before any device call beyond their limits (FFVD_OK for no groups, records or rows)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_moment_grouped_args import COMMON, _explicit, _fused, _with

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffvd_abi.h")
SYMBOLS = ("ffvd_op_filter_records_grouped", "ffvd_op_posterior_filter_records_grouped")
R, STEPS = 3, 4
SKIP = {"negative steps", "negative ctrl_offset", "too few control rows for the steps", "control inputs of another width", "S0s of another G",
        "S0s of another D", "an S0 that is not symmetric", "an S0 that is not finite"}       # (arguments the records replace; BAD below has theirs)


def _records(a, explicit, R=R, steps=STEPS, J=1, G=3, D=2):
    """moment_grouped's keyword arguments -> the record functions': Y_records, control_records, x0s in place of x_lasts / steps"""
    a = dict(a)
    a.pop("steps")
    a.pop("ctrl_offset")
    C = np.shape(a["control_inputs"])[1]
    if explicit:
        a.pop("control_inputs")
        a.pop("x_lasts")
        a["x0s"] = np.zeros((R, D))
    a["control_records"] = np.zeros((R, steps, C)) if C else None
    a["Y_records"] = np.zeros((R, steps, J))
    return a


def _call(explicit, **kw):
    a = _with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **kw)
    return (pr.filter_records_grouped if explicit else pr.posterior_filter_records_grouped)(**a)


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP))
def test_model_mismatches_are_rejected_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        a = _records(COMMON[what](make), explicit)
        with pytest.raises(ValueError):
            (pr.filter_records_grouped if explicit else pr.posterior_filter_records_grouped)(**a, **EMISSION)


def test_linear_kernels_are_rejected_by_the_moment_limits(no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError, match="SquaredExponential"):
            (pr.filter_records_grouped if explicit else pr.posterior_filter_records_grouped)(**_records(COMMON["LinearK"](make), explicit), **EMISSION)


NANS = np.full((R, STEPS, 1), np.nan)
BAD = {
    "observations with two axes": dict(Y_records=np.zeros((STEPS, 1))),
    "observations with four axes": dict(Y_records=np.zeros((R, STEPS, 1, 1))),
    "no records": dict(Y_records=np.zeros((0, STEPS, 1)), control_records=np.zeros((0, STEPS, 1))),
    "no rows": dict(Y_records=np.zeros((R, 0, 1)), control_records=np.zeros((R, 0, 1))),
    "observations of another J": dict(Y_records=np.zeros((R, STEPS, 2))),
    "an infinite observation": dict(Y_records=np.where(np.arange(R * STEPS).reshape(R, STEPS, 1) == 5, np.inf, 0.0)),
    "a minus-infinite observation": dict(Y_records=np.where(np.arange(R * STEPS).reshape(R, STEPS, 1) == 7, -np.inf, 0.0)),
    "controls of another R": dict(control_records=np.zeros((R + 1, STEPS, 1))),
    "controls of another length": dict(control_records=np.zeros((R, STEPS + 1, 1))),
    "controls of another width": dict(control_records=np.zeros((R, STEPS, 2))),
    "controls of one record": dict(control_records=np.zeros((STEPS, 1))),
    "no controls for a model that has them": dict(control_records=None),
    "a control row inside a record that is not finite": dict(control_records=np.where(np.arange(R * STEPS).reshape(R, STEPS, 1) == 2, np.nan, 0.0)),
    "lengths of another R": dict(lengths=[STEPS] * (R + 1)),
    "a scalar length": dict(lengths=STEPS),
    "a length of zero": dict(lengths=[STEPS, 0, STEPS]),
    "a negative length": dict(lengths=[STEPS, -1, STEPS]),
    "a length beyond the rows": dict(lengths=[STEPS, STEPS + 1, STEPS]),
    "a fractional length": dict(lengths=[STEPS, 2.5, STEPS]),
    "an observation beyond a record's length": dict(lengths=[STEPS, 2, STEPS]),
    "a partly observed row beyond a record's length": dict(lengths=[STEPS, STEPS, 3], CC=np.ones((2, 2)), DD=np.zeros(2), log_Rchols=np.zeros(2),
                                                            Y_records=np.concatenate((np.zeros((R, STEPS, 1)), NANS), axis=2)),
    "negative records_per_pass": dict(records_per_pass=-1),
    "a fractional records_per_pass": dict(records_per_pass=1.5),
    "x0s of another R": dict(x0s=np.zeros((R + 1, 2))),
    "x0s of another D": dict(x0s=np.zeros((R, 3))),
    "x0s of another G": dict(x0s=np.zeros((2, R, 2))),
    "x0s of one state": dict(x0s=np.zeros(2)),
    "S0s of another R": dict(S0s=np.zeros((R + 1, 2, 2))),
    "S0s of another D": dict(S0s=np.zeros((R, 3, 3))),
    "S0s of another G": dict(S0s=np.zeros((2, R, 2, 2))),
    "S0s of one state": dict(S0s=np.zeros((2, 2))),
    "an S0 that is not symmetric": dict(S0s=np.tile(np.array([[1.0, 0.5], [0.4, 1.0]]), (R, 1, 1))),
    "an S0 that is not finite": dict(S0s=np.full((3, R, 2, 2), np.nan)),
    "CC of another D": dict(CC=np.ones((3, 1))),
    "J = 9": dict(CC=np.ones((2, 9)), DD=np.zeros(9), log_Rchols=np.zeros((9, 9)), Y_records=np.zeros((R, STEPS, 9))),
    "a noise deviation that is not finite": dict(log_Rchols=np.full((1, 1), np.inf)),
    "unknown q_mode": dict(q_mode="slice0"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_records_start_and_emission_are_checked_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **BAD[what])


def test_the_explicit_call_needs_start_means_and_the_messages_name_the_argument(no_device):
    with pytest.raises(ValueError, match="x0s"):
        _call(True, x0s=None)
    for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                     (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records"),
                     (dict(lengths=[STEPS, 2, STEPS]), "Y_records"), (dict(S0s=np.zeros((2, 2))), "S0s")):
        for explicit in (True, False):
            with pytest.raises(ValueError, match=name):
                _call(explicit, **kw)


def test_well_formed_arguments_and_the_broadcast_forms_reach_the_library(monkeypatch):
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    S0 = np.array([[1.0, 0.5], [0.5, 1.0]])
    Y = np.zeros((R, STEPS, 1))
    Y[1, 2:] = np.nan
    Y[0, 1] = np.nan
    forms = [dict(), dict(x0s=np.zeros((R, 2))), dict(x0s=np.zeros((3, R, 2))), dict(S0s=np.tile(S0, (R, 1, 1))), dict(S0s=np.tile(S0, (3, R, 1, 1))),
             dict(Y_records=Y, lengths=[STEPS, 2, STEPS]), dict(Y_records=Y, lengths=np.array([STEPS, 3, STEPS])), dict(Y_records=Y),
             dict(lengths=[STEPS, 2.0, STEPS], Y_records=Y), dict(records_per_pass=2), dict(smooth=True, q_mode="intent", Y_train_std=1.7)]
    for kw in forms:
        for explicit in (True, False):
            with pytest.raises(Reached):
                _call(explicit, **kw)
    with pytest.raises(Reached):                                  # the fused call may leave the start to the training states
        _call(False, x0s=None)
    for explicit, make in ((True, _explicit), (False, _fused)):   # a model without control inputs takes None
        a = _records(make(C=0), explicit)
        assert a["control_records"] is None
        with pytest.raises(Reached):
            (pr.filter_records_grouped if explicit else pr.posterior_filter_records_grouped)(**a, **EMISSION)
    for f in (pr.filter_records_grouped, pr.posterior_filter_records_grouped):
        sig = inspect.signature(f).parameters
        for k, d in (("lengths", None), ("S0s", None), ("q_mode", "reference"), ("smooth", False), ("Y_train_std", 1.0), ("records_per_pass", 0)):
            assert sig[k].default == d and sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
        assert "method" not in sig
    assert list(inspect.signature(pr.filter_records_grouped).parameters)[:12] == [
        "Lm_inverse_seqs", "Zs", "kerns", "U_vals", "q_sqrts", "x0s", "control_records", "Y_records", "Qs", "CC", "DD", "log_Rchols"]
    assert "not re-weighted" in pr.filter_grouped.__doc__ and "EQUAL weights" in pr.filter_records_grouped.__doc__


def test_the_packing_masks_the_rows_beyond_a_record():
    Y = np.zeros((R, STEPS, 1))
    Y[1, 2:] = np.nan
    ctrl = np.ones((R, STEPS, 1))
    ctrl[1, 3] = np.nan                                           # (not read: beyond the record)
    r = pr._pack_records("t", 3, 2, 1, np.arange(R * 2.0).reshape(R, 2), ctrl, Y, [STEPS, 2, STEPS], None, 0)
    assert r["live"].tolist() == [[True] * 4, [True, True, False, False], [True] * 4]
    assert np.all(r["ctrl"][1, 2:] == 0.0) and np.all(r["ctrl"][r["live"]] == 1.0) and np.all(ctrl[1, :3] == 1.0)
    assert r["x0"].shape == (3, R, 2) and np.array_equal(r["x0"][2], np.arange(R * 2.0).reshape(R, 2)) and r["x0"].flags.c_contiguous
    assert r["S0"] is None and r["lengths"].tolist() == [4, 2, 4] and (r["R"], r["steps"], r["J"], r["rpp"]) == (R, STEPS, 1, 0)
    out = dict(m_pred=np.zeros((3, R * STEPS, 2)), S_pred=np.zeros((3, R * STEPS, 2, 2)), lpd_joint=np.zeros((3, R * STEPS)),
               predict_y=np.zeros((R * STEPS, 1)), lpd_mix=np.where(np.isnan(Y), np.nan, -1.0).reshape(R * STEPS, 1))
    res = pr._records_dict(r, 3, out, 1.0)
    assert res["m_pred"].shape == (3, R, STEPS, 2) and res["S_pred"].shape == (3, R, STEPS, 2, 2) and res["predict_y"].shape == (R, STEPS, 1)
    for k in ("m_pred", "S_pred", "lpd_joint"):
        assert np.all(np.isnan(res[k][:, 1, 2:])) and np.all(np.isfinite(res[k][:, 1, :2])) and np.all(np.isfinite(res[k][:, [0, 2]])), k
    assert np.all(np.isnan(res["predict_y"][1, 2:])) and np.all(np.isfinite(res["predict_y"][1, :2]))
    assert res["ll"].tolist() == [-1.0] * R and res["RMSE"].tolist() == [0.0] * R and res["ll_all"] == -1.0 and res["ll_joint"].shape == (R,)


def test_the_filter_dict_keeps_its_scalars():
    """`_filter_dict`'s scalars were moved into `_filter_scalars`: the definitions, restated"""
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((40, 2))
    Y[3] = np.nan
    Y[5, 0] = np.nan
    out = dict(lpd_mix=np.where(np.isnan(Y), np.nan, rng.standard_normal(Y.shape)), lpd_joint=rng.standard_normal((3, 40)),
               predict_y=rng.standard_normal(Y.shape))
    res = pr._filter_dict(dict(Y=Y), out, 1.7)
    seen = ~np.isnan(Y)
    rows = seen.any(axis=1)
    lj = out["lpd_joint"][:, rows]
    assert res["ll"] == float(np.mean(out["lpd_mix"][seen])) and res["ll_original_units"] == res["ll"] - float(np.log(1.7))
    assert res["ll_joint"] == pytest.approx(float(np.mean(np.log(np.mean(np.exp(lj), axis=0)))), rel=1e-13)
    s30 = seen[:30]
    assert res["RMSE"] == float(np.sqrt(np.mean((Y[:30][s30] - out["predict_y"][:30][s30]) ** 2)) * 1.7)
    assert set(res) == set(out) | {"ll", "ll_joint", "ll_original_units", "RMSE"}
    empty = pr._filter_dict(dict(Y=np.full((3, 1), np.nan)), dict(lpd_mix=np.full((3, 1), np.nan), lpd_joint=np.full((2, 3), np.nan),
                                                                 predict_y=np.zeros((3, 1))), 1.0)
    assert all(np.isnan(empty[k]) for k in ("ll", "ll_joint", "ll_original_units", "RMSE"))


# ---- model level -----------------------------------------------------------------------------------------------------------------------
class _Layer:
    def __init__(self, C, U):
        self.Z, self.kernel, self.U = np.zeros((5, 2 + C)), _explicit(C=C)["kerns"], U


class _Lik:
    CC, DD, log_Rchols = EMISSION["CC"], EMISSION["DD"], EMISSION["log_Rchols"]


class _Model:
    """a stand-in for DGPSSM: what filter_records reads"""
    _host_stale = False
    num_chains, output_dim = 3, 2
    Y = np.zeros((6, 1))
    Q = np.ones(2)
    likelihood = _Lik()

    def __init__(self, C=1, U_collapse=True):
        self.U_collapse = U_collapse
        self.layers = [_Layer(C, np.zeros((5, 2)))]
        self.control_inputs = np.zeros((6, C))
        self._X_chains = [np.full((7, 2), float(s)) for s in range(3)]


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    sig = inspect.signature(DGPSSM.filter_records).parameters
    assert list(sig) == ["self", "Y_records", "control_records", "lengths", "x0", "S0", "smooth", "q_mode", "Y_train_std", "records_per_pass"]
    assert sig["control_records"].default is None and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, None, False, "reference", 1.0, 0]
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    with pytest.raises(ValueError, match="q_mode"):
        DGPSSM.filter_records(_Model(), Y, ctrl, q_mode="slice0")
    for bad in (np.zeros((STEPS, 1)), np.zeros((R, STEPS, 2)), np.zeros((0, STEPS, 1))):
        with pytest.raises(ValueError, match="Y_records"):
            DGPSSM.filter_records(_Model(), bad, ctrl)
    with pytest.raises(ValueError, match="control_records"):     # a fresh trial has no default controls
        DGPSSM.filter_records(_Model(), Y)
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((2, R, 2)), np.zeros((3, R, 3))):
        with pytest.raises(ValueError, match="x0"):
            DGPSSM.filter_records(_Model(), Y, ctrl, x0=bad)
    with pytest.raises(ValueError, match="S0"):
        DGPSSM.filter_records(_Model(), Y, ctrl, S0=np.zeros((R, 2)))
    seen = {}
    monkeypatch.setattr(pr, "posterior_filter_records_grouped", lambda *a, **kw: seen.update(fused=(a, kw)) or "fused")
    monkeypatch.setattr(pr, "filter_records_grouped", lambda *a, **kw: seen.update(explicit=(a, kw)) or "explicit")
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    m = _Model()
    assert DGPSSM.filter_records(m, Y, ctrl, lengths=[4, 2, 4], smooth=True, records_per_pass=2, Y_train_std=1.7) == "fused"
    a, kw = seen["fused"]
    assert a[0] is m.layers[0].Z and a[2] == m._X_chains and a[4] is m.control_inputs and a[5] is ctrl and np.array_equal(a[6], Y)
    assert kw == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", smooth=True, Y_train_std=1.7, records_per_pass=2, x0s=None)
    for x0, S0 in ((np.arange(2.0), np.eye(2)), (np.zeros((R, 2)), np.zeros((R, 2, 2))), (np.zeros((3, R, 2)), np.zeros((3, R, 2, 2)))):
        DGPSSM.filter_records(m, Y, ctrl, x0=x0, S0=S0)
        kw = seen["fused"][1]
        assert kw["x0s"].shape == (3, R, 2) and kw["S0s"].shape == (3, R, 2, 2) and np.array_equal(kw["x0s"][1, 2], np.broadcast_to(x0, (3, R, 2))[1, 2])
    e = _Model(U_collapse=False)
    assert DGPSSM.filter_records(e, Y, ctrl) == "explicit"
    a, kw = seen["explicit"]
    assert a[0] == "Lm" and a[3] == [e.layers[0].U] * 3 and a[4] is None and a[6] is ctrl and "x0s" not in kw and kw["S0s"] is None
    assert a[5].shape == (3, R, 2) and all(np.all(a[5][s] == float(s)) for s in range(3))        # every record at its chain's last state
    DGPSSM.filter_records(e, Y, ctrl, x0=np.arange(2.0))
    assert np.array_equal(seen["explicit"][0][5], np.broadcast_to(np.arange(2.0), (3, R, 2)))
    assert DGPSSM.filter_records(_Model(C=0), Y) == "fused" and seen["fused"][0][5] is None        # no controls: None is what it takes


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/ffvd_abi.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbols_are_declared_beside_the_single_record_ones_and_bound():
    for new, old in zip(SYMBOLS, ("ffvd_op_filter_linear_grouped", "ffvd_op_posterior_filter_linear_grouped")):
        d, o = _declaration(new), _declaration(old)
        assert [a for a in d if a not in ("int R", "int records_per_pass")] == o
        assert d.index("int R") == d.index("int q_mode") + 1 and d.index("int records_per_pass") == d.index("const double *Y_obs") + 1
        sig, osig = _lib._SIGNATURES[new], _lib._SIGNATURES[old]
        assert sig[0] is ctypes.c_int and len(sig[1]) == len(d) == len(osig[1]) + 2
        ints = [i for i, a in enumerate(d) if a.startswith("int ")]
        assert [i for i, t in enumerate(sig[1]) if t is ctypes.c_int] == ints
        assert new in _lib.exported_symbols()
    text = open(HEADER).read()
    assert "x_lasts G x R x D" in text and "G * R * steps * D * D < 2^31" in text


def test_the_symbols_are_exported():
    for s in SYMBOLS:
        assert hasattr(_lib.load(), s)


OUT_NAMES = ("mp", "Sp", "mf", "Sf", "X_", "lpd", "lj", "ms", "Ss", "ym", "yt", "lm", "lg")


def _abi(fused, *, G=2, R=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=3, kind=0, gpp=0, q_mode=0, J=1, rpp=0, null=(), sd=1.0, y=0.0,
         small=False):
    """One ABI call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL; small: the arrays are
    not sized by R and steps (calls that must return before anything is read)."""
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
        rc = lib.ffvd_op_posterior_filter_records_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"], 1e-5,
                                                          gpp, q_mode, R, None, None, p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_op_filter_records_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, q_mode, R, p["xl"], None,
                                                p["cr"], C, steps, p["lq"], *tail)
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
        assert rc == E and b"many records" in msg and b"SE kernel only" in msg
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
