"""Argument checks of the linearised filter, without a GPU: `method` of prediction.filter_grouped / posterior_filter_grouped is checked
in the packing stage, before the library is loaded ("moment" and "linearised" are accepted, the message names them);
forecast_grouped / posterior_forecast_grouped take "moment" only (the fan has no linearised rule) and reject everything else the same
way; DGPSSM.filter_heldout keeps its pinned parameter list and DGPSSM.filter_heldout_linearised has the same one;
ffvd_op_filter_linear_grouped / ffvd_op_posterior_filter_linear_grouped are declared in the header with the argument lists of the
moment-matching entry points, are exported where the library is built, and reject what those reject (the cases, the call and the
helpers of tests/test_filter_grouped_args.py, imported, through a stand-in that hands them the new symbols)."""
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import BAD_ABI, E, EMISSION, _abi, _filter_args, no_device  # noqa: F401  (no_device: a fixture)
from test_moment_grouped_args import _explicit, _fused

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffvd_abi.h")
NEW = {"ffvd_op_filter_grouped": "ffvd_op_filter_linear_grouped", "ffvd_op_posterior_filter_grouped": "ffvd_op_posterior_filter_linear_grouped"}
BAD_METHODS = ("ekf", "linearized", "Moment", "", None, 1, b"moment")


def _calls():
    """(function, well-formed keyword arguments) of the four prediction-level calls that take `method`"""
    fe, ff = _filter_args(_explicit(), True), _filter_args(_fused(), False)
    return [(pr.filter_grouped, dict(fe, **EMISSION)), (pr.posterior_filter_grouped, dict(ff, **EMISSION)),
            (pr.forecast_grouped, dict(fe, **EMISSION, horizon=1)), (pr.posterior_forecast_grouped, dict(ff, **EMISSION, horizon=1))]


@pytest.mark.parametrize("method", BAD_METHODS, ids=repr)
def test_an_unknown_method_raises_before_the_library_is_loaded(method, no_device):
    for f, kw in _calls():
        with pytest.raises(ValueError, match="method") as info:
            f(**kw, method=method)
        assert "'moment'" in str(info.value) and "'linearised'" in str(info.value), f.__name__


def test_the_forecast_fan_rejects_the_linearised_method_before_the_library_is_loaded(no_device):
    for f, kw in _calls()[2:]:
        with pytest.raises(ValueError, match="method") as info:
            f(**kw, method="linearised")
        assert "forecast" in str(info.value) and "'moment'" in str(info.value)


def test_the_accepted_methods_reach_the_library(monkeypatch):
    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(_lib, "load", reached)
    calls = _calls()
    for f, kw in calls:
        with pytest.raises(Reached):
            f(**kw)
        with pytest.raises(Reached):
            f(**kw, method="moment")
    for f, kw in calls[:2]:
        for smooth in (False, True):
            with pytest.raises(Reached):
                f(**kw, method="linearised", smooth=smooth)
    for f, _ in calls:
        par = inspect.signature(f).parameters["method"]
        assert par.default == "moment" and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert pr.FILTER_METHODS == ("moment", "linearised")


def test_the_model_level_calls():
    from ffvd_amd.dgp_model import DGPSSM
    a, b = inspect.signature(DGPSSM.filter_heldout).parameters, inspect.signature(DGPSSM.filter_heldout_linearised).parameters
    assert list(a) == list(b) and all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a if k != "self")

    class Stub:
        _host_stale = False
        Y = np.zeros((4, 1))

    for f in (DGPSSM.filter_heldout, DGPSSM.filter_heldout_linearised):          # stopped before any parameter or device is touched
        with pytest.raises(ValueError, match="q_mode"):
            f(Stub(), np.zeros((2, 1)), q_mode="slice0")
        with pytest.raises(ValueError, match="Y_test"):
            f(Stub(), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="method"):
        DGPSSM._filter_heldout(Stub(), "filter_heldout", "ekf", np.zeros((2, 1)), None, None, None, False, "reference", 1.0)


def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/ffvd_abi.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_new_symbols_are_declared_with_the_argument_lists_of_the_existing_ones():
    for old, new in NEW.items():
        assert _declaration(new) == _declaration(old)
        assert _lib._SIGNATURES[new] == _lib._SIGNATURES[old]
    text = open(HEADER).read()
    assert "A S A^T + diag(v + Q)" in text and "cross_t = S A^T" in text


def test_the_new_symbols_are_exported_and_bound():
    for s in NEW.values():
        assert s in _lib.exported_symbols() and hasattr(_lib.load(), s)


class _Linear:
    """The library with the linearised entry points under the names of the moment-matching ones (for the imported `_abi`)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, NEW.get(name, name))


@pytest.fixture
def linear_lib(monkeypatch):
    lib = _lib.load()
    monkeypatch.setattr(_lib, "load", lambda: _Linear(lib))
    return lib


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused, linear_lib):
    rc, outs = _abi(fused, **ov)
    assert rc == E, rc
    who = NEW["ffvd_op_posterior_filter_grouped" if fused else "ffvd_op_filter_grouped"]
    assert who.encode() + b": bad argument" in linear_lib.ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_other_kernels_are_refused_with_a_message_that_says_why(linear_lib):
    for fused in (False, True):
        for kind in (1, 2):
            rc, _ = _abi(fused, kind=kind)
            msg = linear_lib.ffvd_last_error(None)
            assert rc == E and b"linearised filter" in msg and b"SE kernel only" in msg


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov, linear_lib):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())
