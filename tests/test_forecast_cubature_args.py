"""Argument checks of the cubature forecasts, without a GPU: ffvd_op_forecast_cubature_grouped /
ffvd_op_posterior_forecast_cubature_grouped are declared in the header with the argument lists of the linearised (and hence the
moment-matching) forecast entry points, are bound and exported where the library is built, and reject what those reject (the cases,
the call and the helpers of tests/test_forecast_grouped_args.py, imported, through a stand-in that hands them the new symbols):
shapes, the origin rules, horizon, tracks_per_pass; LinearK and Matern are refused with a message that names the cubature forecasts;
prediction.forecast_cubature_grouped / posterior_forecast_cubature_grouped take the parameters of the linearised functions name by
name and raise ValueError before the library is loaded for everything those reject; FILTER_METHODS keeps its two entries and
forecast_grouped(method=...) keeps raising for anything but "moment"; DGPSSM.forecast_heldout and forecast_heldout_linearised keep
their pinned parameter lists and DGPSSM.forecast_heldout_cubature has the same one."""
import inspect
import os
import re

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import BAD_FILTER, EMISSION, SKIP, _filter_args
from test_forecast_grouped_args import BAD_BOTH, BAD_PUBLIC, E, _abi, no_device  # noqa: F401  (no_device: a fixture)
from test_moment_grouped_args import BAD_EXPLICIT, BAD_FUSED, COMMON, _explicit, _fused, _with

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffvd_abi.h")
NEW = {"ffvd_op_forecast_grouped": "ffvd_op_forecast_cubature_grouped",
       "ffvd_op_posterior_forecast_grouped": "ffvd_op_posterior_forecast_cubature_grouped"}
PAIRS = ((pr.forecast_linear_grouped, pr.forecast_cubature_grouped), (pr.posterior_forecast_linear_grouped, pr.posterior_forecast_cubature_grouped))


# ---- the header, the ctypes table, the library ---------------------------------------------------------------------------------------
def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/ffvd_abi.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_new_symbols_are_declared_with_the_argument_lists_of_the_existing_ones():
    for old, new in NEW.items():
        assert _declaration(new) == _declaration(old) == _declaration(old.replace("forecast_grouped", "forecast_linear_grouped"))
        assert _lib._SIGNATURES[new] == _lib._SIGNATURES[old]
    assert "mu' = mu + mbar" in open(HEADER).read()


def test_the_new_symbols_are_exported_and_bound():
    for s in NEW.values():
        assert s in _lib.exported_symbols() and hasattr(_lib.load(), s)


class _Cubature:
    """The library with the cubature entry points under the names of the moment-matching ones (for the imported `_abi`)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, NEW.get(name, name))


@pytest.fixture
def cubature_lib(monkeypatch):
    lib = _lib.load()
    monkeypatch.setattr(_lib, "load", lambda: _Cubature(lib))
    return lib


@pytest.mark.parametrize("ov", BAD_BOTH + [dict(null=("f",)), dict(null=("xl",)), dict(null=("W",))], ids=str)
def test_explicit_abi_rejects_bad_arguments_without_a_device(ov, cubature_lib):
    rc, outs = _abi(False, **ov)
    assert rc == E, rc
    assert b"ffvd_op_forecast_cubature_grouped: bad argument" in cubature_lib.ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


@pytest.mark.parametrize("ov", BAD_BOTH + [dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))], ids=str)
def test_fused_abi_rejects_bad_arguments_without_a_device(ov, cubature_lib):
    rc, outs = _abi(True, **ov)
    assert rc == E, rc
    assert b"ffvd_op_posterior_forecast_cubature_grouped: bad argument" in cubature_lib.ffvd_last_error(None)
    assert all(np.all(v == 7.0) for v in outs.values())


def test_other_kernels_are_refused_with_a_message_that_says_why(cubature_lib):
    for fused in (False, True):
        for kind in (1, 2):
            rc, _ = _abi(fused, kind=kind)
            msg = cubature_lib.ffvd_last_error(None)
            assert rc == E and b"cubature forecasts" in msg and b"SE kernel only" in msg


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(G=0, n_models=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov, cubature_lib):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7.0) for v in outs.values())


# ---- the public functions ------------------------------------------------------------------------------------------------------------
def _call(explicit, a, **kw):
    kw = dict(dict(horizon=1), **kw)
    return (pr.forecast_cubature_grouped if explicit else pr.posterior_forecast_cubature_grouped)(**_filter_args(a, explicit), **EMISSION, **kw)


def test_the_parameter_lists_are_those_of_the_linearised_forecasts_name_by_name():
    for old, new in PAIRS:
        a, b = inspect.signature(old).parameters, inspect.signature(new).parameters
        assert list(a) == list(b) and "method" not in b
        assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in b)
    assert "EQUAL weights" in pr.forecast_cubature_grouped.__doc__


def test_the_method_argument_of_the_family_is_what_it_was(no_device):
    assert pr.FILTER_METHODS == ("moment", "linearised")
    for explicit, make in ((True, _explicit), (False, _fused)):
        fn = pr.forecast_grouped if explicit else pr.posterior_forecast_grouped
        for method in ("cubature", "linearised", "ckf"):
            with pytest.raises(ValueError, match="method"):
                fn(**_filter_args(make(), explicit), **EMISSION, horizon=1, method=method)


@pytest.mark.parametrize("what", sorted(BAD_PUBLIC))
def test_public_functions_reject_the_forecast_arguments_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError):
            _call(explicit, make(), **BAD_PUBLIC[what])


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP) + sorted(BAD_EXPLICIT))
def test_explicit_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_explicit) if what in COMMON else BAD_EXPLICIT[what]()
    with pytest.raises(ValueError):
        _call(True, a)


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP) + sorted(BAD_FUSED))
def test_fused_call_rejects_mismatches_before_the_library_is_loaded(what, no_device):
    a = COMMON[what](_fused) if what in COMMON else BAD_FUSED[what]()
    with pytest.raises(ValueError):
        _call(False, a)


def test_linear_kernels_are_named(no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError, match="LinearK"):
            _call(explicit, COMMON["LinearK"](make))


def test_a_method_argument_is_not_taken(no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(TypeError, match="method"):
            _call(explicit, make(), method="cubature")


@pytest.mark.parametrize("what", sorted(BAD_FILTER))
def test_observations_and_emission_are_checked_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        a = _with(_with(_filter_args(make(), explicit), **EMISSION), **BAD_FILTER[what])
        with pytest.raises(ValueError):
            (pr.forecast_cubature_grouped if explicit else pr.posterior_forecast_cubature_grouped)(**a, horizon=1)


def test_well_formed_arguments_reach_the_new_symbols(monkeypatch):
    class Reached(Exception):
        pass

    class Lib:
        def __getattr__(self, name):
            raise Reached(name)
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    for explicit, make in ((True, _explicit), (False, _fused)):
        for kw in (dict(horizon=1), dict(horizon=3), dict(horizon=2, stride=2), dict(horizon=2, origins=[1]), dict(horizon=1, origins=[0, 2]),
                   dict(horizon=1, return_tracks=True, return_filter=True, tracks_per_pass=2)):
            with pytest.raises(Reached, match="ffvd_op_forecast_cubature_grouped" if explicit else "ffvd_op_posterior_forecast_cubature_grouped"):
                _call(explicit, make(), **kw)
        with pytest.raises(Reached):
            _call(explicit, make(C=0), horizon=2)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_the_model_level_calls():
    from ffvd_amd.dgp_model import DGPSSM
    a = inspect.signature(DGPSSM.forecast_heldout).parameters
    assert list(a) == ["self", "Y_test", "control_inputs", "horizon", "stride", "origins", "x0", "S0", "q_mode", "Y_train_std", "return_tracks"]
    for f in (DGPSSM.forecast_heldout_linearised, DGPSSM.forecast_heldout_cubature):
        b = inspect.signature(f).parameters
        assert list(a) == list(b) and all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a if k != "self")

    class Stub:
        _host_stale = False
        Y = np.zeros((4, 1))

    # stopped before any parameter or device is touched
    for f in (DGPSSM.forecast_heldout, DGPSSM.forecast_heldout_linearised, DGPSSM.forecast_heldout_cubature):
        with pytest.raises(ValueError, match="q_mode"):
            f(Stub(), np.zeros((2, 1)), q_mode="slice0")
        with pytest.raises(ValueError, match="Y_test"):
            f(Stub(), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="method"):
        DGPSSM._forecast_heldout(Stub(), "forecast_heldout", "ekf", np.zeros((2, 1)), None, 1, 1, None, None, None, "reference", 1.0, False)
