"""Argument checks of the fully adapted particle filter over many records, without a GPU: the checks of
tests/test_filter_particle_args.py for prediction.filter_adapted_records_grouped / posterior_filter_adapted_records_grouped and
DGPSSM.filter_records_adapted.  They share the bootstrap pair's packing (`_pack_records`, `_pack_particles`), so every malformed
argument raises ValueError before the library is loaded and the message names the adapted function; well-formed arguments in all three
layouts of the draws reach ffvd_particle_adapted_records_grouped / ffvd_posterior_particle_adapted_records_grouped, which are
declared in the header with the bootstrap pair's argument lists, bound in _lib.py, exported where the library is built, and return
FFVD_EINVAL before any device call beyond their limits (FFVD_OK for no groups, records or rows)."""
import ctypes
import inspect

import numpy as np
import pytest

import test_filter_particle_args as tp
from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_filter_records_args import BAD, R, SKIP, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import COMMON, _explicit, _fused, _with

SYMBOLS = ("ffvd_particle_adapted_records_grouped", "ffvd_posterior_particle_adapted_records_grouped")
BOOTSTRAP = ("ffvd_op_filter_particle_records_grouped", "ffvd_op_posterior_filter_particle_records_grouped")
G, D, N, S0, _draws = tp.G, tp.D, tp.N, tp.S0, tp._draws


def _fn(explicit):
    return pr.filter_adapted_records_grouped if explicit else pr.posterior_filter_adapted_records_grouped


def _call(explicit, **kw):
    a = _with(_with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **_draws()), **kw)
    if "Y_records" in kw and "eps" not in kw and np.ndim(kw["Y_records"]) == 3 and np.shape(kw["Y_records"])[1] != STEPS:
        a.update(_draws(steps=np.shape(kw["Y_records"])[1]))
    return _fn(explicit)(**a)


@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP))
def test_model_mismatches_are_rejected_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError):
            _fn(explicit)(**_records(COMMON[what](make), explicit), **EMISSION, **_draws())


def test_linear_kernels_are_rejected_by_the_moment_limits(no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError, match="SquaredExponential"):
            _fn(explicit)(**_records(COMMON["LinearK"](make), explicit), **EMISSION, **_draws())


@pytest.mark.parametrize("what", sorted(BAD))
def test_every_error_of_the_records_packing_raises_before_the_library_is_loaded(what, no_device):
    kw = dict(BAD[what])
    if "S0s" in kw:
        kw["xi0"] = np.zeros((N, D))                              # (so that the start covariance itself is what is refused)
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **kw)


@pytest.mark.parametrize("what", sorted(tp.BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "filter_adapted_records_grouped: (eps|unif|xi0|return_particles)"):
            _call(explicit, **tp.BAD_DRAWS[what])


def test_the_messages_name_the_function_and_the_argument(no_device):
    with pytest.raises(ValueError, match="filter_adapted_records_grouped: x0s"):
        _call(True, x0s=None)
    for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                     (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records"),
                     (_draws(n=1), r"eps: the number of particles N must lie in \[2, 2048\]"), (dict(S0s=S0), "xi0")):
        for explicit in (True, False):
            who = ("" if explicit else "posterior_") + "filter_adapted_records_grouped"
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call(explicit, **kw)


def test_well_formed_arguments_in_every_layout_reach_the_adapted_symbols(monkeypatch):
    class Reached(Exception):
        pass
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                seen.append((name, a))
                raise Reached()
            return f
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    Y = np.zeros((R, STEPS, 1))
    Y[1, 2:] = np.nan
    inner = STEPS * N * D
    layouts = (((), (0, 0), (0, 0), (0, 0)), ((R,), (0, inner), (0, STEPS), (0, N * D)),
               ((G, R), (R * inner, inner), (R * STEPS, STEPS), (R * N * D, N * D)))
    for lead, es, us, xs in layouts:
        for kw in (dict(), dict(Y_records=Y, lengths=[STEPS, 2, STEPS], records_per_pass=2, q_mode="intent", Y_train_std=1.7),
                   dict(S0s=S0, xi0=np.zeros(lead + (N, D)), return_particles=True)):
            for explicit in (True, False):
                with pytest.raises(Reached):
                    _call(explicit, **_draws(lead=lead), **kw)
                name, a = seen[-1]
                assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
                p = 26 if explicit else 28                        # N follows records_per_pass
                assert a[p] == N and (a[p + 2], a[p + 3]) == es and (a[p + 5], a[p + 6]) == us
                assert (a[p + 8], a[p + 9]) == (xs if "xi0" in kw else (0, 0)) and (a[p + 7] is None) == ("xi0" not in kw)
                tail = a[p + 10:] if explicit else a[p + 10:-1]
                assert len(tail) == 14 and (tail[12] is None) == (tail[13] is None) == ("return_particles" not in kw)
                assert all(t is not None for t in tail[:12])
    with pytest.raises(Reached):                                  # the fused call may leave the start to the training states
        _call(False, x0s=None)
    with pytest.raises(Reached):                                  # R = 1: a single record
        _call(True, Y_records=Y[:1], control_records=np.zeros((1, STEPS, 1)), x0s=np.zeros((1, 2)))
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_the_signatures_are_the_bootstrap_pair_s(no_device):
    for new, old in ((pr.filter_adapted_records_grouped, pr.filter_particle_records_grouped),
                     (pr.posterior_filter_adapted_records_grouped, pr.posterior_filter_particle_records_grouped)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        assert list(a) == list(b)
        assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    doc = pr.filter_adapted_records_grouped.__doc__
    for words in ("optimal proposal", "Pitt & Shephard", "X_{t+1}", "carried INTO row t", "log_evidence", "bit for bit"):
        assert words in doc, words
    assert "X_{t+1}" in pr.posterior_filter_adapted_records_grouped.__doc__


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    sig, old = inspect.signature(DGPSSM.filter_records_adapted).parameters, inspect.signature(DGPSSM.filter_records_particle).parameters
    assert list(sig) == list(old) and all(sig[k].default == old[k].default and sig[k].kind == old[k].kind for k in sig)
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    for kw, msg in ((dict(noise="common"), "filter_records_adapted: noise"), (dict(noise=None), "filter_records_adapted: noise"),
                    (dict(num_particles=1), "filter_records_adapted: num_particles"), (dict(num_particles=2049), "num_particles"),
                    (dict(num_particles=64.0), "num_particles"), (dict(num_particles=True), "num_particles"),
                    (dict(q_mode="slice0"), "filter_records_adapted: q_mode"), (dict(x0=np.zeros(3)), "x0")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.filter_records_adapted(_Model(), Y, ctrl, seed=1, **kw)
    with pytest.raises(ValueError, match="filter_records_adapted: Y_records"):
        DGPSSM.filter_records_adapted(_Model(), np.zeros((STEPS, 1)), ctrl, seed=1)
    with pytest.raises(ValueError, match="control_records"):
        DGPSSM.filter_records_adapted(_Model(), Y, seed=1)
    big, n = np.zeros((400, 200, 1)), 2048
    nbytes = 8 * 3 * 400 * (200 * n * 2 + 200)
    with pytest.raises(ValueError, match=f"{nbytes} bytes"):
        DGPSSM.filter_records_adapted(_Model(), big, np.zeros((400, 200, 1)), num_particles=n, seed=1, noise="independent")
    seen = {}
    names = ("posterior_filter_adapted_records_grouped", "filter_adapted_records_grouped", "posterior_filter_particle_records_grouped",
             "filter_particle_records_grouped")
    for name in names:
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    m, e = _Model(), _Model(U_collapse=False)
    kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7)
    rng = np.random.default_rng(5)
    want = dict(eps=rng.standard_normal((STEPS, 16, 2)), unif=rng.random((STEPS,)))
    assert DGPSSM.filter_records_adapted(m, Y, ctrl, num_particles=16, seed=5, **kw) == "posterior_filter_adapted_records_grouped"
    a, k = seen["posterior_filter_adapted_records_grouped"]
    assert k == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", Y_train_std=1.7, records_per_pass=2, x0s=None, xi0=None, return_particles=False)
    assert len(a) == 12 and np.array_equal(a[10], want["eps"]) and np.array_equal(a[11], want["unif"])
    # the same seed gives the bootstrap call the same draws in the same order
    for noise, lead in (("per_record", (R,)), ("independent", (3, R))):
        args = dict(num_particles=16, seed=5, noise=noise, S0=np.eye(2), x0=np.arange(2.0), return_particles=True)
        assert DGPSSM.filter_records_adapted(e, Y, ctrl, **args) == "filter_adapted_records_grouped"
        assert DGPSSM.filter_records_particle(e, Y, ctrl, **args) == "filter_particle_records_grouped"
        (a, k), (b, kb) = seen["filter_adapted_records_grouped"], seen["filter_particle_records_grouped"]
        assert a[0] == "Lm" and a[5].shape == (3, R, 2) and len(a) == 14 and a[12].shape == lead + (STEPS, 16, 2) and a[13].shape == lead + (STEPS,)
        assert k["xi0"].shape == lead + (16, 2) and k["S0s"].shape == (3, R, 2, 2) and k["return_particles"] is True and "smooth" not in k
        assert np.array_equal(a[12], b[12]) and np.array_equal(a[13], b[13]) and np.array_equal(k["xi0"], kb["xi0"])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_with_the_bootstrap_argument_lists_and_bound():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, BOOTSTRAP):
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols()
        assert not new.startswith("ffvd_op_")
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")
        assert _declaration(new) == _declaration(old)
        assert _lib._SIGNATURES[new][1] == _lib._SIGNATURES[old][1]
    for words in ("Pitt & Shephard", "optimal proposal", "FILTERED set", "carried INTO row t", "a pivot <= 0 gives a zero column"):
        assert words in text, words


def test_the_symbols_are_exported():
    for s in SYMBOLS:
        assert hasattr(_lib.load(), s)


class _Adapted:
    """the library with the two bootstrap entry points answered by the adapted ones: tests/test_filter_particle_args.py's `_abi` as is"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, dict(zip(BOOTSTRAP, SYMBOLS)).get(name, name))


def _abi(monkeypatch, fused, **ov):
    lib = _lib.load()
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "load", lambda: _Adapted(lib))
        return tp._abi(fused, **ov)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", tp.BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused, monkeypatch):
    rc, outs = _abi(monkeypatch, fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


def test_the_messages_say_why(monkeypatch):
    lib = _lib.load()
    for fused in (False, True):
        rc, _ = _abi(monkeypatch, fused, kind=1)
        msg = lib.ffvd_last_error(None)
        assert rc == E and b"adapted particle filter of many records" in msg and b"SE kernel only" in msg
        rc, _ = _abi(monkeypatch, fused, G=2, R=1 << 20, steps=1 << 8, small=True)
        assert rc == E and b"G * R * steps * D * D < 2^31" in lib.ffvd_last_error(None)
        rc, _ = _abi(monkeypatch, fused, n=2049)
        assert rc == E and b"2 <= N <= 2048" in lib.ffvd_last_error(None)
    for ov in (dict(null=("f",)), dict(null=("xl",)), dict(null=("W",))):
        assert _abi(monkeypatch, False, **ov)[0] == E
    for ov in (dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))):
        assert _abi(monkeypatch, True, **ov)[0] == E


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(fused, ov, monkeypatch):
    rc, outs = _abi(monkeypatch, fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
