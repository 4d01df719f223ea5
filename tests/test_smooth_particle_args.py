"""Argument checks of the particle smoother over many records, without a GPU: prediction.smooth_particle_records_grouped /
posterior_smooth_particle_records_grouped take the parameters of the two particle filter functions and run their packing stages, so
every ValueError of tests/test_filter_particle_args.py fires before the library is loaded, under the new names; well-formed arguments
reach the two new symbols with `lengths` and the seven new outputs behind the filter's; DGPSSM.smooth_records_particle has the
parameters of filter_records_particle, draws what it draws and hands the two forms on; ffvd_particle_smooth_records_grouped /
ffvd_posterior_particle_smooth_records_grouped are declared in the header, bound in _lib.py and exported, and return FFVD_EINVAL
before any device call beyond their limits."""
import ctypes
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_filter_particle_args import BAD_DRAWS, D, G, N, S0, _draws
from test_filter_particle_args import SYMBOLS as FILTER_SYMBOLS
from test_filter_records_args import BAD, R, SKIP, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import COMMON, _explicit, _fused, _with

SYMBOLS = ("ffvd_particle_smooth_records_grouped", "ffvd_posterior_particle_smooth_records_grouped")
NEW = ["const int *lengths", "double *m_smooth", "double *S_smooth", "double *ess_smooth", "double *w_smooth", "double *weights",
       "double *trans_mean", "double *trans_var"]


def _fn(explicit):
    return pr.smooth_particle_records_grouped if explicit else pr.posterior_smooth_particle_records_grouped


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


@pytest.mark.parametrize("what", sorted(BAD))
def test_every_error_of_the_records_packing_raises_before_the_library_is_loaded(what, no_device):
    kw = dict(BAD[what])
    if "S0s" in kw:
        kw["xi0"] = np.zeros((N, D))
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **kw)


@pytest.mark.parametrize("what", sorted(BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "smooth_particle_records_grouped: (eps|unif|xi0|return_particles)"):
            _call(explicit, **BAD_DRAWS[what])


def test_the_messages_name_the_function_and_the_argument(no_device):
    with pytest.raises(ValueError, match="smooth_particle_records_grouped: x0s"):
        _call(True, x0s=None)
    for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                     (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records"),
                     (_draws(n=1), r"eps: the number of particles N must lie in \[2, 2048\]"), (dict(S0s=S0), "xi0")):
        for explicit in (True, False):
            who = ("" if explicit else "posterior_") + "smooth_particle_records_grouped"
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call(explicit, **kw)


def test_well_formed_arguments_reach_the_new_symbols_with_the_lengths_and_the_new_outputs(monkeypatch):
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
    for kw, lens in ((dict(), [STEPS] * R), (dict(Y_records=Y, lengths=[STEPS, 2, STEPS], records_per_pass=2), [STEPS, 2, STEPS]),
                     (dict(S0s=S0, xi0=np.zeros((N, D)), return_particles=True), [STEPS] * R)):
        for explicit in (True, False):
            with pytest.raises(Reached):
                _call(explicit, **kw)
            name, a = seen[-1]
            assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
            assert len(a) == len(_lib._SIGNATURES[FILTER_SYMBOLS[not explicit]][1]) + 8
            p = 26 if explicit else 28                            # N follows records_per_pass
            tail = a[p + 10:] if explicit else a[p + 10:-1]
            assert len(tail) == 22 and (tail[12] is None) == (tail[13] is None) == ("return_particles" not in kw)
            assert [tail[14][r] for r in range(R)] == lens        # int32 lengths, always sent
            assert all(t is not None for t in tail[15:18])        # m_smooth, S_smooth, ess_smooth
            assert all((t is None) == ("return_particles" not in kw) for t in tail[18:])
            assert explicit or a[-1] is None                      # U_means stays last
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_the_signatures_are_the_filter_functions(no_device):
    for new, old in ((pr.smooth_particle_records_grouped, pr.filter_particle_records_grouped),
                     (pr.posterior_smooth_particle_records_grouped, pr.posterior_filter_particle_records_grouped)):
        assert inspect.signature(new) == inspect.signature(old)
    doc = pr.smooth_particle_records_grouped.__doc__
    for words in ("m_smooth", "S_smooth", "ess_smooth", "w_smooth", "weights", "trans_mean", "trans_var", "Doucet", "exactly 0"):
        assert words in doc, words
    assert pr.FILTER_METHODS == ("moment", "linearised")
    assert "smooth_particle_records_grouped" in pr.filter_particle_records_grouped.__doc__


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    assert inspect.signature(DGPSSM.smooth_records_particle) == inspect.signature(DGPSSM.filter_records_particle)
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    for kw, msg in ((dict(noise="common"), "smooth_records_particle: noise"), (dict(num_particles=1), "smooth_records_particle: num_particles"),
                    (dict(q_mode="slice0"), "smooth_records_particle: q_mode"), (dict(x0=np.zeros(3)), "x0")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.smooth_records_particle(_Model(), Y, ctrl, seed=1, **kw)
    seen = {}
    names = ("posterior_smooth_particle_records_grouped", "smooth_particle_records_grouped", "posterior_filter_particle_records_grouped",
             "filter_particle_records_grouped")
    for name in names:
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7, num_particles=16, seed=5)
    for model, smooth, filt in ((_Model(), names[0], names[2]), (_Model(U_collapse=False), names[1], names[3])):
        assert DGPSSM.smooth_records_particle(model, Y, ctrl, **kw) == smooth
        assert DGPSSM.filter_records_particle(model, Y, ctrl, **kw) == filt
        (a, k), (b, kb) = seen[smooth], seen[filt]                # the same seed: the same draws, the same arguments
        assert k == kb and len(a) == len(b)
        assert np.array_equal(a[-2], b[-2]) and np.array_equal(a[-1], b[-1]) and a[-2].shape == (STEPS, 16, 2)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, FILTER_SYMBOLS):
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols() and hasattr(_lib.load(), new)
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")
        d, c = _declaration(new), _declaration(old)
        assert len(_lib._SIGNATURES[new][1]) == len(d)
        k = c.index("int *ancestors")
        assert d[:k + 1] == c[:k + 1] and d[k + 1:k + 9] == NEW and d[k + 9:] == c[k + 1:]     # (U_means stays last)
        sig, old_sig = _lib._SIGNATURES[new][1], _lib._SIGNATURES[old][1]
        assert sig[:k + 1] == old_sig[:k + 1] and sig[k + 9:] == old_sig[k + 1:]
        assert sig[k + 1] == ctypes.POINTER(ctypes.c_int) and all(t == ctypes.POINTER(ctypes.c_double) for t in sig[k + 2:k + 9])
    for words in ("Doucet", "w_smooth[n-1] = W_{n-1} / sum W_{n-1}", "no offspring: exactly 0", "nothing is renormalised", "(3 D + 3) N doubles"):
        assert words in text, words


def _abi(fused, *, G=2, R=2, M=4, D=2, C=1, T=5, steps=3, kind=0, J=1, n=4, lengths=None, null_new=False, null_all=False):
    """One call on zero inputs with every output buffer filled with 7"""
    P = D + C
    ng, nr, st, nn = max(G, 1), max(R, 1), max(steps, 1), min(max(n, 1), 4096)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((1, M, P)), lv=np.zeros((1, D)), ll=np.zeros((1, D, P)), X=np.zeros((ng, T + 1, D)), cf=np.zeros((T, C)),
             cr=np.zeros((nr, st, C)), lq=np.zeros((ng, D)), f=np.zeros((ng, M, D)), xl=np.zeros((ng, nr, D)), CC=np.ones((D, J)),
             DD=np.zeros(J), sd=np.ones(J), Y=np.zeros((nr, st, J)), eps=np.zeros((ng, nr, st, nn, D)), unif=np.full((ng, nr, st), 0.5))
    vec, mat, row = (ng, nr, st, D), (ng, nr, st, D, D), (ng, nr, st)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, lpd=row + (J,), lj=row, ym=(nr, st, J), yt=(nr, st, J), lm=(nr, st, J), lg=(nr, st, J),
                  ess=row, le=(ng, nr), par=row + (nn, D))
    new = dict(ms=vec, Ss=mat, es=row, ws=row + (nn,), W=row + (nn,), tm=row + (nn, D), tv=row + (nn, D))
    outs = {k: np.full(s, 7.0) for k, s in list(shapes.items()) + list(new.items()) + [("U", (ng, M, D))]}
    anc = np.full(row + (nn,), 7, dtype=np.int32)
    p = {k: dp(v) for k, v in list(a.items()) + list(outs.items())}
    ip = ctypes.POINTER(ctypes.c_int)
    lens = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    draws = (n, p["eps"], R * steps * n * D, steps * n * D, p["unif"], R * steps, steps, None, 0, 0)
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"], 0) + draws + tuple(None if null_all else p[k] for k in shapes) + \
        (None if null_all else anc.ctypes.data_as(ip), None if lens is None else lens.ctypes.data_as(ip)) + \
        tuple(None if null_new or null_all else p[k] for k in new)
    if fused:
        rc = lib.ffvd_posterior_particle_smooth_records_grouped(kind, G, 1, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"], 1e-5,
                                                                0, 0, R, None, None, p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(D)]
        Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_particle_smooth_records_grouped(kind, G, 1, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, 0, R, p["xl"], None, p["cr"],
                                                      C, steps, p["lq"], *tail)
    outs["anc"] = anc
    return rc, outs


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(kind=1), dict(D=9, C=0), dict(M=2049), dict(J=9), dict(n=1), dict(n=2049), dict(G=-1), dict(R=-1),
                                dict(lengths=[3, 0]), dict(lengths=[4, 3]), dict(lengths=[-1, 3]), dict(null_all=True)], ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused):
    rc, outs = _abi(fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


def test_the_message_names_the_lengths():
    for fused in (False, True):
        rc, _ = _abi(fused, lengths=[3, 0])
        assert rc == E and b"lengths must lie in [1, steps]" in _lib.load().ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
