"""Argument checks of particle smoothing and backward simulation on the adapted filter's sets, without a GPU:
prediction.smooth_adapted_records_grouped / backsim_adapted_records_grouped and their posterior forms take the parameters of the
bootstrap pairs and run their packing stages, so every ValueError fires before the library is loaded, under the new names;
well-formed arguments reach the four new symbols with the bootstrap lists WITHOUT `weights`; DGPSSM.smooth_records_adapted and
sample_records_adapted draw the adapted filter's draws first; the four symbols are declared in the header, bound in _lib.py and
exported, and return FFVD_EINVAL before any device call beyond their limits."""
import ctypes
import inspect

import numpy as np
import pytest

import test_backsim_particle_args as tba
import test_smooth_particle_args as tsa
from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_filter_adapted_args import SYMBOLS as FILTER_SYMBOLS
from test_filter_particle_args import BAD_DRAWS, D, G, N, S0, _draws
from test_filter_records_args import BAD, R, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import _explicit, _fused, _with

SMOOTH = ("ffvd_particle_adapted_smooth_records_grouped", "ffvd_posterior_particle_adapted_smooth_records_grouped")
BACKSIM = ("ffvd_particle_adapted_backsim_records_grouped", "ffvd_posterior_particle_adapted_backsim_records_grouped")
NEW_SMOOTH = [a for a in tsa.NEW if a != "double *weights"]
NEW_BACKSIM = [a for a in tba.NEW if a != "double *weights"]
NB = tba.NB
FNS = {("smooth", True): "smooth_adapted_records_grouped", ("smooth", False): "posterior_smooth_adapted_records_grouped",
       ("backsim", True): "backsim_adapted_records_grouped", ("backsim", False): "posterior_backsim_adapted_records_grouped"}
FORMS = [(what, explicit) for what in ("smooth", "backsim") for explicit in (True, False)]


def _call(what, explicit, **kw):
    a = _with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **_draws())
    if what == "backsim":
        a = _with(a, unif_bs=np.full((STEPS, NB), 0.5))
    a = _with(a, **kw)
    if "Y_records" in kw and "eps" not in kw and np.ndim(kw["Y_records"]) == 3 and np.shape(kw["Y_records"])[1] != STEPS:
        a.update(_draws(steps=np.shape(kw["Y_records"])[1]))
        if what == "backsim":
            a["unif_bs"] = np.full((np.shape(kw["Y_records"])[1], NB), 0.5)
    return getattr(pr, FNS[what, explicit])(**a)


@pytest.mark.parametrize("bad", sorted(BAD))
def test_every_error_of_the_records_packing_raises_before_the_library_is_loaded(bad, no_device):
    kw = dict(BAD[bad])
    if "S0s" in kw:
        kw["xi0"] = np.zeros((N, D))
    for what, explicit in FORMS:
        with pytest.raises(ValueError):
            _call(what, explicit, **kw)


@pytest.mark.parametrize("bad", sorted(BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(bad, no_device):
    for what, explicit in FORMS:
        with pytest.raises(ValueError, match=f"^{FNS[what, explicit]}: (eps|unif|xi0|return_particles)"):
            _call(what, explicit, **BAD_DRAWS[bad])


@pytest.mark.parametrize("bad", [None, np.full((STEPS,), 0.5), np.full((STEPS + 1, NB), 0.5), np.full((R + 1, STEPS, NB), 0.5),
                                 np.full((STEPS, 0), 0.5), np.full((STEPS, 4097), 0.5), np.full((STEPS, NB), 1.0),
                                 np.full((STEPS, NB), -0.1), np.full((STEPS, NB), np.nan)],
                         ids=lambda b: "None" if b is None else str(np.shape(b)) + str(np.ravel(b)[:1]))
def test_every_malformed_unif_bs_raises_before_the_library_is_loaded(bad, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError, match=f"^{FNS['backsim', explicit]}: unif_bs"):
            _call("backsim", explicit, unif_bs=bad)


def test_the_messages_name_the_function_and_the_argument(no_device):
    for what, explicit in FORMS:
        who = FNS[what, explicit]
        for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                         (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records"),
                         (_draws(n=1), r"eps: the number of particles N must lie in \[2, 2048\]"), (dict(S0s=S0), "xi0")):
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call(what, explicit, **kw)
    for what in ("smooth", "backsim"):
        with pytest.raises(ValueError, match=f"^{FNS[what, True]}: x0s"):
            _call(what, True, x0s=None)


def test_well_formed_arguments_reach_the_new_symbols_without_weights(monkeypatch):
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
        stacks = "return_particles" in kw
        for what, explicit in FORMS:
            with pytest.raises(Reached):
                _call(what, explicit, **kw)
            name, a = seen[-1]
            new = NEW_SMOOTH if what == "smooth" else NEW_BACKSIM
            assert name == (SMOOTH if what == "smooth" else BACKSIM)[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
            assert len(a) == len(_lib._SIGNATURES[FILTER_SYMBOLS[not explicit]][1]) + len(new)
            boot = name.replace("particle_adapted", "particle")
            assert len(a) == len(_lib._SIGNATURES[boot][1]) - 1                     # the bootstrap list without `weights`
            tail = a[-len(new):] if explicit else a[-len(new) - 1:-1]
            assert [tail[0][r] for r in range(R)] == lens                           # int32 lengths, always sent
            if what == "smooth":
                assert all(t is not None for t in tail[1:4])                        # m_smooth, S_smooth, ess_smooth
                assert len(tail[4:]) == 3 and all((t is None) != stacks for t in tail[4:])          # w_smooth, trans_mean, trans_var
            else:
                assert (tail[1], tail[3], tail[4]) == (NB, 0, 0) and tail[2] is not None
                assert all(t is not None for t in tail[5:10])                       # trajectories .. lag_cov
                assert len(tail[10:]) == 2 and all((t is None) != stacks for t in tail[10:])        # trans_mean, trans_var
            assert explicit or a[-1] is None                                        # U_means stays last
    assert {s for s, _ in seen} == set(SMOOTH + BACKSIM)


def test_the_signatures_are_the_bootstrap_pairs(no_device):
    for new, old in (("smooth_adapted_records_grouped", "smooth_particle_records_grouped"),
                     ("backsim_adapted_records_grouped", "backsim_particle_records_grouped")):
        for prefix in ("", "posterior_"):
            assert inspect.signature(getattr(pr, prefix + new)) == inspect.signature(getattr(pr, prefix + old))
    doc = pr.smooth_adapted_records_grouped.__doc__
    for words in ("m_smooth", "S_smooth", "ess_smooth", "w_smooth", "trans_mean", "trans_var", "1 / N", "no fold", "unweighted particle estimate",
                  "not the Rao-Blackwellised"):
        assert words in doc, words
    doc = pr.backsim_adapted_records_grouped.__doc__
    for words in ("trajectories", "traj_index", "m_traj", "S_traj", "lag_cov", "without an ancestor indirection", "w_smooth[t, k]"):
        assert words in doc, words
    for doc in (pr.filter_adapted_records_grouped.__doc__, inspect.getdoc(__import__("ffvd_amd.dgp_model", fromlist=["DGPSSM"]).DGPSSM.filter_records_adapted)):
        assert "No smoothing" not in doc and "no smoothing" not in doc and "adapted" in doc
    assert "smooth_adapted_records_grouped" in pr.filter_adapted_records_grouped.__doc__


def test_the_model_level_calls_draw_the_adapted_filters_draws_first(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    assert inspect.signature(DGPSSM.smooth_records_adapted) == inspect.signature(DGPSSM.filter_records_adapted)
    assert inspect.signature(DGPSSM.sample_records_adapted) == inspect.signature(DGPSSM.sample_records_particle)
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    for fn in ("smooth_records_adapted", "sample_records_adapted"):
        for kw, msg in ((dict(noise="common"), f"{fn}: noise"), (dict(num_particles=1), f"{fn}: num_particles"), (dict(q_mode="slice0"), f"{fn}: q_mode"),
                        (dict(x0=np.zeros(3)), "x0")):
            with pytest.raises(ValueError, match=msg):
                getattr(DGPSSM, fn)(_Model(), Y, ctrl, seed=1, **kw)
    for bad in (0, 4097, 2.5, True):
        with pytest.raises(ValueError, match="sample_records_adapted: num_trajectories"):
            DGPSSM.sample_records_adapted(_Model(), Y, ctrl, seed=1, num_trajectories=bad)
    seen = {}
    names = [p + f for f in ("smooth_adapted_records_grouped", "backsim_adapted_records_grouped", "filter_adapted_records_grouped")
             for p in ("posterior_", "")]
    for name in names:
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    for noise in ("shared", "per_record", "independent"):
        kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7, num_particles=16, seed=5, noise=noise)
        for model, pre in ((_Model(), "posterior_"), (_Model(U_collapse=False), "")):
            smooth, samp, filt = (pre + f for f in ("smooth_adapted_records_grouped", "backsim_adapted_records_grouped", "filter_adapted_records_grouped"))
            assert DGPSSM.smooth_records_adapted(model, Y, ctrl, **kw) == smooth
            assert DGPSSM.sample_records_adapted(model, Y, ctrl, num_trajectories=9, **kw) == samp
            assert DGPSSM.filter_records_adapted(model, Y, ctrl, **kw) == filt
            (a, k), (s, ks), (b, kb) = seen[smooth], seen[samp], seen[filt]
            assert k == kb and ks == kb and len(a) == len(b) and len(s) == len(b) + 1
            assert np.array_equal(a[-2], b[-2]) and np.array_equal(a[-1], b[-1]) and a[-2].shape[-3:] == (STEPS, 16, 2)
            assert np.array_equal(s[-3], b[-2]) and np.array_equal(s[-2], b[-1])
            rng = np.random.default_rng(5)
            lead = b[-1].shape[:-1]
            rng.standard_normal(lead + (STEPS, 16, 2)), rng.random(lead + (STEPS,))
            np.testing.assert_array_equal(s[-1], rng.random(lead + (STEPS, 9)))       # drawn after the filter's


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported():
    text = open(_declaration.__globals__["HEADER"]).read()
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    types = dict(smooth=[ip] + [dp] * 6, backsim=[ip, ctypes.c_int, dp, ctypes.c_longlong, ctypes.c_longlong, dp, ip] + [dp] * 5)
    for what, symbols, new_args in (("smooth", SMOOTH, NEW_SMOOTH), ("backsim", BACKSIM, NEW_BACKSIM)):
        for new, old in zip(symbols, FILTER_SYMBOLS):
            assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols() and hasattr(_lib.load(), new)
            assert not new.startswith("ffvd_op_")
            assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")
            d, c = _declaration(new), _declaration(old)
            assert len(_lib._SIGNATURES[new][1]) == len(d)
            k, n = c.index("int *ancestors"), len(new_args)
            assert d[:k + 1] == c[:k + 1] and d[k + 1:k + 1 + n] == new_args and d[k + 1 + n:] == c[k + 1:]     # (U_means stays last)
            boot = _declaration(new.replace("particle_adapted", "particle"))
            assert d == [a for a in boot if a != "double *weights"]                 # the bootstrap list without `weights`
            sig, old_sig = _lib._SIGNATURES[new][1], _lib._SIGNATURES[old][1]
            assert sig[:k + 1] == old_sig[:k + 1] and sig[k + 1 + n:] == old_sig[k + 1:] and sig[k + 1:k + 1 + n] == types[what]
    for words in ("w_smooth[n-1, i] = 1 / N", "no fold through the ancestors", "not the Rao-Blackwellised", "no ancestor indirection",
                  "(3 D + 2) N doubles"):
        assert words in text, words
    assert "There is no smoother, no backward simulation" not in text


def _abi(what, fused, *, G=2, R=2, M=4, D=2, C=1, T=5, steps=3, kind=0, J=1, n=4, B=3, lengths=None, null_all=False, null_u=False, stride=None,
         u=0.5):
    """One call on zero inputs with every output buffer filled with 7"""
    P = D + C
    ng, nr, st, nn, nb = max(G, 1), max(R, 1), max(steps, 1), min(max(n, 1), 4096), min(max(B, 1), 5000)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((1, M, P)), lv=np.zeros((1, D)), ll=np.zeros((1, D, P)), X=np.zeros((ng, T + 1, D)), cf=np.zeros((T, C)),
             cr=np.zeros((nr, st, C)), lq=np.zeros((ng, D)), f=np.zeros((ng, M, D)), xl=np.zeros((ng, nr, D)), CC=np.ones((D, J)),
             DD=np.zeros(J), sd=np.ones(J), Y=np.zeros((nr, st, J)), eps=np.zeros((ng, nr, st, nn, D)), unif=np.full((ng, nr, st), 0.5),
             ub=np.full((ng, nr, st, nb), u))
    vec, mat, row = (ng, nr, st, D), (ng, nr, st, D, D), (ng, nr, st)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, lpd=row + (J,), lj=row, ym=(nr, st, J), yt=(nr, st, J), lm=(nr, st, J), lg=(nr, st, J),
                  ess=row, le=(ng, nr), par=row + (nn, D))
    new = dict(ms=vec, Ss=mat, es=row, ws=row + (nn,), tm=row + (nn, D), tv=row + (nn, D)) if what == "smooth" else \
        dict(mt=vec, St=mat, lc=mat, tm=row + (nn, D), tv=row + (nn, D))
    outs = {k: np.full(s, 7.0) for k, s in list(shapes.items()) + list(new.items()) + [("U", (ng, M, D)), ("traj", (ng, nr, nb, st, D))]}
    anc, idx = np.full(row + (nn,), 7, dtype=np.int32), np.full(row + (nb,), 7, dtype=np.int32)
    p = {k: dp(v) for k, v in list(a.items()) + list(outs.items())}
    ip = ctypes.POINTER(ctypes.c_int)
    lens = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    draws = (n, p["eps"], R * steps * n * D, steps * n * D, p["unif"], R * steps, steps, None, 0, 0)
    sg, sr = (R * steps * B, steps * B) if stride is None else stride
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"], 0) + draws + tuple(None if null_all else p[k] for k in shapes) + \
        (None if null_all else anc.ctypes.data_as(ip), None if lens is None else lens.ctypes.data_as(ip))
    if what == "backsim":
        tail += (B, None if null_u else p["ub"], sg, sr, None if null_all else p["traj"], None if null_all else idx.ctypes.data_as(ip))
    tail += tuple(None if null_all else p[k] for k in new)
    name = (SMOOTH if what == "smooth" else BACKSIM)[fused]
    if fused:
        rc = getattr(lib, name)(kind, G, 1, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"], 1e-5, 0, 0, R, None, None, p["cr"],
                                steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(D)]
        Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = getattr(lib, name)(kind, G, 1, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, 0, R, p["xl"], None, p["cr"], C, steps, p["lq"],
                                *tail)
    outs.update(anc=anc, idx=idx)
    return rc, outs, name


COMMON_BAD = [dict(kind=1), dict(D=9, C=0), dict(M=2049), dict(J=9), dict(n=1), dict(n=2049), dict(G=-1), dict(R=-1), dict(lengths=[3, 0]),
              dict(lengths=[4, 3]), dict(lengths=[-1, 3]), dict(null_all=True)]
BACKSIM_BAD = [dict(B=0), dict(B=4097), dict(B=-1), dict(null_u=True), dict(stride=(0, 7)), dict(stride=(5, 0)), dict(stride=(3 * 3, 3 * 3)),
               dict(u=1.0), dict(u=-0.5), dict(u=np.nan)]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("what,ov", [("smooth", o) for o in COMMON_BAD] + [("backsim", o) for o in COMMON_BAD + BACKSIM_BAD], ids=str)
def test_abi_rejects_bad_arguments_without_a_device(what, ov, fused):
    rc, outs, name = _abi(what, fused, **ov)
    assert rc == E, rc
    assert name.encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


def test_the_messages_say_why():
    lib = _lib.load()
    for what in ("smooth", "backsim"):
        for fused in (False, True):
            rc, _, _ = _abi(what, fused, lengths=[3, 0])
            assert rc == E and b"lengths must lie in [1, steps]" in lib.ffvd_last_error(None)
            rc, _, _ = _abi(what, fused, kind=1)
            msg = lib.ffvd_last_error(None)
            assert rc == E and b"adapted particle filter of many records" in msg and b"SE kernel only" in msg
            rc, _, _ = _abi(what, fused, n=2049)
            assert rc == E and b"2 <= N <= 2048" in lib.ffvd_last_error(None)
    for fused in (False, True):
        for ov in (dict(B=0), dict(null_u=True), dict(stride=(0, 7))):
            rc, _, _ = _abi("backsim", fused, **ov)
            assert rc == E and b"1 <= B <= 4096" in lib.ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("what", ["smooth", "backsim"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(what, fused, ov):
    rc, outs, _ = _abi(what, fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
    if what == "backsim":
        assert _abi(what, fused, B=0, **ov)[0] == E                # B is checked even then
