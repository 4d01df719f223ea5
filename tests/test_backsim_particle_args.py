"""Argument checks of the particle backward simulation over many records, without a GPU: prediction.backsim_particle_records_grouped /
posterior_backsim_particle_records_grouped take the parameters of the two particle smoothing functions plus `unif_bs` and run their
packing stages, so every ValueError fires before the library is loaded, under the new names; well-formed arguments reach the two new
symbols with `lengths`, B, unif_bs, its strides and the eight outputs behind the filter's; DGPSSM.sample_records_particle draws what
filter_records_particle draws and then the backward uniforms; ffvd_particle_backsim_records_grouped /
ffvd_posterior_particle_backsim_records_grouped are declared in the header, bound in _lib.py and exported, and return FFVD_EINVAL
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
from test_filter_records_args import BAD, R, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import _explicit, _fused, _with

SYMBOLS = ("ffvd_particle_backsim_records_grouped", "ffvd_posterior_particle_backsim_records_grouped")
NEW = ["const int *lengths", "int B", "const double *unif_bs", "long long unif_bs_stride_g", "long long unif_bs_stride_r",
       "double *trajectories", "int *traj_index", "double *m_traj", "double *S_traj", "double *lag_cov", "double *weights",
       "double *trans_mean", "double *trans_var"]
NB = 5


def _fn(explicit):
    return pr.backsim_particle_records_grouped if explicit else pr.posterior_backsim_particle_records_grouped


def _call(explicit, **kw):
    a = _with(_with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **_draws()), unif_bs=np.full((STEPS, NB), 0.5))
    a = _with(a, **kw)
    if "Y_records" in kw and "eps" not in kw and np.ndim(kw["Y_records"]) == 3 and np.shape(kw["Y_records"])[1] != STEPS:
        a.update(_draws(steps=np.shape(kw["Y_records"])[1]))
        a["unif_bs"] = np.full((np.shape(kw["Y_records"])[1], NB), 0.5)
    return _fn(explicit)(**a)


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
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "backsim_particle_records_grouped: (eps|unif|xi0|return_particles)"):
            _call(explicit, **BAD_DRAWS[what])


@pytest.mark.parametrize("bad", [None, np.full((STEPS,), 0.5), np.full((STEPS + 1, NB), 0.5), np.full((R + 1, STEPS, NB), 0.5),
                                 np.full((G, R + 1, STEPS, NB), 0.5), np.full((STEPS, 0), 0.5), np.full((STEPS, 4097), 0.5),
                                 np.full((STEPS, NB), 1.0), np.full((STEPS, NB), -0.1), np.full((STEPS, NB), np.nan),
                                 np.full((2, 2, 2, STEPS, NB), 0.5)], ids=lambda b: "None" if b is None else str(np.shape(b)) + str(np.ravel(b)[:1]))
def test_every_malformed_unif_bs_raises_before_the_library_is_loaded(bad, no_device):
    for explicit in (True, False):
        who = ("" if explicit else "posterior_") + "backsim_particle_records_grouped"
        with pytest.raises(ValueError, match=f"^{who}: unif_bs"):
            _call(explicit, unif_bs=bad)


def test_well_formed_arguments_reach_the_new_symbols(monkeypatch):
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
    shared, per_rec, full = np.full((STEPS, NB), 0.5), np.full((R, STEPS, 3), 0.25), np.full((G, R, STEPS, 2), 0.75)
    for kw, lens, (nb, sg, sr) in ((dict(), [STEPS] * R, (NB, 0, 0)),
                                   (dict(Y_records=Y, lengths=[STEPS, 2, STEPS], records_per_pass=2, unif_bs=per_rec), [STEPS, 2, STEPS],
                                    (3, 0, STEPS * 3)),
                                   (dict(S0s=S0, xi0=np.zeros((N, D)), return_particles=True, unif_bs=full), [STEPS] * R,
                                    (2, R * STEPS * 2, STEPS * 2))):
        for explicit in (True, False):
            with pytest.raises(Reached):
                _call(explicit, **kw)
            name, a = seen[-1]
            assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
            assert len(a) == len(_lib._SIGNATURES[FILTER_SYMBOLS[not explicit]][1]) + len(NEW)
            tail = a[-len(NEW):] if explicit else a[-len(NEW) - 1:-1]
            assert [tail[0][r] for r in range(R)] == lens         # int32 lengths, always sent
            assert tuple(tail[1:5:1][i] for i in (0, 2, 3)) == (nb, sg, sr) and tail[2] is not None
            assert all(t is not None for t in tail[5:10])         # trajectories .. lag_cov
            assert all((t is None) == ("return_particles" not in kw) for t in tail[10:])
            assert explicit or a[-1] is None                      # U_means stays last
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_the_signatures_are_the_smoothing_functions_plus_unif_bs(no_device):
    for new, old in ((pr.backsim_particle_records_grouped, pr.smooth_particle_records_grouped),
                     (pr.posterior_backsim_particle_records_grouped, pr.posterior_smooth_particle_records_grouped)):
        a, b = list(inspect.signature(new).parameters.values()), list(inspect.signature(old).parameters.values())
        k = [p.name for p in a].index("unif_bs")
        assert a[k - 1].name == "unif" and a[:k] + a[k + 1:] == b
    doc = pr.backsim_particle_records_grouped.__doc__
    for words in ("trajectories", "traj_index", "m_traj", "S_traj", "lag_cov", "Godsill", "w_smooth[t, k]", "tot >= 1"):
        assert words in doc, words
    assert "not built" not in pr.smooth_particle_records_grouped.__doc__.split("backward simulation")[1]
    assert "backsim_particle_records_grouped" in pr.smooth_particle_records_grouped.__doc__


def test_the_model_level_call_hands_on_the_filters_draws(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    new, old = inspect.signature(DGPSSM.sample_records_particle).parameters, inspect.signature(DGPSSM.filter_records_particle).parameters
    assert [p for p in new if p != "num_trajectories"] == list(old)
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    for kw, msg in ((dict(noise="common"), "sample_records_particle: noise"), (dict(num_particles=1), "sample_records_particle: num_particles"),
                    (dict(num_trajectories=0), "sample_records_particle: num_trajectories"),
                    (dict(num_trajectories=4097), "sample_records_particle: num_trajectories"),
                    (dict(num_trajectories=2.5), "sample_records_particle: num_trajectories"),
                    (dict(q_mode="slice0"), "sample_records_particle: q_mode")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.sample_records_particle(_Model(), Y, ctrl, seed=1, **kw)
    seen = {}
    names = ("posterior_backsim_particle_records_grouped", "backsim_particle_records_grouped", "posterior_filter_particle_records_grouped",
             "filter_particle_records_grouped")
    for name in names:
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    for noise, lead in (("shared", ()), ("per_record", (R,)), ("independent", (2, R))):
        kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7, num_particles=16, seed=5, noise=noise)
        for model, samp, filt in ((_Model(), names[0], names[2]), (_Model(U_collapse=False), names[1], names[3])):
            assert DGPSSM.sample_records_particle(model, Y, ctrl, num_trajectories=9, **kw) == samp
            assert DGPSSM.filter_records_particle(model, Y, ctrl, **kw) == filt
            (a, k), (b, kb) = seen[samp], seen[filt]              # the same seed: exactly the filter's draws, then unif_bs
            assert k == kb and len(a) == len(b) + 1
            assert np.array_equal(a[-3], b[-2]) and np.array_equal(a[-2], b[-1]) and a[-3].shape[-3:] == (STEPS, 16, 2)
            assert a[-1].shape[-2:] == (STEPS, 9) and a[-1].shape[:-2] == a[-2].shape[:-1]
            rng = np.random.default_rng(5)
            lead_shape = a[-2].shape[:-1]
            rng.standard_normal(lead_shape + (STEPS, 16, 2)), rng.random(lead_shape + (STEPS,))
            np.testing.assert_array_equal(a[-1], rng.random(lead_shape + (STEPS, 9)))     # drawn after the filter's


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, FILTER_SYMBOLS):
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols() and hasattr(_lib.load(), new)
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")
        d, c = _declaration(new), _declaration(old)
        assert len(_lib._SIGNATURES[new][1]) == len(d)
        k, n = c.index("int *ancestors"), len(NEW)
        assert d[:k + 1] == c[:k + 1] and d[k + 1:k + 1 + n] == NEW and d[k + 1 + n:] == c[k + 1:]     # (U_means stays last)
        smooth = _declaration(new.replace("backsim", "smooth"))
        assert d[:k + 2] == smooth[:k + 2]                        # the smoothing call's list up to and including lengths
        sig, old_sig = _lib._SIGNATURES[new][1], _lib._SIGNATURES[old][1]
        ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        assert sig[:k + 1] == old_sig[:k + 1] and sig[k + 1 + n:] == old_sig[k + 1:]
        assert sig[k + 1:k + 1 + n] == [ip, ctypes.c_int, dp, ctypes.c_longlong, ctypes.c_longlong, dp, ip] + [dp] * 6
    for words in ("Godsill", "k_{n-1} = min(#{k: cdf_k <= u tot}, N - 1)", "tot >= 1 always", "1 <= B <= 4096", "(4 D + 3) N doubles"):
        assert words in text, words


def _abi(fused, *, G=2, R=2, M=4, D=2, C=1, T=5, steps=3, n=4, B=3, lengths=None, null_u=False, stride=None, u=0.5):
    """One call on zero inputs with every output buffer filled with 7"""
    P, J = D + C, 1
    ng, nr, st, nb = max(G, 1), max(R, 1), max(steps, 1), min(max(B, 1), 5000)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((1, M, P)), lv=np.zeros((1, D)), ll=np.zeros((1, D, P)), X=np.zeros((ng, T + 1, D)), cf=np.zeros((T, C)),
             cr=np.zeros((nr, st, C)), lq=np.zeros((ng, D)), f=np.zeros((ng, M, D)), xl=np.zeros((ng, nr, D)), CC=np.ones((D, J)),
             DD=np.zeros(J), sd=np.ones(J), Y=np.zeros((nr, st, J)), eps=np.zeros((ng, nr, st, n, D)), unif=np.full((ng, nr, st), 0.5),
             ub=np.full((ng, nr, st, nb), u))
    vec, mat, row = (ng, nr, st, D), (ng, nr, st, D, D), (ng, nr, st)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, lpd=row + (J,), lj=row, ym=(nr, st, J), yt=(nr, st, J), lm=(nr, st, J), lg=(nr, st, J),
                  ess=row, le=(ng, nr), par=row + (n, D))
    new = dict(mt=vec, St=mat, lc=mat, W=row + (n,), tm=row + (n, D), tv=row + (n, D))
    outs = {k: np.full(s, 7.0) for k, s in list(shapes.items()) + list(new.items()) + [("U", (ng, M, D)), ("traj", (ng, nr, nb, st, D))]}
    anc, idx = np.full(row + (n,), 7, dtype=np.int32), np.full(row + (nb,), 7, dtype=np.int32)
    p = {k: dp(v) for k, v in list(a.items()) + list(outs.items())}
    ip = ctypes.POINTER(ctypes.c_int)
    lens = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    draws = (n, p["eps"], R * steps * n * D, steps * n * D, p["unif"], R * steps, steps, None, 0, 0)
    sg, sr = (R * steps * B, steps * B) if stride is None else stride
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"], 0) + draws + tuple(p[k] for k in shapes) + \
        (anc.ctypes.data_as(ip), None if lens is None else lens.ctypes.data_as(ip), B, None if null_u else p["ub"], sg, sr, p["traj"],
         idx.ctypes.data_as(ip)) + tuple(p[k] for k in new)
    if fused:
        rc = lib.ffvd_posterior_particle_backsim_records_grouped(0, G, 1, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"], 1e-5,
                                                                 0, 0, R, None, None, p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(D)]
        Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_particle_backsim_records_grouped(0, G, 1, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, 0, R, p["xl"], None, p["cr"],
                                                       C, steps, p["lq"], *tail)
    outs.update(anc=anc, idx=idx)
    return rc, outs


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(B=0), dict(B=4097), dict(B=-1), dict(null_u=True), dict(stride=(0, 7)), dict(stride=(5, 0)),
                                dict(stride=(3 * 3, 3 * 3)), dict(u=1.0), dict(u=-0.5), dict(u=np.nan), dict(n=1), dict(n=2049),
                                dict(lengths=[3, 0]), dict(lengths=[4, 3]), dict(G=-1)], ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused):
    rc, outs = _abi(fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


def test_the_message_names_the_limits_of_the_backward_simulation():
    for fused in (False, True):
        for ov in (dict(B=0), dict(null_u=True), dict(stride=(0, 7))):
            rc, _ = _abi(fused, **ov)
            assert rc == E and b"1 <= B <= 4096" in _lib.load().ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
    rc, _ = _abi(fused, B=0, **ov)                                # B is checked even then
    assert rc == E
