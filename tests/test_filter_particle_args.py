"""Argument checks of the particle filter over many records, without a GPU: prediction.filter_particle_records_grouped /
posterior_filter_particle_records_grouped run the packing stage of the records functions (`_pack_records`) and their own
(`_pack_particles`): every error of tests/test_filter_records_args.py and every malformed draw (N out of range, the layouts of eps /
unif / xi0, xi0 without S0s and S0s without xi0, a uniform outside [0, 1), a draw that is not finite) raises ValueError before the
library is loaded, well-formed arguments in all three layouts reach it; there is no `smooth`; DGPSSM.filter_records_particle checks
`noise`, `num_particles` and the 1 GiB limit of independent draws, draws by the seed and hands the two forms on;
ffvd_op_filter_particle_records_grouped / ffvd_op_posterior_filter_particle_records_grouped are declared in the header, bound in
_lib.py, exported where the library is built, and return FFVD_EINVAL before any device call beyond their limits (FFVD_OK for no groups,
records or rows)."""
import ctypes
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_filter_records_args import BAD, R, SKIP, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import COMMON, _explicit, _fused, _with

SYMBOLS = ("ffvd_op_filter_particle_records_grouped", "ffvd_op_posterior_filter_particle_records_grouped")
G, D, N = 3, 2, 6


def _fn(explicit):
    return pr.filter_particle_records_grouped if explicit else pr.posterior_filter_particle_records_grouped


def _draws(steps=STEPS, n=N, lead=()):
    return dict(eps=np.zeros(lead + (steps, n, D)), unif=np.full(lead + (steps,), 0.5))


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


S0 = np.tile(0.1 * np.eye(D), (R, 1, 1))
BAD_DRAWS = {
    "one particle": _draws(n=1),
    "2049 particles": _draws(n=2049),
    "eps with two axes": dict(eps=np.zeros((N, D))),
    "eps with six axes": dict(eps=np.zeros((1, G, R, STEPS, N, D))),
    "eps of another D": dict(eps=np.zeros((STEPS, N, D + 1))),
    "eps of another length": dict(eps=np.zeros((STEPS + 1, N, D))),
    "eps of another R": dict(eps=np.zeros((R + 1, STEPS, N, D))),
    "eps of another G": dict(eps=np.zeros((G + 1, R, STEPS, N, D))),
    "eps of two records": dict(eps=np.zeros((2, STEPS, N, D))),
    "an eps that is not finite": dict(eps=np.where(np.arange(STEPS * N * D).reshape(STEPS, N, D) == 7, np.nan, 0.0)),
    "an infinite eps": dict(eps=np.where(np.arange(STEPS * N * D).reshape(STEPS, N, D) == 9, np.inf, 0.0)),
    "unif of another length": dict(unif=np.full(STEPS + 1, 0.5)),
    "unif of another R": dict(unif=np.full((R + 1, STEPS), 0.5)),
    "unif of another G": dict(unif=np.full((G + 1, R, STEPS), 0.5)),
    "a scalar unif": dict(unif=0.5),
    "a uniform of one": dict(unif=np.array([0.5, 1.0, 0.5, 0.5])),
    "a negative uniform": dict(unif=np.array([0.5, -1e-9, 0.5, 0.5])),
    "a uniform that is not finite": dict(unif=np.array([0.5, np.nan, 0.5, 0.5])),
    "S0s without xi0": dict(S0s=S0),
    "xi0 without S0s": dict(xi0=np.zeros((N, D))),
    "xi0 of another N": dict(S0s=S0, xi0=np.zeros((N + 1, D))),
    "xi0 of another D": dict(S0s=S0, xi0=np.zeros((N, D + 1))),
    "xi0 of another R": dict(S0s=S0, xi0=np.zeros((R + 1, N, D))),
    "xi0 of another G": dict(S0s=S0, xi0=np.zeros((G + 1, R, N, D))),
    "an xi0 that is not finite": dict(S0s=S0, xi0=np.full((N, D), np.nan)),
    "return_particles that is no bool": dict(return_particles="yes"),
}


@pytest.mark.parametrize("what", sorted(BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "filter_particle_records_grouped: (eps|unif|xi0|return_particles)"):
            _call(explicit, **BAD_DRAWS[what])


def test_the_messages_name_the_function_and_the_argument(no_device):
    with pytest.raises(ValueError, match="filter_particle_records_grouped: x0s"):
        _call(True, x0s=None)
    for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                     (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records"),
                     (_draws(n=1), r"eps: the number of particles N must lie in \[2, 2048\]"), (dict(S0s=S0), "xi0")):
        for explicit in (True, False):
            who = ("" if explicit else "posterior_") + "filter_particle_records_grouped"
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call(explicit, **kw)


def test_well_formed_arguments_in_every_layout_reach_the_particle_symbols(monkeypatch):
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


def test_the_signatures_have_the_draws_and_no_smoother(no_device):
    for new, old in ((pr.filter_particle_records_grouped, pr.filter_records_grouped),
                     (pr.posterior_filter_particle_records_grouped, pr.posterior_filter_records_grouped)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        pos = [k for k in b if b[k].kind is not inspect.Parameter.KEYWORD_ONLY]
        assert [k for k in a if a[k].kind is not inspect.Parameter.KEYWORD_ONLY] == pos + ["eps", "unif"]
        assert set(a) - set(b) == {"eps", "unif", "xi0", "return_particles"} and set(b) - set(a) == {"smooth"}
        assert a["xi0"].default is None and a["return_particles"].default is False
        assert all(a[k].default == b[k].default for k in set(a) & set(b))
    assert pr.FILTER_METHODS == ("moment", "linearised")
    doc = pr.filter_particle_records_grouped.__doc__
    assert "EQUAL weights" in doc and "smoothing is not built" in doc and "systematic" in doc and "log_evidence" in doc


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    sig = inspect.signature(DGPSSM.filter_records_particle).parameters
    assert list(sig) == ["self", "Y_records", "control_records", "num_particles", "lengths", "x0", "S0", "q_mode", "Y_train_std", "records_per_pass",
                         "seed", "noise", "return_particles"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, 256, None, None, None, "reference", 1.0, 0, None, "shared", False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    assert list(inspect.signature(DGPSSM.filter_records).parameters) == ["self", "Y_records", "control_records", "lengths", "x0", "S0", "smooth",
                                                                         "q_mode", "Y_train_std", "records_per_pass"]
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    for kw, msg in ((dict(noise="common"), "filter_records_particle: noise"), (dict(noise=None), "filter_records_particle: noise"),
                    (dict(num_particles=1), "filter_records_particle: num_particles"), (dict(num_particles=2049), "num_particles"),
                    (dict(num_particles=64.0), "num_particles"), (dict(num_particles=True), "num_particles"),
                    (dict(q_mode="slice0"), "filter_records_particle: q_mode"), (dict(x0=np.zeros(3)), "x0")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.filter_records_particle(_Model(), Y, ctrl, seed=1, **kw)
    with pytest.raises(ValueError, match="filter_records_particle: Y_records"):
        DGPSSM.filter_records_particle(_Model(), np.zeros((STEPS, 1)), ctrl, seed=1)
    with pytest.raises(ValueError, match="control_records"):
        DGPSSM.filter_records_particle(_Model(), Y, seed=1)
    # independent draws beyond 1 GiB are refused with the byte count, before anything is drawn: S R (steps N D + steps) doubles
    big, n = np.zeros((400, 200, 1)), 2048
    nbytes = 8 * 3 * 400 * (200 * n * 2 + 200)
    assert nbytes > 2 ** 30
    with pytest.raises(ValueError, match=f"{nbytes} bytes"):
        DGPSSM.filter_records_particle(_Model(), big, np.zeros((400, 200, 1)), num_particles=n, seed=1, noise="independent")
    seen = {}
    for name in ("posterior_filter_particle_records_grouped", "filter_particle_records_grouped"):
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    m, e = _Model(), _Model(U_collapse=False)
    kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7)
    rng = np.random.default_rng(5)
    want = dict(eps=rng.standard_normal((STEPS, 16, 2)), unif=rng.random((STEPS,)))
    assert DGPSSM.filter_records_particle(m, Y, ctrl, num_particles=16, seed=5, **kw) == "posterior_filter_particle_records_grouped"
    a, k = seen["posterior_filter_particle_records_grouped"]
    assert k == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", Y_train_std=1.7, records_per_pass=2, x0s=None, xi0=None, return_particles=False)
    assert len(a) == 12 and np.array_equal(a[10], want["eps"]) and np.array_equal(a[11], want["unif"])
    for noise, lead in (("per_record", (R,)), ("independent", (3, R))):                   # explicit U; the layouts of the draws; a start covariance
        assert DGPSSM.filter_records_particle(e, Y, ctrl, num_particles=16, seed=5, noise=noise, S0=np.eye(2), x0=np.arange(2.0),
                                              return_particles=True) == "filter_particle_records_grouped"
        a, k = seen["filter_particle_records_grouped"]
        assert a[0] == "Lm" and a[5].shape == (3, R, 2) and len(a) == 14 and a[12].shape == lead + (STEPS, 16, 2) and a[13].shape == lead + (STEPS,)
        assert k["xi0"].shape == lead + (16, 2) and k["S0s"].shape == (3, R, 2, 2) and k["return_particles"] is True and "smooth" not in k
        assert np.all((a[13] >= 0.0) & (a[13] < 1.0))
    Y1, c1 = Y[:1], ctrl[:1]                                       # R = 1: a single record
    assert DGPSSM.filter_records_particle(e, Y1, c1, seed=2) == "filter_particle_records_grouped"
    assert seen["filter_particle_records_grouped"][0][12].shape == (STEPS, 256, 2)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_after_the_cubature_ones_and_bound():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, ("ffvd_op_filter_cubature_records_grouped", "ffvd_op_posterior_filter_cubature_records_grouped")):
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols()
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")
        d, c = _declaration(new), _declaration(old)
        assert len(_lib._SIGNATURES[new][1]) == len(d) and not any("smooth" in a or "cross" in a for a in d)
        k = c.index("int records_per_pass")
        assert d[:k + 1] == c[:k + 1]                             # the argument lists agree up to records_per_pass
        assert d[k + 1:k + 11] == ["int N", "const double *eps", "long long eps_stride_g", "long long eps_stride_r", "const double *unif",
                                   "long long unif_stride_g", "long long unif_stride_r", "const double *xi0", "long long xi0_stride_g",
                                   "long long xi0_stride_r"]
        rest = [a for a in c[k + 1:] if not any(w in a for w in ("smooth", "cross"))]
        mine = [a for a in d[k + 11:] if a not in ("double *ess", "double *log_evidence", "double *particles", "int *ancestors")]
        assert mine == rest and d.index("int *ancestors") == d.index("double *particles") + 1
    for words in ("systematic", "log_evidence", "No adaptive resampling", "clamped into [0, N)", "2 <= N <= 2048"):
        assert words in text


def test_the_symbols_are_exported():
    for s in SYMBOLS:
        assert hasattr(_lib.load(), s)


OUT_NAMES = ("mp", "Sp", "mf", "Sf", "lpd", "lj", "ym", "yt", "lm", "lg", "ess", "le", "par")


def _abi(fused, *, G=2, R=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=3, kind=0, gpp=0, q_mode=0, J=1, rpp=0, n=4, null=(), sd=1.0, y=0.0,
         eps=0.0, unif=0.5, strides=None, S0=False, small=False):
    """One call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL; small: the arrays are not
    sized by R and steps; strides: (eps_g, eps_r, unif_g, unif_r, xi0_g, xi0_r), None: the full layout."""
    P = D + C if P is None else P
    ng, nm, nr, st, Pp, Jp, nn = max(G, 1), max(n_models, 1), 1 if small else max(R, 1), 1 if small else max(steps, 1), max(P, 1), max(J, 1), \
        1 if small else min(max(n, 1), 4096)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((ng, T + 1, D)), cf=np.zeros((max(T, 1), max(C, 1))),
             cr=np.zeros((nr, st, max(C, 1))), lq=np.zeros((ng, D)), f=np.zeros((ng, M, D)), xl=np.zeros((ng, nr, D)), CC=np.ones((D, Jp)),
             DD=np.zeros(Jp), sd=np.full(Jp, sd), Y=np.full((nr, st, Jp), y), eps=np.full((ng, nr, st, nn, D), eps), unif=np.full((ng, nr, st), unif),
             xi0=np.zeros((ng, nr, nn, D)), S0=np.tile(np.eye(D), (ng, nr, 1, 1)))
    vec, mat = (ng, nr, st, D), (ng, nr, st, D, D)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, lpd=(ng, nr, st, Jp), lj=(ng, nr, st), ym=(nr, st, Jp), yt=(nr, st, Jp), lm=(nr, st, Jp),
                  lg=(nr, st, Jp), ess=(ng, nr, st), le=(ng, nr), par=(ng, nr, st, nn, D), U=(ng, M, D))
    outs = {k: np.full(s, 7.0) for k, s in shapes.items()}
    anc = np.full((ng, nr, st, nn), 7, dtype=np.int32)
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    ap = None if "anc" in null else anc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    if strides is None:
        strides = (R * steps * n * D, steps * n * D, R * steps, steps, R * n * D, n * D)
    draws = (n, p["eps"], strides[0], strides[1], p["unif"], strides[2], strides[3], p["xi0"] if S0 else None, strides[4], strides[5])
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"], rpp) + draws + tuple(p[k] for k in OUT_NAMES) + (ap,)
    s0 = p["S0"] if S0 else None
    if fused:
        rc = lib.ffvd_op_posterior_filter_particle_records_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T,
                                                                   p["lq"], 1e-5, gpp, q_mode, R, None, s0, p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_op_filter_particle_records_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, q_mode, R, p["xl"],
                                                         s0, p["cr"], C, steps, p["lq"], *tail)
    outs["anc"] = anc
    return rc, outs


BAD_ABI = [dict(kind=1), dict(kind=2), dict(D=9, C=0), dict(D=2, C=31), dict(M=2049), dict(M=0), dict(D=0), dict(J=9), dict(J=0), dict(q_mode=2),
           dict(G=3, n_models=2), dict(G=-1), dict(steps=-1), dict(R=-1), dict(rpp=-1), dict(P=2), dict(null=("Z",)), dict(null=("lv",)),
           dict(null=("ll",)), dict(null=("lq",)), dict(null=("cr",)), dict(null=("CC",)), dict(null=("DD",)), dict(null=("sd",)), dict(null=("Y",)),
           dict(null=OUT_NAMES + ("anc",)), dict(sd=0.0), dict(sd=np.nan), dict(y=np.inf), dict(y=-np.inf),
           dict(G=2, R=1 << 20, steps=1 << 8, small=True), dict(n=1), dict(n=0), dict(n=2049), dict(n=-3), dict(null=("eps",)), dict(null=("unif",)),
           dict(S0=True, null=("xi0",)), dict(eps=np.nan), dict(eps=np.inf), dict(unif=1.0), dict(unif=-0.25), dict(unif=np.nan),
           dict(strides=(5, 24, 6, 3, 16, 8)), dict(strides=(48, 23, 6, 3, 16, 8)), dict(strides=(48, 24, 6, 2, 16, 8)),
           dict(strides=(48, 24, 6, 3, 16, 7)), dict(strides=(25, 0, 6, 3, 16, 8)), dict(strides=(-48, 24, 6, 3, 16, 8)),
           dict(G=2, R=1 << 10, steps=1 << 8, n=2048, small=True)]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused):
    rc, outs = _abi(fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


def test_the_messages_say_why():
    lib = _lib.load()
    for fused in (False, True):
        rc, _ = _abi(fused, kind=1)
        msg = lib.ffvd_last_error(None)
        assert rc == E and b"particle filter of many records" in msg and b"SE kernel only" in msg
        rc, _ = _abi(fused, G=2, R=1 << 20, steps=1 << 8, small=True)
        assert rc == E and b"G * R * steps * D * D < 2^31" in lib.ffvd_last_error(None)
        rc, _ = _abi(fused, n=2049)
        assert rc == E and b"2 <= N <= 2048" in lib.ffvd_last_error(None)
    for ov in (dict(null=("f",)), dict(null=("xl",)), dict(null=("W",))):
        assert _abi(False, **ov)[0] == E
    for ov in (dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))):
        assert _abi(True, **ov)[0] == E


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
