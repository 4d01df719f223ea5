"""The C ABI of the particle forecasts, without a GPU: ffvd_op_forecast_particle_grouped / ffvd_op_posterior_forecast_particle_grouped
are declared in the header after the cubature forecasts with their argument lists plus the draws and the four new outputs, bound in
_lib.py with as many arguments as are declared, exported where the library is built, and return FFVD_EINVAL before any device call
beyond their limits (FFVD_OK for no groups or rows)."""
import ctypes

import numpy as np
import pytest

from ffvd_amd import _lib
from test_forecast_cubature_args import _declaration

E = _lib.FFVD_EINVAL
SYMBOLS = ("ffvd_op_forecast_particle_grouped", "ffvd_op_posterior_forecast_particle_grouped")
SIGNATURES = [_lib._SIGNATURES[s] for s in SYMBOLS]                    # (at import: without the symbols nothing here runs)
OLD = ("ffvd_op_forecast_cubature_grouped", "ffvd_op_posterior_forecast_cubature_grouped")
DRAWS = ["int N", "const double *eps", "long long eps_stride_g", "const double *unif", "long long unif_stride_g", "const double *xi0",
         "long long xi0_stride_g", "const double *eps_fc", "long long eps_fc_stride_g", "long long eps_fc_stride_b"]
NEW_OUT = ["double *ess", "double *log_evidence", "double *fc_lpd", "double *fc_particles"]


def test_the_symbols_are_declared_after_the_cubature_ones_with_the_declared_argument_counts():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, OLD):
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols()
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_moment_summary(")
        d, c = _declaration(new), _declaration(old)
        assert len(_lib._SIGNATURES[new][1]) == len(d) == len(c) + len(DRAWS) + len(NEW_OUT)
        k = c.index("int tracks_per_pass")
        assert d[:k + 1] == c[:k + 1] and d[k + 1:k + 1 + len(DRAWS)] == DRAWS
        assert d[k + 1 + len(DRAWS):] == c[k + 1:] + NEW_OUT
        sig = _lib._SIGNATURES[new][1]
        assert sig[:k + 1] == _lib._SIGNATURES[old][1][:k + 1] and sig[k + 1] is ctypes.c_int
        assert [sig[k + 1 + i] for i in (2, 4, 6, 8, 9)] == [ctypes.c_longlong] * 5
    for words in ("without weighting or\n * resampling", "fc_lpd_mix = log mean_g exp(fc_lpd[g])", "G * B * horizon * N * D < 2^31"):
        assert words in text


def test_the_symbols_are_exported():
    for s in SYMBOLS:
        assert hasattr(_lib.load(), s)


FILTER_OUT = ("mp", "Sp", "mf", "Sf", "X_", "lpd", "lj", "ms", "Ss", "ym", "yt", "lm", "lg")
FC_OUT = ("mfc", "Sfc", "fym", "fyt", "flm", "flg", "ess", "le", "flp", "fpa")
NO = ("X_", "ms", "Ss")                                            # cross and the smoother: NULL in a particle call


def _abi(fused, *, G=2, n_models=1, M=4, D=2, C=1, P=None, T=5, steps=6, kind=0, gpp=0, q_mode=0, J=1, null=NO, sd=1.0, y=0.0, horizon=2,
         origins=(0, 1, 3), n_origins=None, tpp=0, n=4, eps=0.0, unif=0.5, efc=0.0, strides=None, S0=False, small=False):
    """One call on zero inputs with every output buffer filled with 7; `null`: the arguments passed as NULL; strides: (eps_g, unif_g,
    xi0_g, eps_fc_g, eps_fc_b), None: the full layout; small: the draws are not sized by the scalars."""
    P = D + C if P is None else P
    B = len(origins) if n_origins is None else n_origins
    ng, nm, st, Pp, Jp, nb, h = max(G, 1), max(n_models, 1), max(steps, 1), max(P, 1), max(J, 1), max(B, 1), 1 if small else max(horizon, 1)
    nn = 1 if small else min(max(n, 1), 4096)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((nm, M, Pp)), lv=np.zeros((nm, D)), ll=np.zeros((nm, D, Pp)), X=np.zeros((ng, T + 1, D)), cf=np.zeros((max(T, 1), max(C, 1))),
             cr=np.zeros((st, max(C, 1))), lq=np.zeros((ng, D)), f=np.zeros((ng, M, D)), xl=np.zeros((ng, D)), CC=np.ones((D, Jp)), DD=np.zeros(Jp),
             sd=np.full(Jp, sd), Y=np.full((st, Jp), y), eps=np.full((ng, st, nn, D), eps), unif=np.full((ng, st), unif), xi0=np.zeros((ng, nn, D)),
             S0=np.tile(np.eye(D), (ng, 1, 1)), efc=np.full((ng, nb, h, nn, D), efc))
    vec, mat = (ng, st, D), (ng, st, D, D)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, X_=mat, lpd=(ng, st, Jp), lj=(ng, st), ms=vec, Ss=mat, ym=(st, Jp), yt=(st, Jp), lm=(st, Jp),
                  lg=(st, Jp), mfc=(ng, nb, h, D), Sfc=(ng, nb, h, D, D), fym=(nb, h, Jp), fyt=(nb, h, Jp), flm=(nb, h, Jp), flg=(nb, h, Jp),
                  ess=(ng, st), le=(ng,), flp=(ng, nb, h, Jp), fpa=(ng, nb, h, nn, D), U=(ng, M, D))
    outs = {k: np.full(s, 7.0) for k, s in shapes.items()}
    p = {k: (None if k in null else dp(v)) for k, v in list(a.items()) + list(outs.items())}
    org = np.asarray(origins, dtype=np.int32)
    op = None if "origins" in null else org.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    if strides is None:
        strides = (steps * n * D, steps, n * D, B * horizon * n * D, horizon * n * D)
    draws = (n, p["eps"], strides[0], p["unif"], strides[1], p["xi0"] if S0 else None, strides[2], p["efc"], strides[3], strides[4])
    filt = (p["CC"], p["DD"], p["sd"], J, p["Y"]) + tuple(p[k] for k in FILTER_OUT)
    fc = (horizon, op, B, tpp) + draws + tuple(p[k] for k in FC_OUT)
    s0 = p["S0"] if S0 else None
    if fused:
        rc = lib.ffvd_op_posterior_forecast_particle_grouped(kind, G, n_models, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"],
                                                             1e-5, gpp, q_mode, None, s0, p["cr"], steps, *filt, p["U"], *fc)
    else:
        Wm = [np.eye(M) for _ in range(nm * D)]
        Wt = None if "W" in null else (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = lib.ffvd_op_forecast_particle_grouped(kind, G, n_models, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, q_mode, p["xl"], s0,
                                                   p["cr"], C, steps, p["lq"], *filt, *fc)
    return rc, outs


# (the strides of the default call -- steps 6, n 4, D 2, B 3, horizon 2 -- are (48, 6, 8, 48, 16))
BAD_ABI = [dict(kind=1), dict(kind=2), dict(D=9, C=0), dict(M=2049), dict(M=0), dict(D=0), dict(J=9), dict(J=0), dict(q_mode=2), dict(G=3, n_models=2),
           dict(G=-1), dict(steps=-1), dict(P=2), dict(null=NO + ("Z",)), dict(null=NO + ("lq",)), dict(null=NO + ("cr",)), dict(null=NO + ("CC",)),
           dict(null=NO + ("Y",)), dict(null=FILTER_OUT + FC_OUT), dict(sd=0.0), dict(y=np.inf),
           dict(horizon=0), dict(origins=(), n_origins=0), dict(null=NO + ("origins",)), dict(origins=(0, 3, 1)), dict(origins=(0, 1, 4)),
           dict(origins=(0,), horizon=6), dict(tpp=-1),
           dict(null=("ms", "Ss")), dict(null=("X_", "Ss")), dict(null=("X_", "ms")),                    # cross / the smoother asked for
           dict(n=1), dict(n=0), dict(n=2049), dict(n=-3), dict(null=NO + ("eps",)), dict(null=NO + ("unif",)), dict(null=NO + ("efc",)),
           dict(S0=True, null=NO + ("xi0",)), dict(eps=np.nan), dict(eps=np.inf), dict(unif=1.0), dict(unif=-0.25), dict(unif=np.nan),
           dict(efc=np.nan), dict(efc=-np.inf),
           dict(strides=(47, 6, 8, 48, 16)), dict(strides=(48, 5, 8, 48, 16)), dict(strides=(48, 6, 7, 48, 16), S0=True),
           dict(strides=(48, 6, 8, 47, 16)), dict(strides=(48, 6, 8, 48, 15)), dict(strides=(48, 6, 8, 32, 0)), dict(strides=(-48, 6, 8, 48, 16)),
           dict(G=4, steps=1 << 17, origins=(0,), horizon=1, n=2048, small=True),                          # G steps N D = 2^32
           dict(G=4, steps=1 << 10, origins=tuple(range(512)), horizon=256, n=2048, small=True)]           # G B h N D = 2^32


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
        assert rc == E and b"particle forecasts" in msg and b"SE kernel only" in msg
        rc, _ = _abi(fused, n=2049)
        assert rc == E and b"2 <= N <= 2048" in lib.ffvd_last_error(None)
        rc, _ = _abi(fused, G=4, steps=1 << 10, origins=tuple(range(512)), horizon=256, n=2048, small=True)
        assert rc == E and b"G * B * h * N * D < 2^31" in lib.ffvd_last_error(None)
        rc, _ = _abi(fused, null=("ms", "Ss"))
        assert rc == E and b"no cross covariance and no smoother" in lib.ffvd_last_error(None)
    for ov in (dict(null=NO + ("f",)), dict(null=NO + ("xl",)), dict(null=NO + ("W",))):
        assert _abi(False, **ov)[0] == E
    for ov in (dict(T=0), dict(gpp=-1), dict(null=NO + ("X",)), dict(null=NO + ("cf",))):
        assert _abi(True, **ov)[0] == E


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(G=0, n_models=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov):
    rc, outs = _abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
