"""Argument checks of the particle filter with adaptive resampling over many records, without a GPU:
prediction.filter_adaptive_records_grouped / posterior_filter_adaptive_records_grouped, adaptive_records_seeded /
posterior_adaptive_records_seeded and DGPSSM.filter_records_adaptive.  They share the bootstrap pair's packing (`_pack_records`,
`_pack_particles`, `_pack_seeded`), so every malformed argument raises ValueError before the library is loaded and the message names
the function; well-formed arguments reach the four symbols in the documented order -- the bootstrap lists with ess_threshold behind
the draws and weights, resampled behind ancestors -- which are declared in the header, bound in _lib.py, exported where the library is
built, and return FFVD_EINVAL before any device call beyond their limits or for a bad threshold (FFVD_OK for no groups, records or
rows)."""
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

SYMBOLS = ("ffvd_particle_adaptive_records_grouped", "ffvd_posterior_particle_adaptive_records_grouped")
SEEDED = ("ffvd_particle_adaptive_seeded_records_grouped", "ffvd_posterior_particle_adaptive_seeded_records_grouped")
BOOTSTRAP = ("ffvd_op_filter_particle_records_grouped", "ffvd_op_posterior_filter_particle_records_grouped")
G, D, N, S0, _draws = tp.G, tp.D, tp.N, tp.S0, tp._draws
BAD_THRESHOLDS = (np.nan, np.inf, -np.inf, -0.1, -1e-300, "0.5", None, True, [0.5], 0.5 + 0j)
DRAW_NAMES = ["int N", "const double *eps", "long long eps_stride_g", "long long eps_stride_r", "const double *unif",
              "long long unif_stride_g", "long long unif_stride_r", "const double *xi0", "long long xi0_stride_g", "long long xi0_stride_r"]


def _fn(explicit, seeded=False):
    if seeded:
        return pr.adaptive_records_seeded if explicit else pr.posterior_adaptive_records_seeded
    return pr.filter_adaptive_records_grouped if explicit else pr.posterior_filter_adaptive_records_grouped


def _call(explicit, **kw):
    a = _with(_with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **_draws()), **kw)
    if "Y_records" in kw and "eps" not in kw and np.ndim(kw["Y_records"]) == 3 and np.shape(kw["Y_records"])[1] != STEPS:
        a.update(_draws(steps=np.shape(kw["Y_records"])[1]))
    return _fn(explicit)(**a)


def _call_seeded(explicit, **kw):
    a = _with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), **dict(dict(seed=3, num_particles=N), **kw))
    return _fn(explicit, True)(**a)


# ---- before the library is loaded --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(set(COMMON) - SKIP))
def test_model_mismatches_are_rejected_before_the_library_is_loaded(what, no_device):
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError):
            _fn(explicit)(**_records(COMMON[what](make), explicit), **EMISSION, **_draws())
        with pytest.raises(ValueError):
            _fn(explicit, True)(**_records(COMMON[what](make), explicit), **EMISSION, seed=1, num_particles=N)


@pytest.mark.parametrize("what", sorted(BAD))
def test_every_error_of_the_records_packing_raises_before_the_library_is_loaded(what, no_device):
    kw = dict(BAD[what])
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **dict(kw, xi0=np.zeros((N, D))) if "S0s" in kw else kw)
        with pytest.raises(ValueError):
            _call_seeded(explicit, **kw)


@pytest.mark.parametrize("what", sorted(tp.BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "filter_adaptive_records_grouped: (eps|unif|xi0|return_particles)"):
            _call(explicit, **tp.BAD_DRAWS[what])


@pytest.mark.parametrize("thr", BAD_THRESHOLDS, ids=repr)
def test_a_bad_threshold_raises_before_the_library_is_loaded(thr, no_device):
    for explicit in (True, False):
        pre = "" if explicit else "posterior_"
        with pytest.raises(ValueError, match=f"^{pre}filter_adaptive_records_grouped: ess_threshold"):
            _call(explicit, ess_threshold=thr)
        with pytest.raises(ValueError, match=f"^{pre}adaptive_records_seeded: ess_threshold"):
            _call_seeded(explicit, ess_threshold=thr)


def test_every_malformed_seeded_scalar_raises_before_the_library_is_loaded(no_device):
    for explicit in (True, False):
        who = ("" if explicit else "posterior_") + "adaptive_records_seeded"
        for kw, name in ((dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(seed=1.0), "seed"), (dict(seed=None), "seed"),
                         (dict(seed=True), "seed"), (dict(noise="common"), "noise"), (dict(noise=0), "noise"), (dict(num_particles=1), "num_particles"),
                         (dict(num_particles=2049), "num_particles"), (dict(num_particles=64.0), "num_particles"),
                         (dict(return_particles=1), "return_particles"), (dict(lengths=[STEPS, 0, STEPS]), "lengths"),
                         (dict(records_per_pass=-1), "records_per_pass")):
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call_seeded(explicit, **kw)
    with pytest.raises(ValueError, match="^adaptive_records_seeded: x0s"):
        _call_seeded(True, x0s=None)


def test_the_messages_name_the_function_and_the_argument(no_device):
    with pytest.raises(ValueError, match="filter_adaptive_records_grouped: x0s"):
        _call(True, x0s=None)
    for kw, name in ((dict(lengths=[STEPS, 0, STEPS]), "lengths"), (dict(records_per_pass=-1), "records_per_pass"),
                     (dict(control_records=None), "control_records"), (dict(Y_records=np.zeros((STEPS, 1))), "Y_records"),
                     (_draws(n=1), r"eps: the number of particles N must lie in \[2, 2048\]"), (dict(S0s=S0), "xi0")):
        for explicit in (True, False):
            who = ("" if explicit else "posterior_") + "filter_adaptive_records_grouped"
            with pytest.raises(ValueError, match=f"^{who}: {name}"):
                _call(explicit, **kw)


# ---- what reaches the library --------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _recording_library(monkeypatch):
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                seen.append((name, a))
                raise _Reached()
            return f
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    return seen


def test_well_formed_arguments_in_every_layout_reach_the_adaptive_symbols(monkeypatch):
    seen = _recording_library(monkeypatch)
    Y = np.zeros((R, STEPS, 1))
    Y[1, 2:] = np.nan
    inner = STEPS * N * D
    layouts = (((), (0, 0), (0, 0), (0, 0)), ((R,), (0, inner), (0, STEPS), (0, N * D)),
               ((G, R), (R * inner, inner), (R * STEPS, STEPS), (R * N * D, N * D)))
    for lead, es, us, xs in layouts:
        for kw, thr in ((dict(), 0.5), (dict(Y_records=Y, lengths=[STEPS, 2, STEPS], records_per_pass=2, q_mode="intent", Y_train_std=1.7,
                                          ess_threshold=0), 0.0),
                        (dict(S0s=S0, xi0=np.zeros(lead + (N, D)), return_particles=True, ess_threshold=np.float32(2.0)), 2.0)):
            for explicit in (True, False):
                with pytest.raises(_Reached):
                    _call(explicit, **_draws(lead=lead), **kw)
                name, a = seen[-1]
                assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
                p = 26 if explicit else 28                        # N follows records_per_pass
                assert a[p] == N and (a[p + 2], a[p + 3]) == es and (a[p + 5], a[p + 6]) == us
                assert (a[p + 8], a[p + 9]) == (xs if "xi0" in kw else (0, 0)) and (a[p + 7] is None) == ("xi0" not in kw)
                assert isinstance(a[p + 10], float) and a[p + 10] == thr                       # ess_threshold follows the draws
                tail = a[p + 11:] if explicit else a[p + 11:-1]
                assert len(tail) == 16 and (tail[12] is None) == (tail[13] is None) == (tail[14] is None) == ("return_particles" not in kw)
                assert all(t is not None for t in tail[:12]) and tail[15] is not None          # resampled is always returned
                assert explicit or a[-1] is None                                               # U_means stays last
    with pytest.raises(_Reached):                                 # the fused call may leave the start to the training states
        _call(False, x0s=None)
    with pytest.raises(_Reached):                                 # R = 1: a single record
        _call(True, Y_records=Y[:1], control_records=np.zeros((1, STEPS, 1)), x0s=np.zeros((1, 2)))
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_well_formed_seeded_arguments_reach_the_seeded_symbols(monkeypatch):
    seen = _recording_library(monkeypatch)
    for mode, noise in enumerate(pr.PARTICLE_NOISE):
        for kw in (dict(), dict(S0s=S0, return_particles=True, ess_threshold=0.25, seed=2 ** 64 - 1)):
            for explicit in (True, False):
                with pytest.raises(_Reached):
                    _call_seeded(explicit, noise=noise, **kw)
                name, a = seen[-1]
                assert name == SEEDED[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
                p = 26 if explicit else 28
                assert a[p:p + 4] == (N, kw.get("seed", 3), mode, kw.get("ess_threshold", 0.5))   # N, seed, noise, ess_threshold
                tail = a[p + 4:] if explicit else a[p + 4:-1]
                assert len(tail) == 16 and (tail[12] is None) == (tail[14] is None) == ("return_particles" not in kw) and tail[15] is not None
    assert {s for s, _ in seen} == set(SEEDED)


def test_the_signatures_are_the_bootstrap_pair_s_plus_the_threshold(no_device):
    for new, old in ((pr.filter_adaptive_records_grouped, pr.filter_particle_records_grouped),
                     (pr.posterior_filter_adaptive_records_grouped, pr.posterior_filter_particle_records_grouped)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        assert [k for k in a if k != "ess_threshold"] == list(b)
        assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in b)
        assert a["ess_threshold"].default == 0.5 and a["ess_threshold"].kind == inspect.Parameter.KEYWORD_ONLY
    for new in (pr.adaptive_records_seeded, pr.posterior_adaptive_records_seeded):
        a = inspect.signature(new).parameters
        assert a["seed"].default is inspect.Parameter.empty and a["num_particles"].default == 256 and a["ess_threshold"].default == 0.5
        assert a["noise"].default == "shared" and "eps" not in a and "rule" not in a and "stage" not in a
    doc = pr.filter_adaptive_records_grouped.__doc__
    for words in ("ADAPTIVE resampling", "ess_threshold * N", "bit for bit", "log_evidence", "resampled", "weights", "not built"):
        assert words in doc, words
    assert "filter_adaptive_records_grouped" in pr.filter_particle_records_grouped.__doc__


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    sig = inspect.signature(DGPSSM.filter_records_adaptive).parameters
    old = inspect.signature(DGPSSM.filter_records_particle).parameters
    assert [k for k in sig if k not in ("ess_threshold", "draws")] == list(old)
    assert all(sig[k].default == old[k].default and sig[k].kind == old[k].kind for k in old)
    assert sig["ess_threshold"].default == 0.5 and sig["draws"].default == "numpy"
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    who = "filter_records_adaptive"
    for kw, msg in ((dict(noise="common"), f"{who}: noise"), (dict(num_particles=1), f"{who}: num_particles"), (dict(num_particles=True), "num_particles"),
                    (dict(q_mode="slice0"), f"{who}: q_mode"), (dict(x0=np.zeros(3)), "x0"), (dict(draws="host"), f"{who}: draws"),
                    (dict(draws=None), f"{who}: draws"), (dict(draws="device", seed=None), f"{who}: seed"),
                    (dict(draws="device", seed=1.5), f"{who}: seed"), (dict(draws="device", seed=-1), f"{who}: seed"),
                    (dict(draws="device", seed=True), f"{who}: seed"), (dict(draws="device", noise="common"), f"{who}: noise"),
                    (dict(draws="device", num_particles=2049), f"{who}: num_particles")) + \
            tuple((dict(ess_threshold=t, draws=d), f"{who}: ess_threshold") for t in BAD_THRESHOLDS for d in ("numpy", "device")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.filter_records_adaptive(_Model(), Y, ctrl, **dict(dict(seed=1), **kw))
    with pytest.raises(ValueError, match=f"{who}: Y_records"):
        DGPSSM.filter_records_adaptive(_Model(), np.zeros((STEPS, 1)), ctrl, seed=1)
    with pytest.raises(ValueError, match="control_records"):
        DGPSSM.filter_records_adaptive(_Model(), Y, seed=1)
    seen = {}
    names = ("posterior_filter_adaptive_records_grouped", "filter_adaptive_records_grouped", "posterior_adaptive_records_seeded",
             "adaptive_records_seeded", "filter_particle_records_grouped")
    for name in names:
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    m, e = _Model(), _Model(U_collapse=False)
    kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7)
    rng = np.random.default_rng(5)
    want = dict(eps=rng.standard_normal((STEPS, 16, 2)), unif=rng.random((STEPS,)))
    assert DGPSSM.filter_records_adaptive(m, Y, ctrl, num_particles=16, seed=5, **kw) == "posterior_filter_adaptive_records_grouped"
    a, k = seen["posterior_filter_adaptive_records_grouped"]
    assert k == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", Y_train_std=1.7, records_per_pass=2, x0s=None, xi0=None, return_particles=False,
                     ess_threshold=0.5)
    assert len(a) == 12 and np.array_equal(a[10], want["eps"]) and np.array_equal(a[11], want["unif"])
    # draws="numpy": the same seed gives the bootstrap method's draws in the same order
    for noise, lead in (("per_record", (R,)), ("independent", (3, R))):
        args = dict(num_particles=16, seed=5, noise=noise, S0=np.eye(2), x0=np.arange(2.0), return_particles=True)
        assert DGPSSM.filter_records_adaptive(e, Y, ctrl, ess_threshold=0.25, **args) == "filter_adaptive_records_grouped"
        assert DGPSSM.filter_records_particle(e, Y, ctrl, **args) == "filter_particle_records_grouped"
        (a, k), (b, kb) = seen["filter_adaptive_records_grouped"], seen["filter_particle_records_grouped"]
        assert a[0] == "Lm" and len(a) == 14 and a[12].shape == lead + (STEPS, 16, 2) and k["ess_threshold"] == 0.25 and "smooth" not in k
        assert np.array_equal(a[12], b[12]) and np.array_equal(a[13], b[13]) and np.array_equal(k["xi0"], kb["xi0"])
        assert set(k) == set(kb) | {"ess_threshold"}
    # draws="device": nothing is drawn on the host; the seeded functions get the scalars
    assert DGPSSM.filter_records_adaptive(m, Y, ctrl, num_particles=16, seed=9, draws="device", noise="per_record", ess_threshold=0, **kw) == \
        "posterior_adaptive_records_seeded"
    a, k = seen["posterior_adaptive_records_seeded"]
    assert len(a) == 10 and k == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", Y_train_std=1.7, records_per_pass=2, x0s=None,
                                      num_particles=16, ess_threshold=0.0, seed=9, noise="per_record", return_particles=False)
    assert DGPSSM.filter_records_adaptive(e, Y, ctrl, num_particles=16, seed=9, draws="device") == "adaptive_records_seeded"
    a, k = seen["adaptive_records_seeded"]
    assert a[0] == "Lm" and len(a) == 12 and k["seed"] == 9 and k["noise"] == "shared" and "xi0" not in k and "smooth" not in k


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_in_the_documented_order_and_bound():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, seeded, old in zip(SYMBOLS, SEEDED, BOOTSTRAP):
        for s in (new, seeded):
            assert _lib._SIGNATURES[s][0] is ctypes.c_int and s in _lib.exported_symbols() and not s.startswith("ffvd_op_")
            assert text.index("ffvd_posterior_particle_seeded_records_grouped(") < text.index(s + "(") < text.index("ffvd_op_forecast_grouped(")
        d, ds, c = _declaration(new), _declaration(seeded), _declaration(old)
        assert len(_lib._SIGNATURES[new][1]) == len(d) and len(_lib._SIGNATURES[seeded][1]) == len(ds)
        k = c.index("int records_per_pass")
        assert d[:k + 11] == c[:k + 11] and d[k + 1:k + 11] == DRAW_NAMES              # the bootstrap list up to the draws
        assert d[k + 11] == "double ess_threshold"
        i = c.index("int *ancestors")
        assert d[k + 12:i + 2] == c[k + 11:i + 1]                                       # m_pred .. ancestors
        assert d[i + 2:i + 4] == ["double *weights", "int *resampled"] and d[i + 4:] == c[i + 1:]   # (U_means stays last)
        assert ds == d[:k + 1] + ["int N", "unsigned long long seed", "int noise"] + d[k + 11:]
        sig, sigs = _lib._SIGNATURES[new][1], _lib._SIGNATURES[seeded][1]
        assert sig[k + 11] is ctypes.c_double and sig[i + 3] is ctypes.POINTER(ctypes.c_int) and sigs[k + 2] is ctypes.c_ulonglong
        assert sig[:k + 11] == _lib._SIGNATURES[old][1][:k + 11]
    for words in ("ADAPTIVE (ESS-triggered) resampling", "ess_threshold * N", "resampled[t] = 1", "finite and >= 0",
                  "ffvd_particle_draws(seed, noise, ..)"):
        assert words in text, words
    assert "No adaptive resampling" in text                       # the bootstrap call's own paragraph stands


def test_the_symbols_are_exported():
    for s in SYMBOLS + SEEDED:
        assert hasattr(_lib.load(), s)


class _Adaptive:
    """the library with the two bootstrap entry points answered by the adaptive ones (seeded: by the seeded ones, with a fixed seed and
    the noise mode of the strides): tests/test_filter_particle_args.py's `_abi` as is.  The outputs the bootstrap list does not have
    are filled with 7 and kept in `extra`."""

    def __init__(self, lib, thr, seeded, extra):
        self._lib, self._thr, self._seeded, self._extra = lib, thr, seeded, extra

    def __getattr__(self, name):
        if name not in BOOTSTRAP:
            return getattr(self._lib, name)
        fused = name == BOOTSTRAP[1]

        def f(*a):
            p = 28 if fused else 26
            head, draws, outs = a[:p], a[p:p + 10], a[p + 10:]
            G, R, steps, n = a[1], a[17 if fused else 13], a[21 if fused else 18], a[p]
            w = np.full((max(G, 1), max(R, 1), max(steps, 1), min(max(n, 1), 4096)), 7.0)
            rs = np.full((max(G, 1), max(R, 1), max(steps, 1)), 7, dtype=np.int32)
            self._extra.update(weights=w, resampled=rs)
            mine = (_lib.dptr(w), rs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
            if all(o is None for o in outs[:14]):                 # (the case with no output at all: none of the new ones either)
                mine = (None, None)
            outs = outs[:14] + mine + outs[14:]
            if self._seeded:
                return getattr(self._lib, SEEDED[fused])(*head, n, 5, 2, self._thr, *outs)
            return getattr(self._lib, SYMBOLS[fused])(*head, *draws, self._thr, *outs)
        return f


def _abi(monkeypatch, fused, thr=0.5, seeded=False, **ov):
    lib, extra = _lib.load(), {}
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "load", lambda: _Adaptive(lib, thr, seeded, extra))
        rc, outs = tp._abi(fused, **ov)
    outs.update(extra)
    return rc, outs


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", tp.BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused, monkeypatch):
    rc, outs = _abi(monkeypatch, fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


SEEDED_BAD_ABI = [ov for ov in tp.BAD_ABI if not ({"eps", "unif", "strides"} & set(ov)) and "eps" not in ov.get("null", ()) and
                  "unif" not in ov.get("null", ()) and "xi0" not in ov.get("null", ())]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", SEEDED_BAD_ABI, ids=str)
def test_seeded_abi_rejects_bad_arguments_without_a_device(ov, fused, monkeypatch):
    """tests/test_filter_particle_args.py's list without the cases that are about the caller's draw arrays"""
    rc, outs = _abi(monkeypatch, fused, seeded=True, **ov)
    assert rc == E, rc
    assert SEEDED[fused].encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


@pytest.mark.parametrize("seeded", [False, True], ids=["drawn", "seeded"])
@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("thr", [np.nan, np.inf, -np.inf, -0.5, -1e-300], ids=repr)
def test_abi_rejects_a_bad_threshold_without_a_device(thr, fused, seeded, monkeypatch):
    for ov in (dict(), dict(G=0), dict(steps=0)):                 # (also where there is nothing to do)
        rc, outs = _abi(monkeypatch, fused, thr=thr, seeded=seeded, **ov)
        msg = _lib.load().ffvd_last_error(None)
        assert rc == E and (SEEDED if seeded else SYMBOLS)[fused].encode() + b": bad argument" in msg and b"ess_threshold" in msg
        assert all(np.all(v == 7) for v in outs.values())


def test_the_messages_say_why(monkeypatch):
    lib = _lib.load()
    for fused in (False, True):
        rc, _ = _abi(monkeypatch, fused, kind=1)
        msg = lib.ffvd_last_error(None)
        assert rc == E and b"adaptive particle filter of many records" in msg and b"SE kernel only" in msg
        rc, _ = _abi(monkeypatch, fused, G=2, R=1 << 20, steps=1 << 8, small=True)
        assert rc == E and b"G * R * steps * D * D < 2^31" in lib.ffvd_last_error(None)
        rc, _ = _abi(monkeypatch, fused, n=2049)
        assert rc == E and b"2 <= N <= 2048" in lib.ffvd_last_error(None)
    for ov in (dict(null=("f",)), dict(null=("xl",)), dict(null=("W",))):
        assert _abi(monkeypatch, False, **ov)[0] == E
    for ov in (dict(T=0), dict(gpp=-1), dict(null=("X",)), dict(null=("cf",))):
        assert _abi(monkeypatch, True, **ov)[0] == E


def test_the_seeded_abi_rejects_a_bad_noise_mode():
    lib = _lib.load()
    n = len(_lib._SIGNATURES[SEEDED[0]][1])
    for noise in (-1, 3):
        args = [0, 0, 1, None, None, 4, 3, 2, None, None, None, None, 0, 0, None, None, None, 1, 0, None, None, None, None, 1, None, 0, 4, 1, noise, 0.5]
        rc = getattr(lib, SEEDED[0])(*args, *([None] * (n - len(args))))
        assert rc == E and b"noise 0, 1 or 2" in lib.ffvd_last_error(None)


@pytest.mark.parametrize("seeded", [False, True], ids=["drawn", "seeded"])
@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0), dict(steps=0, J=3)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(fused, seeded, ov, monkeypatch):
    for thr in (0.0, 0.5, 2.0):
        rc, outs = _abi(monkeypatch, fused, thr=thr, seeded=seeded, **ov)
        assert rc == _lib.FFVD_OK
        assert all(np.all(v == 7) for v in outs.values())
