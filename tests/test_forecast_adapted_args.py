"""Argument checks of the adapted particle forecasts, without a GPU.  prediction.forecast_adapted_grouped /
posterior_forecast_adapted_grouped have the parameters of the bootstrap fan's two functions and run their packing stages: a malformed
draw raises ValueError before the library is loaded, well-formed arguments reach `ffvd_particle_adapted_forecast_grouped` /
`ffvd_posterior_particle_adapted_forecast_grouped` with the strides they imply.  The two symbols are declared with the argument lists of
the bootstrap fan's, bound with as many arguments, exported, and return FFVD_EINVAL before any device call beyond their limits -- wrong
strides, N out of range, draws that are not finite, an origin with o + h >= n, a kernel that is not SE -- with every output untouched.
DGPSSM.forecast_heldout_adapted has the parameters of forecast_heldout_particle and draws the same draws from the same seed."""
import inspect

import numpy as np
import pytest

import test_forecast_particle_abi as abi
import test_forecast_particle_args as base
from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_forecast_cubature_args import _declaration
from test_forecast_grouped_args import no_device  # noqa: F401  (a fixture)
from test_moment_grouped_args import COMMON, _explicit, _fused

SYMBOLS = ("ffvd_particle_adapted_forecast_grouped", "ffvd_posterior_particle_adapted_forecast_grouped")
SIGNATURES = [_lib._SIGNATURES[s] for s in SYMBOLS]                    # (at import: without the symbols nothing here runs)
PUBLIC = (pr.posterior_forecast_adapted_grouped, pr.forecast_adapted_grouped)
E = _lib.FFVD_EINVAL


@pytest.fixture
def adapted(monkeypatch):
    """the argument builders of the bootstrap fan's tests, aimed at the adapted functions and symbols"""
    monkeypatch.setattr(base, "PUBLIC", PUBLIC)
    real = _lib.load()

    class Lib:
        def __getattr__(self, name):
            return getattr(real, dict(zip(abi.SYMBOLS, SYMBOLS)).get(name, name))
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    return real


# ---- the public functions ---------------------------------------------------------------------------------------------------------------
def test_the_signatures_are_those_of_the_particle_forecasts(no_device):
    for new, old in ((pr.forecast_adapted_grouped, pr.forecast_particle_grouped),
                     (pr.posterior_forecast_adapted_grouped, pr.posterior_forecast_particle_grouped)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        assert list(a) == list(b)
        assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in b)
    doc = pr.forecast_adapted_grouped.__doc__
    assert "no draw enters" in doc and "no ancestor is read" in doc and "bit for bit" in doc


@pytest.mark.parametrize("what", sorted(base.BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(what, no_device, monkeypatch):
    monkeypatch.setattr(base, "PUBLIC", PUBLIC)
    for explicit in (True, False):
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "forecast_adapted_grouped: (eps|unif|xi0|eps_fc|return_particles)"):
            base._call(explicit, **base.BAD_DRAWS[what])


def test_horizon_origins_and_kernels_are_checked_before_the_library_is_loaded(no_device, monkeypatch):
    monkeypatch.setattr(base, "PUBLIC", PUBLIC)
    for explicit, make in ((True, _explicit), (False, _fused)):
        with pytest.raises(ValueError, match="LinearK"):
            base._call(explicit, COMMON["LinearK"](make))
        for kw in (dict(horizon=base.STEPS), dict(horizon=0), dict(horizon=2, origins=[2]), dict(horizon=1, origins=[2, 1])):
            with pytest.raises(ValueError):                        # (origins=[2], horizon 2: o + h >= n = 4)
                base._call(explicit, **kw)
        with pytest.raises(ValueError, match="tracks_per_pass"):
            base._call(explicit, tracks_per_pass=-1)


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
    monkeypatch.setattr(base, "PUBLIC", PUBLIC)
    G, D, STEPS, N, H, B = base.G, base.D, base.STEPS, base.N, base.H, base.B
    ne, nx, nf = STEPS * N * D, N * D, H * N * D
    layouts = (((), (), 0, 0, 0, (0, 0)), ((), (B,), 0, 0, 0, (0, nf)), ((G,), (G, B), ne, STEPS, nx, (B * nf, nf)))
    for lead, lead_fc, eg, ug, xg, fs in layouts:
        for kw in (dict(), dict(q_mode="intent", tracks_per_pass=1, return_tracks=True, return_filter=True),
                   dict(S0s=base.S0, xi0=np.zeros(lead + (N, D)), return_particles=True)):
            for explicit in (True, False):
                with pytest.raises(Reached):
                    base._call(explicit, **base._draws(lead=lead, lead_fc=lead_fc), **kw)
                name, a = seen[-1]
                assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
                p = 41 if explicit else 44                        # N follows tracks_per_pass
                assert a[p - 4] == H and a[p - 2] == B and a[p - 1] == kw.get("tracks_per_pass", 0)
                assert a[p] == N and a[p + 2] == eg and a[p + 4] == ug and (a[p + 8], a[p + 9]) == fs
                assert a[p + 6] == (xg if "xi0" in kw else 0) and (a[p + 5] is None) == ("xi0" not in kw)
                tail = a[p + 10:]
                assert len(tail) == 10 and (tail[9] is None) == ("return_particles" not in kw)
    assert {s for s, _ in seen} == set(SYMBOLS)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_bound_and_exported_with_the_particle_forecasts_argument_lists():
    text = open(_declaration.__globals__["HEADER"]).read()
    for new, old in zip(SYMBOLS, abi.SYMBOLS):
        assert _lib._SIGNATURES[new][0] is _lib._SIGNATURES[old][0] and new in _lib.exported_symbols() and hasattr(_lib.load(), new)
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_moment_summary(")
        assert _declaration(new) == _declaration(old)
        assert _lib._SIGNATURES[new][1] == _lib._SIGNATURES[old][1]
    assert not any(s.startswith("ffvd_op_") for s in SYMBOLS)      # (kept out of the lists that enumerate that prefix)


# (the strides of the default call -- steps 6, n 4, D 2, B 3, horizon 2 -- are (48, 6, 8, 48, 16))
BAD_ABI = [dict(kind=1), dict(kind=2),                                                                     # a kernel that is not SE
           dict(n=1), dict(n=0), dict(n=2049), dict(n=-3),                                                 # N out of range
           dict(efc=np.nan), dict(efc=-np.inf), dict(eps=np.nan), dict(eps=np.inf), dict(unif=1.0), dict(unif=np.nan),
           dict(origins=(0, 1, 4)), dict(origins=(0,), horizon=6), dict(origins=(0, 3, 1)), dict(horizon=0),   # o + h >= n; order; h
           dict(strides=(47, 6, 8, 48, 16)), dict(strides=(48, 5, 8, 48, 16)), dict(strides=(48, 6, 7, 48, 16), S0=True),
           dict(strides=(48, 6, 8, 47, 16)), dict(strides=(48, 6, 8, 48, 15)), dict(strides=(48, 6, 8, 32, 0)), dict(strides=(-48, 6, 8, 48, 16)),
           dict(null=abi.NO + ("efc",)), dict(null=abi.NO + ("eps",)), dict(S0=True, null=abi.NO + ("xi0",)),
           dict(null=("ms", "Ss")), dict(null=abi.NO + ("origins",)), dict(D=9, C=0), dict(J=9), dict(tpp=-1),
           dict(G=4, steps=1 << 10, origins=tuple(range(512)), horizon=256, n=2048, small=True)]           # G B h N D = 2^32


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", BAD_ABI, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused, adapted):
    rc, outs = abi._abi(fused, **ov)
    assert rc == E, rc
    assert SYMBOLS[fused].encode() + b": bad argument" in adapted.ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


def test_the_messages_say_why(adapted):
    for fused in (False, True):
        rc, _ = abi._abi(fused, kind=1)
        msg = adapted.ffvd_last_error(None)
        assert rc == E and b"adapted particle forecasts" in msg and b"SE kernel only" in msg
        rc, _ = abi._abi(fused, n=2049)
        assert rc == E and b"2 <= N <= 2048" in adapted.ffvd_last_error(None)
        rc, _ = abi._abi(fused, null=("ms", "Ss"))
        assert rc == E and b"no cross covariance and no smoother" in adapted.ffvd_last_error(None)


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", [dict(G=0), dict(steps=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_or_steps(fused, ov, adapted):
    rc, outs = abi._abi(fused, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _same(x, y):
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if x is None or isinstance(x, (str, bool, int, float)):
        return type(x) is type(y) and x == y
    return np.array_equal(x, y)


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    a = inspect.signature(DGPSSM.forecast_heldout_particle).parameters
    b = inspect.signature(DGPSSM.forecast_heldout_adapted).parameters
    assert list(a) == list(b) and all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    Y = np.zeros((8, 1))
    for kw, msg in ((dict(noise="per_record"), "forecast_heldout_adapted: noise"), (dict(num_particles=1), "forecast_heldout_adapted: num_particles"),
                    (dict(num_particles=2049), "num_particles"), (dict(q_mode="slice0"), "forecast_heldout_adapted: q_mode"),
                    (dict(horizon=8), "horizon"), (dict(origins=[3, 1]), "origins")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.forecast_heldout_adapted(base._Model(), Y, seed=1, **dict(dict(horizon=2), **kw))
    seen = {}
    for name in ("posterior_forecast_particle_grouped", "forecast_particle_grouped", "posterior_forecast_adapted_grouped", "forecast_adapted_grouped"):
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    # the same seed: the same draws and the same arguments as forecast_heldout_particle, in both forms
    for U_collapse, (mine, theirs), kw in ((True, ("posterior_forecast_adapted_grouped", "posterior_forecast_particle_grouped"), dict(stride=2)),
                                           (False, ("forecast_adapted_grouped", "forecast_particle_grouped"),
                                            dict(noise="independent", S0=np.eye(2), x0=np.arange(2.0), origins=[1, 4], return_tracks=True))):
        assert DGPSSM.forecast_heldout_adapted(base._Model(U_collapse), Y, None, 2, num_particles=16, seed=5, **kw) == mine
        assert DGPSSM.forecast_heldout_particle(base._Model(U_collapse), Y, None, 2, num_particles=16, seed=5, **kw) == theirs
        (a1, k1), (a2, k2) = seen[mine], seen[theirs]
        assert len(a1) == len(a2) and set(k1) == set(k2)
        assert all(_same(x, y) for x, y in zip(a1, a2))
        assert all(_same(k1[k], k2[k]) for k in k1)
    rng = np.random.default_rng(5)
    want = dict(eps=rng.standard_normal((8, 16, 2)), unif=rng.random((8,)), eps_fc=rng.standard_normal((2, 16, 2)))
    a1 = seen["posterior_forecast_adapted_grouped"][0]
    assert all(np.array_equal(a1[11 + i], want[n]) for i, n in enumerate(("eps", "unif", "eps_fc")))
