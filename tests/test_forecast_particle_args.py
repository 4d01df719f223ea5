"""Argument checks of the particle forecasts, without a GPU: prediction.forecast_particle_grouped /
posterior_forecast_particle_grouped run the packing stages of the cubature forecasts and their own (`_pack_particle_forecast`): every
shape and value check -- the model, the observations and the emission, horizon and origins, the layouts of eps / unif / xi0 /
eps_fc, draws that are not finite, a uniform outside [0, 1), xi0 against S0s, N outside [2, 2048], the 2^31 limits, LinearK -- raises
ValueError before the library is loaded; well-formed arguments in every layout reach the two symbols with the strides they imply;
forecast_grouped(method=...) keeps raising for anything but "moment"; DGPSSM.forecast_heldout_particle has the parameters of
forecast_heldout plus num_particles, seed and noise, draws by the seed and hands the two forms on."""
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import BAD_FILTER, EMISSION, SKIP, _filter_args
from test_forecast_grouped_args import BAD_PUBLIC, no_device  # noqa: F401  (no_device: a fixture)
from test_moment_grouped_args import BAD_EXPLICIT, BAD_FUSED, COMMON, _explicit, _fused, _with

SYMBOLS = ("ffvd_op_forecast_particle_grouped", "ffvd_op_posterior_forecast_particle_grouped")
G, D, STEPS, N, H = 3, 2, 4, 6, 2                                 # (the imported argument builders make G = 3, D = 2, steps = 4)
B = STEPS - H                                                     # the default origins of horizon H


PUBLIC = (pr.posterior_forecast_particle_grouped, pr.forecast_particle_grouped)     # (at import: without them nothing here runs)


def _fn(explicit):
    return PUBLIC[explicit]


def _draws(steps=STEPS, n=N, h=H, lead=(), lead_fc=()):
    return dict(eps=np.zeros(lead + (steps, n, D)), unif=np.full(lead + (steps,), 0.5), eps_fc=np.zeros(lead_fc + (h, n, D)))


def _call(explicit, a=None, **kw):
    a = (_explicit if explicit else _fused)() if a is None else a
    h = kw.get("horizon", H)
    args = _with(_with(_with(_filter_args(a, explicit), **EMISSION), horizon=H, **_draws(h=h if isinstance(h, int) and h > 0 else H)), **kw)
    return _fn(explicit)(**args)


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


@pytest.mark.parametrize("what", sorted(BAD_PUBLIC))
def test_horizon_and_origins_are_checked_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **dict(dict(horizon=1), **BAD_PUBLIC[what]))


@pytest.mark.parametrize("what", sorted(BAD_FILTER))
def test_observations_and_emission_are_checked_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError):
            _call(explicit, **BAD_FILTER[what])


S0 = np.tile(0.1 * np.eye(D), (G, 1, 1))
BAD_DRAWS = {
    "one particle": _draws(n=1),
    "2049 particles": _draws(n=2049),
    "eps with two axes": dict(eps=np.zeros((N, D))),
    "eps with five axes": dict(eps=np.zeros((G, 1, STEPS, N, D))),
    "eps of another D": dict(eps=np.zeros((STEPS, N, D + 1))),
    "eps of another length": dict(eps=np.zeros((STEPS + 1, N, D))),
    "eps of another G": dict(eps=np.zeros((G + 1, STEPS, N, D))),
    "an eps that is not finite": dict(eps=np.where(np.arange(STEPS * N * D).reshape(STEPS, N, D) == 7, np.nan, 0.0)),
    "an infinite eps": dict(eps=np.where(np.arange(STEPS * N * D).reshape(STEPS, N, D) == 9, np.inf, 0.0)),
    "unif of another length": dict(unif=np.full(STEPS + 1, 0.5)),
    "unif of another G": dict(unif=np.full((G + 1, STEPS), 0.5)),
    "a scalar unif": dict(unif=0.5),
    "a uniform of one": dict(unif=np.array([0.5, 1.0, 0.5, 0.5])),
    "a negative uniform": dict(unif=np.array([0.5, -1e-9, 0.5, 0.5])),
    "a uniform that is not finite": dict(unif=np.array([0.5, np.nan, 0.5, 0.5])),
    "S0s without xi0": dict(S0s=S0),
    "xi0 without S0s": dict(xi0=np.zeros((N, D))),
    "xi0 of another N": dict(S0s=S0, xi0=np.zeros((N + 1, D))),
    "xi0 of another D": dict(S0s=S0, xi0=np.zeros((N, D + 1))),
    "xi0 of another G": dict(S0s=S0, xi0=np.zeros((G + 1, N, D))),
    "an xi0 that is not finite": dict(S0s=S0, xi0=np.full((N, D), np.nan)),
    "eps_fc of another horizon": dict(eps_fc=np.zeros((H + 1, N, D))),
    "eps_fc of another N": dict(eps_fc=np.zeros((H, N + 1, D))),
    "eps_fc of another D": dict(eps_fc=np.zeros((H, N, D + 1))),
    "eps_fc of another B": dict(eps_fc=np.zeros((B + 1, H, N, D))),
    "eps_fc of another G": dict(eps_fc=np.zeros((G + 1, B, H, N, D))),
    "eps_fc per group alone": dict(eps_fc=np.zeros((G, H, N, D))) if G != B else dict(eps_fc=np.zeros((G + 1, H, N, D))),
    "eps_fc with two axes": dict(eps_fc=np.zeros((N, D))),
    "an eps_fc that is not finite": dict(eps_fc=np.where(np.arange(H * N * D).reshape(H, N, D) == 5, np.nan, 0.0)),
    "an infinite eps_fc": dict(eps_fc=np.where(np.arange(H * N * D).reshape(H, N, D) == 5, -np.inf, 0.0)),
    "return_particles that is no bool": dict(return_particles="yes"),
}


@pytest.mark.parametrize("what", sorted(BAD_DRAWS))
def test_every_malformed_draw_raises_before_the_library_is_loaded(what, no_device):
    for explicit in (True, False):
        with pytest.raises(ValueError, match=("" if explicit else "posterior_") + "forecast_particle_grouped: (eps|unif|xi0|eps_fc|return_particles)"):
            _call(explicit, **BAD_DRAWS[what])


def test_the_limits_of_two_to_the_31_are_checked_before_the_library_is_loaded(no_device, monkeypatch):
    """G * steps * N * D and G * B * h * N * D: checked on the shapes alone (the layouts are stubbed so that no array of that size is
    made)."""
    seen = []

    def layout(who, name, x, tail, lead):
        seen.append((name, tuple(tail), tuple(lead)))
        return np.zeros(1), (0,) * len(lead)
    monkeypatch.setattr(pr, "_fc_draw_layout", layout)
    eps = np.zeros((1, 2048, D))
    eps = np.lib.stride_tricks.as_strided(eps, shape=(1 << 17, 2048, D), strides=(0,) + eps.strides[1:])        # (no memory behind it)
    with pytest.raises(ValueError, match=r"G \* steps \* N \* D = \d+ must stay below 2\^31"):
        pr._pack_particle_forecast("t", 4, 2, 1 << 17, 1, D, eps, None, None, None, False, False)
    with pytest.raises(ValueError, match=r"G \* B \* horizon \* N \* D = \d+ must stay below 2\^31"):
        pr._pack_particle_forecast("t", 4, 1 << 9, 8, 1 << 8, D, eps[:8], None, None, None, False, False)
    assert ("eps_fc", (1 << 8, 2048, D), (4, 1 << 9)) in seen


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
    ne, nx, nf = STEPS * N * D, N * D, H * N * D
    layouts = (((), (), 0, 0, 0, (0, 0)), ((), (B,), 0, 0, 0, (0, nf)), ((G,), (G, B), ne, STEPS, nx, (B * nf, nf)))
    for lead, lead_fc, eg, ug, xg, fs in layouts:
        for kw in (dict(), dict(q_mode="intent", Y_train_std=1.7, tracks_per_pass=1, return_tracks=True, return_filter=True),
                   dict(S0s=S0, xi0=np.zeros(lead + (N, D)), return_particles=True)):
            for explicit in (True, False):
                with pytest.raises(Reached):
                    _call(explicit, **_draws(lead=lead, lead_fc=lead_fc), **kw)
                name, a = seen[-1]
                assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
                p = 41 if explicit else 44                        # N follows tracks_per_pass
                assert a[p - 4] == H and a[p - 2] == B and a[p - 1] == kw.get("tracks_per_pass", 0)
                assert a[p] == N and a[p + 2] == eg and a[p + 4] == ug and (a[p + 8], a[p + 9]) == fs
                assert a[p + 6] == (xg if "xi0" in kw else 0) and (a[p + 5] is None) == ("xi0" not in kw)
                tail = a[p + 10:]
                assert len(tail) == 10 and (tail[0] is None) == (tail[1] is None) == ("return_tracks" not in kw)
                assert all(t is not None for t in tail[2:6]) and tail[8] is not None
                assert (tail[6] is None) == (tail[7] is None) == ("return_filter" not in kw) and (tail[9] is None) == ("return_particles" not in kw)
    for kw in (dict(horizon=1), dict(horizon=3), dict(horizon=2, origins=[1]), dict(horizon=1, origins=[0, 2])):
        for explicit in (True, False):
            with pytest.raises(Reached):
                _call(explicit, **kw)
    with pytest.raises(Reached):                                  # no control columns
        _call(True, _explicit(C=0))
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_the_signatures_are_those_of_the_cubature_forecasts_with_the_draws(no_device):
    for new, old in ((pr.forecast_particle_grouped, pr.forecast_cubature_grouped),
                     (pr.posterior_forecast_particle_grouped, pr.posterior_forecast_cubature_grouped)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        pos = [k for k in b if b[k].kind is not inspect.Parameter.KEYWORD_ONLY]
        assert [k for k in a if a[k].kind is not inspect.Parameter.KEYWORD_ONLY] == pos + ["eps", "unif", "eps_fc"]
        assert set(a) - set(b) == {"eps", "unif", "eps_fc", "xi0", "return_particles"} and set(b) <= set(a)
        assert a["xi0"].default is None and a["return_particles"].default is False
        assert all(a[k].default == b[k].default for k in b)
    doc = pr.forecast_particle_grouped.__doc__
    assert "EQUAL weights" in doc and "without weighting or resampling" in doc and "lpd_fc" in doc and "common random numbers" in doc


def test_the_method_argument_of_the_family_is_what_it_was(no_device):
    assert pr.FILTER_METHODS == ("moment", "linearised")
    for explicit, make in ((True, _explicit), (False, _fused)):
        fn = pr.forecast_grouped if explicit else pr.posterior_forecast_grouped
        for method in ("particle", "cubature", "linearised", "pf"):
            with pytest.raises(ValueError, match="method"):
                fn(**_filter_args(make(), explicit), **EMISSION, horizon=1, method=method)
        with pytest.raises(TypeError, match="method"):
            _call(explicit, method="particle")


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class _Model:
    """what DGPSSM.forecast_heldout_particle reads before its prediction-level call"""
    _host_stale = False
    num_chains, output_dim = 3, 2
    Y = np.zeros((5, 1))
    control_inputs = np.zeros((20, 1))
    Q = np.ones(2)

    def __init__(self, U_collapse=True):
        self.U_collapse = U_collapse
        self._X_chains = [np.zeros((5, 2)) for _ in range(3)]
        self._rng = np.random.default_rng(0)

        class Layer:
            Z, kernel, U = np.zeros((4, 3)), ["k0", "k1"], np.zeros((4, 2))

        class Lik:
            CC, DD, log_Rchols = np.ones((2, 1)), np.zeros(1), np.zeros((1, 1))
        self.layers, self.likelihood = [Layer()], Lik()


def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    a = inspect.signature(DGPSSM.forecast_heldout).parameters
    b = inspect.signature(DGPSSM.forecast_heldout_particle).parameters
    assert list(a) == ["self", "Y_test", "control_inputs", "horizon", "stride", "origins", "x0", "S0", "q_mode", "Y_train_std", "return_tracks"]
    assert list(b)[:4] == list(a)[:4] and set(b) - set(a) == {"num_particles", "seed", "noise"} and set(a) <= set(b)
    assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a if k != "self")
    assert (b["num_particles"].default, b["seed"].default, b["noise"].default) == (256, None, "shared")
    assert all(b[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("num_particles", "seed", "noise"))
    Y = np.zeros((8, 1))
    for kw, msg in ((dict(noise="per_record"), "forecast_heldout_particle: noise"), (dict(noise=None), "forecast_heldout_particle: noise"),
                    (dict(num_particles=1), "forecast_heldout_particle: num_particles"), (dict(num_particles=2049), "num_particles"),
                    (dict(num_particles=64.0), "num_particles"), (dict(num_particles=True), "num_particles"),
                    (dict(q_mode="slice0"), "forecast_heldout_particle: q_mode"), (dict(horizon=8), "horizon"), (dict(origins=[3, 1]), "origins")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.forecast_heldout_particle(_Model(), Y, seed=1, **dict(dict(horizon=2), **kw))
    with pytest.raises(ValueError, match="forecast_heldout_particle: Y_test"):
        DGPSSM.forecast_heldout_particle(_Model(), np.zeros((8, 3)), seed=1)
    # independent draws beyond 1 GiB are refused with the byte count, before anything is drawn
    big, n, h = np.zeros((2000, 1)), 2048, 10
    nbytes = 8 * (3 * (2000 * n * 2 + 2000) + 3 * 1990 * h * n * 2)
    assert nbytes > 2 ** 30
    with pytest.raises(ValueError, match=f"{nbytes} bytes"):
        DGPSSM.forecast_heldout_particle(_Model(), big, None, h, num_particles=n, seed=1, noise="independent")
    seen = {}
    for name in ("posterior_forecast_particle_grouped", "forecast_particle_grouped"):
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    rng = np.random.default_rng(5)
    want = dict(eps=rng.standard_normal((8, 16, 2)), unif=rng.random((8,)), eps_fc=rng.standard_normal((2, 16, 2)))
    assert DGPSSM.forecast_heldout_particle(_Model(), Y, None, 2, num_particles=16, seed=5, stride=2, Y_train_std=1.7) == \
        "posterior_forecast_particle_grouped"
    a, k = seen["posterior_forecast_particle_grouped"]
    assert len(a) == 14 and a[5] == 5 and a[10] == 2 and all(np.array_equal(a[11 + i], want[n]) for i, n in enumerate(("eps", "unif", "eps_fc")))
    assert k["origins"].tolist() == [0, 2, 4] and k["xi0"] is None and k["x0s"] is None and k["S0s"] is None and k["Y_train_std"] == 1.7
    assert k["q_mode"] == "reference" and k["return_tracks"] is False and "stride" not in k
    e = _Model(U_collapse=False)                                   # explicit U; independent draws; a start covariance
    assert DGPSSM.forecast_heldout_particle(e, Y, None, 2, num_particles=16, seed=5, noise="independent", S0=np.eye(2), x0=np.arange(2.0),
                                            origins=[1, 4], return_tracks=True) == "forecast_particle_grouped"
    a, k = seen["forecast_particle_grouped"]
    assert a[0] == "Lm" and len(a) == 17 and a[13] == 2 and a[14].shape == (3, 8, 16, 2) and a[15].shape == (3, 8) and a[16].shape == (3, 2, 2, 16, 2)
    assert k["xi0"].shape == (3, 16, 2) and k["S0s"].shape == (3, 2, 2) and k["return_tracks"] is True and k["origins"].tolist() == [1, 4]
    assert np.all((a[15] >= 0.0) & (a[15] < 1.0)) and len(a[5]) == 3
