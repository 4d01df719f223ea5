"""Argument checks of the seeded particle calls, without a GPU: prediction.particle_draws, particle_records_seeded and
posterior_particle_records_seeded raise ValueError on every malformed seed, noise mode, rule, stage, particle or trajectory count and
on every mismatch of the records packing before the library is loaded; well-formed arguments reach the two new symbols with rule and
stage in front, (N, seed, noise) where the siblings have their draws, and NULL for what the (rule, stage) does not produce;
DGPSSM.particle_records_seeded checks its arguments through a stand-in model, draws a seed from the model's generator when none is
given and hands the two forms on -- the six NumPy-drawn methods keep their parameter lists; the three symbols are declared in the
header, bound in _lib.py, exported without the ffvd_op_ prefix, and return FFVD_EINVAL before any device call beyond their limits
(FFVD_OK with nothing touched for no groups, records or rows)."""
import ctypes
import inspect

import numpy as np
import pytest

from ffvd_amd import _lib
from ffvd_amd import prediction as pr
from test_filter_grouped_args import E, EMISSION, no_device  # noqa: F401  (no_device: a fixture)
from test_filter_records_args import BAD, R, STEPS, _declaration, _Model, _records
from test_moment_grouped_args import _explicit, _fused, _with

SYMBOLS = ("ffvd_particle_seeded_records_grouped", "ffvd_posterior_particle_seeded_records_grouped")
DRAWS = "ffvd_particle_draws"
FNS = {True: "particle_records_seeded", False: "posterior_particle_records_seeded"}
RULES, STAGES, NOISE = ("bootstrap", "adapted"), ("filter", "smooth", "backsim"), ("shared", "per_record", "independent")
G, D, N, NB = 3, 2, 6, 5
S0 = np.tile(np.array([[1.0, 0.5], [0.5, 1.0]]), (R, 1, 1))


def _call(explicit, **kw):
    a = _with(_with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION), seed=11, num_particles=N)
    return getattr(pr, FNS[explicit])(**_with(a, **kw))


# ---- prediction.particle_draws ---------------------------------------------------------------------------------------------------------
BAD_DRAW_ARGS = {
    "a negative seed": (dict(seed=-1), "seed"), "a seed of 2^64": (dict(seed=2 ** 64), "seed"), "a fractional seed": (dict(seed=1.5), "seed"),
    "a bool for a seed": (dict(seed=True), "seed"), "no seed": (dict(seed=None), "seed"),
    "an unknown noise mode": (dict(noise="common"), "noise"), "a noise index": (dict(noise=2), "noise"), "no noise mode": (dict(noise=None), "noise"),
    "no groups": (dict(G=0), "G"), "no records": (dict(R=0), "R"), "no rows": (dict(steps=0), "steps"), "fractional rows": (dict(steps=4.0), "steps"),
    "one particle": (dict(N=1), "N"), "too many particles": (dict(N=2049), "N"), "D = 0": (dict(D=0), "D"), "D = 9": (dict(D=9), "D"),
    "a negative B": (dict(B=-1), "B"), "B beyond the limit": (dict(B=4097), "B"), "a bool for B": (dict(B=True), "B"),
    "with_xi0 that is no bool": (dict(with_xi0=1), "with_xi0"),
    "more draws than the library indexes": (dict(G=1024, R=1024, steps=64, N=32, noise="shared"), r"G \* R \* steps \* N \* D"),
    "more trajectories than the grid has": (dict(G=1024, R=1024, steps=1, N=2, D=1, B=2048), r"G \* R \* B"),
}


@pytest.mark.parametrize("what", sorted(BAD_DRAW_ARGS))
def test_particle_draws_checks_its_arguments_before_the_library_is_loaded(what, no_device):
    kw, name = BAD_DRAW_ARGS[what]
    a = _with(dict(seed=3, noise="independent", G=2, R=3, steps=4, N=6, D=2), **kw)
    opt = {k: a.pop(k) for k in ("with_xi0", "B") if k in a}
    with pytest.raises(ValueError, match=f"^particle_draws: {name}"):
        pr.particle_draws(a["seed"], a["noise"], a["G"], a["R"], a["steps"], a["N"], a["D"], **opt)


def test_particle_draws_reaches_the_library_with_the_mode_s_shapes(monkeypatch):
    seen = []

    class Lib:
        def ffvd_particle_draws(self, *a):
            seen.append(a)
            return 0
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    for mode, (noise, lead) in enumerate((("shared", ()), ("per_record", (3,)), ("independent", (2, 3)))):
        out = pr.particle_draws(2 ** 64 - 1, noise, 2, 3, 4, 6, 2)
        assert set(out) == {"eps", "unif"} and out["eps"].shape == lead + (4, 6, 2) and out["unif"].shape == lead + (4,)
        a = seen[-1]
        assert a[:8] == (2 ** 64 - 1, mode, 2, 3, 4, 6, 2, 0) and a[8] is not None and a[9] is not None and a[10] is None and a[11] is None
        out = pr.particle_draws(np.int64(5), noise, 2, 3, 4, 6, 2, with_xi0=True, B=NB)
        assert set(out) == {"eps", "unif", "xi0", "unif_bs"} and out["xi0"].shape == lead + (6, 2) and out["unif_bs"].shape == lead + (4, NB)
        assert seen[-1][:8] == (5, mode, 2, 3, 4, 6, 2, NB) and all(p is not None for p in seen[-1][8:])
    assert len(_lib._SIGNATURES[DRAWS][1]) == 12


# ---- prediction.particle_records_seeded / posterior_particle_records_seeded ---------------------------------------------------------------
@pytest.mark.parametrize("bad", sorted(BAD))
def test_every_error_of_the_records_packing_raises_before_the_library_is_loaded(bad, no_device):
    for explicit in (True, False):
        for stage, B in (("filter", 0), ("backsim", NB)):
            with pytest.raises(ValueError):
                _call(explicit, stage=stage, num_trajectories=B, **BAD[bad])


BAD_SEEDED = {
    "a negative seed": (dict(seed=-1), "seed"), "a seed of 2^64": (dict(seed=2 ** 64), "seed"), "a fractional seed": (dict(seed=7.0), "seed"),
    "a bool for a seed": (dict(seed=False), "seed"), "no seed": (dict(seed=None), "seed"), "a generator for a seed": (dict(seed=np.random.default_rng(1)), "seed"),
    "an unknown noise mode": (dict(noise="common"), "noise"), "no noise mode": (dict(noise=None), "noise"), "a noise index": (dict(noise=0), "noise"),
    "an unknown rule": (dict(rule="auxiliary"), "rule"), "a rule index": (dict(rule=1), "rule"), "no rule": (dict(rule=None), "rule"),
    "an unknown stage": (dict(stage="smoother"), "stage"), "a stage index": (dict(stage=2), "stage"), "no stage": (dict(stage=None), "stage"),
    "one particle": (dict(num_particles=1), "num_particles"), "too many particles": (dict(num_particles=2049), "num_particles"),
    "a fractional particle count": (dict(num_particles=64.0), "num_particles"), "a bool for the particles": (dict(num_particles=True), "num_particles"),
    "trajectories of the filter": (dict(num_trajectories=4), "num_trajectories"),
    "trajectories of the smoother": (dict(stage="smooth", num_trajectories=4), "num_trajectories"),
    "a backward simulation without trajectories": (dict(stage="backsim"), "num_trajectories"),
    "too many trajectories": (dict(stage="backsim", num_trajectories=4097), "num_trajectories"),
    "fractional trajectories": (dict(stage="backsim", num_trajectories=2.5), "num_trajectories"),
    "a bool for the trajectories": (dict(stage="backsim", num_trajectories=True), "num_trajectories"),
    "return_particles that is no bool": (dict(return_particles=1), "return_particles"),
}


@pytest.mark.parametrize("what", sorted(BAD_SEEDED))
def test_every_malformed_scalar_raises_before_the_library_is_loaded(what, no_device):
    kw, name = BAD_SEEDED[what]
    for explicit in (True, False):
        with pytest.raises(ValueError, match=f"^{FNS[explicit]}: {name}"):
            _call(explicit, **kw)


def test_the_index_limit_and_the_seed_itself_are_needed(no_device):
    big = _records((_explicit)(G=3), True, R=300, steps=600)
    with pytest.raises(ValueError, match=r"^particle_records_seeded: G \* R \* steps \* N \* D = 2211840000 must stay below 2\^31"):
        pr.particle_records_seeded(**big, **EMISSION, seed=1, num_particles=2048, noise="shared")
    with pytest.raises(ValueError, match="^particle_records_seeded: x0s"):
        _call(True, x0s=None)
    for explicit in (True, False):
        a = _with(_records((_explicit if explicit else _fused)(), explicit), **EMISSION)
        with pytest.raises(TypeError, match="seed"):
            getattr(pr, FNS[explicit])(**a)


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
    forms = ((dict(), [STEPS] * R), (dict(Y_records=Y, lengths=[STEPS, 2, STEPS], records_per_pass=2), [STEPS, 2, STEPS]),
             (dict(S0s=S0, return_particles=True), [STEPS] * R))
    for kw, lens in forms:
        stacks = "return_particles" in kw
        for explicit in (True, False):
            for ri, rule in enumerate(RULES):
                for si, stage in enumerate(STAGES):
                    for ni, noise in enumerate(NOISE):
                        B = NB if stage == "backsim" else 0
                        with pytest.raises(Reached):
                            _call(explicit, rule=rule, stage=stage, noise=noise, seed=2 ** 63 + ni, num_trajectories=B, **kw)
                        name, a = seen[-1]
                        assert name == SYMBOLS[not explicit] and len(a) == len(_lib._SIGNATURES[name][1])
                        assert a[:2] == (ri, si) and a[2] == 0 and a[3] == G                # rule, stage, then kind, G
                        tail = a[-14:] if explicit else a[-15:-1]
                        head = a[:-14] if explicit else a[:-15]
                        assert head[-17:-14] == (N, 2 ** 63 + ni, ni)                       # N, seed, noise where the draws were
                        assert all(p is not None for p in head[-14:-3])                     # m_pred .. ess
                        assert head[-3] is not None and (head[-2] is None) != stacks and (head[-1] is None) != stacks
                        lengths, nb, traj, idx, m_traj, S_traj, lag, w, tm, tv, ms, Ss, es, ws = tail
                        assert nb == B
                        if stage == "filter":
                            assert lengths is None and all(t is None for t in tail[2:])
                            continue
                        assert [lengths[r] for r in range(R)] == lens
                        assert all((t is None) != (stage == "backsim") for t in (traj, idx, m_traj, S_traj, lag))
                        assert all((t is None) != (stage == "smooth") for t in (ms, Ss, es))
                        assert (ws is None) != (stage == "smooth" and stacks)
                        assert (w is None) != (stacks and rule == "bootstrap") and (tm is None) != stacks and (tv is None) != stacks
                        assert explicit or a[-1] is None                                    # U_means stays last
    assert {s for s, _ in seen} == set(SYMBOLS)


def test_the_signatures_are_the_siblings_without_the_draws(no_device):
    for new, old in ((pr.particle_records_seeded, pr.backsim_particle_records_grouped),
                     (pr.posterior_particle_records_seeded, pr.posterior_backsim_particle_records_grouped)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        pos = [k for k in b if b[k].kind is not inspect.Parameter.KEYWORD_ONLY]
        assert [k for k in a if a[k].kind is not inspect.Parameter.KEYWORD_ONLY] == [k for k in pos if k not in ("eps", "unif", "unif_bs")]
        assert set(a) - set(b) == {"seed", "num_particles", "rule", "stage", "noise", "num_trajectories"}
        assert set(b) - set(a) == {"eps", "unif", "unif_bs", "xi0"}
        assert all(a[k].default == b[k].default for k in set(a) & set(b))
        assert a["seed"].default is inspect.Parameter.empty and a["seed"].kind is inspect.Parameter.KEYWORD_ONLY
        assert (a["num_particles"].default, a["rule"].default, a["stage"].default, a["noise"].default, a["num_trajectories"].default) == \
            (256, "bootstrap", "filter", "shared", 0)
    assert pr.PARTICLE_RULES == RULES and pr.PARTICLE_STAGES == STAGES and pr.PARTICLE_NOISE == NOISE
    doc = pr.particle_records_seeded.__doc__
    for words in ("Philox4x32-10", "bit for bit", "particle_draws", "independent", "2^31"):
        assert words in doc, words


# ---- model level -------------------------------------------------------------------------------------------------------------------------
def test_the_model_level_call(monkeypatch):
    from ffvd_amd.dgp_model import DGPSSM
    from ffvd_amd import conditionals_multi_output as cmo
    sig = inspect.signature(DGPSSM.particle_records_seeded).parameters
    assert list(sig) == ["self", "Y_records", "control_records", "rule", "stage", "num_particles", "num_trajectories", "lengths", "x0", "S0",
                         "q_mode", "Y_train_std", "records_per_pass", "seed", "noise", "return_particles"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, "bootstrap", "filter", 256, 0, None, None, None, "reference", 1.0, 0, None, "shared",
                                                       False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    Y, ctrl = np.zeros((R, STEPS, 1)), np.zeros((R, STEPS, 1))
    for kw, msg in ((dict(noise="common"), "particle_records_seeded: noise"), (dict(rule="apf"), "particle_records_seeded: rule"),
                    (dict(stage="sample"), "particle_records_seeded: stage"), (dict(num_particles=1), "particle_records_seeded: num_particles"),
                    (dict(num_particles=True), "num_particles"), (dict(num_trajectories=3), "particle_records_seeded: num_trajectories"),
                    (dict(stage="backsim"), "particle_records_seeded: num_trajectories"), (dict(seed=-3), "particle_records_seeded: seed"),
                    (dict(seed=0.5), "particle_records_seeded: seed"), (dict(q_mode="slice0"), "particle_records_seeded: q_mode"),
                    (dict(x0=np.zeros(3)), "x0"), (dict(return_particles=None), "return_particles")):
        with pytest.raises(ValueError, match=msg):
            DGPSSM.particle_records_seeded(_Model(), Y, ctrl, **_with(dict(seed=1), **kw))
    with pytest.raises(ValueError, match="particle_records_seeded: Y_records"):
        DGPSSM.particle_records_seeded(_Model(), np.zeros((STEPS, 1)), ctrl, seed=1)
    with pytest.raises(ValueError, match="control_records"):
        DGPSSM.particle_records_seeded(_Model(), Y, seed=1)
    # independent draws beyond 1 GiB are NOT refused: nothing is generated on the host; the library's index limit is, with its count
    seen = {}
    for name in ("posterior_particle_records_seeded", "particle_records_seeded"):
        monkeypatch.setattr(pr, name, lambda *a, _n=name, **kw: seen.update({_n: (a, kw)}) or _n)
    monkeypatch.setattr(cmo, "kernel_pre_cal", lambda Z, kern: "Lm")
    big = np.zeros((60, 200, 1))
    assert 8 * 3 * 60 * (200 * 2048 * 2 + 200) > 2 ** 30
    assert DGPSSM.particle_records_seeded(_Model(), big, big, num_particles=2048, seed=1, noise="independent") == "posterior_particle_records_seeded"
    with pytest.raises(ValueError, match=r"G \* R \* steps \* N \* D = 2949120000 must stay below 2\^31"):
        DGPSSM.particle_records_seeded(_Model(), np.zeros((1200, 200, 1)), np.zeros((1200, 200, 1)), num_particles=2048, seed=1)
    m, e = _Model(), _Model(U_collapse=False)
    kw = dict(lengths=[4, 2, 4], records_per_pass=2, Y_train_std=1.7)
    assert DGPSSM.particle_records_seeded(m, Y, ctrl, num_particles=16, seed=5, **kw) == "posterior_particle_records_seeded"
    a, k = seen["posterior_particle_records_seeded"]
    assert len(a) == 10 and k == dict(lengths=[4, 2, 4], S0s=None, q_mode="reference", Y_train_std=1.7, records_per_pass=2, x0s=None, rule="bootstrap",
                                      stage="filter", num_particles=16, num_trajectories=0, seed=5, noise="shared", return_particles=False)
    assert DGPSSM.particle_records_seeded(e, Y, ctrl, rule="adapted", stage="backsim", num_trajectories=9, num_particles=16, seed=2 ** 64 - 1,
                                          noise="independent", S0=np.eye(2), x0=np.arange(2.0), return_particles=True) == "particle_records_seeded"
    a, k = seen["particle_records_seeded"]
    assert a[0] == "Lm" and len(a) == 12 and a[5].shape == (3, R, 2) and k["S0s"].shape == (3, R, 2, 2)
    assert (k["rule"], k["stage"], k["num_trajectories"], k["seed"], k["noise"], k["return_particles"]) == \
        ("adapted", "backsim", 9, 2 ** 64 - 1, "independent", True)
    # seed None: one 64-bit integer from the model's generator, so two models with the same generator state agree and a model moves on
    for mod in (m, e):
        mod._rng = np.random.default_rng(9)
    want = [int(x) for x in np.random.default_rng(9).integers(0, 2 ** 64, size=2, dtype=np.uint64)]
    got = []
    for _ in range(2):
        DGPSSM.particle_records_seeded(m, Y, ctrl, num_particles=16)
        got.append(seen["posterior_particle_records_seeded"][1]["seed"])
    assert got == want and got[0] != got[1] and all(isinstance(s, int) for s in got)
    doc = inspect.getdoc(DGPSSM.particle_records_seeded)
    for words in ("1 GiB refusal", "does not apply", "Philox4x32-10", "does NOT reproduce", "pinned"):
        assert words in doc, words


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
SEEDED_ARGS = ["int N", "unsigned long long seed", "int noise"]
NEW_TAIL = ["const int *lengths", "int B", "double *trajectories", "int *traj_index", "double *m_traj", "double *S_traj", "double *lag_cov",
            "double *weights", "double *trans_mean", "double *trans_var", "double *m_smooth", "double *S_smooth", "double *ess_smooth",
            "double *w_smooth"]


def test_the_symbols_are_declared_bound_and_exported():
    text = open(_declaration.__globals__["HEADER"]).read()
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    for new, old in zip(SYMBOLS, ("ffvd_particle_backsim_records_grouped", "ffvd_posterior_particle_backsim_records_grouped")):
        assert _lib._SIGNATURES[new][0] is ctypes.c_int and new in _lib.exported_symbols() and hasattr(_lib.load(), new)
        assert not new.startswith("ffvd_op_")
        assert text.index(old + "(") < text.index(new + "(") < text.index("ffvd_op_forecast_grouped(")
        d, c = _declaration(new), _declaration(old)
        sig, old_sig = _lib._SIGNATURES[new][1], _lib._SIGNATURES[old][1]
        assert len(sig) == len(d)
        assert d[:2] == ["int rule", "int stage"] and sig[:2] == [ctypes.c_int, ctypes.c_int]
        k = c.index("int N")
        assert d[2:2 + k] == c[:k] and sig[2:2 + k] == old_sig[:k]                          # the head of the backward simulation's list
        assert d[2 + k:5 + k] == SEEDED_ARGS and sig[2 + k:5 + k] == [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int]
        j, jn = c.index("double *m_pred"), d.index("double *m_pred")
        assert jn == 5 + k and j == k + 10                                                  # nine draw arguments gave way to two
        a = c.index("int *ancestors")
        assert d[jn:jn + a - j + 1] == c[j:a + 1] and sig[jn:jn + a - j + 1] == old_sig[j:a + 1]            # m_pred .. ancestors
        tail = d[jn + a - j + 1:]
        assert tail == NEW_TAIL + (["double *U_means"] if "posterior" in new else [])
        assert sig[jn + a - j + 1:] == [ip, ctypes.c_int, dp, ip] + [dp] * 10 + ([dp] if "posterior" in new else [])
        dropped = [x for x in c if x not in d]
        assert dropped == ["const double *eps", "long long eps_stride_g", "long long eps_stride_r", "const double *unif", "long long unif_stride_g",
                           "long long unif_stride_r", "const double *xi0", "long long xi0_stride_g", "long long xi0_stride_r",
                           "const double *unif_bs", "long long unif_bs_stride_g", "long long unif_bs_stride_r"]
    d = _declaration(DRAWS)
    assert d == ["unsigned long long seed", "int noise", "int G", "int R", "int steps", "int N", "int D", "int B", "double *eps", "double *unif",
                 "double *xi0", "double *unif_bs"]
    assert _lib._SIGNATURES[DRAWS] == (ctypes.c_int, [ctypes.c_ulonglong] + [ctypes.c_int] * 7 + [dp] * 4)
    assert DRAWS in _lib.exported_symbols() and hasattr(_lib.load(), DRAWS)
    for words in ("Philox4x32-10", "(p, g, r, stream)", "k1 = (w0 >> 5) 2^26 + (w1 >> 6)", "CONTRACT", "bit for bit", "prefix"):
        assert words in text, words


def _abi(fused, *, rule=0, stage=0, noise=0, G=2, R=2, M=4, D=2, C=1, T=5, steps=3, kind=0, J=1, n=4, B=3, lengths=None, null_all=False,
         seed=2 ** 64 - 1, want=None):
    """One call on zero inputs with every output buffer filled with 7; want: the names of the outputs handed over (None: those the
    (rule, stage) produces)"""
    P = D + C
    ng, nr, st, nn, nb = max(G, 1), max(R, 1), max(steps, 1), min(max(n, 1), 4096), min(max(B, 1), 5000)
    lib, dp = _lib.load(), _lib.dptr
    a = dict(Z=np.zeros((1, M, P)), lv=np.zeros((1, D)), ll=np.zeros((1, D, P)), X=np.zeros((ng, T + 1, D)), cf=np.zeros((T, C)),
             cr=np.zeros((nr, st, C)), lq=np.zeros((ng, D)), f=np.zeros((ng, M, D)), xl=np.zeros((ng, nr, D)), CC=np.ones((D, J)),
             DD=np.zeros(J), sd=np.ones(J), Y=np.zeros((nr, st, J)))
    vec, mat, row = (ng, nr, st, D), (ng, nr, st, D, D), (ng, nr, st)
    shapes = dict(mp=vec, Sp=mat, mf=vec, Sf=mat, lpd=row + (J,), lj=row, ym=(nr, st, J), yt=(nr, st, J), lm=(nr, st, J), lg=(nr, st, J),
                  ess=row, le=(ng, nr), par=row + (nn, D))
    new = dict(traj=(ng, nr, nb, st, D), mt=vec, St=mat, lc=mat, w=row + (nn,), tm=row + (nn, D), tv=row + (nn, D), ms=vec, Ss=mat, es=row,
               ws=row + (nn,))
    if want is None:
        want = {0: set(), 1: {"w", "tm", "tv", "ms", "Ss", "es", "ws"}, 2: {"traj", "idx", "mt", "St", "lc", "w", "tm", "tv"}}.get(stage, set())
        want = want - ({"w"} if rule == 1 else set())
    outs = {k: np.full(s, 7.0) for k, s in list(shapes.items()) + list(new.items()) + [("U", (ng, M, D))]}
    anc, idx = np.full(row + (nn,), 7, dtype=np.int32), np.full(row + (nb,), 7, dtype=np.int32)
    p = {k: dp(v) for k, v in list(a.items()) + list(outs.items())}
    ip = ctypes.POINTER(ctypes.c_int)
    lens = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    give = lambda k: p[k] if k in want and not null_all else None
    tail = (p["CC"], p["DD"], p["sd"], J, p["Y"], 0, n, seed, noise) + tuple(None if null_all else p[k] for k in shapes) + \
        (None if null_all else anc.ctypes.data_as(ip), None if lens is None else lens.ctypes.data_as(ip), B, give("traj"),
         idx.ctypes.data_as(ip) if "idx" in want and not null_all else None) + \
        tuple(give(k) for k in ("mt", "St", "lc", "w", "tm", "tv", "ms", "Ss", "es", "ws"))
    name = SYMBOLS[fused]
    if fused:
        rc = getattr(lib, name)(rule, stage, kind, G, 1, p["Z"], M, P, D, p["lv"], p["ll"], p["X"], p["cf"], C, T, p["lq"], 1e-5, 0, 0, R, None, None,
                                p["cr"], steps, *tail, p["U"])
    else:
        Wm = [np.eye(M) for _ in range(D)]
        Wt = (ctypes.c_void_p * len(Wm))(*[w.ctypes.data for w in Wm])
        rc = getattr(lib, name)(rule, stage, kind, G, 1, Wt, p["Z"], M, P, D, p["lv"], p["ll"], p["f"], None, 0, R, p["xl"], None, p["cr"], C, steps,
                                p["lq"], *tail)
    outs.update(anc=anc, idx=idx)
    return rc, outs, name


ABI_BAD = [dict(rule=2), dict(rule=-1), dict(stage=3), dict(stage=-1), dict(noise=3), dict(noise=-1), dict(kind=1), dict(D=9, C=0), dict(M=2049),
           dict(J=9), dict(n=1), dict(n=2049), dict(G=-1), dict(R=-1), dict(null_all=True), dict(stage=1, lengths=[3, 0]),
           dict(stage=2, lengths=[4, 3]), dict(stage=2, B=0), dict(stage=2, B=4097), dict(stage=2, rule=1, B=-1)]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("ov", ABI_BAD, ids=str)
def test_abi_rejects_bad_arguments_without_a_device(ov, fused):
    rc, outs, name = _abi(fused, **ov)
    assert rc == E, rc
    assert name.encode() + b": bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


NOT_PRODUCED = [(0, 0, ("w",), b"weights"), (0, 0, ("tm", "tv"), b"trans_mean, trans_var"), (0, 0, ("ms",), b"m_smooth"),
                (0, 0, ("traj", "idx"), b"trajectories, traj_index"), (0, 1, ("mt", "St", "lc"), b"m_traj, S_traj, lag_cov"),
                (1, 1, ("w", "ms"), b"weights"), (1, 2, ("w",), b"weights"),
                (0, 2, ("ms", "Ss", "es", "ws"), b"m_smooth, S_smooth, ess_smooth, w_smooth"), (1, 0, ("w", "ws"), b"weights, w_smooth")]


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("rule,stage,want,names", NOT_PRODUCED, ids=str)
def test_an_output_the_rule_and_stage_do_not_produce_must_be_null(rule, stage, want, names, fused):
    rc, outs, name = _abi(fused, rule=rule, stage=stage, want=set(want))
    msg = _lib.load().ffvd_last_error(None)
    assert rc == E and name.encode() + b": bad argument" in msg and b"does not produce " + names + b":" in msg, msg
    assert f"rule {rule}, stage {stage}".encode() in msg
    assert all(np.all(v == 7) for v in outs.values())


def test_lengths_at_the_filter_stage_are_named_too():
    for fused in (False, True):
        rc, _, _ = _abi(fused, lengths=[3, 3])
        assert rc == E and b"does not produce lengths" in _lib.load().ffvd_last_error(None)


def test_the_messages_say_why():
    lib = _lib.load()
    for fused in (False, True):
        rc, _, _ = _abi(fused, rule=2)
        assert rc == E and b"rule 0 or 1, stage 0, 1 or 2 and noise 0, 1 or 2" in lib.ffvd_last_error(None)
        rc, _, _ = _abi(fused, stage=1, lengths=[3, 0])
        assert rc == E and b"lengths must lie in [1, steps]" in lib.ffvd_last_error(None)
        rc, _, _ = _abi(fused, n=2049)
        assert rc == E and b"2 <= N <= 2048" in lib.ffvd_last_error(None)
        rc, _, _ = _abi(fused, stage=2, B=0)
        assert rc == E and b"1 <= B <= 4096" in lib.ffvd_last_error(None)
        for rule, words in ((0, b"the particle filter of many records"), (1, b"adapted particle filter of many records")):
            rc, _, _ = _abi(fused, rule=rule, kind=1)
            msg = lib.ffvd_last_error(None)
            assert rc == E and words in msg and b"SE kernel only" in msg


@pytest.mark.parametrize("fused", [False, True], ids=["explicit", "fused"])
@pytest.mark.parametrize("rule,stage", [(r, s) for r in (0, 1) for s in (0, 1, 2)], ids=str)
@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0)], ids=str)
def test_abi_returns_ok_and_touches_nothing_without_groups_records_or_rows(rule, stage, ov, fused):
    rc, outs, _ = _abi(fused, rule=rule, stage=stage, noise=2, **ov)
    assert rc == _lib.FFVD_OK
    assert all(np.all(v == 7) for v in outs.values())
    if stage == 2:
        assert _abi(fused, rule=rule, stage=stage, B=0, **ov)[0] == E      # B is checked even then


def _draws_abi(**ov):
    a = dict(seed=7, noise=2, G=2, R=2, steps=3, N=4, D=2, B=3, null=())
    a.update(ov)
    ng, nr, st, nn, nb = (min(max(a[k], 1), 8) for k in ("G", "R", "steps", "N", "B"))          # (the rejected sizes get small buffers)
    outs = dict(eps=np.full((ng, nr, st, nn, max(min(a["D"], 8), 1)), 7.0), unif=np.full((ng, nr, st), 7.0), xi0=np.full((ng, nr, nn, 8), 7.0),
                unif_bs=np.full((ng, nr, st, nb), 7.0))
    ptr = [None if k in a["null"] else _lib.dptr(outs[k]) for k in ("eps", "unif", "xi0", "unif_bs")]
    rc = _lib.load().ffvd_particle_draws(a["seed"], a["noise"], a["G"], a["R"], a["steps"], a["N"], a["D"], a["B"], *ptr)
    return rc, outs


@pytest.mark.parametrize("ov", [dict(noise=3), dict(noise=-1), dict(G=-1), dict(R=-1), dict(steps=-1), dict(N=1), dict(N=2049), dict(D=0), dict(D=9),
                                dict(B=-1), dict(B=4097), dict(B=0), dict(G=1024, R=1024, steps=64, N=32, null=("eps", "unif", "xi0", "unif_bs")),
                                dict(G=32768, R=32768, steps=1, N=2, D=1, B=2, null=("eps", "unif", "xi0", "unif_bs"))], ids=str)
def test_the_draws_call_rejects_bad_arguments_without_a_device(ov):
    rc, outs = _draws_abi(**ov)
    assert rc == E and b"ffvd_particle_draws: bad argument" in _lib.load().ffvd_last_error(None)
    assert all(np.all(v == 7) for v in outs.values())


@pytest.mark.parametrize("ov", [dict(G=0), dict(R=0), dict(steps=0), dict(steps=0, B=0, null=("unif_bs",))], ids=str)
def test_the_draws_call_returns_ok_and_touches_nothing_at_a_zero_size(ov):
    rc, outs = _draws_abi(**ov)
    assert rc == _lib.FFVD_OK and all(np.all(v == 7) for v in outs.values())
