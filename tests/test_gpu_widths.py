"""Every latent dimension, output count and input width the filtering family is compiled for, on the device.

The shapes shared by the other files have D in {1, 2, 3, 4, 8}, J in {1, 3} and P = D + C <= 9.  MG_DISPATCH_D instantiates every
kernel of the family for D = 1 .. 8, the kernels stage up to MG_MAXJ = 8 outputs and MAXP = 32 input columns, and
`ps_partial_kernel<J>` exists for J = 1 .. 8.  The fixtures of tests/width_fixtures.py run what the shared shapes leave out: D = 5, 6
and 7 (d5, d6, d7), J = 8 everywhere, P = 8 exactly (d6: the upper edge of the 8-column conditional-gradient kernel), P = 32 with
D = 8 and with D = 3 (p32, p32d3), and the shared-Gamma unit layout at D = 7 and at P = 32 (d7_shared, p32_shared).  Every
(d, p) has a lengthscale of its own there, so a wrong column index shows (tests/test_width_fixtures.py measures by how much, and
checks the margin conditions the identical indices below rest on, without a GPU).

One device call per (fixture, entry point), cached; at most 12 rows, N = 48, M = 40.  Each entry point is compared with the
reference its own file pins it to, by the project's rule: error <= max(4 e_ref, floor) per array with `rule` of
tests/test_gpu_moment_grouped.py and `judge` of tests/test_gpu_filter_records.py (floors 1e-11 + 1e-9 max|ref| on means,
1e-11 + 1e-8 max|ref| on covariances and densities; e_ref is the fp64 reference against np.longdouble, never the device); NaN exactly
where the reference has it; covariances exactly symmetric; ancestors and trajectory indices identical; pooled arrays and scalars against
NumPy on the device's own stacks at 1e-9 (1 + max|ref|).  No tolerance is new.  Every measured error is printed; DESIGN.md section 9,
"Widths", has the largest per entry point.  The single-record entry points take record 0 of the fixture."""
import functools

import numpy as np
import pytest

import forecast_cubature_ref as fcr
import forecast_linear_ref as flr
import forecast_particle_ref as fpr
import particle_backsim_ref as pb
import particle_smoother_ref as psr
import records_ref as rr
import width_fixtures as wf
from ffvd_amd import prediction as pr
from ffvd_amd import conditionals_multi_output as cmo
from particle_fixtures import subset
from test_gpu_conditional_grad_grouped import _reference as grad_reference, check as grad_check
from test_gpu_conditional_grouped import make_xnew
from test_gpu_filter_grouped import COVS, MOMENTS, POOLED, key_of, numpy_densities
from test_gpu_filter_particle import JUDGED
from test_gpu_filter_records import SCALARS, TRACK, judge, live_rows
from test_gpu_forecast_particle import KIND, TRACKS
from test_gpu_moment_grouped import WIDE, _check_summary, rule
from test_gpu_rollout_summary import PS_CHUNK, check as rollout_check
from test_gpu_smooth_particle import judge as judge_smoothed

pytestmark = pytest.mark.gpu

NAMES = wf.NAMES
N, J, R, STEPS, H = wf.N, wf.J, wf.R, wf.STEPS, wf.H
ORIGINS = list(range(STEPS - H))
RECORDS = dict(linearised=pr.filter_records_grouped, cubature=pr.filter_cubature_records_grouped)
PARTICLE = dict(bootstrap=pr.filter_particle_records_grouped, adapted=pr.filter_adapted_records_grouped,
                smoother=pr.smooth_particle_records_grouped)
FANS = dict(moment=pr.forecast_grouped, linearised=pr.forecast_linear_grouped, cubature=pr.forecast_cubature_grouped)


def posterior(fx):
    """the leading arguments of every entry point: the oracle's posterior of the fixture's groups under their one model"""
    gs = fx["gs"]
    return gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], fx["qs"]


def record0(fx):
    """what a single-record entry point takes after the posterior, up to log_Rchols"""
    return (list(fx["x0"][:, 0]), None if fx["ctrl"] is None else fx["ctrl"][0], 0, fx["Y"][0], [g["Q"] for g in fx["gs"]]) + tuple(fx["em"])


def records(fx):
    """what a records entry point takes after the posterior, up to log_Rchols"""
    return (fx["x0"], fx["ctrl"], fx["Y"], [g["Q"] for g in fx["gs"]]) + tuple(fx["em"])


def _kw(fx):
    return dict(lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"])


def call_records(fx, kind):
    return RECORDS[kind](*posterior(fx), *records(fx), smooth=True, **_kw(fx))


def call_particle(fx, kind):
    return PARTICLE[kind](*posterior(fx), *records(fx), fx["eps"], fx["unif"], xi0=fx["xi0"], return_particles=True, **_kw(fx))


def call_backsim(fx):
    return pr.backsim_particle_records_grouped(*posterior(fx), *records(fx), fx["eps"], fx["unif"], fx["unif_bs"], xi0=fx["xi0"],
                                               return_particles=True, **_kw(fx))


@functools.lru_cache(maxsize=None)
def device(name, entry, kind=None):
    """One device call per (fixture, entry point), shared by the checks below (never modified)."""
    fx = wf.fixture(name)
    one = dict(S0s=fx["S0"][:, 0], q_mode=fx["mode"])
    if entry == "moment":
        return pr.moment_grouped(*posterior(fx), list(fx["x0"][:, 0]), None if fx["ctrl"] is None else fx["ctrl"][0], 0, STEPS,
                                 [g["Q"] for g in fx["gs"]], **one)
    if entry == "filter":
        return pr.filter_grouped(*posterior(fx), *record0(fx), smooth=True, method=kind, **one)
    if entry == "fan":
        return FANS[kind](*posterior(fx), *record0(fx), H, return_tracks=True, return_filter=True, **one)
    if entry == "particle_fan":
        return pr.forecast_particle_grouped(*posterior(fx), *record0(fx), H, fx["eps"][:, 0], fx["unif"][:, 0], fx["eps_fc"], xi0=fx["xi0"][:, 0],
                                            return_tracks=True, return_filter=True, return_particles=True, **one)
    if entry == "records":
        return call_records(fx, kind)
    if entry == "particle":
        return call_particle(fx, kind)
    assert entry == "backsim"
    return call_backsim(fx)


def symmetric(out, keys):
    for k in keys:
        np.testing.assert_array_equal(out[k], np.swapaxes(out[k], -1, -2), err_msg=k)      # (NaN rows compare equal to themselves here)


def against_numpy(what, k, got, want, nan_at=None):
    """the rule of the pooled arrays and scalars: NumPy on the device's own stacks at 1e-9 (1 + max|ref|)"""
    got, want = np.asarray(got), np.asarray(want)
    nan_at = np.zeros(want.shape, dtype=bool) if nan_at is None else nan_at
    assert got.shape == want.shape, k
    np.testing.assert_array_equal(np.isnan(got), nan_at, err_msg=k)
    ok = ~nan_at
    tol, err = 1e-9 * (1.0 + float(np.max(np.abs(want[ok])))), float(np.max(np.abs(got[ok] - want[ok])))
    print(f"{what}: {k}: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, k


def pooled_and_scalars(what, out, fx, mixture_of_lpd=False):
    """the pooled arrays and the scalars of a records call (tests/test_gpu_filter_records.py, tests/test_gpu_filter_particle.py)"""
    (CC, DD, _), Y = fx["em"], fx["Y"]
    want = rr.pooled(out["m_pred"], out["S_pred"], CC, DD, fx["sd"], Y)
    if mixture_of_lpd:                                             # a particle filter pools its own per-track densities
        with np.errstate(invalid="ignore"):
            mx = np.max(out["lpd"], axis=0)
            want["lpd_mix"] = mx + np.log(np.mean(np.exp(out["lpd"] - mx[None]), axis=0))
    dead = np.broadcast_to(~live_rows(fx["lengths"], STEPS)[:, :, None], Y.shape)
    nan_at = dict(predict_y=dead, predict_y_var_total=dead, lpd_mix=np.isnan(Y), lpd_gauss=np.isnan(Y))
    for k in POOLED:
        against_numpy(what, k, out[k], want[k], nan_at[k])
    ws = rr.scalars(Y, out["lpd_mix"], out["lpd_joint"], out["predict_y"])
    for k in SCALARS + ("ll_all",):
        assert np.all(np.isfinite(out[k])), k
        against_numpy(what, k, out[k], ws[k])


def pooled_fan(what, out, fx, mixture_of_lpd=False):
    """the pooled arrays of a forecast fan (tests/test_gpu_forecast_grouped.py, tests/test_gpu_forecast_particle.py)"""
    (CC, DD, _) = fx["em"]
    Yt = fx["Y"][0][np.asarray(ORIGINS)[:, None] + 1 + np.arange(H)[None, :]]                # (B, h, J)
    want = rr.pooled(out["m_fc"], out["S_fc"], CC, DD, fx["sd"], Yt)
    if mixture_of_lpd:
        with np.errstate(invalid="ignore"):
            mx = np.max(out["lpd_fc"], axis=0)
            want["lpd_mix"] = mx + np.log(np.mean(np.exp(out["lpd_fc"] - mx[None]), axis=0))
    for k in POOLED:
        against_numpy(what, k, out[k], want[k], np.isnan(Yt) if k.startswith("lpd") else None)
    np.testing.assert_array_equal(out["n_h"], (~np.isnan(Yt)).sum(axis=0))


# ---- the propagation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_moment_grouped(name):
    (m_x, S_x), r = device(name, "moment"), wf.propagation_reference(name)
    assert m_x.shape == r["m"].shape and S_x.shape == r["S"].shape
    rule(f"{name} moment_grouped", "mean", m_x, r["m"], r["e_m"])
    rule(f"{name} moment_grouped", "var", S_x, r["S"], r["e_S"])
    symmetric(dict(S=S_x), ["S"])


# ---- the single-record filters and smoothers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["moment", "linearised"])
@pytest.mark.parametrize("name", NAMES)
def test_filter_grouped(name, method):
    fx, out = wf.fixture(name), device(name, "filter", method)
    ref, e_ref = wf.moment_filter_reference(name) if method == "moment" else wf.linear_filter_reference(name)
    what = f"{name} filter_grouped {method}"
    for k in MOMENTS:
        assert out[k].shape == ref[k].shape, k
        rule(f"{what}: {k}", key_of(k), out[k], ref[k], e_ref[k])
    symmetric(out, COVS)
    np.testing.assert_array_equal(out["m_smooth"][:, -1], out["m_filt"][:, -1])
    np.testing.assert_array_equal(out["S_smooth"][:, -1], out["S_filt"][:, -1])
    # every column of lpd, lpd_joint and the pooled arrays against NumPy on the device's own predicted stacks
    (CC, DD, _), Y = fx["em"], fx["Y"][0]
    seen = ~np.isnan(Y)
    G = len(fx["gs"])
    nan_at = dict(lpd=np.broadcast_to(~seen, (G,) + seen.shape), lpd_joint=np.broadcast_to(~seen.any(axis=1), (G, STEPS)), lpd_mix=~seen,
                  lpd_gauss=~seen)
    for k, w in numpy_densities(out, Y, CC, DD, fx["sd"]).items():
        against_numpy(what, k, out[k], w, nan_at.get(k))
    if method == "linearised":                                     # the records reference has the densities of this rule: record 0
        rref, re = wf.records_reference(name)
        for k in ("lpd", "lpd_joint"):
            w = rref[k][:, 0]
            np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(w), err_msg=k)
            ok = ~np.isnan(w)
            rule(f"{what}: {k}", "var", out[k][ok], w[ok], re[k])


# ---- the Gaussian forecast fans ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(FANS))
@pytest.mark.parametrize("name", NAMES)
def test_forecast_fans(name, kind):
    """horizon 3 from every origin.  The moment fan: every track bit-identical to moment_grouped from the filtered state the call's own
    filter stored, as tests/test_gpu_forecast_grouped.py states it; the linearised and the cubature fan: their references."""
    fx, out = wf.fixture(name), device(name, "fan", kind)
    G, D = len(fx["gs"]), fx["x0"].shape[-1]
    what = f"{name} {kind} fan"
    assert out["origins"].tolist() == ORIGINS and out["m_fc"].shape == (G, len(ORIGINS), H, D) and out["S_fc"].shape == (G, len(ORIGINS), H, D, D)
    symmetric(out, ["S_fc", "S_pred", "S_filt"])
    if kind == "moment":
        flt = device(name, "filter", "moment")
        for k in ("m_pred", "S_pred", "m_filt", "S_filt", "cross", "lpd", "lpd_joint"):
            np.testing.assert_array_equal(out[k], flt[k], err_msg=k)
        for b, o in enumerate(ORIGINS):
            m_x, S_x = pr.moment_grouped(*posterior(fx), list(out["m_filt"][:, o]), None if fx["ctrl"] is None else fx["ctrl"][0], o + 1, H,
                                         [g["Q"] for g in fx["gs"]], S0s=out["S_filt"][:, o], q_mode=fx["mode"])
            np.testing.assert_array_equal(out["m_fc"][:, b], m_x, err_msg=f"m_fc, origin {o}")
            np.testing.assert_array_equal(out["S_fc"][:, b], S_x, err_msg=f"S_fc, origin {o}")
    else:
        CC, DD, _ = fx["em"]
        ref, e_ref = (flr if kind == "linearised" else fcr).reference(fx["gs"], None if fx["ctrl"] is None else fx["ctrl"][0], fx["Y"][0], CC, DD, fx["sd"],
                                                                      fx["qs"], fx["S0"][:, 0], fx["mode"], ORIGINS, H, WIDE)
        assert out["m_fc"].shape == ref["m"].shape and out["S_fc"].shape == ref["S"].shape
        rule(f"{what}: m_fc", "mean", out["m_fc"], ref["m"], e_ref["m"])
        rule(f"{what}: S_fc", "var", out["S_fc"], ref["S"], e_ref["S"])
    assert float(np.min(np.linalg.eigvalsh(out["S_fc"]))) > 0.0
    pooled_fan(what, out, fx)


# ---- the particle forecast fan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forecast_particle_grouped(name):
    fx, out = wf.fixture(name), device(name, "particle_fan")
    CC, DD, _ = fx["em"]
    ref, e_ref = fpr.reference(fx["gs"], None if fx["ctrl"] is None else fx["ctrl"][0], fx["Y"][0], CC, DD, fx["sd"], fx["qs"], fx["x0"][:, 0],
                               fx["S0"][:, 0], fx["mode"], np.asarray(ORIGINS), H, WIDE, fx["eps"][:, 0], fx["unif"][:, 0], fx["eps_fc"], fx["xi0"][:, 0])
    what = f"{name} particle fan"
    for k in TRACKS:
        assert out[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        rule(f"{what}: {k}", KIND[k], out[k][ok], ref[k][ok], e_ref[k])
    symmetric(out, ["S_fc"])
    Yt = fx["Y"][0][np.asarray(ORIGINS)[:, None] + 1 + np.arange(H)[None, :]]
    np.testing.assert_array_equal(np.isnan(out["lpd_fc"]), np.broadcast_to(np.isnan(Yt)[None], out["lpd_fc"].shape))
    pooled_fan(what, out, fx, mixture_of_lpd=True)


# ---- the Gaussian records filters --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(RECORDS))
@pytest.mark.parametrize("name", NAMES)
def test_records_filters(name, kind):
    fx, out = wf.fixture(name), device(name, "records", kind)
    ref, e_ref = wf.records_reference(name) if kind == "linearised" else wf.cubature_reference(name)
    what = f"{name} {kind} records"
    G, D = len(fx["gs"]), fx["x0"].shape[-1]
    assert out["m_pred"].shape == (G, R, STEPS, D) and out["lpd"].shape == (G, R, STEPS, J)
    judge(what, out, ref, e_ref, keys=TRACK)
    symmetric(out, COVS)
    for r, n in enumerate(fx["lengths"]):                          # the last row of the smoother is the filtered one
        np.testing.assert_array_equal(out["m_smooth"][:, r, n - 1], out["m_filt"][:, r, n - 1])
        np.testing.assert_array_equal(out["S_smooth"][:, r, n - 1], out["S_filt"][:, r, n - 1])
    assert float(np.min(np.linalg.eigvalsh(out["S_filt"][:, live_rows(fx["lengths"], STEPS)]))) > 0.0
    pooled_and_scalars(what, out, fx)


# ---- the particle filters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bootstrap", "adapted"])
@pytest.mark.parametrize("name", NAMES)
def test_particle_filters(name, kind):
    """identical ancestors (the margin condition: tests/test_width_fixtures.py); particles, moments and all eight columns of lpd by the
    rule; ess / N by the variance floor"""
    fx, out = wf.fixture(name), device(name, "particle", kind)
    ref, e_ref, wide = wf.bootstrap_reference(name) if kind == "bootstrap" else wf.adapted_reference(name)
    what = f"{name} {kind} particle filter"
    e_le = float(np.max(np.abs(ref["log_evidence"] - wide["log_evidence"]))) if WIDE else 0.0
    rule(f"{what}: log_evidence", "var", out["log_evidence"], ref["log_evidence"], e_le)     # (a sum of lpd_joint: its floor)
    assert out["ancestors"].dtype == np.int32
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judge(what, out, ref, e_ref, keys=JUDGED)
    np.testing.assert_array_equal(np.isnan(out["ess"]), np.isnan(ref["ess"]))
    ok = ~np.isnan(ref["ess"])
    rule(f"{what}: ess / N", "var", out["ess"][ok] / N, ref["ess"][ok] / N, e_ref["ess"] / N)
    symmetric(out, ["S_pred", "S_filt"])
    against_numpy(what, "log_evidence", out["log_evidence"], np.nansum(out["lpd_joint"], axis=2))
    live = live_rows(fx["lengths"], STEPS)
    assert np.all(out["ancestors"][:, ~live] == -1) and np.all(np.isnan(out["particles"][:, ~live]))
    pooled_and_scalars(what, out, fx, mixture_of_lpd=True)


@pytest.mark.parametrize("name", NAMES)
def test_smooth_particle_records_grouped(name):
    """end to end against tests/particle_smoother_ref.py on the oracle's posterior, and its recursion on the device's own stacks"""
    fx, out = wf.fixture(name), device(name, "particle", "smoother")
    CC, DD, _ = fx["em"]
    ref, e_ref = psr.reference(fx["gs"], fx["ctrl"], fx["Y"], CC, DD, fx["sd"], fx["qs"], fx["x0"], fx["S0"], fx["mode"], fx["lengths"], WIDE,
                               fx["eps"], fx["unif"], fx["xi0"])
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    judge_smoothed(f"{name} smoother end to end", out, ref, e_ref, psr.SMOOTHED + psr.KEPT)
    own = psr.on_stacks(out, fx["lengths"])
    wide = psr.on_stacks(out, fx["lengths"], dtype=np.longdouble) if WIDE else own
    e_own = {k: float(np.nanmax(np.abs(own[k] - wide[k]))) / (N if k == "ess_smooth" else 1) for k in psr.SMOOTHED}
    judge_smoothed(f"{name} smoother on its own stacks", out, own, e_own, psr.SMOOTHED)
    symmetric(out, ["S_smooth"])
    flt = device(name, "particle", "bootstrap")
    for k in flt:                                                  # the filter of the call is the filter, bit for bit
        np.testing.assert_array_equal(out[k], flt[k], err_msg=k)


@pytest.mark.parametrize("name", NAMES)
def test_backsim_particle_records_grouped(name):
    """B = 5 trajectories: indices identical to the reference end to end and on the device's own stacks, the gather bit for bit, the
    trajectory moments by the rule (tests/test_gpu_backsim_particle.py)"""
    fx, out = wf.fixture(name), device(name, "backsim")
    ref = wf.backsim_reference(name)[0]
    G, D, B = len(fx["gs"]), fx["x0"].shape[-1], wf.B
    assert out["traj_index"].dtype == np.int32 and out["trajectories"].shape == (G, R, B, STEPS, D)
    np.testing.assert_array_equal(out["ancestors"], ref["ancestors"])
    np.testing.assert_array_equal(out["traj_index"], ref["traj_index"])
    own = pb.on_stacks(out, fx["lengths"], fx["unif_bs"])
    print(f"{name}: backward gap on the device's own stacks {own['gap_bs']:.3e}")
    np.testing.assert_array_equal(out["traj_index"], own["traj_index"])
    for g in range(G):
        for r, ln in enumerate(fx["lengths"]):
            ln = int(ln)
            traj = out["trajectories"][g, r]
            assert np.all(np.isnan(traj[:, ln:]))
            for t in range(ln):
                np.testing.assert_array_equal(traj[:, t], out["particles"][g, r, t][out["traj_index"][g, r, t]], err_msg=f"{(g, r, t)}")
            m, Sm, lag = pb.moments(traj[:, :ln])
            wide = pb.moments(traj[:, :ln], np.longdouble) if WIDE else (m, Sm, lag)
            for k, key, w64, w in (("m_traj", "mean", m, wide[0]), ("S_traj", "var", Sm, wide[1]), ("lag_cov", "var", lag, wide[2])):
                dev, rows = out[k][g, r], ln - 1 if k == "lag_cov" else ln
                assert np.all(np.isnan(dev[rows:])), k
                rule(f"{name} backsim track {(g, r)}: {k}", key, dev[:rows], w64[:rows], float(np.max(np.abs(w64[:rows] - w[:rows]))))
    for k in pb.MOMENTS:                                           # and end to end against the reference's own trajectories
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        rule(f"{name} backsim end to end: {k}", key_of(k), out[k][ok], ref[k][ok], wf.backsim_reference(name)[1][k])
    symmetric(out, ["S_traj"])


# ---- the linearised transition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reference", "intent"])
@pytest.mark.parametrize("name", [n for n in NAMES if not n.endswith("_shared")])
def test_conditional_grad_grouped(name, mode):
    """37 rows of tests/test_gpu_conditional_grouped.make_xnew.  d6 has P = 8: the last column of the 8-wide mean kernel; P = 32
    fills the 32-wide one."""
    fx, (_, c, meta) = wf.fixture(name), wf.model(name)
    gs = fx["gs"]
    Xnew = make_xnew(gs[0]["X"], c, meta["T"], 37)
    qs = [g["orc"]["H"] for g in gs]
    r = dict(f64=grad_reference(gs, Xnew, mode, qs, np.float64), ld=grad_reference(gs, Xnew, mode, qs, np.longdouble))
    out = cmo.conditional_grad_grouped(gs[0]["orc"]["L"], gs[0]["Z"], gs[0]["kern"], [g["orc"]["U"] for g in gs], qs, Xnew, q_mode=mode)
    assert out["dmean"].shape == (len(gs), 37, meta["D"], meta["P"])
    grad_check(f"{name} conditional_grad_grouped {mode}", r, out)


# ---- the summaries: every J the partial kernel is compiled for ---------------------------------------------------------------------------
def _emission(rng, D, j):
    return rng.standard_normal((D, j)), rng.standard_normal(j), np.log(0.2 + 0.3 * rng.random((j, j)))


@pytest.mark.parametrize("j", range(1, 9))
def test_rollout_summary(j):
    """two chunks plus 3 rollouts, 7 steps; at J = 8 also the widest state the operator takes, D = 32"""
    n, steps = 2 * PS_CHUNK + 3, 7
    for D in (5, 32) if j == 8 else (5,):
        rng = np.random.default_rng(100 * j + D)
        px, pv = 2.0 + rng.standard_normal((n, steps, D)), 0.05 + 0.1 * rng.random((n, steps, D))
        CC, DD, lr = _emission(rng, D, j)
        Y = 2.0 * rng.standard_normal((steps, j))
        rollout_check(f"rollout_summary J={j} D={D}", pr.rollout_summary(px, pv, CC, DD, lr, Y, 1.7), px, pv, CC, DD, lr, Y)


@pytest.mark.parametrize("j", range(1, 9))
def test_moment_summary(j):
    """on the reference's own propagated states of p32 (two groups, D = 8), the first j outputs"""
    r, rng = wf.propagation_reference("p32"), np.random.default_rng(40 + j)
    CC, DD, lr = _emission(rng, 8, j)
    Y = (np.einsum("gtk,kj->gtj", r["m"], CC) + DD).mean(axis=0)[:5] + 0.3 * rng.standard_normal((5, j))
    _check_summary(f"moment_summary J={j}", pr.moment_summary(r["m"], r["S"], CC, DD, lr, Y, 1.7), r["m"], r["S"], CC, DD, lr, Y)


# ---- independence at the limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,kind", [("records", "linearised"), ("records", "cubature"), ("particle", "bootstrap"), ("particle", "adapted")])
def test_at_p32_a_group_alone_and_a_record_alone_reproduce_their_slices_bit_for_bit(entry, kind):
    fx, a = wf.fixture("p32"), device("p32", entry, kind)
    fn = call_records if entry == "records" else call_particle
    keys = TRACK if entry == "records" else JUDGED + ("ess", "log_evidence", "ancestors")
    one = fn(subset(fx, groups=[1]), kind)
    for k in keys:
        np.testing.assert_array_equal(one[k][0], a[k][1], err_msg=f"{k}, group 1")
    one = fn(subset(fx, recs=[1]), kind)
    for k in keys:
        np.testing.assert_array_equal(one[k][:, 0], a[k][:, 1], err_msg=f"{k}, record 1")
    for k in POOLED + SCALARS:
        np.testing.assert_array_equal(one[k][0], a[k][1], err_msg=f"{k}, record 1")
