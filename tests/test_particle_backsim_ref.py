"""tests/particle_backsim_ref.py pinned without a GPU: against the exact RTS smoother of the scalar linear-Gaussian model of
tests/test_particle_smoother_ref.py (12 rows, row 4 missing), against the marginal smoother's weights, and the exact properties the
device tests rely on.

The bounds are statistical, with this project's constant 6 and the margins DESIGN.md section 9, "Particle backward simulation"
records.  At N = 1024, B = 256 over 8 seeds, with ess = ess_smooth of the marginal smoother on the same stacks:
  |m_traj - m_RTS| <= 6 sqrt(P_s (1 / B + 1 / ess))
  |S_traj / P_s - 1| <= 6 sqrt(2 / B) + 6 sqrt(2 / min ess)
  |lag_cov - C_t| / sqrt(P_s,t P_s,t+1) <= 6 sqrt((1 + rho_t^2) (1 / B + 1 / min ess)),  C_t = G_t P_s,t+1, G_t = P_f,t A / P_p,t+1."""
import functools

import numpy as np

import particle_backsim_ref as pb
import particle_filter_ref as pf
import particle_smoother_ref as ps
from test_particle_smoother_ref import A, CC, DD, MISSING, Q, ROWS, SD, X0, linear_cond, record, rts

N, B, SEEDS = 1024, 256, 8


def sampled(seed, Y, n=N, b=B, cond=linear_cond, q=Q, keep_cdf=False, dtype=np.float64, unif_bs=None):
    rng = np.random.default_rng(seed)
    eps, unif = rng.standard_normal((Y.shape[0], n, 1)), rng.random(Y.shape[0])
    ub = rng.random((Y.shape[0], b)) if unif_bs is None else unif_bs
    f = pb.run(cond, np.array([X0]), None, Y, CC, DD, SD, np.array([q]), eps, unif, ub, dtype=dtype, keep_cdf=keep_cdf)
    f["unif_bs"] = ub
    return f


@functools.lru_cache(maxsize=None)
def runs():
    """the 8 seeds, computed once and never modified"""
    Y = record()
    return Y, [sampled(300 + s, Y) for s in range(SEEDS)]


def test_against_the_kalman_smoother():
    Y, outs = runs()
    mf, Pf, ms, Ps = rts(Y)
    Pp = A * A * Pf[:-1] + Q                                     # P_p of rows 1 ..
    C = Pf[:-1] * A / Pp * Ps[1:]                                 # the exact lag-one smoothed covariance
    rho = C / np.sqrt(Ps[:-1] * Ps[1:])
    worst_m, worst_v, worst_l, bound_v, bound_l = 0.0, 0.0, 0.0, np.inf, np.inf
    for f in outs:
        ess, least = f["ess_smooth"], float(np.min(f["ess_smooth"]))
        err = np.abs(f["m_traj"][:, 0] - ms)
        lim = 6.0 * np.sqrt(Ps * (1.0 / B + 1.0 / ess))
        worst_m = max(worst_m, float(np.max(err / np.sqrt(Ps / B))))
        assert np.all(err <= lim), (err / lim).max()
        dev = np.abs(f["S_traj"][:, 0, 0] / Ps - 1.0)
        lim_v = 6.0 * np.sqrt(2.0 / B) + 6.0 * np.sqrt(2.0 / least)
        worst_v, bound_v = max(worst_v, float(dev.max())), min(bound_v, lim_v)
        assert np.all(dev <= lim_v), dev.max()
        assert np.isnan(f["lag_cov"][-1, 0, 0])
        dl = np.abs(f["lag_cov"][:-1, 0, 0] - C) / np.sqrt(Ps[:-1] * Ps[1:])
        lim_l = 6.0 * np.sqrt((1.0 + rho * rho) * (1.0 / B + 1.0 / least))
        worst_l, bound_l = max(worst_l, float(dl.max())), min(bound_l, float(lim_l.min()))
        assert np.all(dl <= lim_l), (dl / lim_l).max()
    print(f"largest |m_traj - m_RTS| / sqrt(P_s / B) {worst_m:.3f}; largest |S_traj / P_s - 1| {worst_v:.3f} (smallest bound {bound_v:.3f}, "
          f"its first term {6.0 * np.sqrt(2.0 / B):.3f}); largest lag-one deviation {worst_l:.3f} (smallest bound {bound_l:.3f})")


def test_the_marginals_are_the_marginal_smoothers():
    """N = 16, B = 20000 on one seed's stacks: the frequency of every index against w_smooth of the marginal smoother"""
    n, b = 16, 20000
    f = sampled(17, record(), n=n, b=b)
    worst = 0.0
    for t in range(ROWS):
        freq = np.bincount(f["traj_index"][t], minlength=n) / b
        w = f["w_smooth"][t]
        lim = 6.0 * np.sqrt(w * (1.0 - w) / b) + 1.0 / b
        assert np.all(np.abs(freq - w) <= lim), t
        assert np.all(freq[w == 0.0] == 0.0), t
        worst = max(worst, float(np.max(np.abs(freq - w) / lim)))
    assert any(np.any(f["w_smooth"][t] == 0.0) for t in range(ROWS - 1))          # (the exact zeros are there to be respected)
    print(f"largest |freq - w_smooth| / bound {worst:.3f}")


def test_a_near_deterministic_transition_follows_the_genealogy():
    """the transition of test_a_near_deterministic_transition_is_the_genealogy: p is exactly one-hot at the carried copy of the drawn
    particle, so every trajectory is the ancestral line of its last index"""
    def cond(i, X):
        return (A - 1.0) * X + 1e-3 * np.arange(X.shape[0])[:, None], np.zeros_like(X)
    for missing in ((MISSING,), (MISSING, ROWS - 1)):
        f = sampled(5, record(missing), n=64, b=40, cond=cond, q=1e-12)
        assert len(np.unique(f["ancestors"][0])) < 64              # resampling happened
        line = np.zeros_like(f["traj_index"])
        line[-1] = f["traj_index"][-1]
        for t in range(ROWS - 2, -1, -1):
            line[t] = f["ancestors"][t][line[t + 1]]
        np.testing.assert_array_equal(f["traj_index"], line)


def test_equal_uniform_columns_give_equal_trajectories():
    rng = np.random.default_rng(3)
    ub = rng.random((ROWS, 7))
    ub[:, 5] = ub[:, 1]
    f = sampled(9, record(), n=48, unif_bs=ub)
    np.testing.assert_array_equal(f["traj_index"][:, 5], f["traj_index"][:, 1])
    np.testing.assert_array_equal(f["trajectories"][5], f["trajectories"][1])
    g = sampled(9, record(), n=48, unif_bs=ub[:, [1, 3]])        # a trajectory depends on its own column alone
    np.testing.assert_array_equal(g["traj_index"], f["traj_index"][:, [1, 3]])
    for t in range(ROWS):                                         # the gather
        np.testing.assert_array_equal(f["trajectories"][:, t], f["particles"][t][f["traj_index"][t]])


def test_a_record_of_one_row_draws_from_the_filtered_weights():
    f = sampled(3, record()[:1], n=48, b=500)
    cdf = np.cumsum(f["weights"][0])
    k = np.minimum(np.searchsorted(cdf, f["unif_bs"][0] * cdf[-1], side="right"), 47)
    np.testing.assert_array_equal(f["traj_index"][0], k)
    assert np.all(np.isnan(f["lag_cov"])) and f["m_traj"].shape == (1, 1)
    m, S, _ = ps.moments(f["particles"][0], f["weights"][0] / f["weights"][0].sum())
    assert abs(f["m_traj"][0, 0] - m[0]) <= 6.0 * np.sqrt(S[0, 0] / 500)


def test_with_the_last_row_unobserved_the_last_index_is_the_scaled_uniform():
    f = sampled(3, record((MISSING, ROWS - 1)), n=48, b=300)
    np.testing.assert_array_equal(f["traj_index"][-1], np.minimum(np.floor(f["unif_bs"][-1] * 48).astype(np.int64), 47))


def test_in_extended_precision_the_same_indices_and_moments():
    """fp64 against np.longdouble at N = 256, B = 64: identical indices (the margin says why), moments to 1e-12"""
    Y = record()
    f = sampled(7, Y, n=256, b=64, keep_cdf=True)
    w = sampled(7, Y, n=256, b=64, keep_cdf=True, dtype=np.longdouble)
    gap, drift, same = pb.margin(dict(f, gap_bs=f["gap_bs"]), None, w)
    print(f"gap {gap:.3e}, drift {drift:.3e}")
    assert same and gap >= max(1e-8, 1000.0 * drift)
    np.testing.assert_array_equal(f["traj_index"], w["traj_index"])
    for k in pb.MOMENTS:
        ok = ~np.isnan(f[k])
        np.testing.assert_array_equal(ok, ~np.isnan(w[k]))
        err = float(np.max(np.abs(f[k][ok] - w[k][ok])))
        print(f"{k}: fp64 against longdouble {err:.2e}")
        assert w[k].dtype == np.longdouble and err <= 1e-12, k
