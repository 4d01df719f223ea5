"""Fixtures of tests/test_gpu_score.py and their references (tests/score_ref.py), built without a GPU; tests/test_score_fixtures.py
checks the conditions the device tolerances rest on.  A case is (name, kind, K, steps, n_test, J, Q, D, bimodal): kind "points"
gives a component-major stack x (K, steps, D), kind "moments" Gaussian states m (K, steps, D), S (K, steps, D, D).  K walks the
component tile T_c of the pair kernel: 1, 2, T_c - 1, T_c, T_c + 1, 2 T_c + 3."""
import functools

import numpy as np

import score_ref as sr

TILE = 256                      # ffvd_amd.prediction.SCORE_TILE (tests/test_score_args.py holds the two together)

#        name         kind       K            steps n_test J  Q   D  bimodal
CASES = (("p_k1",     "points",  1,            1,   1,     1, 1,  1,  False),
         ("p_k2",     "points",  2,            7,   7,     3, 3,  4,  False),
         ("p_tile-1", "points",  TILE - 1,     7,   5,     8, 16, 32, False),
         ("p_tile",   "points",  TILE,         1,   1,     3, 0,  4,  False),
         ("p_tile+1", "points",  TILE + 1,     7,   7,     1, 3,  1,  True),
         ("p_2tile+3", "points", 2 * TILE + 3, 7,   7,     3, 16, 4,  True),
         ("m_k1",     "moments", 1,            1,   1,     1, 1,  1,  False),
         ("m_k2",     "moments", 2,            7,   5,     3, 3,  8,  False),
         ("m_tile-1", "moments", TILE - 1,     7,   7,     8, 16, 1,  False),
         ("m_tile",   "moments", TILE,         7,   7,     1, 0,  8,  False),
         ("m_tile+1", "moments", TILE + 1,     1,   1,     3, 3,  8,  True),
         ("m_2tile+3", "moments", 2 * TILE + 3, 7,  7,     3, 16, 8,  True))
NAMES = tuple(c[0] for c in CASES)
CONDITION = 1e-3                # f(q_ref) (max mu - min mu + max sigma) of every (target, level)


def levels_of(Q):
    """Q levels, symmetric about 1/2 (so that coverage has its pairs)"""
    return {0: np.empty(0), 1: np.array([0.5]), 3: np.array([0.05, 0.5, 0.95]), 16: np.linspace(0.03, 0.97, 16)}[Q]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The arrays of a case (never modified): the stack, the emission (CC, DD, log_Rchols as a vector of J), Y (n_test, J) with NaN
    targets in some rows and none in others, the levels."""
    _, kind, K, steps, n_test, J, Q, D, bimodal = CASES[NAMES.index(name)]
    rng = np.random.default_rng(1000 + NAMES.index(name))
    CC = rng.standard_normal((D, J)) / np.sqrt(D)
    CC[0] += np.where(CC[0] >= 0.0, 0.5, -0.5)                     # (no output is blind to latent dim 0, which carries the modes)
    DD, sd = rng.standard_normal(J) * 0.5, 0.3 + 0.3 * rng.random(J)
    x = 0.6 * rng.standard_normal((K, steps, D))
    if bimodal:               # two clusters of components: seven noise deviations apart in the output that sees them farthest apart
        x[:, :, 0] += np.where(np.arange(K) % 2 == 0, -1.0, 1.0)[:, None] * 3.5 * float(np.min(sd / np.abs(CC[0])))
    fx = dict(name=name, kind=kind, K=K, steps=steps, n_test=n_test, J=J, Q=Q, D=D, bimodal=bimodal, CC=CC, DD=DD, lr=np.log(sd), sd=sd,
              x=x, levels=levels_of(Q))
    if kind == "moments":
        L = 0.25 * rng.standard_normal((K, steps, D, D))
        S = L @ np.swapaxes(L, -1, -2)
        fx["S"] = 0.5 * (S + np.swapaxes(S, -1, -2))
        mu, var = sr.components_moments(x, fx["S"], CC, DD, sd)
    else:
        mu, var = sr.components_points(x, CC, DD, sd)
    # targets: drawn from the mixture's own components, so that pit is spread over (0, 1)
    pick = rng.integers(0, K, size=(n_test, J))
    Y = np.take_along_axis(mu[:n_test], pick[:, :, None], axis=2)[:, :, 0] + np.sqrt(np.take_along_axis(var[:n_test], pick[:, :, None],
                                                                                                        axis=2)[:, :, 0]) * rng.standard_normal((n_test, J))
    if n_test > 2:
        Y[1, 0] = np.nan                                           # one entry of row 1, all of row 3; the other rows are complete
        Y[3 % n_test, :] = np.nan
    fx.update(mu=mu, var=var, Y=Y)
    return fx


@functools.lru_cache(maxsize=None)
def reference(name):
    """score_ref on a fixture, computed once and shared (never modified): crps, pit, quantiles, and per (target, level) the
    reference density f(q_ref) and the width max mu - min mu + max sigma"""
    fx = fixture(name)
    ref = sr.score(fx["mu"], fx["var"], fx["Y"], fx["levels"])
    q = ref["quantiles"]
    dens = np.stack([sr.pdf(fx["mu"], fx["var"], q[..., i]) for i in range(q.shape[-1])], axis=-1) if q.shape[-1] else np.empty(q.shape)
    width = np.max(fx["mu"], axis=-1) - np.min(fx["mu"], axis=-1) + np.sqrt(np.max(fx["var"], axis=-1))
    ref.update(density=dens, width=width)
    return ref


def call_args(fx):
    """(function name, positional arguments) of the prediction-level call of a fixture"""
    em = (fx["CC"], fx["DD"], fx["lr"])
    return ("rollout_score", (fx["x"],) + em) if fx["kind"] == "points" else ("moment_score", (fx["x"], fx["S"]) + em)


def split(K):
    """K = G N with the largest G <= 8 that divides K: the [G][T][N][D] layout of the same components"""
    G = max(g for g in range(1, 9) if K % g == 0)
    return G, K // G


def as_particles(x):
    """(K, steps, D) component-major -> (G, steps, N, D) with component k = g N + i"""
    K, steps, D = x.shape
    G, N = split(K)
    return np.ascontiguousarray(np.transpose(x.reshape(G, N, steps, D), (0, 2, 1, 3)))
