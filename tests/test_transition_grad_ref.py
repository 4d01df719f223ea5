"""The mathematics of the linearised transition, pinned without a device: tests/transition_grad_ref.py (the NumPy restatement the GPU
tests compare with) against the oracle's conditional_after_kernel_precalculation for the values, in both q_modes ("intent" per dim, as
tests/test_gpu_conditional_grouped.py's _oracle_cond does), and against central differences of its OWN values in np.longdouble for the
gradients: the difference error at h = 2^-8, 2^-9, 2^-10 must fall by a factor in [3.5, 4.5] per halving (second-order convergence to
the analytic gradient; 4.00 was measured throughout).  The same convergence test pins the centred form of the mixture's variance
gradient.  Tolerances of the values: the project floors 1e-11 + 1e-9 max|ref| (mean) and 1e-11 + 1e-8 max|ref| (var); at most 5.3e-14
and 1.5e-10 (m130) were measured."""
import functools

import numpy as np
import pytest

import moment_ref as mr
import transition_grad_ref as tg
from ffvd_amd import synthetic
from oracle import ffvd_oracle as orc

SHAPES = {"tiny": ("tiny", {}), "ragged": ("ragged", {}), "small": ("small", dict(S=3)), "small200": ("small", dict(M=200, S=3)),
          "m130": ("tiny", dict(M=130, D=1, C=0, T=160)), "d8": ("tiny", dict(M=40, D=8, C=1))}
MODES = ("reference", "intent")
N = 12
WIDE = np.finfo(np.longdouble).eps < 1e-18
needs_longdouble = pytest.mark.skipif(not WIDE, reason="np.longdouble is not wider than 1e-18 on this platform: the central differences "
                                                       "of the reference cannot resolve its gradients")


def make_xnew(X0, c, T, n):
    """the inputs of tests/test_gpu_conditional_grouped.py: rows near the data and rows far from it"""
    rng = np.random.default_rng(7)
    rows = np.concatenate((X0[:T], c[:T]), axis=1)
    near = n - n // 4
    pick = rng.choice(T, size=near, replace=near > T)
    return np.concatenate((rows[pick] + 0.05 * rng.standard_normal((near, rows.shape[1])), 3.0 * rng.standard_normal((n // 4, rows.shape[1]))))


@functools.lru_cache(maxsize=None)
def case(shape, groups=1):
    name, ov = SHAPES[shape]
    p, Y, c, meta = synthetic.make_named(name, **ov)
    T, okern, Q = meta["T"], orc.make_kernels(p, kernel_type=meta["kernel_type"]), np.exp(p["log_Q"])
    L = orc.kernel_pre_cal(p["Z"], okern)
    post = []
    for g in range(groups):
        X = p["X"][g]
        U, H = orc.collapse_u_mean_after_kernel_precalculation(L, np.concatenate((X[:T], c[:T]), axis=1), X, p["Z"], okern, Q)
        post.append((U, np.asarray(H)))
    return dict(Z=p["Z"], kern=okern, L=list(L), post=post, Xnew=make_xnew(p["X"][0], c, T, N), D=meta["D"], P=meta["P"])


def floor(key, ref):
    return 1e-11 + (1e-9 if key == "mean" else 1e-8) * float(np.max(np.abs(ref)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_values_match_the_oracle(shape, mode):
    cs = case(shape)
    U, H = cs["post"][0]
    beta, Gam = mr.posterior_terms(cs["L"], U, H, mode)
    mean, var, _, _ = tg.linearize(cs["Xnew"], cs["Z"], cs["kern"], beta, Gam)
    fn = orc.conditional_after_kernel_precalculation
    if mode == "reference":
        om, ov = fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=H, white=True)
    else:
        outs = [fn(cs["L"], cs["Xnew"], cs["Z"], cs["kern"], U, q_sqrt=H[d:d + 1], white=True) for d in range(cs["D"])]
        om, ov = outs[0][0], np.stack([outs[d][1][:, d] for d in range(cs["D"])], axis=1)
    em, ev = float(np.max(np.abs(mean - om))), float(np.max(np.abs(var - ov)))
    print(f"{shape} {mode}: mean {em:.3e} (floor {floor('mean', om):.3e}), var {ev:.3e} (floor {floor('var', ov):.3e})")
    assert em <= floor("mean", om) and ev <= floor("var", ov)


def _ratios(errs):
    return [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]


@needs_longdouble
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gradients_are_the_limit_of_central_differences(shape):
    t = np.longdouble
    cs = case(shape)
    U, H = cs["post"][0]
    beta, Gam = mr.posterior_terms(cs["L"], U, H, "intent", dtype=t)
    fn = lambda X: tg.linearize(X, cs["Z"], cs["kern"], beta, Gam, dtype=t)[:2]
    _, _, dmean, dvar = tg.linearize(cs["Xnew"], cs["Z"], cs["kern"], beta, Gam, dtype=t)
    em, ev = [], []
    for k in (8, 9, 10):
        fm, fv = tg.central_differences(fn, cs["Xnew"], t(2) ** -k, dtype=t)
        em.append(float(np.max(np.abs(fm - dmean))))
        ev.append(float(np.max(np.abs(fv - dvar))))
    print(f"{shape}: dmean errors {em}, ratios {_ratios(em)}; dvar errors {ev}, ratios {_ratios(ev)}")
    for r in _ratios(em) + _ratios(ev):
        assert 3.5 <= r <= 4.5, (em, ev)


@needs_longdouble
@pytest.mark.parametrize("shape,groups", [("tiny", 3), ("ragged", 2)])
def test_mixture_gradients_are_the_limit_of_central_differences(shape, groups):
    t = np.longdouble
    cs = case(shape, groups)
    terms = [mr.posterior_terms(cs["L"], U, H, "reference", dtype=t) for U, H in cs["post"]]
    groups = lambda X: [tg.linearize(X, cs["Z"], cs["kern"], b, G, dtype=t) for b, G in terms]
    _, _, mdm, mdv = tg.mixture(groups(cs["Xnew"]))
    fn = lambda X: tg.mixture(groups(X))[:2]
    em, ev = [], []
    for k in (8, 9, 10):
        fm, fv = tg.central_differences(fn, cs["Xnew"], t(2) ** -k, dtype=t)
        em.append(float(np.max(np.abs(fm - mdm))))
        ev.append(float(np.max(np.abs(fv - mdv))))
    print(f"{shape}: mix_dmean errors {em}, ratios {_ratios(em)}; mix_dvar errors {ev}, ratios {_ratios(ev)}")
    for r in _ratios(em) + _ratios(ev):
        assert 3.5 <= r <= 4.5, (em, ev)
