"""Hyper-parameters that differ along every axis -- a value fixture for the parity tests (plain helper module, no pytest hooks).

`synthetic.make_workload` draws one variance for every latent dim, one lengthscale per dim for every input, one R and one d for every
output and proportional columns of C: a kernel that reads `loglengthscales[d][p']` with the wrong p', `logvariance` without the
`d_begin` offset of a latent-dim shard or the wrong column of C / d / log_Rchols computes exactly the right answer on such inputs.
`distinct()` replaces those values (and only those: X, Z, U, Y and the control inputs stay as drawn, the draw order of
`make_workload` is untouched) by independent draws per entry.  tests/test_distinct_hypers.py checks on the CPU that the fixture is
distinct, as well conditioned as the workload it replaces, and that each of those index mistakes moves the oracle's nll by at least
1000 x the tolerance of the GPU test that uses the case; tests/test_gpu_distinct_hypers.py runs the HIP paths on it.

The cases, the CPU references (cached: computed once per process, handed out read-only) and the tolerances live here so that the CPU
tests and the GPU tests speak about the same (shape, seed) pairs."""
import functools

import numpy as np

from ffvd_amd import synthetic
from oracle import ffvd_grad_oracle as gorc
from oracle import ffvd_oracle as orc

EPS = np.finfo(np.float64).eps
GRAD_KEYS = ("X", "Z", "logvariance", "loglengthscales", "log_Q", "CC", "DD", "log_Rchols")
ROW_KEYS = ("logvariance", "log_Q", "loglengthscales")        # errors normalised per latent dim d, see grad_errors()
TERMS_B = ("nll_part_prior", "nll_log_likelihood", "x_t_prior_Q", "nll_reg_trace_inverse_Q_B", "later_term1", "later_term2", "nll")
TERMS_A = ("nll_part_prior", "nll_log_likelihood", "x_t_prior_Q", "nll_reg_trace_inverse_Q_B", "nll")


def distinct(params, meta, seed):
    """A copy of `params` whose hyper-parameters differ along every axis (SE: lengthscales log-uniform in [0.7, 5] per (d, p) and
    variances log-uniform in [0.05, 2] per d; LinearK keeps its variances, which already differ per d); Q log-uniform in [0.02, 0.5]
    per d, C = 0.5 N(0, 1) per (d, j), d = 0.3 N(0, 1) per j, R = U(0.2, 0.9) per (j, k) -- so row 0 of log_Rchols, the one the
    likelihood reads (dgp_model.py:250), is not its column 0."""
    rng = np.random.default_rng(seed)
    D, P, J = meta["D"], meta["P"], meta["Ydim"]
    out = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    ll = rng.uniform(np.log(0.7), np.log(5.0), (D, P))
    lv = rng.uniform(np.log(0.05), np.log(2.0), D)
    if meta["kernel_type"] == "SquaredExponential":
        out["loglengthscales"], out["logvariance"] = ll, lv
    out["log_Q"] = rng.uniform(np.log(0.02), np.log(0.5), D)
    out["CC"] = 0.5 * rng.standard_normal((D, J))
    out["DD"] = 0.3 * rng.standard_normal(J)
    out["log_Rchols"] = np.log(rng.uniform(0.2, 0.9, (J, J)))
    return out


# case -> (arguments of synthetic.make_workload, seed of distinct()).  The shapes are the smallest that reach each code path.
CASES = {
    "tiny": (dict(synthetic.CONFIGS["tiny"]), 7),                                          # P = 3
    "ragged": (dict(synthetic.CONFIGS["ragged"]), 7),                                      # P = 5: the fused backward epilogue (P <= 6)
    "p8": (dict(T=160, M=48, D=6, C=2, S=2), 7),                                           # P = 8: the largest the one-launch path takes
    "p9": (dict(T=200, M=40, D=6, C=3, S=2), 7),                                           # P = 9: the generic-P path
    "m256": (dict(T=320, M=256, D=2, C=1, S=2), 7),                                        # Gram route: pair combos
    "m600": (dict(T=700, M=600, D=2, C=1, S=1), 7),                                        # two column groups
    "lin_y2": (dict(T=130, M=40, D=3, C=2, S=2, kernel_type="LinearK", Ydim=2), 7),
    "ragged_y3": (dict(synthetic.CONFIGS["ragged"], Ydim=3), 8),
    "tshard": (dict(synthetic.CONFIGS["ragged"], S=2, D=1), 9),                            # T-shards: S * D < ranks
    "d9": (dict(synthetic.CONFIGS["tiny"], D=9, C=2), 8),                                  # step kernels with more than eight inputs
    "m512": (dict(T=576, M=512, D=4, C=1, S=1), 8),                                        # resident rollout loop at 32 slabs of L^-T
}


def _freeze(obj):
    if isinstance(obj, np.ndarray):
        obj.setflags(write=False)
    elif isinstance(obj, dict):
        for v in obj.values():
            _freeze(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _freeze(v)
    return obj


@functools.lru_cache(maxsize=None)
def base_workload(case):
    """The unmodified workload of a case: (params, Y, c, meta)."""
    cfg, _ = CASES[case]
    cfg = dict(cfg)
    cfg.pop("U_collapse", None)
    return _freeze(synthetic.make_workload(**cfg))


@functools.lru_cache(maxsize=None)
def workload(case):
    """(params, Y, c, meta) of a case with the fixture's hyper-parameters.  Read-only: shared by every test of the process."""
    params, Y, c, meta = base_workload(case)
    return _freeze((distinct(params, meta, CASES[case][1]), Y, c, meta))


def kuu_condition(params, meta):
    """Largest cond(K_uu + 1e-5 I) over the latent dims."""
    kern = orc.make_kernels(params, meta["kernel_type"])
    worst = 0.0
    for k in kern:
        w = np.linalg.eigvalsh(k.K(params["Z"]) + orc.JITTER_MULTI_OUTPUT * np.eye(meta["M"]))
        worst = max(worst, w[-1] / w[0])
    return worst


def gram_route_tolerance(params, meta):
    """Predicted error of the Gram route's nll terms, 4 eps cond(K_uu + jitter I) of the term (test_gpu_elbo.gram_route_tolerance,
    restated here because the CPU tests need it without importing a GPU test module)."""
    return 4.0 * EPS * kuu_condition(params, meta)


# The paths tests/test_gpu_distinct_hypers.py runs each case on, and the tolerance each path puts on the nll (absolute, given the nll):
# what a mutation has to exceed 1000 x for the GPU test to notice it with room to spare.
PATHS = {
    "tiny": ("one_launch", "reference", "gram", "grad", "ops"),
    "ragged": ("one_launch", "reference", "gram", "grad", "ops", "f32c"),
    "p8": ("one_launch", "reference", "gram", "grad"),
    "p9": ("reference", "gram", "grad", "ops"),
    "m256": ("gram", "grad"),
    "m600": ("reference", "gram", "ops"),
    "lin_y2": ("reference", "gram", "grad"),
    "ragged_y3": ("one_launch", "reference", "gram", "grad"),
    "tshard": ("tshard",),
    "d9": ("ops",),
    "m512": ("ops",),
}
GRAD_CASES = ("tiny", "ragged", "p8", "p9", "m256", "ragged_y3")       # gradient tests against the closed form, both branches


def nll_tolerance(case, collapse, nll):
    """The largest tolerance on the nll among the GPU tests that use the case in this branch."""
    params, Y, c, meta = workload(case)
    tols = []
    for path in PATHS[case]:
        if path == "one_launch":
            tols.append(1e-10 * abs(nll))
        elif path == "reference":
            tols.append(1e-9 * abs(nll))
        elif path == "gram" and collapse:
            tols.append(gram_route_tolerance(params, meta) * max(1.0, abs(nll)))
        elif path == "grad":
            tols.append((1e-8 if collapse else 1e-9) * abs(nll))         # the nll check of the gradient tests
        elif path == "ops":
            tols.append(1e-7 * abs(nll))                                # the widest relative tolerance of an operator test
        elif path == "tshard":
            tols.append(1e-7 * abs(nll))
        elif path == "f32c" and collapse:
            tols.append(1e-5)
    return max(tols)


# ---- the index mistakes the fixture is for -----------------------------------------------------------------------------------------
def _roll(key, axis):
    return lambda p: dict(p, **{key: np.roll(p[key], 1, axis=axis)})


MUTATIONS = {
    "roll loglengthscales along p": ("SE", _roll("loglengthscales", 1)),
    "broadcast ls[d][0] over p": ("SE", lambda p: dict(p, loglengthscales=np.repeat(p["loglengthscales"][:, :1], p["loglengthscales"].shape[1], axis=1))),
    "roll logvariance along d": ("D", _roll("logvariance", 0)),
    "roll log_Q along d": ("D", _roll("log_Q", 0)),
    "roll DD": ("Y", _roll("DD", 0)),
    "transpose log_Rchols": ("Y", lambda p: dict(p, log_Rchols=np.ascontiguousarray(p["log_Rchols"].T))),
    "swap CC columns": ("Y", lambda p: dict(p, CC=np.ascontiguousarray(p["CC"][:, ::-1]))),
}


def mutations(meta):
    """The mutations that are not the identity at this shape: lengthscales need the SE kernel, a roll along d needs D > 1, the
    output-side ones Ydim > 1."""
    out = {}
    for name, (needs, fn) in MUTATIONS.items():
        if needs == "SE" and meta["kernel_type"] != "SquaredExponential":
            continue
        if needs == "D" and meta["D"] < 2:
            continue
        if needs == "Y" and meta["Ydim"] < 2:
            continue
        out[name] = fn
    return out


# ---- CPU references ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_reference(case, collapse):
    params, Y, c, meta = workload(case)
    return _freeze(orc.nll_terms_chains(params, Y, c, U_collapse=collapse, kernel_type=meta["kernel_type"]))


def mean_over_chains(per_chain, params):
    """Gradient of the mean-over-chains nll from a per-chain gradient function (X per chain, every other key averaged)."""
    S = params["X"].shape[0]
    out = None
    for s in range(S):
        g = per_chain(dict(params, X=params["X"][s]))
        if out is None:
            out = {k: (np.zeros((S,) + v.shape) if k == "X" else np.zeros_like(v)) for k, v in g.items()}
        for k, v in g.items():
            if k == "X":
                out["X"][s] = v / S
            else:
                out[k] += v / S
    return out


@functools.lru_cache(maxsize=None)
def grad_reference(case, collapse):
    """Closed-form gradient (oracle/ffvd_grad_oracle.py) of the mean-over-chains nll; with 'U' in the explicit-U branch."""
    params, Y, c, meta = workload(case)
    fn = gorc.nll_grad if collapse else gorc.nll_grad_explicit_u
    return _freeze(mean_over_chains(lambda p: fn(p, Y, c), params))


@functools.lru_cache(maxsize=None)
def autograd_reference(case, collapse):
    """torch autograd of the independent restatement (oracle/ffvd_oracle_torch.py): the second CPU gradient reference."""
    from oracle import ffvd_oracle_torch as orct
    params, Y, c, meta = workload(case)
    keys = GRAD_KEYS + (() if collapse else ("U",))
    if meta["kernel_type"] != "SquaredExponential":
        keys = tuple(k for k in keys if k != "loglengthscales")
    Yw, cw = np.array(Y), np.array(c)                            # (torch wants writable arrays)
    return _freeze(mean_over_chains(
        lambda p: orct.nll_and_grad({k: np.array(v) for k, v in p.items()}, Yw, cw, wrt=keys, U_collapse=collapse,
                                    kernel_type=meta["kernel_type"])[1], params))


def grad_errors(got, ref, keys):
    """Worst error per key, relative to the largest reference entry -- of the ROW for the per-latent-dim arrays (logvariance, log_Q,
    loglengthscales): with variances from 0.05 to 2 the rows differ by orders of magnitude and a whole-array maximum would hide a
    wrong small row."""
    out = {}
    for k in keys:
        g, r = np.asarray(got[k], dtype=np.float64).reshape(np.shape(ref[k])), np.asarray(ref[k])
        if k in ROW_KEYS:
            d = np.abs(g - r).reshape(r.shape[0], -1).max(axis=1)
            scale = np.abs(r).reshape(r.shape[0], -1).max(axis=1)
            out[k] = float(np.max(d / (scale + 1e-300)))
        else:
            out[k] = float(np.max(np.abs(g - r)) / (np.max(np.abs(r)) + 1e-300))
    return out


@functools.lru_cache(maxsize=None)
def reference_disagreement(case, collapse):
    """Disagreement of the two CPU gradient references (closed form against torch autograd) on a case, per key, in the normalisation
    of grad_errors -- computed from the references themselves, never from a HIP result.  Measured: 3.3e-9 at worst (dZ at M = 256,
    cond(K_uu) 1e7), 1.2e-9 on the lengthscales of the explicit-U branch there, below 1e-9 everywhere else."""
    keys = GRAD_KEYS + (() if collapse else ("U",))
    return grad_errors(grad_reference(case, collapse), autograd_reference(case, collapse), keys)


def grad_bound(case, collapse, key, tol):
    """The larger of the project's tolerance for the path and 10 x the disagreement of the two CPU references on that case and key: a
    GPU gradient cannot be asked to agree with one reference more closely than the references agree with each other."""
    return max(tol, 10.0 * reference_disagreement(case, collapse)[key])
