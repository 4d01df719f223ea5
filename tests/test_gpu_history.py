"""GPU, handles: no result may depend on what device memory held before the call.

Two claims, both asserted bit for bit (the library has no atomics and fixed summation orders, so there is no tolerance and no CPU
oracle here):

* a handle whose every allocation starts as NaN bytes (FFVD_WS_POISON=1, read per handle in create_impl) computes what a handle on
  whatever hipMalloc returned computes -- a kernel that leans on fresh memory being zero fails here;
* a call leaves nothing behind: after calls with other parameters, failed factorisations, forward-only calls between backward
  passes, the enqueue-only form and timed iterations, the same call gives the bits it gave first, and the bits of a fresh handle.

CONFIGS names one engine configuration per workspace layout / schedule of create_impl, alloc_grad_workspace, train.hip and comm.hip;
COVERS says which handle buffers each one exercises (tests/test_history_coverage.py keeps that list complete against the sources).
"""
import functools

import numpy as np
import pytest

from ffvd_amd import _lib, synthetic
from ffvd_amd.engine import ElboEngine

pytestmark = pytest.mark.gpu

NO_TINY = {"FFVD_NO_TINY": "1"}


def _tshard_case(name, ov, nshard, grad, dupz=False):
    return dict(workload=("named", name, ov), mode="tshard", nshard=nshard, grad=grad, kw=dict(route="gram"), dupz=dupz)


# id -> configuration.  workload: ("named", name, overrides) / ("workload", kwargs); kw: ElboEngine keywords; env: switches read when a
# handle is created; mode: fwd | grad | tshard | train | train_rccl.  dupz: the row also goes through the coincident-inducing-points
# failure, which needs handles created with jitter = 0.0 that can still evaluate p1.  The flag is set exactly where the kernel is the
# SE kernel and lambda_min / lambda_max of K_uu(Z) WITHOUT jitter exceeds DUPZ_MIN_EIG_RATIO for every latent dim
# (tests/test_history_coverage.py computes the ratio on the CPU and holds the flags to this rule).  The other rows cannot evaluate p1
# at jitter = 0.0: LinearK's K_uu has rank P << M, and the inducing inputs of `combos`, `m600`, `m1024` (ratio ~1e-17, some eigenvalues
# negative in fp64) and of the `ragged` D = 1 T-shard rows (1.7e-12) make a K_uu that only the jitter keeps positive definite.
DUPZ_MIN_EIG_RATIO = 1e-11


def k_uu_eig_ratio(key):
    """min over the latent dims of lambda_min / lambda_max of K_uu(Z) without jitter (SE kernel; None for LinearK), on the CPU"""
    from oracle import ffvd_oracle as orc
    params, _, _, meta = _workload(key)
    if meta["kernel_type"] != "SquaredExponential":
        return None
    ratio = np.inf
    for d in range(meta["D"]):
        w = np.linalg.eigvalsh(orc.SquaredExponential(params["logvariance"][d], params["loglengthscales"][d]).K(params["Z"]))
        ratio = min(ratio, float(w[0] / w[-1]))
    return ratio


CONFIGS = {
    "tinyB": dict(workload=("named", "tiny", {}), mode="fwd", kw={}, dupz=True),
    "tinyB-gram": dict(workload=("named", "tiny", {}), mode="fwd", kw=dict(route="gram"), dupz=True),
    "tinyB-grad": dict(workload=("named", "tiny", {}), mode="grad", kw=dict(route="gram"), dupz=True),
    "tinyA": dict(workload=("named", "tiny", dict(U_collapse=False)), mode="fwd", kw={}, dupz=True),
    "tinyA-grad": dict(workload=("named", "tiny", dict(U_collapse=False)), mode="grad", kw={}, dupz=True),
    "A-mk": dict(workload=("named", "ragged", dict(U_collapse=False)), mode="fwd", kw={}, env=NO_TINY, dupz=True),
    "A-grad-mk": dict(workload=("named", "ragged", dict(U_collapse=False)), mode="grad", kw={}, env=NO_TINY, dupz=True),
    "ref-mk": dict(workload=("named", "ragged", {}), mode="fwd", kw={}, env=NO_TINY, dupz=True),
    "gram-mk": dict(workload=("named", "ragged", {}), mode="fwd", kw=dict(route="gram"), env=NO_TINY, dupz=True),
    "gram-grad-P5": dict(workload=("named", "ragged", {}), mode="grad", kw=dict(route="gram"), env=NO_TINY, dupz=True),
    "gram-grad-P7": dict(workload=("named", "tiny", dict(T=130, M=40, D=5, C=2, S=2)), mode="grad", kw=dict(route="gram"), env=NO_TINY,
                         dupz=True),
    "ref-grad": dict(workload=("named", "ragged", {}), mode="grad", kw={}, env=NO_TINY, dupz=True),
    "combos": dict(workload=("named", "c2", dict(M=256, T=320, S=3, D=2)), mode="fwd", kw=dict(route="gram"), env=NO_TINY),
    "combos-gsplit1": dict(workload=("named", "c2", dict(M=256, T=320, S=3, D=2)), mode="fwd", kw=dict(route="gram"),
                           env=dict(NO_TINY, FFVD_GSPLIT="1")),
    "m600-ref": dict(workload=("workload", dict(T=700, D=2, C=1, M=600, S=1)), mode="fwd", kw={}),
    "m600-gram": dict(workload=("workload", dict(T=700, D=2, C=1, M=600, S=1)), mode="fwd", kw=dict(route="gram")),
    "passes-1": dict(workload=("named", "small", {}), mode="fwd", kw=dict(chains_per_pass=1), env=NO_TINY, dupz=True),
    "passes-3": dict(workload=("named", "small", {}), mode="fwd", kw=dict(chains_per_pass=3), env=NO_TINY, dupz=True),
    "passes-3-gram": dict(workload=("named", "small", {}), mode="fwd", kw=dict(chains_per_pass=3, route="gram"), env=NO_TINY, dupz=True),
    "linA": dict(workload=("named", "small_lin", {}), mode="fwd", kw={}, env=NO_TINY),
    "linA-wide": dict(workload=("named", "small_lin", {}), mode="fwd", kw={}, env=dict(NO_TINY, FFVD_NO_LINEAR_LOWRANK="1")),
    "linA-grad": dict(workload=("named", "small_lin", {}), mode="grad", kw={}, env=NO_TINY),
    "linB-grad": dict(workload=("named", "small_lin", dict(U_collapse=True)), mode="grad", kw=dict(route="gram"), env=NO_TINY),
    "f32c": dict(workload=("named", "ragged", {}), mode="fwd", kw=dict(dtype="f32c"), dupz=True),
    "f32c-grad": dict(workload=("named", "ragged", {}), mode="grad", kw=dict(dtype="f32c"), dupz=True),
    "tshard-small": _tshard_case("small", dict(S=1, D=2), 3, False, dupz=True),
    "tshard-ragged": _tshard_case("ragged", dict(S=2, D=1), 4, False),
    "tshard-lin": _tshard_case("small_lin", dict(S=1, D=2, U_collapse=True), 2, False),
    "tshard-grad-small": _tshard_case("small", dict(S=1, D=2), 3, True, dupz=True),
    "tshard-grad-ragged": _tshard_case("ragged", dict(S=2, D=1), 4, True),
    "tshard-grad-lin": _tshard_case("small_lin", dict(S=1, D=2, U_collapse=True), 2, True),
    "tshard-grad-small3": _tshard_case("small", dict(S=3, D=3), 2, True, dupz=True),
    "train": dict(workload=("named", "small", {}), mode="train", kw=dict(route="gram"), dupz=True),
    "train-mk": dict(workload=("named", "small", {}), mode="train", kw=dict(route="gram"), env=NO_TINY, dupz=True),
    "train-A": dict(workload=("named", "tiny", dict(U_collapse=False)), mode="train", kw={}, dupz=True),
    "train-rccl": dict(workload=("named", "small", {}), mode="train_rccl", kw=dict(route="gram"), dupz=True),
    "c2-16": dict(workload=("named", "c2", dict(S=16)), mode="fwd", kw=dict(route="gram"), dupz=True),
    "c2-32": dict(workload=("named", "c2", {}), mode="fwd", kw=dict(route="gram"), dupz=True),
    "c2-32-grad": dict(workload=("named", "c2", {}), mode="grad", kw=dict(route="gram"), dupz=True),
    "m1024": dict(workload=("workload", dict(T=1024, D=2, C=1, M=1024, S=16)), mode="fwd", kw=dict(route="gram")),
}

# The buffers every handle has and every call goes through (parameters, data, the K_uu chain, the result block) ...
_BASE = ("prior_sums", "X", "Z", "U", "logvar", "loglen", "logQ", "CC", "DD", "logR", "Y", "ctrl", "variance", "len", "Zs", "zz", "Kuu",
         "rowsq", "fmean", "hterms", "chain_terms", "chain_partial", "resblk", "dinvK", "dinvH")
_TINY = ("tiny_scratch", "tiny_flags", "tiny_dargs")
_GRAM = ("F", "H", "Kcopy", "Linv", "Kinv", "trpart", "kterms", "growpart")
# ... and the backward-pass workspace of alloc_grad_workspace: shared part, whitened (collapsed) part, explicit-U part
_GRAD = ("Acopy", "u", "LAinv", "Gamma", "gam_part", "uku", "rsum", "ez", "kfu", "cs_part", "etx_part", "rx2_part", "dz_unit", "dll_unit",
         "dls_unit", "Asum", "GamSum", "Gs", "gsum", "P1", "KGK", "Epsi", "rsum2", "ez2", "cs2", "etx2", "rx22", "dz_kuu", "dll_kuu", "dls_kuu",
         "shared_part", "pack")
_WHITE = ("T1", "wv", "bw", "Ident", "P2", "P3")
_GRAD_A = ("Gu", "Gsum", "r", "dalpha", "xsq", "ucol", "beta", "du", "GammaA", "Lclean", "ucolA", "F", "Kcopy", "Linv", "Kinv", "trpart", "kterms")

# configuration id -> handle buffers (member names of ffvd_handle / its GradWs, as they appear in dev_alloc(h, &...)) that the
# configuration allocates (a conditional one is listed only where the condition is known to hold).  `d` is the staging block of ffvd_allreduce_sum (comm.hip names it so).
COVERS = {
    "tinyB": _BASE + _TINY + ("F", "H", "Kf2"),
    "tinyB-gram": _BASE + _TINY + _GRAM,
    "tinyB-grad": _BASE + _TINY + _GRAM + _GRAD + _WHITE + ("rp",),
    "tinyA": _BASE + _TINY,
    "tinyA-grad": _BASE + _TINY + _GRAD + _GRAD_A + ("rp",),
    "A-mk": _BASE,
    "A-grad-mk": _BASE + _GRAD + _GRAD_A + ("rp",),
    "ref-mk": _BASE + ("F", "Kf2", "H"),
    "gram-mk": _BASE + _GRAM + ("gpart",),
    "gram-grad-P5": _BASE + _GRAM + _GRAD + _WHITE + ("rp", "gpart"),
    "gram-grad-P7": _BASE + _GRAM + _GRAD + _WHITE + ("E",),
    "ref-grad": _BASE + ("F", "Kf2", "H", "Kcopy", "Linv", "Kinv", "trpart", "kterms", "fsq") + _GRAD + _WHITE + ("rp",),
    "combos": _BASE + _GRAM + ("gpart",),
    "combos-gsplit1": _BASE + _GRAM,
    "m600-ref": _BASE + ("F", "Kf2", "H"),
    "m600-gram": _BASE + _GRAM,
    "passes-1": _BASE + ("F", "Kf2", "H"),
    "passes-3": _BASE + ("F", "Kf2", "H"),
    "passes-3-gram": _BASE + _GRAM,
    "linA": _BASE + ("lrpart",),
    "linA-wide": _BASE,
    "linA-grad": _BASE + _GRAD + _GRAD_A + ("E",),
    "linB-grad": _BASE + _GRAM + _GRAD + _WHITE + ("E", "xsq"),
    "f32c": _BASE + ("Kf32", "F32", "Linv32", "sqpart", "sqsum", "H"),
    "f32c-grad": _BASE + ("Kf32", "F32", "Linv32", "sqpart", "sqsum", "H", "Kcopy", "Linv", "Kinv", "trpart", "kterms", "Gam32") + _GRAD + _WHITE,
    "tshard-small": _BASE + _GRAM[:-1] + ("tsbuf",),
    "tshard-ragged": _BASE + _GRAM[:-1] + ("tsbuf",),
    "tshard-lin": _BASE + _GRAM[:-1] + ("tsbuf",),
    "tshard-grad-small": _BASE + _GRAM[:-1] + ("tsbuf",) + _GRAD + _WHITE + ("rp",),
    "tshard-grad-ragged": _BASE + _GRAM[:-1] + ("tsbuf",) + _GRAD + _WHITE + ("rp",),
    "tshard-grad-lin": _BASE + _GRAM[:-1] + ("tsbuf",) + _GRAD + _WHITE + ("rp", "xsq"),
    "tshard-grad-small3": _BASE + _GRAM[:-1] + ("tsbuf",) + _GRAD + _WHITE + ("rp",),
    "train": _BASE + _GRAM + _GRAD + _WHITE + ("rp", "adam_m", "adam_v", "hmc"),
    "train-mk": _BASE + _GRAM + _GRAD + _WHITE + ("rp", "adam_m", "adam_v", "hmc"),
    "train-A": _BASE + _TINY + _GRAD + _GRAD_A + ("rp", "adam_m", "adam_v", "hmc"),
    "train-rccl": _BASE + _GRAM + _GRAD + _WHITE + ("rp", "adam_m", "adam_v", "hmc", "d"),
    "c2-16": _BASE + _GRAM + ("graw",),
    "c2-32": _BASE + _GRAM,
    "c2-32-grad": _BASE + _GRAM + _GRAD + _WHITE + ("rp",),
    "m1024": _BASE + _GRAM + ("gtail",),
}

IDS = list(CONFIGS)


@functools.lru_cache(maxsize=None)
def _workload(key):
    """(params, Y, control, meta) of a configuration, built once per module (the c2 workloads take a second each) and never written to."""
    kind, *rest = CONFIGS[key]["workload"]
    if kind == "named":
        out = synthetic.make_named(rest[0], **rest[1])
    else:
        out = synthetic.make_workload(**rest[0])
    for a in list(out[0].values()) + [out[1], out[2]]:
        a.setflags(write=False)
    return out


def _perturbed(params):
    """p2: every parameter array differs from p1 (same shapes, still a well-conditioned problem)."""
    rng = np.random.default_rng(20240607)
    p = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    p["X"] = p["X"] + 0.02 * rng.standard_normal(p["X"].shape)
    p["Z"] = p["Z"] + 0.01 * rng.standard_normal(p["Z"].shape)
    p["U"] = p["U"] + 0.05 * rng.standard_normal(p["U"].shape)
    p["logvariance"] = p["logvariance"] + 0.05
    p["loglengthscales"] = p["loglengthscales"] - 0.03 * (1.0 + np.arange(p["loglengthscales"].shape[1]))[None, :] / p["loglengthscales"].shape[1]
    p["log_Q"] = p["log_Q"] + 0.04
    p["CC"] = p["CC"] * 1.1
    p["DD"] = p["DD"] + 0.01
    p["log_Rchols"] = p["log_Rchols"] + 0.02
    return p


def _nan_x(params):
    """one entry of X of one chain (the last) is NaN: the failure of test_non_finite_inputs_are_reported_not_propagated"""
    bad = dict(params, X=np.array(params["X"], dtype=np.float64))
    bad["X"][-1, min(7, bad["X"].shape[1] - 2), 0] = np.nan
    return bad


def _dup_z(params):
    """two inducing points coincide: the failure of test_not_positive_definite_is_reported (needs a handle with jitter = 0.0)"""
    p = dict(params, Z=np.array(params["Z"], dtype=np.float64))
    p["Z"][5] = p["Z"][4]
    return p


def _named(sums, S):
    return {n: np.float64(sums[i] / S) for i, n in enumerate(_lib.TERM_NAMES)}


class Plain:
    """One ElboEngine; f = one forward iteration (mode fwd) or forward + backward (mode grad)."""

    def __init__(self, key, **over):
        cfg = CONFIGS[key]
        self.params, Y, c, self.meta = _workload(key)
        m = self.meta
        self.grad = cfg["mode"] == "grad"
        kw = dict(cfg["kw"], **over)
        self.e = ElboEngine(m["T"], m["D"], m["C"], m["M"], m["S"], Ydim=m["Ydim"], kernel_type=m["kernel_type"], U_collapse=m["U_collapse"],
                            grad=self.grad, **kw)
        self.e.set_data(Y, c)

    def f(self, p):
        e, S = self.e, self.meta["S"]
        if self.grad:
            t, g = e.nll_and_grad(p)
            out = {"sums8": t["sums8"], "nll_per_chain": t["nll_per_chain"]}
            out.update({"d" + k: v for k, v in g.items()})
        else:
            out = {"sums8": e.elbo_sums(p), "nll_per_chain": e.chain_nll()}
        out.update(_named(out["sums8"], S))
        return out

    def history(self, p2):
        """every other call the configuration allows, in between two f(p1)"""
        e = self.e
        self.f(p2)
        with pytest.raises(np.linalg.LinAlgError):
            self.f(_nan_x(self.params)) if self.meta["U_collapse"] else self._nan_call_a()
        if self.grad:
            self.f(self.params)
            e.nll_terms(p2)                          # a forward-only call between two backward passes
            self.f(p2)
        e.set_params(p2)
        e.elbo_async()
        e.sync()
        assert e.time_elbo(2) > 0

    def _nan_call_a(self):
        # explicit-U branch: no per-chain factorisation sees X, a NaN there comes back as a non-finite sum, not as a return code
        out = self.f(_nan_x(self.params))
        if not np.all(np.isfinite(out["sums8"])):
            raise np.linalg.LinAlgError("non-finite sums")

    def fail_dup_z(self):
        with pytest.raises(np.linalg.LinAlgError):
            self.f(_dup_z(self.params))

    def stalls(self):
        return int(self.e.lib.ffvd_stall_recoveries(self.e._h))

    def close(self):
        self.e.close()


class TShards:
    """The T-shard engines of one job in one process, the exchange summed on the host as the all-reduce would."""

    def __init__(self, key, **over):
        from ffvd_amd.distributed import shard_range
        cfg = CONFIGS[key]
        self.params, Y, c, self.meta = _workload(key)
        m = self.meta
        self.grad = cfg["grad"]
        self.engines, self.ranges = [], []
        try:
            for r in range(cfg["nshard"]):
                t0, tc = shard_range(m["T"], cfg["nshard"], r)
                e = ElboEngine(tc, m["D"], m["C"], m["M"], m["S"], kernel_type=m["kernel_type"], t_shard=(t0, m["T"]), grad=self.grad,
                               **dict(cfg["kw"], **over))
                self.engines.append(e)
                self.ranges.append((t0, tc))
                e.set_data(Y[t0: t0 + tc], c[t0: t0 + tc])
        except BaseException:
            self.close()
            raise

    def f(self, p):
        S = self.meta["S"]
        out = {}
        bufs = []
        for r, (e, (t0, tc)) in enumerate(zip(self.engines, self.ranges)):
            e.set_params(dict(p, X=np.ascontiguousarray(p["X"][:, t0: t0 + tc + 1])))
            bufs.append(e.tshard_local())
            out["local%d" % r] = bufs[-1]
        total = np.sum(bufs, axis=0)
        if not self.grad:
            for r, e in enumerate(self.engines):
                out["sums8_%d" % r] = e.tshard_finish(total)
        else:
            blocks = [e.tshard_finish_grad(total) for e in self.engines]
            block = np.sum(blocks, axis=0)
            for r, e in enumerate(self.engines):
                out["block%d" % r] = blocks[r]
                sums, g = e.tshard_grad_fetch(block)
                out["sums8_%d" % r] = sums
                out.update({"d%s_%d" % (k, r): v for k, v in g.items()})
        out.update(_named(out["sums8_0"], S))
        return out

    def history(self, p2):
        self.f(p2)
        with pytest.raises(np.linalg.LinAlgError):
            self.f(_nan_x(self.params))
        if self.grad:
            self.f(self.params)
            self._forward_only(p2)                   # a forward-only call (local rows + finish) between two backward passes
            self.f(p2)

    def _forward_only(self, p):
        bufs = []
        for e, (t0, tc) in zip(self.engines, self.ranges):
            e.set_params(dict(p, X=np.ascontiguousarray(p["X"][:, t0: t0 + tc + 1])))
            bufs.append(e.tshard_local())
        total = np.sum(bufs, axis=0)
        for e in self.engines:
            e.tshard_finish(total)

    def fail_dup_z(self):
        with pytest.raises(np.linalg.LinAlgError):
            self.f(_dup_z(self.params))

    def stalls(self):
        return sum(int(e.lib.ffvd_stall_recoveries(e._h)) for e in self.engines)

    def close(self):
        for e in self.engines:
            e.close()


ADAM_STEPS = SGHMC_STEPS = 3


class Trainer:
    """A training trajectory on one handle: three Adam steps, three SG-HMC steps, one more Adam step (whose update reads the
    optimiser state the earlier ones left: the ABI has no getter for the moments).  The plain steps, or the one-rank native-RCCL
    sharded steps (mode train_rccl: ffvd_adam_step_allreduce / ffvd_sghmc_step_allreduce)."""

    def __init__(self, key, **over):
        cfg = CONFIGS[key]
        self.params, Y, c, self.meta = _workload(key)
        m = self.meta
        self.sh = None
        if cfg["mode"] == "train_rccl":
            from ffvd_amd.distributed import ShardedElbo
            self.sh = ShardedElbo({k: np.array(v) for k, v in self.params.items()}, Y, c, m, rank=0, world=1, mode="chains", device=0,
                                  always_reduce=True, grad=True, **dict(cfg["kw"], **over))
            self.e = self.sh.engine
        else:
            self.e = ElboEngine(m["T"], m["D"], m["C"], m["M"], m["S"], kernel_type=m["kernel_type"], U_collapse=m["U_collapse"], grad=True,
                                **dict(cfg["kw"], **over))
            self.e.set_data(Y, c)
        rng = np.random.default_rng(5)
        self.noise = [{"logvariance": rng.standard_normal(m["D"]), "log_Q": rng.standard_normal(m["D"]),
                       "Z": rng.standard_normal((m["M"], m["P"]))} for _ in range(SGHMC_STEPS)]

    def _adam(self):
        return (self.sh or self.e).adam_step(0.003)["nll"]

    def _sghmc(self, noise, burn):
        return (self.sh or self.e).sghmc_step(noise, burn_in=burn)["nll"]

    def _failed_step(self, step, fail):
        """a step on a trajectory with one NaN in X (fail = "nan") or two coincident inducing points (fail = "dupz", handles with
        jitter = 0.0): it must raise and change nothing, then the trajectory goes on from where it was"""
        e = self.e
        cur = e.get_params()
        k = "X" if fail == "nan" else "Z"
        bad = cur[k].copy()
        if fail == "nan":
            bad[-1, 7, 0] = np.nan
        else:
            bad[5] = bad[4]
        e.update_params({k: bad})
        with pytest.raises(np.linalg.LinAlgError):
            step()
        after = e.get_params()
        for n in cur:
            if n != k:
                np.testing.assert_array_equal(after[n], cur[n], err_msg="failed step moved " + n)
        np.testing.assert_array_equal(after[k], bad, err_msg="failed step moved " + k)
        e.update_params({k: cur[k]})

    def f(self, p, fail=None):
        e = self.e
        e.set_params(p)
        nlls = []
        for i in range(ADAM_STEPS):
            if fail and i == 1:
                if fail == "dupz" or self.meta["U_collapse"]:      # (explicit-U branch: no factorisation sees X, nothing reports a NaN there)
                    self._failed_step(self._adam, fail)
                e.nll_terms()                         # ... and a forward-only call and timed iterations between two steps
                e.time_elbo(2)
            nlls.append(self._adam())
        for i in range(SGHMC_STEPS):
            # (explicit-U branch: the Adam step above is its failed step.  Two equal rows of K_uu leave the pivot x - fl(x / sqrt(x))^2,
            #  which rounding makes zero, negative or a tiny positive number; with the Z this trajectory has reached here it comes out
            #  positive in both latent dims of `tiny`, the factorisation "succeeds" and nothing is reported)
            if fail and i == 1 and self.meta["U_collapse"]:
                self._failed_step(lambda: self._sghmc(self.noise[i], i < 2), fail)
            nlls.append(self._sghmc(self.noise[i], i < 2))
        nlls.append(self._adam())
        out = {"nll_steps": np.array(nlls)}
        if self.sh:                                   # the handle's staging block of ffvd_allreduce_sum (one rank: the identity)
            out["reduced"] = e.allreduce_host(np.arange(1.0, 41.0))
        out.update({"p_" + k: v for k, v in e.get_params().items()})
        return out

    def stalls(self):
        return int(self.e.lib.ffvd_stall_recoveries(self.e._h))

    def close(self):
        (self.sh or self.e).close()


def _subject(key, **over):
    mode = CONFIGS[key]["mode"]
    return (TShards if mode == "tshard" else Trainer if mode.startswith("train") else Plain)(key, **over)


def _env(monkeypatch, key, poison):
    for k in ("FFVD_NO_TINY", "FFVD_GSPLIT", "FFVD_NO_LINEAR_LOWRANK", "FFVD_WS_POISON"):
        monkeypatch.delenv(k, raising=False)
    for k, v in CONFIGS[key].get("env", {}).items():
        monkeypatch.setenv(k, v)
    if poison:
        monkeypatch.setenv("FFVD_WS_POISON", "1")


def assert_same_bits(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def assert_finite(res, what):
    for k, v in res.items():
        assert np.all(np.isfinite(v)), "%s: %s is not finite" % (what, k)


@pytest.mark.parametrize("key", IDS)
def test_poisoned_workspace_changes_nothing(key, monkeypatch):
    """The same calls on a handle created with FFVD_WS_POISON=1 and on one created without: equal bits in the 8 sums, every named term,
    nll_per_chain, every gradient array (train: the nll of every step, the parameters after the steps), all of it finite, and no
    iteration re-run after a bounded wait."""
    params = _workload(key)[0]
    p2 = _perturbed(params)
    results = []
    for poison in (False, True):
        _env(monkeypatch, key, poison)
        s = _subject(key)
        try:
            results.append([s.f(params), s.f(p2)])
            assert s.stalls() == 0
        finally:
            s.close()
    for i, name in enumerate(("f(p1)", "f(p2)")):
        assert_finite(results[0][i], key + " " + name)
        assert_same_bits(results[1][i], results[0][i], key + " poisoned " + name)


@pytest.mark.parametrize("poison", [False, True], ids=["fresh", "poisoned"])
@pytest.mark.parametrize("key", IDS)
def test_a_call_leaves_nothing_behind(key, poison, monkeypatch):
    """r1 = f(p1); then every other call the configuration allows (other parameters, a NaN in X, a forward-only call between two backward
    passes, the enqueue-only form, timed iterations); then f(p1) again: the bits of r1, and of a fresh handle's f(p1).  Where K_uu
    is positive definite without jitter the same around the coincident-inducing-points failure on handles created with jitter = 0.0.
    Training: a trajectory with a failed step (and forward-only calls) in its middle is the trajectory without them; the step fails on
    a NaN in X (collapsed branch) and, on jitter = 0.0 handles, on coincident inducing points (both branches).  Both the
    failures are numerical errors reported by return code.  `poisoned`: the handle that goes through the history starts as NaN bytes."""
    params = _workload(key)[0]
    p2 = _perturbed(params)
    mode = CONFIGS[key]["mode"]
    _env(monkeypatch, key, False)
    fresh = _subject(key)
    try:
        want = fresh.f(params)
    finally:
        fresh.close()
    assert_finite(want, key)
    _env(monkeypatch, key, poison)
    s = _subject(key)
    try:
        if mode.startswith("train"):
            assert_same_bits(s.f(params, fail="nan"), want, key + ": trajectory with a failed step")
        else:
            r1 = s.f(params)
            s.history(p2)
            again = s.f(params)
            assert_same_bits(again, r1, key + ": after the history")
            assert_same_bits(again, want, key + ": against a fresh handle")
        assert s.stalls() == 0
    finally:
        s.close()
    if not CONFIGS[key].get("dupz"):
        return
    _env(monkeypatch, key, False)
    fresh = _subject(key, jitter=0.0)
    try:
        want0 = fresh.f(params)
    finally:
        fresh.close()
    assert_finite(want0, key + " jitter 0")
    _env(monkeypatch, key, poison)
    s = _subject(key, jitter=0.0)
    try:
        if mode.startswith("train"):
            assert_same_bits(s.f(params, fail="dupz"), want0, key + ": trajectory with a step that failed on coincident inducing points")
        else:
            r1 = s.f(params)
            s.fail_dup_z()
            again = s.f(params)
            assert_same_bits(again, r1, key + ": after coincident inducing points")
            assert_same_bits(again, want0, key + ": jitter 0 against a fresh handle")
        assert s.stalls() == 0
    finally:
        s.close()
