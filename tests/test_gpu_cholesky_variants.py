"""The three implementations of the batched Cholesky, each FORCED (FFVD_CHOL=right|left|flow) and checked against an
extended-precision reference (tests/cholesky_ref.py; tests/test_cholesky_ref.py shows on the CPU what the criterion can tell apart):

  right  potrf_panel_kernel / potrf_trail_kernel<PIPE>     two launches per block step
  left   potrf_ll_kernel<PIPE>                             one launch per block column; what stall recovery and n > 4096 fall back to
  flow   potrf_df_kernel                                   one launch per batch

FFVD_CHOL is read once per process, so every variant runs in ONE child process that makes all its calls and stores every factor,
info, return code, message and wall time; the parent builds the same seeded inputs and does all the checking.  A fourth child
without FFVD_CHOL pins the automatic choice (batch >= 32: flow, below: right) bit for bit against the forced ones.

Accuracy, all three variants at every (n, batch):

  n = 1, 16, 17, 63, 64, 65; batch 3    the 16-wide sub-block and 64-wide block edges; flow below 8 matrices (padding workgroups)
  n = 130, batch 6                      three block rows, identity padding to 192; condition up to 1e10: the refinement step of the
                                        panel substitution (multiplication by inverted 16 x 16 sub-blocks) is what keeps these within
                                        the bound; rows and columns scaled by 2^-200 ... 2^200
  n = 200, batch 6; n = 320, batch 2    four and five block rows
  n = 130, batch 33                     4 * 8 + 1 matrices
  n = 320, batch 52                     260 block rows in the flow launch (not the fine mode, still one per compute unit); more than 512
                                        trailing tiles: potrf_trail_kernel<false>
  n = 130, batch 257                    potrf_ll_kernel<false> (more than 512 row blocks), potrf_trail_kernel<false>, 33 x 8 matrices

Criterion per matrix: return code 0, info 0, an exactly zero strict upper triangle, a positive diagonal, and on the lower triangle
|A - L L^T| <= max(4 omega_LAPACK(A), 4 u) |L||L|^T in long double (cholesky_ref has the definition and the reasons for the factors).
Then: what is not positive definite is reported with the first bad pivot by every variant, a bad matrix spoils no neighbour and makes
no block row of the flow launch wait; the strict upper triangle of the input is ignored, L may alias A, a repeated call repeats its
bits; kernel_pre_cal (identity rows riding through the factorisation) under every variant."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cholesky_ref as cr
from ffvd_amd import _lib
from ffvd_amd import conditionals_multi_output as cmo
from oracle import ffvd_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("right", "left", "flow")
EPS = np.finfo(np.float64).eps
KPC = {"right": ((100, 2), (130, 2)), "left": ((100, 2), (130, 2)), "flow": ((100, 2), (130, 2)),
       "auto": ((100, 2), (130, 2), (70, 33))}                # (M, kernels); 33 kernels: the flow launch by batch size

_CHILD = r"""
import sys, time
import numpy as np
import cholesky_ref as cr
from ffvd_amd import _lib
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.kernels import SquaredExponential

lib = _lib.load()
out = {}


def chol(key, A, alias=False, with_info=True):
    src = np.array(A, dtype=np.float64, order="C")
    batch, n = src.shape[0], src.shape[1]
    L = src if alias else np.full_like(src, np.nan)
    info = np.full(batch, -7, dtype=np.int32)
    ip = info.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)) if with_info else None
    t0 = time.perf_counter()
    rc = lib.ffvd_op_cholesky(_lib.dptr(src), n, batch, _lib.dptr(L), ip)
    el = time.perf_counter() - t0
    out[key + ".L"], out[key + ".info"], out[key + ".rc"], out[key + ".time"] = L, info, np.int64(rc), np.float64(el)
    out[key + ".msg"] = np.str_(lib.ffvd_last_error(None).decode())


full = sys.argv[2] == "full"
if full:
    for fam, n, batch in cr.accuracy_keys():
        chol(f"acc_{fam}_{n}_{batch}", cr.stack(fam, n, batch))
    good40, bad40, info40, good7, bad7, info7 = cr.nonpd_batches()
    chol("warm40", good40)                  # a good call of the same shape first: the bad call's time is the factorisation's
    chol("bad40", bad40)
    chol("warm7", good7)
    chol("bad7", bad7)
    chol("bad7_noinfo", bad7, with_info=False)
    A = cr.stack("K5", 130, 3)
    chol("clean", A)
    U = np.array(A)
    U[:, np.triu_indices(130, 1)[0], np.triu_indices(130, 1)[1]] = np.nan
    chol("nanupper", U)
    chol("alias", A, alias=True)
    chol("repeat", A)
chol("disp31", cr.stack("K5", 130, 31))
chol("disp32", cr.stack("K5", 130, 32))
for spec in sys.argv[3].split(","):
    M, nk = (int(v) for v in spec.split("x"))
    Z, logvar, loglen = cr.kpc_inputs(M, nk)
    kern = [SquaredExponential(Z.shape[1], variance=np.exp(logvar[d]), lengthscales=np.exp(loglen[d])) for d in range(nk)]
    out[f"kpc_{M}_{nk}"] = np.stack(cmo.kernel_pre_cal(Z, kern))
np.savez(sys.argv[1], **out)
"""

_done = {}            # variant -> dict of arrays, or the text a failed child left
_dead = []            # a child that ended by signal or at its time limit: no further child is started


def child(variant):
    """Everything the child of `variant` ("right", "left", "flow", or "auto": FFVD_CHOL unset) computed.  One child per variant and
    module, strictly one after another."""
    if variant not in _done:
        if _dead:
            pytest.fail(f"not started: the {_dead[0][0]} child ended abnormally\n{_dead[0][1]}")
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
        for k in ("FFVD_CHOL", "FFVD_DF_FINE", "FFVD_DF_DEFER"):
            env.pop(k, None)
        if variant != "auto":
            env["FFVD_CHOL"] = variant
        tmp = tempfile.mkdtemp(prefix="ffvd_chol_")
        path = os.path.join(tmp, variant + ".npz")
        spec = ",".join(f"{m}x{k}" for m, k in KPC[variant])
        try:
            try:
                run = subprocess.run([sys.executable, "-c", _CHILD, path, "dispatch" if variant == "auto" else "full", spec],
                                     env=env, capture_output=True, text=True, timeout=240)
            except subprocess.TimeoutExpired as e:
                tail = (e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or ""))[-2000:]
                _dead.append((variant, "time limit of 240 s\n" + tail))
                _done[variant] = _dead[0][1]
            else:
                if run.returncode < 0:
                    _dead.append((variant, f"signal {-run.returncode}\n{run.stderr[-2000:]}"))
                    _done[variant] = _dead[0][1]
                elif run.returncode != 0:
                    _done[variant] = f"exit status {run.returncode}\n{run.stderr[-2000:]}"
                else:
                    with np.load(path, allow_pickle=False) as z:
                        _done[variant] = {k: z[k] for k in z.files}
        finally:
            if os.path.exists(path):
                os.remove(path)
            os.rmdir(tmp)
    got = _done[variant]
    if not isinstance(got, dict):
        pytest.fail(f"the {variant} child failed: {got}")
    return got


def call(variant, key):
    z = child(variant)
    return {f: z[f"{key}.{f}"] for f in ("L", "info", "rc", "time", "msg")}


# ------------------------------------------------------------------------------------------------------------------------------
# the accuracy criterion
# ------------------------------------------------------------------------------------------------------------------------------
def check_factors(variant, fam, n, A, L, seeds_of, subset, what=""):
    """Every L[b] against A[b]: structure, then the backward-error criterion -- in long double for b in `subset`, for the others the
    same inequality in fp64 with the bound enlarged by gamma_n (the evaluation's own rounding) and omega_LAPACK the largest of the
    subset.  Returns the worst omega_GPU / omega_LAPACK of the subset."""
    batch = A.shape[0]
    iu = np.triu_indices(n, 1)
    worst = 0.0
    for b in range(batch):
        tag = f"{what}variant {variant}, family {fam}, n {n}, b {b}"
        assert np.all(L[b][iu] == 0.0), f"{tag}: the strict upper triangle is not exactly zero"
        assert np.all(np.diagonal(L[b]) > 0.0), f"{tag}: diagonal not positive"
    w_sub = {b: cr.lapack_omega(fam, n, seeds_of[b]) for b in subset}
    for b in subset:
        R, S = cr.residual(A[b], L[b])
        ratio = cr.omega_of(R, S) / w_sub[b] if w_sub[b] > 0 else cr.omega_of(R, S) / cr.U
        unit = "omega_LAPACK" if w_sub[b] > 0 else "u (LAPACK's factor is exact)"
        worst = max(worst, ratio if w_sub[b] > 0 else 0.0)
        assert cr.within(R, S, cr.bound_for(w_sub[b])), \
            f"{what}variant {variant}, family {fam}, n {n}, b {b}: omega_GPU = {ratio:.3g} {unit}, bound max(4 omega_LAPACK, 4 u)"
    rest = [b for b in range(batch) if b not in w_sub]
    if rest:
        bound = cr.bound_for(max(w_sub.values())) + cr.gamma(n)
        Lr, Ar = L[rest], A[rest]
        R = np.abs(np.tril(Ar - Lr @ np.swapaxes(Lr, 1, 2)))
        S = np.tril(np.abs(Lr) @ np.swapaxes(np.abs(Lr), 1, 2))
        ok = np.all(R <= bound * S, axis=(1, 2))
        for i in np.flatnonzero(~ok):
            ratio = cr.omega_of(R[i], S[i]) / max(w_sub.values())
            pytest.fail(f"{what}variant {variant}, family {fam}, n {n}, b {rest[i]}: omega_GPU (fp64 evaluation) = {ratio:.3g} x the "
                        f"largest omega_LAPACK of the long double subset; bound 4 omega_LAPACK + gamma_n")
    return worst


@pytest.mark.parametrize("fam,n,batch", cr.accuracy_keys(), ids=lambda v: str(v))
@pytest.mark.parametrize("variant", VARIANTS)
def test_factor_within_four_times_lapacks_backward_error(variant, fam, n, batch):
    got = call(variant, f"acc_{fam}_{n}_{batch}")
    assert int(got["rc"]) == 0 and not got["info"].any(), (variant, fam, n, int(got["rc"]), got["info"], str(got["msg"]))
    assert "gave up" not in str(got["msg"])                      # no silent stall recovery
    worst = check_factors(variant, fam, n, cr.stack(fam, n, batch), got["L"], cr.seeds(n, batch), cr.extended_subset(n, batch))
    print(f"omega_GPU / omega_LAPACK: variant {variant} family {fam} n {n} batch {batch} worst {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# matrices that are not positive definite
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_first_bad_pivot_is_reported_and_neighbours_are_untouched(variant):
    """Seven bad matrices in a batch of 40 (n = 130: three block rows, 62 rows of padding): a negative Schur pivot at 0, 63 (end of a
    block), 64 (start of the next) and 129 (the last real row), an exactly zero pivot at 15, a NaN pivot at 16 (first of a 16-wide
    sub-block), +inf below the diagonal -- the dataflow kernel's blocked diagonal factor detects these otherwise than the one-wavefront
    factor of the other two variants, and writes info from several workgroups of a matrix."""
    good40, bad40, info40, good7, bad7, info7 = cr.nonpd_batches()
    got = call(variant, "bad40")
    assert int(got["rc"]) == _lib.FFVD_ENOTPD, (int(got["rc"]), str(got["msg"]))
    assert "matrix 1 " in str(got["msg"]) and "pivot 0)" in str(got["msg"]), str(got["msg"])
    assert np.array_equal(got["info"], info40), (variant, got["info"])
    good = np.flatnonzero(info40 == 0)
    sd = cr.seeds(cr.NONPD_N, cr.NONPD_BATCH)
    check_factors(variant, "W", cr.NONPD_N, good40[good], got["L"][good], [sd[b] for b in good], list(range(len(good))),
                  what="beside bad matrices: ")
    warm = call(variant, "warm40")
    assert int(warm["rc"]) == 0 and not warm["info"].any()
    assert np.array_equal(warm["L"][good], got["L"][good])        # ... and the very bits of the all-good batch
    # the same seven alone: bad at every b
    got7 = call(variant, "bad7")
    assert int(got7["rc"]) == _lib.FFVD_ENOTPD and "matrix 0 " in str(got7["msg"]), (int(got7["rc"]), str(got7["msg"]))
    assert np.array_equal(got7["info"], info7), (variant, got7["info"])
    assert int(call(variant, "warm7")["rc"]) == 0 and not call(variant, "warm7")["info"].any()
    noinfo = call(variant, "bad7_noinfo")                         # info = NULL
    assert int(noinfo["rc"]) == _lib.FFVD_ENOTPD and np.all(noinfo["info"] == -7)
    for g in (got, got7, noinfo):
        assert "gave up" not in str(g["msg"])
    if variant == "flow":
        # every wait of the dataflow launch is bounded by 1 s (DF_SPIN_TICKS at 100 MHz): a launch in which a bad pivot made rows wait
        # cannot end sooner, and stall recovery would then hide it behind a correct result
        for g in (got, got7, noinfo):
            assert float(g["time"]) < 1.0, float(g["time"])


# ------------------------------------------------------------------------------------------------------------------------------
# the contract of ffvd_op_cholesky
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_upper_triangle_ignored_aliasing_and_repeatability(variant):
    clean = call(variant, "clean")
    assert int(clean["rc"]) == 0 and not clean["info"].any() and np.all(np.isfinite(clean["L"]))
    for other in ("nanupper", "alias", "repeat"):
        got = call(variant, other)
        assert int(got["rc"]) == 0, (other, int(got["rc"]), str(got["msg"]))
        assert np.array_equal(got["info"], clean["info"]), other
        assert np.array_equal(got["L"], clean["L"]), f"{variant}: '{other}' differs from the clean call"


# ------------------------------------------------------------------------------------------------------------------------------
# identity rows riding through the factorisation
# ------------------------------------------------------------------------------------------------------------------------------
KPC_CASES = [(v, m, k) for v in VARIANTS + ("auto",) for m, k in KPC[v]]


@pytest.mark.parametrize("variant,M,nk", KPC_CASES, ids=lambda v: str(v))
def test_kernel_pre_cal_under_every_variant(variant, M, nk):
    """The criteria of test_gpu_predict_shapes.test_kernel_pre_cal_at_large_m, unchanged, at M = 100 and 130 (two and three block rows,
    padded) under each variant, and with 33 kernels (the dataflow launch by batch size, identity rows in it) at M = 70."""
    W = child(variant)[f"kpc_{M}_{nk}"]
    Z, logvar, loglen = cr.kpc_inputs(M, nk)
    okern = [orc.SquaredExponential(logvar[d], loglen[d]) for d in range(nk)]
    ref = orc.kernel_pre_cal(Z, okern)
    assert W.shape == (nk, M, M)
    for d in range(nk):
        A = okern[d].K(Z) + cmo.JITTER * np.eye(M)
        ev = np.linalg.eigvalsh(A)
        kappa = ev[-1] / ev[0]
        assert np.all(np.tril(W[d], -1) == 0.0)
        res = np.abs(W[d].T @ A @ W[d] - np.eye(M)).max()
        assert res < 4 * EPS * kappa, (variant, d, res, kappa)
        rel = np.abs(W[d] - ref[d]).max() / np.abs(ref[d]).max()
        assert rel < 4 * EPS * kappa, (variant, d, rel, kappa)


# ------------------------------------------------------------------------------------------------------------------------------
# the automatic choice
# ------------------------------------------------------------------------------------------------------------------------------
def test_automatic_choice_is_right_looking_below_32_matrices_and_dataflow_from_32():
    """chol_variant: batch >= 32 takes the dataflow launch, fewer the right-looking launches; and each variant gives the same bits in
    another process."""
    for key, forced in (("disp31", "right"), ("disp32", "flow")):
        auto, ref = call("auto", key), call(forced, key)
        assert int(auto["rc"]) == 0 and int(ref["rc"]) == 0 and not auto["info"].any() and not ref["info"].any()
        assert np.array_equal(auto["L"], ref["L"]), f"{key}: the automatic choice is not bit-identical to FFVD_CHOL={forced}"
