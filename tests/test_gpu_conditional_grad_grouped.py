"""The linearised transition on the device: mean and variance of f(x, c) of G posteriors with their input gradients, explicit form
(`ffvd_op_conditional_grad_grouped`, conditionals_multi_output.conditional_grad_grouped), fused with the collapsed posteriors
(`ffvd_op_posterior_conditional_grad_grouped`, prediction.posterior_conditional_grad_grouped) and through DGPSSM.linearize.

Reference and rule.  The reference is tests/transition_grad_ref.py on the ORACLE's posterior of each group (orc.kernel_pre_cal ->
orc.collapse_u_mean_after_kernel_precalculation -> moment_ref.posterior_terms), evaluated twice: in np.float64 and in np.longdouble.
e_ref is the largest difference between the two, per array -- the reference's own rounding error, never measured on the device --
and the device must satisfy  |device - longdouble reference| <= max(4 e_ref, floor)  per array, with the project's floors taken at the
array's largest reference magnitude: 1e-11 + 1e-9 max|ref| for mean, dmean, mix_mean, mix_dmean and 1e-11 + 1e-8 max|ref| for var,
dvar, mix_var, mix_dvar.  Where np.longdouble is no wider than np.float64 e_ref is 0 and the floors alone hold.  Every error is
printed.  Mixture references are formed from the per-group references (transition_grad_ref.mixture).

Xnew is make_xnew of tests/test_gpu_conditional_grouped.py (rows near the data and rows far from it, default_rng(7)).
Shapes: tiny (M = 24, D = 2, P = 3), ragged (M = 77, D = 3, P = 5), small200 (M = 200: two column tiles, the last one ragged), m130
(K_uu at the jitter's condition number), d8 (M = 40, D = 8, P = 9); N = 37, 130 (past one row tile), 257 in passes of 128.

The fused form is held to the rule on the well-conditioned shapes.  Its posterior is formed on the device, so at m130 the distance to
a reference built on the oracle's posterior is a property of the posterior operator, which has its own tests; there, and everywhere
else, the fused call must equal bit for bit the explicit call on what collapse_u_mean_grouped returns (the same launches on the
same bits)."""
import ctypes
import functools

import numpy as np
import pytest

import moment_ref as mr
import transition_grad_ref as tg
from ffvd_amd import _lib, synthetic
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.kernels import LinearK
from ffvd_amd.prediction import posterior_conditional_grad_grouped
from oracle import ffvd_oracle as orc
from test_gpu_conditional_grouped import _group, _model, make_xnew
from test_gpu_conditional_grouped import case as cg_case, check as cg_check, refs as cg_refs, run_explicit as cg_run_explicit

pytestmark = pytest.mark.gpu

SHAPES = {"tiny": ("tiny", {}), "ragged": ("ragged", {}), "small200": ("small", dict(M=200, S=3)),
          "m130": ("tiny", dict(M=130, D=1, C=0, T=160)), "d8": ("tiny", dict(M=40, D=8, C=1))}
MODES = ("reference", "intent")
KEYS = cmo.GRAD_KEYS
GROUP_KEYS, MIX_KEYS = KEYS[:4], KEYS[4:]


def floor(key, ref):
    return 1e-11 + (1e-9 if key.endswith("mean") else 1e-8) * float(np.max(np.abs(ref)))


def rule(what, key, dev, ref64, refld):
    """|device - longdouble reference| <= max(4 x |fp64 reference - longdouble reference|, the project's floor for this array)"""
    e_new = float(np.max(np.abs(np.asarray(dev, dtype=np.longdouble) - refld)))
    e_ref = float(np.max(np.abs(np.asarray(ref64, dtype=np.longdouble) - refld)))
    bound = max(4.0 * e_ref, floor(key, ref64))
    print(f"{what}: {key}: device {e_new:.3e}, reference e_ref {e_ref:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(dev)), f"{what}: {key}"
    assert e_new <= bound, f"{what}: {key}: {e_new:.3e} > max(4 x {e_ref:.3e}, {floor(key, ref64):.3e})"


@functools.lru_cache(maxsize=None)
def case(shape, per_model, G=None):
    """case() of tests/test_gpu_conditional_grouped.py over this file's shapes: the workload's own chains under one model, or G groups
    under its seeded perturbations (default_rng(1000 + g)) with one model each."""
    name, ov = SHAPES[shape]
    if G is not None:
        ov = dict(ov, S=G)
    params, Y, c, meta = synthetic.make_named(name, **ov)
    gs = []
    for g in range(meta["S"]):
        q, X = dict(params), params["X"][g]
        if per_model:
            rng = np.random.default_rng(1000 + g)
            q["logvariance"] = params["logvariance"] + 0.05 * rng.standard_normal(params["logvariance"].shape)
            q["loglengthscales"] = params["loglengthscales"] + 0.05 * rng.standard_normal(params["loglengthscales"].shape)
            q["Z"] = params["Z"] + 0.01 * rng.standard_normal(params["Z"].shape)
            q["log_Q"] = params["log_Q"] + 0.05 * rng.standard_normal(params["log_Q"].shape)
            X = X + 0.1 * rng.standard_normal(X.shape)
        gs.append(_group(q, c, meta, X))
    return gs, c, meta, per_model


def _reference(gs, Xnew, mode, qs, dtype):
    """per group (mean, var, dmean, dvar) on the oracle's posterior with the q stacks `qs` (None: no q_sqrt), then the mixture"""
    groups = []
    for g, q in zip(gs, qs):
        beta, Gam = mr.posterior_terms(g["orc"]["L"], g["orc"]["U"], q, mode, dtype=dtype)
        groups.append(tg.linearize(Xnew, g["Z"], g["okern"], beta, Gam, dtype=dtype))
    out = {k: np.stack([grp[i] for grp in groups]) for i, k in enumerate(GROUP_KEYS)}
    out.update(zip(MIX_KEYS, tg.mixture(groups)))
    return out


@functools.lru_cache(maxsize=None)
def refs(shape, per_model, G, N, mode, with_q=True):
    """Xnew and the reference in fp64 and in longdouble; computed once per (case, N, mode), shared by the tests, never modified."""
    gs, c, meta, _ = case(shape, per_model, G)
    Xnew = make_xnew(gs[0]["X"], c, meta["T"], N)
    qs = [g["orc"]["H"] if with_q else None for g in gs]
    return dict(Xnew=Xnew, f64=_reference(gs, Xnew, mode, qs, np.float64), ld=_reference(gs, Xnew, mode, qs, np.longdouble))


def check(what, r, out, keys=KEYS):
    for k in keys:
        if out[k] is None:
            continue
        assert out[k].shape == r["f64"][k].shape, (k, out[k].shape)
        rule(what, k, out[k], r["f64"][k], r["ld"][k])


def _models(cs, sel=None):
    gs, c, meta, per_model = cs
    sel = gs if sel is None else sel
    if per_model:
        return [g["Z"] for g in sel], [g["kern"] for g in sel]
    return gs[0]["Z"], gs[0]["kern"]


def run_explicit(cs, Xnew, mode, src="orc", with_q=True, groups=None, qs=None, **kw):
    gs, c, meta, per_model = cs
    sel = gs if groups is None else [gs[i] for i in groups]
    Zs, kerns = _models(cs, sel)
    Ls = [g[src]["L"] for g in sel] if per_model else gs[0][src]["L"]
    if qs is None:
        qs = [g[src]["H"] for g in sel] if with_q else None
    return cmo.conditional_grad_grouped(Ls, Zs, kerns, [g[src]["U"] for g in sel], qs, Xnew, q_mode=mode, **kw)


def run_fused(cs, Xnew, mode, **kw):
    gs, c, meta, _ = cs
    Zs, kerns = _models(cs)
    return posterior_conditional_grad_grouped(Zs, kerns, [g["X"] for g in gs], [g["Q"] for g in gs], c, Xnew, q_mode=mode, **kw)


def same(a, b, keys=KEYS):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# the smallest shapes at which the kernels can go wrong: one tile with everything ragged; two row tiles; two column tiles with a
# ragged last one; the ill-conditioned K_uu; P = 9 (the 32-wide mean kernel, two rounds of the epilogue); one model per group
CASES = [("tiny", False, None, 37), ("ragged", False, None, 130), ("small200", False, None, 130), ("m130", False, None, 37),
         ("d8", False, None, 37), ("tiny", True, 5, 37), ("ragged", True, 5, 130)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G,N", CASES, ids=lambda v: str(v))
def test_explicit_form_against_the_reference(shape, per_model, G, N, mode):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, N, mode)
    out = run_explicit(cs, r["Xnew"], mode)
    assert set(out) == set(KEYS) and np.all(out["var"] > 0)
    check(f"{shape} N={N} {mode} explicit", r, out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,per_model,G,N", [c for c in CASES if c[0] != "m130"], ids=lambda v: str(v))
def test_fused_form_against_the_reference(shape, per_model, G, N, mode):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, N, mode)
    out = run_fused(cs, r["Xnew"], mode, return_U=True)
    assert out["U_means"].shape == (len(cs[0]), cs[2]["M"], cs[2]["D"])
    check(f"{shape} N={N} {mode} fused", r, out)


@pytest.mark.parametrize("shape,per_model,G,N", [("m130", False, None, 37), ("small200", False, None, 130), ("tiny", True, 5, 37)],
                         ids=lambda v: str(v))
def test_fused_form_equals_the_explicit_form_on_the_device_posterior(shape, per_model, G, N):
    cs = case(shape, per_model, G)
    gs, c, meta, _ = cs
    Xnew = make_xnew(gs[0]["X"], c, meta["T"], N)
    Zs, kerns = _models(cs)
    U, Hinv, Lm = cmo.collapse_u_mean_grouped(Zs, kerns, [g["X"] for g in gs], c, [g["Q"] for g in gs])
    Ls = [list(Lm[m]) for m in range(len(gs))] if per_model else list(Lm[0])
    for mode in MODES:
        fused = run_fused(cs, Xnew, mode, return_U=True)
        np.testing.assert_array_equal(fused["U_means"], U)
        same(fused, cmo.conditional_grad_grouped(Ls, Zs, kerns, list(U), list(Hinv), Xnew, q_mode=mode))


@pytest.mark.parametrize("shape,per_model,G,N", [("tiny", False, None, 37), ("ragged", True, 5, 130)], ids=lambda v: str(v))
def test_explicit_u_without_q_sqrt(shape, per_model, G, N):
    cs, r = case(shape, per_model, G), refs(shape, per_model, G, N, "reference", False)
    out = run_explicit(cs, r["Xnew"], "reference", with_q=False)
    check(f"{shape} no q_sqrt", r, out)
    assert np.max(np.abs(refs(shape, per_model, G, N, "reference")["f64"]["dvar"] - r["f64"]["dvar"])) > 1e-6
    if not per_model:           # one model, no q: Gamma = W W^T is formed once and the variance side does not depend on the group
        for g in range(1, len(cs[0])):
            np.testing.assert_array_equal(out["var"][g], out["var"][0])
            np.testing.assert_array_equal(out["dvar"][g], out["dvar"][0])
        assert np.max(np.abs(out["dmean"][1] - out["dmean"][0])) > 1e-6


@pytest.mark.parametrize("mode", MODES)
def test_a_dense_q_slice(mode):
    """an upper-triangular slice plus a seeded strict lower part: Gamma = W (I - q q^T) W^T with a q that is not triangular"""
    cs = case("ragged", False)
    gs, c, meta, _ = cs
    M, D = meta["M"], meta["D"]
    Xnew, rng = refs("ragged", False, None, 130, mode)["Xnew"], np.random.default_rng(21)
    dense = [g["orc"]["H"] + 0.01 * np.tril(rng.standard_normal((D, M, M)), -1) for g in gs]
    r = dict(f64=_reference(gs, Xnew, mode, dense, np.float64), ld=_reference(gs, Xnew, mode, dense, np.longdouble))
    check(f"dense q, {mode}", r, run_explicit(cs, Xnew, mode, qs=dense))
    tri = refs("ragged", False, None, 130, mode)["f64"]
    assert np.max(np.abs(r["f64"]["dvar"] - tri["dvar"])) > 1e-6 * np.max(np.abs(tri["dvar"]))           # the lower part is seen


def test_the_two_q_modes_agree_on_dim_0_and_differ_elsewhere():
    cs = case("tiny", False)
    Xnew = refs("tiny", False, None, 37, "reference")["Xnew"]
    a, b = run_explicit(cs, Xnew, "reference"), run_explicit(cs, Xnew, "intent")
    for k in ("mean", "dmean", "mix_mean", "mix_dmean"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["var"][:, :, 0], b["var"][:, :, 0])
    np.testing.assert_array_equal(a["dvar"][:, :, 0], b["dvar"][:, :, 0])
    assert np.max(np.abs(a["dvar"][:, :, 1:] - b["dvar"][:, :, 1:])) > 1e-4


@pytest.mark.parametrize("shape,per_model,N", [("tiny", True, 37), ("small200", False, 130), ("d8", False, 37)])
def test_a_group_alone_equals_the_group_among_the_others(shape, per_model, N):
    G = 5 if per_model else None
    cs = case(shape, per_model, G)
    gs, c, meta, _ = cs
    Xnew = make_xnew(gs[0]["X"], c, meta["T"], N)
    for mode in MODES:
        out = run_explicit(cs, Xnew, mode, summary=False)
        for g in range(len(gs)):
            one = run_explicit(cs, Xnew, mode, groups=[g], summary=False)
            for k in GROUP_KEYS:
                np.testing.assert_array_equal(one[k][0], out[k][g], err_msg=f"{k} group {g}")


@pytest.mark.parametrize("form", ["explicit", "fused"])
def test_three_row_passes_equal_one_pass_bit_for_bit(form):
    """N = 257 in passes of 128, 128 and 1 rows"""
    cs, r = case("small200", False), refs("small200", False, None, 257, "intent")
    run = run_explicit if form == "explicit" else run_fused
    one, three = run(cs, r["Xnew"], "intent"), run(cs, r["Xnew"], "intent", rows_per_pass=128)
    check(f"small200 N=257 intent {form} passes of 128", r, three)
    same(one, three)


def test_a_row_does_not_depend_on_the_other_rows():
    """rows 0..36 of the N = 130 call equal the N = 37 call on those rows (one row tile against two, other padding)"""
    cs = case("ragged", False)
    X130 = refs("ragged", False, None, 130, "reference")["Xnew"]
    big, small = run_explicit(cs, X130, "reference"), run_explicit(cs, np.ascontiguousarray(X130[:37]), "reference")
    for k in GROUP_KEYS:
        np.testing.assert_array_equal(big[k][:, :37], small[k], err_msg=k)
    for k in MIX_KEYS:
        np.testing.assert_array_equal(big[k][:37], small[k], err_msg=k)


def test_unrequested_outputs_change_nothing_in_the_others():
    cs, r = case("ragged", False), refs("ragged", False, None, 130, "reference")
    full = run_explicit(cs, r["Xnew"], "reference")
    only_groups, only_mix = run_explicit(cs, r["Xnew"], "reference", summary=False), run_explicit(cs, r["Xnew"], "reference", per_group=False)
    mean_only = run_explicit(cs, r["Xnew"], "reference", summary=False, variance=False)
    assert all(only_groups[k] is None for k in MIX_KEYS) and all(only_mix[k] is None for k in GROUP_KEYS)
    assert all(mean_only[k] is None for k in KEYS if k not in ("mean", "dmean"))
    same(only_groups, full, GROUP_KEYS)
    same(only_mix, full, MIX_KEYS)
    same(mean_only, full, ("mean", "dmean"))


@pytest.mark.parametrize("shape,N", [("tiny", 37), ("ragged", 130)])
def test_values_and_differences_of_the_existing_value_path(shape, N):
    """mean / var of the new call obey the rule of tests/test_gpu_conditional_grouped.py (the oracle's conditional as reference, the
    one-group device operator as yardstick), and central differences of the EXISTING conditional_grouped at h = 2^-8 and 2^-9 differ
    from the new dmean / dvar by errors whose ratio lies in [3.5, 4.5]: second-order convergence towards the new gradients.  At these
    two shapes the device's own value error (at most 3e-12) times 1 / h is below 2 % of the truncation error."""
    cs, r = cg_case(shape, False), cg_refs(shape, False, None, N, "intent")
    Xnew = r["Xnew"]
    out = run_explicit(cs, Xnew, "intent")
    cg_check(f"{shape} values of the new call", r, "dev_explicit", out["mean"], out["var"], out["mix_mean"], out["mix_var"])
    errs = {"dmean": [], "dvar": []}
    for k in (8, 9):
        h = 2.0 ** -k
        fn = lambda X: cg_run_explicit(cs, np.ascontiguousarray(X), "intent", summary=False)[:2]
        fm, fv = tg.central_differences(fn, Xnew, h)
        errs["dmean"].append(float(np.max(np.abs(fm - out["dmean"]))))
        errs["dvar"].append(float(np.max(np.abs(fv - out["dvar"]))))
    for key, (e8, e9) in errs.items():
        print(f"{shape}: {key}: central-difference error {e8:.3e} (h = 2^-8), {e9:.3e} (h = 2^-9), ratio {e8 / e9:.3f}")
        assert 3.5 <= e8 / e9 <= 4.5, (key, e8, e9)


@pytest.mark.parametrize("mode", MODES)
def test_linearize_of_a_collapsed_model(mode):
    params, Y, c, meta = synthetic.make_named("tiny", S=3)
    r, D = refs("tiny", False, None, 37, mode), meta["D"]
    mod = _model(params, Y, c, meta, 3, True)
    mod.set_X(params["X"])
    out = mod.linearize(r["Xnew"], q_mode=mode)
    assert set(out) == set(KEYS) | {"A", "B", "mix_A", "mix_B"}
    assert out["A"].shape == (3, 37, D, D) and out["B"].shape == (3, 37, D, meta["P"] - D)
    assert out["mix_A"].shape == (37, D, D) and out["mix_B"].shape == (37, D, meta["P"] - D)
    check(f"linearize {mode}", r, out)
    _check_ab(out, D)
    pooled = mod.linearize(r["Xnew"], q_mode=mode, per_chain=False)
    assert all(pooled[k] is None for k in GROUP_KEYS + ("A", "B"))
    same(pooled, out, MIX_KEYS + ("mix_A", "mix_B"))
    tr = mod.predict_transition(r["Xnew"], q_mode=mode)
    cg_check(f"linearize {mode} against predict_transition's rule", cg_refs("tiny", False, None, 37, mode), "dev_fused", out["mean"],
             out["var"], out["mix_mean"], out["mix_var"])
    assert np.max(np.abs(tr["mean"] - out["mean"])) < 1e-9


def _check_ab(out, D):
    """A = I + dmean[..., :D] and B = dmean[..., D:], bit for bit.  A - I gives dmean's bits back off the diagonal; on the diagonal
    1 + x is rounded to the spacing of doubles near A and the subtraction may round once more: two half-spacings, 2^-52 max(1, |A|)."""
    for a_key, b_key, key in (("A", "B", "dmean"), ("mix_A", "mix_B", "mix_dmean")):
        A, B, dm = out[a_key], out[b_key], out[key]
        np.testing.assert_array_equal(A, np.eye(D) + dm[..., :D])
        np.testing.assert_array_equal(B, dm[..., D:])
        off = ~np.eye(D, dtype=bool)
        np.testing.assert_array_equal((A - np.eye(D))[..., off], dm[..., :D][..., off])
        assert np.max(np.abs((A - np.eye(D)) - dm[..., :D])) <= 2.0 ** -52 * max(1.0, float(np.max(np.abs(A))))


def test_linearize_of_an_explicit_u_model():
    """one group, whatever the number of chains: f does not depend on X; no q_sqrt term"""
    params, Y, c, meta = synthetic.make_named("tiny", S=3)
    Xnew, D = make_xnew(params["X"][0], c, meta["T"], 37), meta["D"]
    mod = _model(params, Y, c, meta, 3, False)
    out = mod.linearize(Xnew)
    assert out["mean"].shape == (1, 37, D) and out["dvar"].shape == (1, 37, D, meta["P"]) and out["A"].shape == (1, 37, D, D)
    okern = orc.make_kernels(params, kernel_type=meta["kernel_type"])
    g = dict(Z=params["Z"], okern=okern, orc=dict(L=list(orc.kernel_pre_cal(params["Z"], okern)), U=params["U"]))
    r = dict(f64=_reference([g], Xnew, "reference", [None], np.float64), ld=_reference([g], Xnew, "reference", [None], np.longdouble))
    check("explicit-U model", r, out)
    _check_ab(out, D)


def _abi_call(kind, G, M, D, P, N):
    """ffvd_op_conditional_grad_grouped on one-double stand-ins: only the scalar checks may run"""
    lib = _lib.load()
    z = np.zeros(1)
    p, t = _lib.dptr(z), (ctypes.c_void_p * 1)(z.ctypes.data)
    rc = lib.ffvd_op_conditional_grad_grouped(kind, G, 1, t, p, M, P, D, p, p, p, None, 0, p, N, 0, p, p, p, p, None, None, None, None)
    return rc, lib.ffvd_last_error(None), z


def test_linear_kernel_and_oversized_requests_are_rejected_and_no_rows_is_ok():
    rc, msg, z = _abi_call(1, 2, 4, 2, 3, 5)
    assert rc == _lib.FFVD_EINVAL and b"SE kernel only" in msg and z[0] == 0.0
    rc, msg, z = _abi_call(0, 2, 1, 1, 2, 1 << 29)                      # G * D * N * P = 2^31, G * N * D = 2^30
    assert rc == _lib.FFVD_EINVAL and b"bad argument" in msg and z[0] == 0.0
    rc, msg, z = _abi_call(0, 2, 4, 2, 3, 0)
    assert rc == _lib.FFVD_OK and z[0] == 0.0
    cs = case("tiny", False)
    gs, c, meta, _ = cs
    with pytest.raises(ValueError, match="SE kernel only"):
        cmo.conditional_grad_grouped(gs[0]["orc"]["L"], gs[0]["Z"], [LinearK(meta["P"], variance=0.1) for _ in range(meta["D"])],
                                     [g["orc"]["U"] for g in gs], None, np.zeros((3, meta["P"])))
    empty = run_explicit(cs, np.zeros((0, meta["P"])), "reference")
    assert empty["dmean"].shape == (len(gs), 0, meta["D"], meta["P"]) and empty["mix_dvar"].shape == (0, meta["D"], meta["P"])
