"""The child process of tests/test_gpu_cache_poison.py: every `ffvd_op_*` entry point that takes device scratch, called through the
Python layer on fixtures the GPU test modules build, the whole list once forwards and once in reverse order (a cached block is
reused by a request within 4 x of its size: reversing makes blocks change hands between different operators).

`python cache_poison_script.py OUT.npz` writes every output array under "<pass>/<call>/<key>", and under "called/<call>" the entry
points the library really saw during that call.  CALLS is read on the CPU too (tests/test_history_coverage.py): importing this module
touches neither the library nor the device; the fixtures are built inside the functions.
"""
import functools
import sys

import numpy as np

# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """A particle fixture (tests/particle_fixtures.py: groups with the oracle's posterior, records with gaps and lengths, emission, draws)
    plus `c`, the control rows of the posterior, and the case's name."""
    import particle_fixtures as fxt
    from ffvd_amd import synthetic
    from test_gpu_filter_grouped import CASES
    from test_gpu_moment_grouped import case
    if name == "m300":       # M = 300, T = 320: the ragged last column tile
        fx, c = fxt.edge_m300(), synthetic.make_named("tiny", M=300, T=320, S=2)[2]
    else:
        args = {"ragged": CASES[2], "m130": CASES[4], "d8": CASES[5]}[name]
        fx, c = fxt.case_fixture(*args), case(*args[:3])[1]
    T = fx["gs"][0]["X"].shape[0] - 1
    return dict(fx, c=np.ascontiguousarray(c[:T]), T=T, name=name)


def _with_particles(fx, n, seed):
    """the fixture with n particles per track (13 leaves the 8-particle slab ragged; 64 fills it)"""
    import particle_fixtures as fxt
    G, R, steps = fx["eps"].shape[:3]
    return dict(fx, **fxt.draws(seed, G, R, steps, n, fx["x0"].shape[-1], fx["S0"] is not None))


def _with_forecast(fx, h, origins, seed):
    """record 0 alone, with the forecast draws of `origins`"""
    import forecast_particle_fixtures as fpx
    import particle_fixtures as fxt
    return fpx._with_forecast(fxt.subset(fx, recs=[0]), h, origins, seed)


def _models(fx, src="orc"):
    gs = fx["gs"]
    if fx["per_model"]:
        return [g[src]["L"] for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs], [g[src]["U"] for g in gs], fx["qs"]
    return gs[0][src]["L"], gs[0]["Z"], gs[0]["kern"], [g[src]["U"] for g in gs], fx["qs"]


def _fused(fx):
    gs = fx["gs"]
    Zs, kerns = ([g["Z"] for g in gs], [g["kern"] for g in gs]) if fx["per_model"] else (gs[0]["Z"], gs[0]["kern"])
    return Zs, kerns, [g["X"] for g in gs], [g["Q"] for g in gs]


def _Qs(fx):
    return [g["Q"] for g in fx["gs"]]


def _one(x):
    return None if x is None else x[:, 0]


def _ctrl_all(fx):
    """posterior rows [0, T) followed by record 0's rows: the control_inputs of a fused single-sequence call (ctrl_offset = T)"""
    return fx["c"] if fx["ctrl"] is None else np.concatenate((fx["c"], fx["ctrl"][0]), axis=0)


def _targets(fx, n):
    """held-out targets of a summary: the first n rows of record 0, its unobserved entries filled in (the summaries take no gaps)"""
    return np.nan_to_num(fx["Y"][0][:n])


def _records_meta(fx):
    """what says where a records filter documents NaN: the records' lengths and their observations (NaN = unobserved)"""
    return dict(lengths=np.asarray(fx["lengths"]), Y=np.asarray(fx["Y"]))


def _rpp(fx):
    """records per pass: more than one pass, and with three records a last pass that is not full"""
    return 2 if fx["Y"].shape[0] > 2 else 1


def _xnew(fx, N):
    from test_gpu_conditional_grouped import make_xnew
    return make_xnew(fx["gs"][0]["X"], fx["c"], fx["T"], N)


# ---- the calls --------------------------------------------------------------------------------------------------------------------------
FIXTURES = ("ragged", "m130", "d8", "m300")
CALLS = []          # (label, entry points the call must reach, function of no arguments returning arrays)


def call(label, *symbols):
    def deco(fn):
        CALLS.append((label, symbols, fn))
        return fn
    return deco


def _single(name):
    """group 0 of a fixture as the one-group operators take it"""
    fx = _fixture(name)
    g = fx["gs"][0]
    X = g["X"]
    return fx, g, X, np.concatenate((X[:-1], fx["c"]), axis=1)


for _name in FIXTURES:
    @call("kernels " + _name, "ffvd_op_kernel_matrix", "ffvd_op_kernel_diag")
    def _kernels(name=_name):
        fx, g, X, xc = _single(name)
        return [(k.K(g["Z"]), k.K(xc, g["Z"]), k.Kdiag(xc)) for k in g["kern"]]

    @call("cholesky trsm " + _name, "ffvd_op_cholesky", "ffvd_op_trsm")
    def _chol(name=_name):
        from ffvd_amd import _lib
        fx, g, X, xc = _single(name)
        lib, M = _lib.load(), g["Z"].shape[0]
        A = np.ascontiguousarray(np.stack([k.K(g["Z"]) + 1e-5 * np.eye(M) for k in g["kern"]]))
        L, info = np.empty_like(A), np.zeros(len(A), dtype=np.int32)
        assert lib.ffvd_op_cholesky(_lib.dptr(A), M, len(A), _lib.dptr(L), info.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))) == 0
        B = np.ascontiguousarray(g["kern"][0].K(g["Z"], xc[:37]))
        Xs = np.empty_like(B)
        assert lib.ffvd_op_trsm(_lib.dptr(np.ascontiguousarray(L[0])), M, _lib.dptr(B), B.shape[1], _lib.dptr(Xs)) == 0
        return np.tril(L), info, Xs

    @call("posterior " + _name, "ffvd_op_kernel_pre_cal", "ffvd_op_collapse", "ffvd_op_collapse_u_mean")
    def _posterior(name=_name):
        from ffvd_amd import conditionals_multi_output as cmo
        fx, g, X, xc = _single(name)
        L = cmo.kernel_pre_cal(g["Z"], g["kern"])
        terms = cmo.collapse_after_kernel_precalculation(L, xc, X, g["Z"], g["kern"], g["Q"], fx["T"], fx["T"])
        return list(L), terms, cmo.collapse_u_mean_after_kernel_precalculation(L, xc, X, g["Z"], g["kern"], g["Q"])

    for _N in (37, 130):
        @call("conditional %s N=%d" % (_name, _N), "ffvd_op_conditional", "ffvd_op_conditional_precalc", "ffvd_op_conditional_cov",
              "ffvd_op_conditional_precalc_cov", "ffvd_op_get_rand_full_cov", "ffvd_op_get_rand")
        def _conditional(name=_name, N=_N):
            from ffvd_amd import conditionals_multi_output as cmo, utils
            fx, g, X, xc = _single(name)
            Xnew, o = _xnew(fx, N), g["orc"]
            out = [cmo.conditional(Xnew, g["Z"], g["kern"], o["U"], white=True),
                   cmo.conditional(Xnew, g["Z"], g["kern"], o["U"], white=True, q_sqrt=o["H"]),
                   cmo.conditional_after_kernel_precalculation(o["L"], Xnew, g["Z"], g["kern"], o["U"], q_sqrt=o["H"], white=True),
                   cmo.conditional_after_kernel_precalculation(o["L"], Xnew, g["Z"], g["kern"], o["U"], white=True)]
            full = [cmo.conditional(Xnew, g["Z"], g["kern"], o["U"], white=True, full_cov=True, q_sqrt=o["H"]),
                    cmo.conditional_after_kernel_precalculation(o["L"], Xnew, g["Z"], g["kern"], o["U"], q_sqrt=o["H"], white=True, full_cov=True)]
            eps = np.random.default_rng(N).standard_normal(np.shape(out[0][0]))
            draws = [utils.get_rand(full[0], eps, full_cov=True), utils.get_rand(full[1], eps, full_cov=True), utils.get_rand(out[1], eps)]
            return out, full, draws


@call("likelihood", "ffvd_op_predict_mean", "ffvd_op_logdensity_norm_diag")
def _likelihood():
    from ffvd_amd import likelihoods
    rng = np.random.default_rng(7)
    N, D, J = 301, 4, 2
    X, y = rng.standard_normal((N, D)), rng.standard_normal((N, J))
    lik = likelihoods.Gaussian(J, D, CC=rng.standard_normal((D, J)), DD=rng.standard_normal(J), RR_chol=np.array([[0.4, 0.9], [1.0, 1.0]]))
    ym = lik.predict_mean(X)
    return ym, likelihoods.logdensity_norm_diag(y, ym, lik.Rchols[0]), likelihoods.logdensity_norm_diag_nonvec(y, ym, lik.Rchols[0])


@call("optimiser operators", "ffvd_op_adam_step", "ffvd_op_sghmc_step")
def _optim():
    from ffvd_amd import optim
    rng = np.random.default_rng(11)
    th, g, z = rng.standard_normal(257), rng.standard_normal(257), rng.standard_normal(257)
    a, s = optim.AdamState(th.shape), optim.SghmcState(th.shape)
    return optim.adam_step(th, g, a, 0.01), a.m, a.v, optim.sghmc_step(th, g, s, z, X_N=97, burn_in=True), s.xi, s.g, s.g2, s.p


for _name in FIXTURES:
    for _q in ("none", "upper", "dense"):
        @call("rollout %s q=%s" % (_name, _q), "ffvd_op_rollout", "ffvd_op_rollout_summary")
        def _rollout(name=_name, q=_q):
            from ffvd_amd.prediction import rollout, rollout_summary
            fx, g, X, xc = _single(name)
            rng, o, steps, R, D = np.random.default_rng(5), g["orc"], 6, 13, X.shape[1]
            H = None if q == "none" else o["H"] if q == "upper" else o["H"] + 0.01 * np.tril(rng.standard_normal(o["H"].shape), -1)
            ctrl = np.concatenate((fx["c"], rng.standard_normal((steps, fx["c"].shape[1]))))
            px, pv = rollout(o["L"], g["Z"], g["kern"], o["U"], H, X[-1], ctrl, fx["T"], steps, g["Q"], rng.standard_normal((steps, R, D)))
            CC, DD, lr = fx["em"]
            return px, pv, rollout_summary(px, pv, CC, DD, lr, Y_test=_targets(fx, steps))


@call("pg_sweep ragged", "ffvd_op_pg_sweep")
def _pg_sweep():
    from ffvd_amd import synthetic
    from ffvd_amd.prediction import pg_sweep
    fx, g, X, xc = _single("ragged")
    params, Y, c, meta = synthetic.make_named("ragged")
    rng, T, R, D = np.random.default_rng(9), fx["T"], 13, X.shape[1]
    return pg_sweep(g["orc"]["L"], g["Z"], g["kern"], params["U"], X, Y, fx["c"], params["CC"], params["DD"], np.exp(params["log_Rchols"]),
                    g["Q"], rng.standard_normal((R, D)), rng.standard_normal((T, R, D)), rng.random((T, R)))


def _rollout_args(fx, R, steps, q):
    gs = fx["gs"]
    rng = np.random.default_rng(13)
    ctrl = np.concatenate((fx["c"], rng.standard_normal((steps, fx["c"].shape[1]))))
    eps = rng.standard_normal((steps, len(gs), R, gs[0]["X"].shape[1]))
    return ([g["orc"]["L"] for g in gs], [g["Z"] for g in gs], [g["kern"] for g in gs], [g["orc"]["U"] for g in gs],
            [g["orc"]["H"] for g in gs] if q else None, [g["X"][-1] for g in gs], ctrl, fx["T"], steps, _Qs(fx), eps)


for _name in FIXTURES:
    @call("rollout_grouped " + _name, "ffvd_op_rollout_grouped", "ffvd_op_rollout_grouped_summary")
    def _rollout_grouped(name=_name):
        from ffvd_amd import prediction as pr
        fx = _fixture(name)
        a = _rollout_args(fx, 13, 5, name != "m130")
        CC, DD, lr = fx["em"]
        return pr.rollout_grouped(*a), pr.rollout_grouped_summary(*a, CC, DD, lr, Y_test=_targets(fx, 5), return_rollouts=True)

    @call("posterior_grouped " + _name, "ffvd_op_posterior_grouped", "ffvd_op_posterior_rollout_grouped",
          "ffvd_op_posterior_rollout_grouped_summary")
    def _posterior_grouped(name=_name):
        from ffvd_amd import conditionals_multi_output as cmo, prediction as pr
        fx = _fixture(name)
        Zs, kerns, Xs, Qs = _fused(fx)
        a = _rollout_args(fx, 13, 5, True)
        ctrl, eps = a[6], a[10]
        CC, DD, lr = fx["em"]
        return (cmo.collapse_u_mean_grouped(Zs, kerns, Xs, fx["c"], Qs, groups_per_pass=1),
                pr.posterior_rollout_grouped(Zs, kerns, Xs, Qs, ctrl, fx["T"], 5, eps, groups_per_pass=1, return_U=True),
                pr.posterior_rollout_grouped_summary(Zs, kerns, Xs, Qs, ctrl, fx["T"], 5, eps, CC, DD, lr, Y_test=_targets(fx, 5),
                                                     return_rollouts=True, return_U=True))

    for _N in (37, 130):
        @call("conditional_grouped %s N=%d" % (_name, _N), "ffvd_op_conditional_grouped", "ffvd_op_posterior_conditional_grouped",
              "ffvd_op_conditional_grad_grouped", "ffvd_op_posterior_conditional_grad_grouped")
        def _conditional_grouped(name=_name, N=_N):
            from ffvd_amd import conditionals_multi_output as cmo, prediction as pr
            fx = _fixture(name)
            Xnew, fused, kw = _xnew(fx, N), _fused(fx), dict(q_mode=fx["mode"], rows_per_pass=16)
            return (cmo.conditional_grouped(*_models(fx), Xnew, **kw), cmo.conditional_grad_grouped(*_models(fx), Xnew, **kw),
                    pr.posterior_conditional_grouped(*fused, fx["c"], Xnew, groups_per_pass=1, return_U=True, **kw),
                    pr.posterior_conditional_grad_grouped(*fused, fx["c"], Xnew, groups_per_pass=1, return_U=True, **kw))

    @call("moment_grouped " + _name, "ffvd_op_moment_grouped", "ffvd_op_posterior_moment_grouped", "ffvd_op_moment_summary")
    def _moment_grouped(name=_name):
        from ffvd_amd import prediction as pr
        fx = _fixture(name)
        steps, ci = int(fx["lengths"][0]), _ctrl_all(fx)
        kw = dict(S0s=_one(fx["S0"]), q_mode=fx["mode"])
        given = pr.moment_grouped(*_models(fx), list(_one(fx["x0"])), ci, fx["T"], steps, _Qs(fx), **kw)
        fused = pr.posterior_moment_grouped(*_fused(fx), ci, fx["T"], steps, groups_per_pass=1, return_U=True, **kw)
        CC, DD, lr = fx["em"]
        return given, fused, pr.moment_summary(given[0], given[1], CC, DD, lr, Y_test=_targets(fx, steps))

    for _method in ("moment", "linearised"):
        @call("filter_grouped %s %s" % (_name, _method), "ffvd_op_filter_grouped" if _method == "moment" else "ffvd_op_filter_linear_grouped",
              "ffvd_op_posterior_filter_grouped" if _method == "moment" else "ffvd_op_posterior_filter_linear_grouped")
        def _filter_grouped(name=_name, method=_method):
            from ffvd_amd import prediction as pr
            fx = _fixture(name)
            Y0 = fx["Y"][0][: int(fx["lengths"][0])]
            kw = dict(S0s=_one(fx["S0"]), q_mode=fx["mode"], smooth=True, method=method)
            return (pr.filter_grouped(*_models(fx), _one(fx["x0"]), _ctrl_all(fx), fx["T"], Y0, _Qs(fx), *fx["em"], **kw),
                    pr.posterior_filter_grouped(*_fused(fx), _ctrl_all(fx), fx["T"], Y0, *fx["em"], x0s=_one(fx["x0"]), groups_per_pass=1, **kw))

    for _rule, _given, _post in (("linearised", "filter_records_grouped", "posterior_filter_records_grouped"),
                                 ("cubature", "filter_cubature_records_grouped", "posterior_filter_cubature_records_grouped")):
        @call("records %s %s" % (_name, _rule), "ffvd_op_" + _given, "ffvd_op_" + _post)
        def _records(name=_name, given=_given, post=_post):
            from ffvd_amd import prediction as pr
            fx = _fixture(name)
            kw = dict(lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], smooth=True, records_per_pass=_rpp(fx))
            return (getattr(pr, given)(*_models(fx), fx["x0"], fx["ctrl"], fx["Y"], _Qs(fx), *fx["em"], **kw),
                    getattr(pr, post)(*_fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"], x0s=fx["x0"], groups_per_pass=1, **kw),
                    _records_meta(fx))

    for _n in (13, 64):
        @call("records %s particle n=%d" % (_name, _n), "ffvd_op_filter_particle_records_grouped",
              "ffvd_op_posterior_filter_particle_records_grouped")
        def _particle_records(name=_name, n=_n):
            import particle_fixtures as fxt
            from ffvd_amd import prediction as pr
            fx = _with_particles(_fixture(name), n, 1300 + n)
            kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], records_per_pass=_rpp(fx), return_particles=True)
            return (fxt.call(fx, records_per_pass=_rpp(fx)),
                    pr.posterior_filter_particle_records_grouped(*_fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"], fx["eps"], fx["unif"],
                                                                 x0s=fx["x0"], groups_per_pass=1, **kw),
                    _records_meta(fx))

    for _rule in ("grouped", "linear_grouped", "cubature_grouped"):
        @call("forecast %s %s" % (_name, _rule), "ffvd_op_forecast_" + _rule, "ffvd_op_posterior_forecast_" + _rule)
        def _forecast(name=_name, rule=_rule):
            from ffvd_amd import prediction as pr
            fx = _fixture(name)
            n = int(fx["lengths"][0])
            Y0, org = fx["Y"][0][:n], [0, 2, 3]           # (three origins x the fixture's groups: never a multiple of 128 tracks)
            kw = dict(origins=org, S0s=_one(fx["S0"]), q_mode=fx["mode"], return_tracks=True, return_filter=True, tracks_per_pass=2)
            return (getattr(pr, "forecast_" + rule)(*_models(fx), _one(fx["x0"]), _ctrl_all(fx), fx["T"], Y0, _Qs(fx), *fx["em"], 2, **kw),
                    getattr(pr, "posterior_forecast_" + rule)(*_fused(fx), _ctrl_all(fx), fx["T"], Y0, *fx["em"], 2, x0s=_one(fx["x0"]),
                                                              groups_per_pass=1, **kw))

    for _n in (13, 64):
        @call("forecast %s particle n=%d" % (_name, _n), "ffvd_op_forecast_particle_grouped", "ffvd_op_posterior_forecast_particle_grouped")
        def _particle_forecast(name=_name, n=_n):
            import forecast_particle_fixtures as fpx
            from ffvd_amd import prediction as pr
            base = _fixture(name)
            steps = int(base["lengths"][0])
            cut = dict(base, Y=base["Y"][:, :steps], ctrl=None if base["ctrl"] is None else base["ctrl"][:, :steps])
            fx = _with_forecast(_with_particles(cut, n, 1400 + n), 2, (0, 2, 3), 1500 + n)
            fx = dict(fx, eps=fx["eps"][:, :, :steps], unif=fx["unif"][:, :, :steps])
            kw = dict(xi0=_one(fx["xi0"]), origins=fx["origins"], S0s=_one(fx["S0"]), q_mode=fx["mode"], return_tracks=True, return_filter=True,
                      return_particles=True, tracks_per_pass=2)
            ci = fx["c"] if fx["ctrl"] is None else np.concatenate((fx["c"], fx["ctrl"][0]), axis=0)
            return (fpx.call(fx, tracks_per_pass=2),
                    pr.posterior_forecast_particle_grouped(*_fused(fx), ci, fx["T"], fx["Y"][0], *fx["em"], fx["h"], _one(fx["eps"]),
                                                           _one(fx["unif"]), fx["eps_fc"], x0s=_one(fx["x0"]), groups_per_pass=1, **kw))


def called_symbols():
    """every entry point some call of CALLS names"""
    return sorted({s for _, symbols, _ in CALLS for s in symbols})


# ---- the run ----------------------------------------------------------------------------------------------------------------------------
def flatten(prefix, value, out):
    if value is None:
        return
    if isinstance(value, dict):
        for k, v in value.items():
            flatten("%s/%s" % (prefix, k), v, out)
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            flatten("%s/%d" % (prefix, i), v, out)
    else:
        out[prefix] = np.asarray(value)


def main(path):
    from ffvd_amd import _lib
    lib = _lib.load()
    seen = []
    for name in _lib.exported_symbols():
        if name.startswith("ffvd_op_"):
            def counted(*a, _fn=getattr(lib, name), _name=name):
                seen.append(_name)
                return _fn(*a)
            setattr(lib, name, counted)
    out = {}
    for tag, order in (("fwd", CALLS), ("rev", CALLS[::-1])):
        for label, symbols, fn in order:
            del seen[:]
            flatten("%s/%s" % (tag, label), fn(), out)
            out["called/" + label] = np.array(sorted(set(seen)))
    assert lib.ffvd_op_release_cache() == 0
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
