"""The child process of tests/test_gpu_filter_adaptive.py::test_poisoned_operator_cache_changes_nothing: the four entry points of the
adaptive particle filter (`ffvd_particle_adaptive_records_grouped`, `ffvd_posterior_particle_adaptive_records_grouped` and their
seeded forms) on the particle fixtures of tests/cache_poison_script.py, the whole list once forwards and once in reverse order in one
process.  The carried log-weights live in a scratch block that other calls have used, and only the launch at t = 0 writes them: what
that script's list protects for the `ffvd_op_*` entry points -- no result may depend on what a cached scratch block held before -- is
tested here for these four, whose names keep them out of that list (as tests/adapted_poison_script.py does for the adapted filter's).

`python adaptive_poison_script.py OUT.npz` writes every output array under "<pass>/<call>/<form>/<key>" and the records' lengths and
observations under "<pass>/<call>/4/..."."""
import sys

import numpy as np

import cache_poison_script as base

SYMBOLS = ("ffvd_particle_adaptive_records_grouped", "ffvd_posterior_particle_adaptive_records_grouped",
           "ffvd_particle_adaptive_seeded_records_grouped", "ffvd_posterior_particle_adaptive_seeded_records_grouped")
# fixture, N, threshold, noise of the seeded forms: every fixture, two particle counts, rows of both kinds (0.3), none (0) and all (2)
PLAN = (("ragged", 13, 0.3, "independent"), ("m130", 64, 0.3, "per_record"), ("d8", 13, 0.0, "shared"), ("m300", 64, 2.0, "independent"))
CALLS = []


def _add(name, n, thr, noise):
    def fn():
        from ffvd_amd import prediction as pr
        fx = base._with_particles(base._fixture(name), n, 2300 + n)
        kw = dict(ess_threshold=thr, lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], records_per_pass=base._rpp(fx),
                  return_particles=True)
        sk = dict(kw, seed=2300 + n, num_particles=n, noise=noise)
        given = (*base._models(fx), fx["x0"], fx["ctrl"], fx["Y"], base._Qs(fx), *fx["em"])
        fused = (*base._fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"])
        return (pr.filter_adaptive_records_grouped(*given, fx["eps"], fx["unif"], xi0=fx["xi0"], **kw),
                pr.posterior_filter_adaptive_records_grouped(*fused, fx["eps"], fx["unif"], xi0=fx["xi0"], x0s=fx["x0"], groups_per_pass=1, **kw),
                pr.adaptive_records_seeded(*given, **sk),
                pr.posterior_adaptive_records_seeded(*fused, x0s=fx["x0"], groups_per_pass=1, **sk),
                base._records_meta(fx))
    CALLS.append(("adaptive %s n=%d thr=%g %s" % (name, n, thr, noise), fn))


for _plan in PLAN:
    _add(*_plan)


def main(path):
    from ffvd_amd import _lib
    lib = _lib.load()
    seen = []
    for name in SYMBOLS:
        def counted(*a, _fn=getattr(lib, name), _name=name):
            seen.append(_name)
            return _fn(*a)
        setattr(lib, name, counted)
    out = {}
    for tag, order in (("fwd", CALLS), ("rev", CALLS[::-1])):
        for label, fn in order:
            del seen[:]
            base.flatten("%s/%s" % (tag, label), fn(), out)
            out["called/" + label] = np.array(sorted(set(seen)))
    assert lib.ffvd_op_release_cache() == 0
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
