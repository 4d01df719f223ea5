"""The child process of tests/test_gpu_smooth_adapted.py::test_poisoned_operator_cache_changes_nothing: the four entry points of
particle smoothing and backward simulation on the adapted sets (`ffvd_particle_adapted_smooth_records_grouped`,
`ffvd_particle_adapted_backsim_records_grouped` and their posterior forms) on N = 13 and N = 64 particle fixtures of
tests/cache_poison_script.py, the whole list once forwards and once in reverse order in one process.  What that script's list protects
for the `ffvd_op_*` entry points -- no result may depend on what a cached scratch block held before -- is tested here for these
four, whose names keep them out of that list.

`python adapted_smooth_poison_script.py OUT.npz` writes every output array under "<pass>/<call>/<form>/<key>" (forms 0 .. 3: smoothing,
fused smoothing, backward simulation, fused backward simulation) and the records' lengths and observations under "<pass>/<call>/4/..."."""
import sys

import numpy as np

import cache_poison_script as base

SYMBOLS = ("ffvd_particle_adapted_smooth_records_grouped", "ffvd_posterior_particle_adapted_smooth_records_grouped",
           "ffvd_particle_adapted_backsim_records_grouped", "ffvd_posterior_particle_adapted_backsim_records_grouped")
FIXTURES = ("ragged", "m300")
B = 5
CALLS = []


def _add(name, n):
    def fn():
        import adapted_smooth_fixtures as sfx
        from ffvd_amd import prediction as pr
        fx = base._with_particles(base._fixture(name), n, 1500 + n)
        fx = sfx.with_uniforms(fx, B, 1600 + n)
        rpp = base._rpp(fx)
        kw = dict(xi0=fx["xi0"], lengths=fx["lengths"], S0s=fx["S0"], q_mode=fx["mode"], records_per_pass=rpp, return_particles=True)
        fused = (*base._fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"], fx["eps"], fx["unif"])
        return (sfx.call(fx, "smooth", records_per_pass=rpp),
                pr.posterior_smooth_adapted_records_grouped(*fused, x0s=fx["x0"], groups_per_pass=1, **kw),
                sfx.call(fx, "backsim", records_per_pass=rpp),
                pr.posterior_backsim_adapted_records_grouped(*fused, fx["unif_bs"], x0s=fx["x0"], groups_per_pass=1, **kw),
                base._records_meta(fx))
    CALLS.append(("adapted smooth %s particle n=%d" % (name, n), fn))


for _name in FIXTURES:
    for _n in (13, 64):
        _add(_name, _n)


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
