"""The child process of tests/test_gpu_forecast_adapted.py::test_poisoned_operator_cache_changes_nothing: the two adapted particle
forecast entry points (`ffvd_particle_adapted_forecast_grouped`, `ffvd_posterior_particle_adapted_forecast_grouped`) on particle fixtures
of tests/cache_poison_script.py with N = 13 or N = 64 (h = 2, origins (0, 2, 3), two tracks per pass), the whole list once forwards
and once in reverse order in one process.  What that script's list protects for the `ffvd_op_*` entry points -- no result may depend on
what a cached scratch block held before -- is tested here for these two, whose names keep them out of that list (as
tests/adapted_poison_script.py does for the adapted filter's).

`python adapted_fan_poison_script.py OUT.npz` writes every output array under "<pass>/<call>/<form>/<key>"."""
import sys

import numpy as np

import cache_poison_script as base

SYMBOLS = ("ffvd_particle_adapted_forecast_grouped", "ffvd_posterior_particle_adapted_forecast_grouped")
CALLS = []


def _add(name, n):
    def fn():
        import forecast_adapted_fixtures as fax
        from ffvd_amd import prediction as pr
        whole = base._fixture(name)
        steps = int(whole["lengths"][0])
        cut = dict(whole, Y=whole["Y"][:, :steps], ctrl=None if whole["ctrl"] is None else whole["ctrl"][:, :steps])
        fx = base._with_forecast(base._with_particles(cut, n, 1800 + n), 2, (0, 2, 3), 1900 + n)
        fx = dict(fx, eps=fx["eps"][:, :, :steps], unif=fx["unif"][:, :, :steps])
        kw = dict(xi0=base._one(fx["xi0"]), origins=fx["origins"], S0s=base._one(fx["S0"]), q_mode=fx["mode"], return_tracks=True,
                  return_filter=True, return_particles=True, tracks_per_pass=2)
        ci = fx["c"] if fx["ctrl"] is None else np.concatenate((fx["c"], fx["ctrl"][0]), axis=0)
        return (fax.call(fx, tracks_per_pass=2),
                pr.posterior_forecast_adapted_grouped(*base._fused(fx), ci, fx["T"], fx["Y"][0], *fx["em"], fx["h"], base._one(fx["eps"]),
                                                      base._one(fx["unif"]), fx["eps_fc"], x0s=base._one(fx["x0"]), groups_per_pass=1, **kw))
    CALLS.append(("adapted forecast %s particle n=%d" % (name, n), fn))


for _name, _n in (("ragged", 13), ("m130", 64), ("d8", 13), ("m300", 64)):
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
