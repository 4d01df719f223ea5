"""The child process of tests/test_gpu_particle_seeded.py::test_poisoned_operator_cache_changes_nothing: the three entry points of the
seeded particle draws (`ffvd_particle_draws`, `ffvd_particle_seeded_records_grouped`, `ffvd_posterior_particle_seeded_records_grouped`)
on the particle fixtures of tests/cache_poison_script.py, the whole list once forwards and once in reverse order in one process.  The
fill launch writes into scratch blocks that other calls have used: what that script's list protects for the `ffvd_op_*` entry points
-- no result may depend on what a cached scratch block held before -- is tested here for these three, whose names keep them out of
that list (as tests/adapted_poison_script.py does for the adapted filter's).

`python seeded_poison_script.py OUT.npz` writes every output array under "<pass>/<call>/<form>/<key>" and the records' lengths and
observations under "<pass>/<call>/3/..."."""
import sys

import numpy as np

import cache_poison_script as base

SYMBOLS = ("ffvd_particle_draws", "ffvd_particle_seeded_records_grouped", "ffvd_posterior_particle_seeded_records_grouped")
B = 5
# fixture, N, rule, stage, noise: every fixture, both particle counts, every value of the three axes
PLAN = (("ragged", 13, "bootstrap", "backsim", "independent"), ("m130", 13, "adapted", "smooth", "per_record"),
        ("d8", 13, "bootstrap", "filter", "shared"), ("m300", 48, "adapted", "backsim", "independent"),
        ("m300", 13, "bootstrap", "smooth", "shared"))
CALLS = []


def _add(name, n, rule, stage, noise):
    def fn():
        from ffvd_amd import prediction as pr
        fx = base._fixture(name)
        G, (R, steps), D = len(fx["gs"]), fx["Y"].shape[:2], fx["x0"].shape[-1]
        nb = B if stage == "backsim" else 0
        kw = dict(seed=1900 + n, num_particles=n, rule=rule, stage=stage, noise=noise, num_trajectories=nb, lengths=fx["lengths"], S0s=fx["S0"],
                  q_mode=fx["mode"], records_per_pass=base._rpp(fx), return_particles=True)
        return (pr.particle_draws(1900 + n, noise, G, R, steps, n, D, with_xi0=fx["S0"] is not None, B=nb),
                pr.particle_records_seeded(*base._models(fx), fx["x0"], fx["ctrl"], fx["Y"], base._Qs(fx), *fx["em"], **kw),
                pr.posterior_particle_records_seeded(*base._fused(fx), fx["c"], fx["ctrl"], fx["Y"], *fx["em"], x0s=fx["x0"], groups_per_pass=1, **kw),
                base._records_meta(fx))
    CALLS.append(("seeded %s n=%d %s %s %s" % (name, n, rule, stage, noise), fn))


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
