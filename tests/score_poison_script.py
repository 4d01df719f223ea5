"""The child process of tests/test_gpu_score.py::test_poisoned_operator_cache_changes_nothing: the two score entry points
(`ffvd_score_points`, `ffvd_score_moments`) on fixtures of tests/score_fixtures.py, the whole list once forwards and once in reverse
order in one process.  The staged mixtures, the pair partials of every pass and the outputs live in scratch blocks that other calls
have used: what tests/cache_poison_script.py protects for the `ffvd_op_*` entry points -- no result may depend on what a cached
scratch block held before -- is tested here for these two, whose names keep them out of that list (as
tests/adaptive_poison_script.py does for the adaptive filter's).

`python score_poison_script.py OUT.npz` writes every output array under "<pass>/<call>/<form>/<key>" and under "called/<call>" the
entry points the library saw during that call."""
import sys

import numpy as np

import cache_poison_script as base
import score_fixtures as sf

SYMBOLS = ("ffvd_score_points", "ffvd_score_moments")
# fixture of each kind, targets per pass: one tile and several, one pass and several, blocks that change hands between the two symbols
PLAN = (("p_tile-1", "m_tile-1", 0), ("p_2tile+3", "m_2tile+3", 8), ("p_k2", "m_tile", 1), ("p_tile+1", "m_k2", 3))
CALLS = []


def _add(points, moments, tpp):
    def fn():
        from ffvd_amd import prediction as pr
        p, m = sf.fixture(points), sf.fixture(moments)
        kw = lambda fx: dict(levels=fx["levels"], Y_train_std=1.7, targets_per_pass=tpp)
        em = lambda fx: (fx["CC"], fx["DD"], fx["lr"], fx["Y"])
        return (pr.rollout_score(p["x"], *em(p), **kw(p)), pr.particle_score(sf.as_particles(p["x"]), *em(p), **kw(p)),
                pr.moment_score(m["x"], m["S"], *em(m), **kw(m)))
    CALLS.append(("score %s %s tpp=%d" % (points, moments, tpp), fn))


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
