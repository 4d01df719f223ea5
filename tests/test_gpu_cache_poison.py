"""GPU, operators: no `ffvd_op_*` result may depend on what a cached scratch block held before.

FFVD_OP_CACHE_POISON=1 (op_scratch.h, read once per process) makes every block the operator cache hands out start as NaN bytes.
tests/cache_poison_script.py calls every entry point that takes device scratch -- the one-group operators, the grouped rollouts,
posteriors, conditionals and their linearisation, moments, the four filter rules and the four forecast fans, given and fused, and
the summaries -- on shapes with padded rows of K (M = 77, 130, 40, 300), ragged last tiles (N = 37, 130; 13 and 64 particles) and
several passes with a last one that is not full, twice in one process, the second time in reverse order.  The script runs in a child
process without and with the poison; every output must agree bit for bit (assert_array_equal: NaN-aware, integers included).
99 calls of the list per pass; the two child processes together take 7 s on an MI355X, most of it the CPU side of the fixtures.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import cache_poison_script as script

pytestmark = pytest.mark.gpu

# Outputs with a documented NaN position (include/ffvd_abi.h, prediction.py): the log densities of unobserved entries of Y (NaN marks
# them) in every filter and forecast; and in the records filters every per-track (G, R, steps, ...) and pooled (R, steps, J) array in
# the rows at and beyond a record's length.  Everything else -- every live row of every record included -- must be finite.
POOLED = ("predict_y", "predict_y_var_total", "lpd_mix", "lpd_gauss")
WHOLE = ("ll", "ll_joint", "ll_original_units", "RMSE", "ll_all", "log_evidence")


def _must_be_finite(key, a, npz):
    """boolean mask (broadcastable to a) of the entries of output `key` that have no documented NaN"""
    tag, label, rest = key.split("/", 2)
    name = rest.split("/")[-1]
    if label.startswith(("filter_grouped ", "forecast ")):
        return np.full(a.shape, "lpd" not in name)
    if label.startswith("records ") and rest.startswith("2/"):                   # (the script's own copy of lengths and Y)
        return np.zeros(a.shape, dtype=bool)
    if not label.startswith("records ") or name in WHOLE or a.ndim < 2:
        return np.ones(a.shape, dtype=bool)
    lengths, Y = npz["%s/%s/2/lengths" % (tag, label)], npz["%s/%s/2/Y" % (tag, label)]
    R, steps, J = Y.shape
    live = np.arange(steps)[None, :] < lengths[:, None]                          # (R, steps)
    seen = ~np.isnan(Y) & live[:, :, None]                                       # (R, steps, J)
    if name in POOLED:
        assert a.shape == (R, steps, J), key
        return seen if "lpd" in name else np.broadcast_to(live[:, :, None], a.shape)
    if name == "U" or a.shape[1:3] != (R, steps):                                # (the fused forms' posterior means)
        return np.ones(a.shape, dtype=bool)
    if name == "lpd":
        mask = seen[None]
    elif name == "lpd_joint":
        mask = np.any(seen, axis=2)[None]
    else:
        mask = live[None]
    return np.broadcast_to(mask.reshape(mask.shape + (1,) * (a.ndim - mask.ndim)), a.shape)


def test_poisoned_operator_cache_changes_nothing(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, FFVD_OP_CACHE_POISON=mode, PYTHONPATH=os.pathsep.join((root, os.path.join(root, "tests"))))
        path = str(tmp_path / f"ops{mode}.npz")
        run = subprocess.run([sys.executable, script.__file__, path], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-3000:]
        outs[mode] = np.load(path)
    clean, poisoned = outs["0"], outs["1"]
    assert sorted(clean.files) == sorted(poisoned.files)
    for label, symbols, _ in script.CALLS:                    # the call list is what it says it is: the library saw these entry points
        assert set(symbols) <= set(clean["called/" + label].tolist()), (label, symbols, clean["called/" + label])
    results = [k for k in clean.files if not k.startswith("called/")]
    assert len(results) > 20 * len(script.CALLS)
    for k in results:
        if clean[k].dtype.kind == "f":
            assert np.all(np.isfinite(clean[k][_must_be_finite(k, clean[k], clean)])), k
        np.testing.assert_array_equal(poisoned[k], clean[k], err_msg=k)
    for k in results:                                         # the second, reversed pass repeats the first: nothing is left behind either
        if k.startswith("fwd/"):
            np.testing.assert_array_equal(clean["rev/" + k[4:]], clean[k], err_msg=k)
            np.testing.assert_array_equal(poisoned["rev/" + k[4:]], clean[k], err_msg=k)
