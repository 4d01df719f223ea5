"""The linearised filter (method="linearised") against the moment-matched filter (method="moment") of the same build, in one process on
the same GPU, with the protocol of tools/bench_filter_group.py (the model builder, time limit and statistics of
tools/bench_moment_group.py are imported): wall time around the calls, uploads, the posteriors and the final synchronisation included;
every side warmed up twice, then the sides measured alternately, median of --repeats runs with min-max.  No ratio is fixed in advance.

  1. `DGPSSM.filter_heldout` against `DGPSSM.filter_heldout_linearised` over 200 observed rows, without and with smooth=True, at the
     actuator shape (S = 10) and config 2 (S = 32): collapsed U, one Gamma per (chain, dim);
  2. the same two rules through `prediction.filter_grouped` on an explicit U shared by the chains (no q slices: one Gamma per dim for
     all chains), where the linearised step reads units = D instead of S D matrices;
  3. what the cheaper rule costs in fit: ll, ll_joint and RMSE of both methods on the actuator fixture (tests/golden, three chains,
     40 held-out rows) and at the two shapes -- reported, not asserted;
  4. per-launch times of the linearised step from a kernel trace the tool starts itself, one child process per form:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_linear.py --kernel-only SHAPE:FORM

    python tools/bench_filter_linear.py [--repeats 5] [--out profiles/filter_linear.json] [--commit HASH] [--limit 120] [--no-trace]

Every GPU step runs under a time limit of its own (an alarm whose default action ends the process); a child runs under a timeout."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from bench_moment_group import SHAPES, STEPS, fixture_model, limit, model, stats, timed_ms
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import prediction as pr

FORMS = ("collapsed", "explicit")
FIT = ("ll", "ll_joint", "RMSE")


def explicit_call(mod, cc, Y_test, Lm, method, smooth=False):
    """The filter on the layer's explicit U, shared by the chains, without q slices: Gamma = W W^T per dim"""
    S, lay, lik = mod.num_chains, mod.layers[-1], mod.likelihood
    return pr.filter_grouped(Lm, lay.Z, lay.kernel, [lay.U] * S, None, [mod._X_chains[s][-1] for s in range(S)], cc, mod.Y.shape[0], Y_test,
                             mod.Q, lik.CC, lik.DD, lik.log_Rchols, smooth=smooth, method=method)


def kernel_figures(path, cfg, form):
    """The step kernels in a rocprofv3 kernel_stats.csv -> calls, mean duration per launch and, for the linearised step, the rate at
    which it reads Gamma (units Mp^2 doubles per launch)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    Mp = -(-cfg["M"] // 64) * 64
    units = cfg["D"] * (cfg["S"] if form == "collapsed" else 1)
    out = {}
    for key, pick in (("linear_step", lambda n: "mg_linear_kernel" in n), ("moment_filter_step", lambda n: "mg_step_kernel" in n and "true" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:70], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    if "linear_step" in out:
        nbytes = units * Mp * Mp * 8
        out["linear_step"].update(gamma_mb_per_launch=round(nbytes / 1e6, 2), workgroups=cfg["S"] * cfg["D"] * -(-cfg["M"] // 16),
                                  gamma_gb_per_s=round(nbytes / (out["linear_step"]["mean_launch_us"] * 1e3), 1))
    return out


def kernel_trace(shape, form, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of each method at `shape` in `form`."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{shape}:{form}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0], SHAPES[shape], form) if found else dict(skipped="no kernel_stats.csv was written")


def fit_of(out):
    return {k.lower(): out[k] for k in FIT}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="SHAPE:FORM", help="three calls of each method at SHAPE in FORM (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        shape, form = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[shape], STEPS)
            Lm = cmo.kernel_pre_cal(mod.layers[-1].Z, mod.layers[-1].kernel) if form == "explicit" else None
        for _ in range(3):
            for method in pr.FILTER_METHODS:
                with limit(a.limit):
                    if form == "explicit":
                        f = explicit_call(mod, cc, Y_test, Lm, method)
                    else:
                        f = (mod.filter_heldout if method == "moment" else mod.filter_heldout_linearised)(Y_test, cc)
        print(json.dumps(dict(shape=shape, form=form, ll=f["ll"], rmse=f["RMSE"])))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    with limit(a.limit):
        fmod, fc, fY = fixture_model()
        fixture = dict(moment=fit_of(fmod.filter_heldout(fY, fc)), linearised=fit_of(fmod.filter_heldout_linearised(fY, fc)))
    print(json.dumps(dict(actuator_fixture=fixture)), flush=True)
    rows, trace = [], {}
    for name in [s for s in a.shapes.split(",") if s]:
        cfg = SHAPES[name]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, STEPS)
            Lm = cmo.kernel_pre_cal(mod.layers[-1].Z, mod.layers[-1].kernel)
        out = {}
        sides = {
            "moment": lambda: mod.filter_heldout(Y_test, cc),
            "linearised": lambda: mod.filter_heldout_linearised(Y_test, cc),
            "moment_smooth": lambda: mod.filter_heldout(Y_test, cc, smooth=True),
            "linearised_smooth": lambda: mod.filter_heldout_linearised(Y_test, cc, smooth=True),
            "explicit_moment": lambda: explicit_call(mod, cc, Y_test, Lm, "moment"),
            "explicit_linearised": lambda: explicit_call(mod, cc, Y_test, Lm, "linearised"),
        }

        def run(k):
            out[k] = sides[k]()

        for _ in range(2):                                      # every side warmed up twice
            for k in sides:
                timed_ms(lambda: run(k), a.limit)
        ts = {k: [] for k in sides}
        for _ in range(a.repeats):                              # alternating, so that all see the same neighbours on the machine
            for k in sides:
                ts[k].append(timed_ms(lambda: run(k), a.limit))
        med = {k: statistics.median(v) for k, v in ts.items()}
        row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], steps=STEPS, ms_median_min_max={k: stats(v) for k, v in ts.items()},
                   moment_over_linearised=round(med["moment"] / med["linearised"], 3),
                   moment_over_linearised_smooth=round(med["moment_smooth"] / med["linearised_smooth"], 3),
                   moment_over_linearised_explicit=round(med["explicit_moment"] / med["explicit_linearised"], 3),
                   fit={k: fit_of(out[k]) for k in ("moment", "linearised", "explicit_moment", "explicit_linearised")},
                   largest_difference_in_m_filt=float(np.max(np.abs(out["moment"]["m_filt"] - out["linearised"]["m_filt"]))))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not a.no_trace:
            trace[name] = {form: kernel_trace(name, form, 4 * a.limit) for form in FORMS}
            print(json.dumps({name: trace[name]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_linear.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.filter_heldout_linearised: ffvd_op_posterior_filter_linear_grouped (linearised step launches)",
               baseline="DGPSSM.filter_heldout: ffvd_op_posterior_filter_grouped (moment-matched step launches), of the same build",
               timing="wall time around the call, synchronisation included; alternating after two warm-up calls per side",
               actuator_fixture=fixture, points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
