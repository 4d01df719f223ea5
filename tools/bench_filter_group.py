"""The filter against the moment-matched prediction it extends, in one process on the same GPU, with the protocol of
tools/bench_moment_group.py (its model builder, time limit and statistics are imported): wall time around the calls, uploads, the
posteriors and the final synchronisation included; every side warmed up twice, then measured alternately, median of --repeats runs
with min-max.  No ratio is fixed in advance.

  1. `DGPSSM.filter_heldout` over 200 observed rows, without and with smooth=True, against `DGPSSM.predict_moments` of the same build
     (200 steps, the same rows as Y_test) at the actuator shape (S = 10) and config 2 (S = 32);
  2. the filter call with no observation at all (`prediction.posterior_filter_grouped`, every entry NaN) against
     `prediction.posterior_moment_grouped` on the same inputs: what the filter form of the step launch costs by itself;
  3. per-launch times of the filter step and of the smoother from a kernel trace the tool starts itself, in a child process:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_group.py --kernel-only SHAPE

    python tools/bench_filter_group.py [--repeats 5] [--out profiles/filter_group.json] [--commit HASH] [--limit 120] [--no-trace]

Every GPU step runs under a time limit of its own (an alarm whose default action ends the process); the child runs under a timeout."""
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
from bench_moment_group import SHAPES, STEPS, limit, model, stats, timed_ms
from ffvd_amd import prediction as pr


def kernel_figures(path, steps):
    """The step kernels and the smoother in a rocprofv3 kernel_stats.csv -> calls and mean duration per launch (and per step)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, pick in (("filter_step", lambda n: "mg_step_kernel" in n and "true" in n), ("moment_step", lambda n: "mg_step_kernel" in n and "true" not in n),
                      ("smoother", lambda n: "mg_smooth_kernel" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:70], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    if "smoother" in out:
        out["smoother"]["us_per_step"] = round(out["smoother"]["mean_launch_us"] / steps, 4)
    return out


def kernel_trace(shape, seconds):
    """One child under rocprofv3 (kernel trace only): three filter calls with smoothing and three moment calls at `shape`."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", shape]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0], STEPS) if found else dict(skipped="no kernel_stats.csv was written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="SHAPE", help="three smoothed filter calls and three moment calls at SHAPE (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[a.kernel_only], STEPS)
        for _ in range(3):
            with limit(a.limit):
                f = mod.filter_heldout(Y_test, cc, smooth=True)
            with limit(a.limit):
                mod.predict_moments(cc, STEPS, Y_test=Y_test)
        print(json.dumps(dict(shape=a.kernel_only, ll=f["ll"], rmse=f["RMSE"])))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace = [], {}
    for name in [s for s in a.shapes.split(",") if s]:
        cfg = SHAPES[name]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, STEPS)
        S, D = meta["S"], meta["D"]
        lay, lik, n_train = mod.layers[-1], mod.likelihood, mod.Y.shape[0]
        Xs, nan = [mod._X_chains[s] for s in range(S)], np.full_like(Y_test, np.nan)
        out = {}
        sides = {
            "moment": lambda: mod.predict_moments(cc, STEPS, Y_test=Y_test),
            "filter": lambda: mod.filter_heldout(Y_test, cc),
            "filter_smooth": lambda: mod.filter_heldout(Y_test, cc, smooth=True),
            "moment_call": lambda: pr.posterior_moment_grouped(lay.Z, lay.kernel, Xs, mod.Q, cc, n_train, STEPS),
            "filter_call_no_observations": lambda: pr.posterior_filter_grouped(lay.Z, lay.kernel, Xs, mod.Q, cc, n_train, nan, lik.CC, lik.DD,
                                                                               lik.log_Rchols),
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
        same = bool(np.array_equal(out["filter_call_no_observations"]["m_pred"], out["moment_call"][0]) and
                    np.array_equal(out["filter_call_no_observations"]["S_pred"], out["moment_call"][1]))
        row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=D, S=S, steps=STEPS, ms_median_min_max={k: stats(v) for k, v in ts.items()},
                   filter_over_moment=round(med["filter"] / med["moment"], 3),
                   filter_smooth_over_moment=round(med["filter_smooth"] / med["moment"], 3),
                   smoothing_ms=round(med["filter_smooth"] - med["filter"], 3),
                   no_observation_call_over_moment_call=round(med["filter_call_no_observations"] / med["moment_call"], 3),
                   no_observation_call_bit_identical_to_moment_call=same,
                   one_step=dict(ll=out["filter"]["ll"], ll_joint=out["filter"]["ll_joint"], rmse=out["filter"]["RMSE"]),
                   free_run=dict(ll=out["moment"]["ll"], rmse=out["moment"]["RMSE"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not a.no_trace:
            trace[name] = kernel_trace(name, 4 * a.limit)
            print(json.dumps({name: trace[name]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_group.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.filter_heldout: ffvd_op_posterior_filter_grouped (filter step launches, the smoother, the pooled summary)",
               baseline="DGPSSM.predict_moments: ffvd_op_posterior_moment_grouped with its summary, of the same build",
               timing="wall time around the call, synchronisation included; alternating after two warm-up calls per side",
               points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
