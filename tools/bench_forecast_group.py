"""Rolling-origin forecasts in one call against the composed path a user had before, in one process on the same GPU, with the protocol
of tools/bench_moment_group.py (its model builder, time limit and statistics are imported): wall time around calls that end in a
synchronisation, uploads and the posteriors included; every side warmed up twice, then measured alternately, median of --repeats
runs with min-max.  No ratio is fixed in advance: `faster` names the faster side at each shape.

Workload: a record of 200 rows, horizon 10, collapsed U.  Actuator shape (T = 512, M = 100, D = 4, S = 10): stride 1, 190 origins.
Config 2 (T = 4096, M = 512, D = 4, S = 32): stride 10, 19 origins -- its step launch is VALU-bound at 436 us per 32 groups, so 190
origins would be a run of about a second per call (32 x 190 tracks x 11 launches), which measures nothing the 19 do not.

  one_call   `DGPSSM.forecast_heldout`: ffvd_op_posterior_forecast_grouped (posteriors, filter, fan passes, pooled summary);
  composed   `collapse_u_mean_grouped` once, `filter_grouped` once, then one `moment_grouped` call per origin from the downloaded
             filtered states (each uploads the posterior again and forms beta and Gamma again), pooled by `moment_summary`;
  filter     `DGPSSM.filter_heldout` alone: one_call - filter is what the tracks cost.

    python tools/bench_forecast_group.py [--repeats 5] [--out profiles/forecast_group.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_forecast_group.py --kernel-only SHAPE

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
from bench_moment_group import SHAPES, limit, model, stats, timed_ms
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import prediction as pr

ROWS, HORIZON = 200, 10
STRIDE = {"actuator": 1, "config2": 10}
WHY = ("stride 1 at the actuator shape (190 origins), stride 10 at config 2 (19 origins): config 2's step is VALU-bound at 436 us per "
       "32 groups, so 190 origins would be a run of about a second per call")


def kernel_figures(path, cfg, B):
    """The fan and the filter step kernels in a rocprofv3 kernel_stats.csv -> calls, mean duration per launch, and for the fan the
    time per track and the pair-table elements per second (G B npair M^2 per launch)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, pick in (("fan_step", lambda n: "mg_step_kernel" in n and "MomentFanArgs" in n),
                      ("filter_step", lambda n: "mg_step_kernel" in n and "MomentFilterArgs" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    for key, units in (("fan_step", G * B), ("filter_step", G)):
        if key in out:
            us = out[key]["mean_launch_us"]
            # (the last launch of a run only finishes a step: h of h + 1 fan launches, 200 of 201 filter launches carry a table)
            out[key].update(units_per_launch=units, us_per_unit=round(us / units, 4),
                            pair_table_elements_per_second=round(units * (D * (D + 1) // 2) * M * M / (us * 1e-6), 1))
    return out


def kernel_trace(shape, seconds):
    """One child under rocprofv3 (kernel trace only): three forecast calls at `shape`."""
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
        B = len(range(0, ROWS - HORIZON, STRIDE[shape]))
        return kernel_figures(found[0], SHAPES[shape], B) if found else dict(skipped="no kernel_stats.csv was written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="SHAPE", help="three forecast calls at SHAPE and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[a.kernel_only], ROWS)
        for _ in range(3):
            with limit(a.limit):
                f = mod.forecast_heldout(Y_test, cc, HORIZON, stride=STRIDE[a.kernel_only])
        print(json.dumps(dict(shape=a.kernel_only, rmse_h=f["rmse_h"][:, 0].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace = [], {}
    print(json.dumps(dict(workload=WHY)), flush=True)
    for name in [s for s in a.shapes.split(",") if s]:
        cfg, stride = SHAPES[name], STRIDE[name]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        S, D = meta["S"], meta["D"]
        lay, lik, n_train = mod.layers[-1], mod.likelihood, mod.Y.shape[0]
        Xs, origins = [mod._X_chains[s] for s in range(S)], list(range(0, ROWS - HORIZON, stride))
        B = len(origins)
        out = {}

        def composed():
            U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, Xs, cc, mod.Q)
            Ls, Us, Hs, Qs = list(Lm[0]), list(U), list(Hinv), [mod.Q] * S
            f = pr.filter_grouped(Ls, lay.Z, lay.kernel, Us, Hs, [x[-1] for x in Xs], cc, n_train, Y_test, Qs, lik.CC, lik.DD, lik.log_Rchols)
            m_fc, S_fc = np.empty((S, B, HORIZON, D)), np.empty((S, B, HORIZON, D, D))
            for b, o in enumerate(origins):
                m_fc[:, b], S_fc[:, b] = pr.moment_grouped(Ls, lay.Z, lay.kernel, Us, Hs, list(f["m_filt"][:, o]), cc, n_train + o + 1, HORIZON,
                                                           Qs, S0s=f["S_filt"][:, o])
            Yt = np.concatenate([Y_test[o + 1: o + 1 + HORIZON] for o in origins])
            pooled = pr.moment_summary(m_fc.reshape(S, B * HORIZON, D), S_fc.reshape(S, B * HORIZON, D, D), lik.CC, lik.DD, lik.log_Rchols, Yt)
            return dict(m_fc=m_fc, S_fc=S_fc, predict_y=pooled["predict_y"].reshape(B, HORIZON, -1))

        sides = {
            "one_call": lambda: mod.forecast_heldout(Y_test, cc, HORIZON, stride=stride, return_tracks=True),
            "composed": composed,
            "filter": lambda: mod.filter_heldout(Y_test, cc),
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
        one, two = out["one_call"], out["composed"]
        tracks_ms = med["one_call"] - med["filter"]
        row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=D, S=S, rows=ROWS, horizon=HORIZON, stride=stride, origins=B, tracks=S * B,
                   ms_median_min_max={k: stats(v) for k, v in ts.items()},
                   composed_over_one_call=round(med["composed"] / med["one_call"], 3),
                   faster="one_call" if med["one_call"] < med["composed"] else "composed",
                   tracks_ms_over_the_filter=round(tracks_ms, 3), us_per_forecast_launch=round(tracks_ms * 1e3 / (HORIZON + 1), 3),
                   us_per_track_step=round(tracks_ms * 1e3 / (S * B * HORIZON), 4),
                   one_call_launches=(ROWS + 1) + (HORIZON + 1), composed_launches=(ROWS + 1) + B * (HORIZON + 1),
                   largest_difference_between_the_routes=dict(m_fc=float(np.max(np.abs(one["m_fc"] - two["m_fc"]))),
                                                              S_fc=float(np.max(np.abs(one["S_fc"] - two["S_fc"]))),
                                                              predict_y=float(np.max(np.abs(one["predict_y"] - two["predict_y"])))),
                   rmse_h=one["rmse_h"][:, 0].tolist(), ll_h=one["ll_h"][:, 0].tolist())
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not a.no_trace:
            trace[name] = kernel_trace(name, 4 * a.limit)
            print(json.dumps({name: trace[name]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_forecast_group.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats, workload=WHY,
               new_path="DGPSSM.forecast_heldout: ffvd_op_posterior_forecast_grouped (posteriors, filter launches, fan passes, pooled summary)",
               baseline="collapse_u_mean_grouped once, filter_grouped once, one moment_grouped call per origin, moment_summary: of the same build",
               timing="wall time around calls that end in a synchronisation; alternating after two warm-up calls per side",
               points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
