"""Linearised rolling-origin forecasts in one call against the moment fan of the same build and against the composed linearised path a
user had before, in one process on the same GPU, with the protocol of tools/bench_forecast_group.py (model builder, time limit and
statistics of tools/bench_moment_group.py): wall time around calls that end in a synchronisation, uploads and the posteriors included;
every side warmed up twice, then measured alternately, median of --repeats runs with min-max.  No ratio is fixed in advance.

Workload: a record of 200 rows, horizon 10, collapsed U.  Actuator shape (T = 512, M = 100, D = 4, S = 10): stride 1, 190 origins.
Config 2 (T = 4096, M = 512, D = 4, S = 32): stride 10, 19 origins, all sides; and stride 1, 190 origins, the new call only (the
moment fan needs about a second per call there, which is why that run never existed).

  linear     `DGPSSM.forecast_heldout_linearised`: ffvd_op_posterior_forecast_linear_grouped (posteriors, linearised filter, passes of
             two launches per step, pooled summary);
  moment     `DGPSSM.forecast_heldout`: the moment fan;
  composed   `collapse_u_mean_grouped` once, `filter_grouped(method="linearised")` over the record, then per origin one
             `filter_grouped(method="linearised")` call from (m_filt[o], S_filt[o]) over h all-NaN rows with the control offset moved.

The new call's tracks are compared with the composed path's against the project's floors (1e-11 + 1e-9 max|.| on means, 1e-11 + 1e-8
max|.| on covariances); the largest differences go into the JSON.  ll_h / rmse_h of the two rules are reported side by side.

    python tools/bench_forecast_linear.py [--repeats 5] [--out profiles/forecast_linear.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_forecast_linear.py --kernel-only POINT

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
# point -> (shape, stride, sides)
POINTS = {"actuator": ("actuator", 1, ("linear", "moment", "composed")), "config2": ("config2", 10, ("linear", "moment", "composed")),
          "config2_stride1": ("config2", 1, ("linear",))}
PEAK_FP64_MFMA = 78.6e12


def kernel_figures(path, cfg, B):
    """The state and the product kernel in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; for the product its
    flop/s (2 tracks D Mp^2 per launch) against the fp64 MFMA peak and the bytes of Gamma it reads per second (once per row tile)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, pick in (("state", lambda n: "mg_lfan_state_kernel" in n), ("product", lambda n: "mg_lfan_var_kernel" in n),
                      ("filter_step", lambda n: "mg_linear_kernel" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    Mp = (M + 63) // 64 * 64
    if "product" in out:
        us = out["product"]["mean_launch_us"]
        flop, gam = 2.0 * G * B * D * Mp * Mp, 8.0 * G * D * Mp * Mp * ((B + 127) // 128)
        out["product"].update(tracks=G * B, flop_per_launch=flop, tflops=round(flop / (us * 1e-6) / 1e12, 3),
                              fraction_of_fp64_mfma_peak=round(flop / (us * 1e-6) / PEAK_FP64_MFMA, 4),
                              gamma_gbytes_per_second=round(gam / (us * 1e-6) / 1e9, 1))
    if "state" in out:
        out["state"].update(tracks=G * B, us_per_track=round(out["state"]["mean_launch_us"] / (G * B), 5))
    return out


def kernel_trace(point, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the new path at `point`."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    shape, stride, _ = POINTS[point]
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", point]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        B = len(range(0, ROWS - HORIZON, stride))
        return kernel_figures(found[0], SHAPES[shape], B) if found else dict(skipped="no kernel_stats.csv was written")


def floor(key, ref):
    return 1e-11 + (1e-9 if key == "mean" else 1e-8) * float(np.max(np.abs(ref)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default="actuator,config2,config2_stride1")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT", help="three calls of the new path at POINT and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        shape, stride, _ = POINTS[a.kernel_only]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[shape], ROWS)
        for _ in range(3):
            with limit(a.limit):
                f = mod.forecast_heldout_linearised(Y_test, cc, HORIZON, stride=stride)
        print(json.dumps(dict(point=a.kernel_only, rmse_h=f["rmse_h"][:, 0].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace, models = [], {}, {}
    for point in [s for s in a.points.split(",") if s]:
        shape, stride, names = POINTS[point]
        cfg = SHAPES[shape]
        if shape not in models:
            with limit(a.limit):
                models[shape] = model(cfg, ROWS)
        mod, cc, Y_test, meta = models[shape]
        S, D = meta["S"], meta["D"]
        lay, lik, n_train = mod.layers[-1], mod.likelihood, mod.Y.shape[0]
        Xs, origins = [mod._X_chains[s] for s in range(S)], list(range(0, ROWS - HORIZON, stride))
        B = len(origins)
        out = {}

        def composed():
            U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, Xs, cc, mod.Q)
            Ls, Us, Hs, Qs = list(Lm[0]), list(U), list(Hinv), [mod.Q] * S
            post = (Ls, lay.Z, lay.kernel, Us, Hs)
            em = (Qs, lik.CC, lik.DD, lik.log_Rchols)
            f = pr.filter_grouped(*post, [x[-1] for x in Xs], cc, n_train, Y_test, *em, method="linearised")
            nan = np.full((HORIZON, Y_test.shape[1]), np.nan)
            m_fc, S_fc = np.empty((S, B, HORIZON, D)), np.empty((S, B, HORIZON, D, D))
            for b, o in enumerate(origins):
                t = pr.filter_grouped(*post, list(f["m_filt"][:, o]), cc, n_train + o + 1, nan, *em, S0s=f["S_filt"][:, o], method="linearised")
                m_fc[:, b], S_fc[:, b] = t["m_pred"], t["S_pred"]
            return dict(m_fc=m_fc, S_fc=S_fc)

        sides = {"linear": lambda: mod.forecast_heldout_linearised(Y_test, cc, HORIZON, stride=stride, return_tracks=True),
                 "moment": lambda: mod.forecast_heldout(Y_test, cc, HORIZON, stride=stride, return_tracks=True),
                 "composed": composed}
        sides = {k: sides[k] for k in names}

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
        lin = out["linear"]
        row = dict(point=point, shape=shape, T=cfg["T"], M=cfg["M"], D=D, S=S, rows=ROWS, horizon=HORIZON, stride=stride, origins=B,
                   tracks=S * B, ms_median_min_max={k: stats(v) for k, v in ts.items()},
                   linear_launches=(ROWS + 1) + (2 * HORIZON + 1), rmse_h=dict(linear=lin["rmse_h"][:, 0].tolist()),
                   ll_h=dict(linear=lin["ll_h"][:, 0].tolist()))
        if "moment" in out:
            row["moment_over_linear"] = round(med["moment"] / med["linear"], 3)
            row["rmse_h"]["moment"], row["ll_h"]["moment"] = out["moment"]["rmse_h"][:, 0].tolist(), out["moment"]["ll_h"][:, 0].tolist()
            row["largest_difference_between_the_rules"] = dict(m_fc=float(np.max(np.abs(lin["m_fc"] - out["moment"]["m_fc"]))))
        if "composed" in out:
            two = out["composed"]
            dm, dS = float(np.max(np.abs(lin["m_fc"] - two["m_fc"]))), float(np.max(np.abs(lin["S_fc"] - two["S_fc"])))
            fm, fS = floor("mean", two["m_fc"]), floor("var", two["S_fc"])
            row.update(composed_over_linear=round(med["composed"] / med["linear"], 3),
                       faster="linear" if med["linear"] < med["composed"] else "composed",
                       composed_launches=(ROWS + 1) + B * (HORIZON + 1),
                       largest_difference_from_the_composed_path=dict(m_fc=dm, S_fc=dS, floor_m_fc=fm, floor_S_fc=fS,
                                                                      within_the_floors=bool(dm <= fm and dS <= fS)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not a.no_trace:
            trace[point] = kernel_trace(point, 4 * a.limit)
            print(json.dumps({point: trace[point]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_forecast_linear.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.forecast_heldout_linearised: ffvd_op_posterior_forecast_linear_grouped (posteriors, linearised filter "
                        "launches, passes of a state and a product launch per step, pooled summary)",
               baselines=dict(moment="DGPSSM.forecast_heldout (the moment fan) of the same build",
                              composed="collapse_u_mean_grouped once, filter_grouped(method='linearised') over the record, one "
                                       "filter_grouped(method='linearised') call per origin over h all-NaN rows: of the same build"),
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
