"""Particle rolling-origin forecasts in one call against the composed form a user had before and against the cubature fan of the same
build, in one process on the same GPU, with the protocol of tools/bench_forecast_cubature.py (model builder, time limit and statistics
of tools/bench_moment_group.py): wall time around calls that end in a synchronisation, the draws, uploads, downloads and the
posteriors included; every side warmed up once, then measured alternately, median of --repeats runs with min-max.  No ratio is fixed
in advance.

Workload: a record of 200 rows, horizon 10, collapsed U, stride 10 (19 origins) and stride 1 (190 origins); N = 64 / 256 / 1024 at
the actuator shape (T = 512, M = 100, D = 4, S = 10), N = 64 / 256 at config 2 (T = 4096, M = 512, D = 4, S = 32) and N = 896 -- the
largest count whose rows fit a pass there -- with 19 origins only.

  particle   `DGPSSM.forecast_heldout_particle`: ffvd_op_posterior_forecast_particle_grouped (posteriors, the particle records launch
             with one record, passes of three launches per forecast step, pooled summary);
  composed   ONE `DGPSSM.filter_records_particle` call with one record per origin, each Y[:o + 1] followed by h all-NaN rows (lengths
             o + 1 + h): B (o + h) track steps where the fan takes n + B h.  Both sides draw with noise="shared", so the composed
             form's tracks are tracks of the same law and not the same numbers (the bit identity of a track with the composed form on
             concatenated draws is what tests/test_gpu_forecast_particle.py asserts; per-record draws at these sizes are gigabytes);
  cubature   `DGPSSM.forecast_heldout_cubature`.

ll_h / rmse_h at k = 1, 5, 10 of the particle and the cubature fan are reported side by side, and on the actuator fixture of the tests
(not timed) those of all four rules.

    python tools/bench_forecast_particle.py [--repeats 5] [--out profiles/forecast_particle.json] [--commit HASH] [--limit 180] [--no-trace]

The kernel figures come from a trace the tool starts itself, in a child process of its own, nothing else traced with it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_forecast_particle.py --kernel-only POINT

The product kernel also runs in the call's filter stage (one record: N rows per group); the launches of the tracks are told from those
by the rows kernel that precedes them in the trace.  Every GPU step runs under a time limit of its own (an alarm whose default action
ends the process); the child runs under a timeout."""
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
from bench_moment_group import SHAPES, fixture_model, limit, model, stats, timed_ms

ROWS, HORIZON, SEED = 200, 10, 7
ALL = ("particle", "composed", "cubature")
# point -> (shape, stride, N)
POINTS = {f"{shape}_{19 if stride == 10 else 190}_n{n}": (shape, stride, n)
          for shape, ns in (("actuator", (64, 256, 1024)), ("config2", (64, 256))) for n in ns for stride in (10, 1)}
POINTS["config2_19_n896"] = ("config2", 10, 896)
PEAK_FP64_MFMA = 78.6e12
AT = (0, 4, 9)                       # horizons 1, 5, 10
CALLS = 3                            # calls of the new path in the traced child


def kernel_figures(path, cfg, B, N):
    """A rocprofv3 kernel_trace.csv -> per kernel of the tracks launches and mean duration per launch, and the time of the three per
    call; for the product (the launches that follow a rows kernel of the fan) its flop/s over the call (2 rows Mp^2 per unit and step,
    rows = tracks * N) against the fp64 MFMA peak."""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    dur = {"state": [], "rows": [], "product": [], "filter_weight": [], "filter_rows": [], "filter_product": []}
    stage = None
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        if "mg_pfan_state_kernel" in name:
            dur["state"].append(us)
        elif "mg_pfan_rows_kernel" in name:
            stage = ""
            dur["rows"].append(us)
        elif "mg_prec_weight_kernel" in name:
            dur["filter_weight"].append(us)
        elif "mg_prec_rows_kernel" in name:
            stage = "filter_"
            dur["filter_rows"].append(us)
        elif "mg_lfan_var_kernel" in name and stage is not None:
            dur[stage + "product"].append(us)
            stage = None
    out = {k: dict(launches=len(v), mean_launch_us=round(sum(v) / len(v), 3), min_launch_us=round(min(v), 3),
                   ms_per_call=round(sum(v) / CALLS * 1e-3, 3)) for k, v in dur.items() if v}
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    Mp = (M + 63) // 64 * 64
    if "product" in out:
        flop = 2.0 * G * B * N * D * Mp * Mp * HORIZON                                   # of the tracks of one call
        per_s = flop / (out["product"]["ms_per_call"] * 1e-3)
        out["product"].update(passes_per_call=out["product"]["launches"] / float(CALLS * HORIZON), rows_per_step=G * B * N * D,
                              flop_per_call=flop, tflops=round(per_s / 1e12, 3), fraction_of_fp64_mfma_peak=round(per_s / PEAK_FP64_MFMA, 4))
    return out


def kernel_trace(point, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the new path at `point`."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    shape, stride, n = POINTS[point]
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", point]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        B = len(range(0, ROWS - HORIZON, stride))
        return kernel_figures(found[0], SHAPES[shape], B, n) if found else dict(skipped="no kernel_trace.csv was written")


def fixture_fit(seconds):
    """The four rules on the actuator fixture (tests/golden/actuator_slim.npz: 400 training rows, three chains, a 40-row held-out
    record, every row an origin): the horizon curves at k = 1, 5, 10.  Reported, not timed."""
    with limit(seconds):
        mod, c, Y_test = fixture_model()
        out = {"particle_n1024": mod.forecast_heldout_particle(Y_test, c, HORIZON, num_particles=1024, seed=SEED),
               "particle_n256": mod.forecast_heldout_particle(Y_test, c, HORIZON, num_particles=256, seed=SEED),
               "moment": mod.forecast_heldout(Y_test, c, HORIZON), "linear": mod.forecast_heldout_linearised(Y_test, c, HORIZON),
               "cubature": mod.forecast_heldout_cubature(Y_test, c, HORIZON)}
    return dict(rows=int(Y_test.shape[0]), origins=int(out["moment"]["origins"].shape[0]), horizons=[k + 1 for k in AT],
                rmse_h={k: [v["rmse_h"][i, 0] for i in AT] for k, v in out.items()}, ll_h={k: [v["ll_h"][i, 0] for i in AT] for k, v in out.items()},
                ll_h_all={k: v["ll_h"][:, 0].tolist() for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--trace-points", default="actuator_190_n256,config2_19_n256,config2_19_n896")
    ap.add_argument("--limit", type=int, default=180, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT", help="three calls of the new path at POINT and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        shape, stride, n = POINTS[a.kernel_only]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[shape], ROWS)
        for _ in range(CALLS):
            with limit(a.limit):
                f = mod.forecast_heldout_particle(Y_test, cc, HORIZON, stride=stride, num_particles=n, seed=SEED)
        print(json.dumps(dict(point=a.kernel_only, rmse_h=f["rmse_h"][:, 0].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace, models = [], {}, {}
    traced = [] if a.no_trace else [s for s in a.trace_points.split(",") if s]
    for point in [s for s in a.points.split(",") if s]:
        shape, stride, n = POINTS[point]
        cfg = SHAPES[shape]
        if shape not in models:
            with limit(a.limit):
                models[shape] = model(cfg, ROWS)
        mod, cc, Y_test, meta = models[shape]
        S, D = meta["S"], meta["D"]
        n_train, J = mod.Y.shape[0], Y_test.shape[1]
        origins = list(range(0, ROWS - HORIZON, stride))
        B = len(origins)
        out = {}
        # the composed form's records: record b is Y[:o + 1] followed by h all-NaN rows, its control rows those the fan reads
        Yr = np.full((B, ROWS, J), np.nan)
        for b, o in enumerate(origins):
            Yr[b, :o + 1] = Y_test[:o + 1]
        lengths = np.asarray([o + 1 + HORIZON for o in origins])
        cr = None if cc is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cc)[n_train: n_train + ROWS], (B, ROWS, np.shape(cc)[1])))
        sides = {"particle": lambda: mod.forecast_heldout_particle(Y_test, cc, HORIZON, stride=stride, num_particles=n, seed=SEED),
                 "composed": lambda: mod.filter_records_particle(Yr, cr, lengths=lengths, num_particles=n, seed=SEED),
                 "cubature": lambda: mod.forecast_heldout_cubature(Y_test, cc, HORIZON, stride=stride)}

        def run(k):
            out[k] = sides[k]()

        for k in sides:                                         # one warm-up per side
            timed_ms(lambda: run(k), a.limit)
        ts = {k: [] for k in sides}
        for _ in range(a.repeats):                              # alternating, so that all see the same neighbours on the machine
            for k in sides:
                ts[k].append(timed_ms(lambda: run(k), a.limit))
        med = {k: statistics.median(v) for k, v in ts.items()}
        row = dict(point=point, shape=shape, T=cfg["T"], M=cfg["M"], D=D, S=S, rows=ROWS, horizon=HORIZON, stride=stride, origins=B, N=n,
                   tracks=S * B, ms_median_min_max={k: stats(v) for k, v in ts.items()}, horizons=[k + 1 for k in AT],
                   rmse_h={k: [out[k]["rmse_h"][i, 0] for i in AT] for k in ("particle", "cubature")},
                   ll_h={k: [out[k]["ll_h"][i, 0] for i in AT] for k in ("particle", "cubature")},
                   composed_over_particle=round(med["composed"] / med["particle"], 3),
                   cubature_over_particle=round(med["cubature"] / med["particle"], 3),
                   composed_track_steps=int(lengths.sum()), particle_track_steps=ROWS + B * HORIZON)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if point in traced:
            trace[point] = kernel_trace(point, 4 * a.limit)
            print(json.dumps({point: trace[point]}), flush=True)
    fixture = fixture_fit(a.limit)
    print(json.dumps(dict(actuator_fixture=fixture)), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_forecast_particle.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.forecast_heldout_particle: ffvd_op_posterior_forecast_particle_grouped (posteriors, the particle records "
                        "launches with one record, passes of a state, a rows and a product launch per step, pooled summary)",
               baselines=dict(composed="one DGPSSM.filter_records_particle call with one record per origin, Y[:o + 1] followed by h all-NaN "
                                       "rows: of the same build; shared draws on both sides",
                              cubature="DGPSSM.forecast_heldout_cubature of the same build"),
               timing="wall time around calls that end in a synchronisation, the draws included; alternating after one warm-up call per side",
               points=rows, kernels=trace or None, actuator_fixture=fixture)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
