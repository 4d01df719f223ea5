"""Cubature rolling-origin forecasts in one call against the linearised fan and the moment fan of the same build and against the composed
cubature path a user had before, in one process on the same GPU, with the protocol of tools/bench_forecast_linear.py (model builder,
time limit and statistics of tools/bench_moment_group.py): wall time around calls that end in a synchronisation, uploads, downloads
and the posteriors included; every side warmed up once, then measured alternately, median of --repeats runs with min-max.  No ratio
is fixed in advance.

Workload: a record of 200 rows, horizon 10, collapsed U, at the actuator shape (T = 512, M = 100, D = 4, S = 10) and at config 2
(T = 4096, M = 512, D = 4, S = 32), each with stride 10 (19 origins) and stride 1 (190 origins).

  cubature   `DGPSSM.forecast_heldout_cubature`: ffvd_op_posterior_forecast_cubature_grouped (posteriors, the cubature records launch
             with one record, passes of two launches per step, pooled summary);
  linear     `DGPSSM.forecast_heldout_linearised`;
  moment     `DGPSSM.forecast_heldout` (the moment fan); at config 2 with 190 origins it is not run: the figure is ten times the
             19-origin one and is marked `scaled_from_19_origins`;
  composed   ONE `DGPSSM.filter_records_cubature` call with one record per origin, each Y[:o + 1] followed by h all-NaN rows
             (lengths o + 1 + h): B (o + h) track steps where the fan takes n + B h.

The new call's tracks are compared with the composed path's rows o + 1 .. o + h of m_pred / S_pred (the largest difference and
whether the bits coincide go into the JSON).  ll_h / rmse_h at k = 1, 5, 10 of the three rules are reported side by side, and the
largest |m_fc - m_fc(moment)| of the linearised and of the cubature fan; the same figures on the actuator fixture of the tests (not
timed).

    python tools/bench_forecast_cubature.py [--repeats 5] [--out profiles/forecast_cubature.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_forecast_cubature.py --kernel-only POINT

The product kernel also runs in the call's filter stage (one record: 2D rows per group); the launches of the tracks are told from
those by the state kernel that precedes them in the trace.  Every GPU step runs under a time limit of its own (an alarm whose default
action ends the process); the child runs under a timeout."""
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

ROWS, HORIZON = 200, 10
ALL = ("cubature", "linear", "moment", "composed")
# point -> (shape, stride, sides)
POINTS = {"actuator_19": ("actuator", 10, ALL), "actuator_190": ("actuator", 1, ALL), "config2_19": ("config2", 10, ALL),
          "config2_190": ("config2", 1, ("cubature", "linear", "composed"))}
PEAK_FP64_MFMA = 78.6e12
AT = (0, 4, 9)                       # horizons 1, 5, 10
CALLS = 3                            # calls of the new path in the traced child


def kernel_figures(path, cfg, B):
    """A rocprofv3 kernel_trace.csv -> per kernel of the tracks (the state kernel -- the last launch of a pass, which writes no kernel
    rows, apart -- and the product launches that follow one) launches and mean duration per launch; for the product its flop/s
    (2 rows Mp^2 per launch, rows = tracks * D dims * 2D points) against the fp64 MFMA peak and the bytes of Gamma it reads per second
    (once per 128-row tile of a unit)."""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    dur = {"state": [], "state_last": [], "product": [], "filter_state": [], "filter_product": []}
    stage, held = None, None                                     # a state launch is filed when the next kernel is known: the last
    for r in rows:                                               # launch of a pass (t = h) writes no kernel rows and has no product
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        product = "mg_lfan_var_kernel" in name
        if held is not None:
            dur["state" if product else "state_last"].append(held)
            held = None
        if "mg_cfan_state_kernel" in name:
            stage, held = "", us
        elif "mg_crec_state_kernel" in name:
            stage = "filter_"
            dur["filter_state"].append(us)
        elif product and stage is not None:
            dur[stage + "product"].append(us)
        elif "mg_" not in name:
            stage = None
    if held is not None:
        dur["state_last"].append(held)
    out = {k: dict(launches=len(v), mean_launch_us=round(sum(v) / len(v), 3), min_launch_us=round(min(v), 3)) for k, v in dur.items() if v}
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    Mp = (M + 63) // 64 * 64
    # a call whose K block exceeds the scratch limit runs in several passes: the work of a step is spread over `passes` launches, so
    # the means per launch are taken against 1 / passes of it
    if "product" in out:
        passes = out["product"]["launches"] / float(CALLS * HORIZON)
        us, nrow = out["product"]["mean_launch_us"], G * B * 2 * D                       # rows per dim: one unit (no q slices here)
        flop, gam = 2.0 * nrow * D * Mp * Mp / passes, 8.0 * D * Mp * Mp * ((nrow + 127) // 128) / passes
        out["product"].update(passes_per_call=passes, rows_per_unit_and_step=nrow, units=D, mean_flop_per_launch=flop,
                              tflops=round(flop / (us * 1e-6) / 1e12, 3), fraction_of_fp64_mfma_peak=round(flop / (us * 1e-6) / PEAK_FP64_MFMA, 4),
                              gamma_gbytes_per_second=round(gam / (us * 1e-6) / 1e9, 1))
    if "state" in out:
        passes = out["state"]["launches"] / float(CALLS * HORIZON)
        us, k_bytes = out["state"]["mean_launch_us"], 8.0 * G * B * D * 2 * D * Mp / passes
        out["state"].update(passes_per_call=passes, tracks_per_step=G * B, us_per_track=round(us * passes / (G * B), 5),
                            k_write_gbytes_per_second=round(k_bytes / (us * 1e-6) / 1e9, 1))
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
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        B = len(range(0, ROWS - HORIZON, stride))
        return kernel_figures(found[0], SHAPES[shape], B) if found else dict(skipped="no kernel_trace.csv was written")


def fixture_fit(seconds):
    """The three rules on the actuator fixture (tests/golden/actuator_slim.npz: 400 training rows, three chains, a 40-row held-out
    record, every row an origin): the horizon curves at k = 1, 5, 10 and the distance of the two cheaper fans from the moment fan.
    Reported, not timed."""
    with limit(seconds):
        mod, c, Y_test = fixture_model()
        out = {k: f(Y_test, c, HORIZON, return_tracks=True) for k, f in (("cubature", mod.forecast_heldout_cubature),
                                                                          ("linear", mod.forecast_heldout_linearised),
                                                                          ("moment", mod.forecast_heldout))}
    return dict(rows=int(Y_test.shape[0]), origins=int(out["moment"]["origins"].shape[0]), horizons=[k + 1 for k in AT],
                rmse_h={k: [v["rmse_h"][i, 0] for i in AT] for k, v in out.items()}, ll_h={k: [v["ll_h"][i, 0] for i in AT] for k, v in out.items()},
                largest_difference_from_the_moment_fan={k: float(np.max(np.abs(out[k]["m_fc"] - out["moment"]["m_fc"]))) for k in ("cubature", "linear")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT", help="three calls of the new path at POINT and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        shape, stride, _ = POINTS[a.kernel_only]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[shape], ROWS)
        for _ in range(CALLS):
            with limit(a.limit):
                f = mod.forecast_heldout_cubature(Y_test, cc, HORIZON, stride=stride)
        print(json.dumps(dict(point=a.kernel_only, rmse_h=f["rmse_h"][:, 0].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace, models, moment19 = [], {}, {}, {}
    for point in [s for s in a.points.split(",") if s]:
        shape, stride, names = POINTS[point]
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
        # the composed path's records: record b is Y[:o + 1] followed by h all-NaN rows, its control rows those the fan reads
        Yr = np.full((B, ROWS, J), np.nan)
        for b, o in enumerate(origins):
            Yr[b, :o + 1] = Y_test[:o + 1]
        lengths = np.asarray([o + 1 + HORIZON for o in origins])
        cr = None if cc is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cc)[n_train: n_train + ROWS], (B, ROWS, np.shape(cc)[1])))

        def composed():
            f = mod.filter_records_cubature(Yr, cr, lengths=lengths)
            m_fc = np.stack([f["m_pred"][:, b, o + 1: o + 1 + HORIZON] for b, o in enumerate(origins)], axis=1)
            S_fc = np.stack([f["S_pred"][:, b, o + 1: o + 1 + HORIZON] for b, o in enumerate(origins)], axis=1)
            return dict(m_fc=m_fc, S_fc=S_fc)

        sides = {"cubature": lambda: mod.forecast_heldout_cubature(Y_test, cc, HORIZON, stride=stride, return_tracks=True),
                 "linear": lambda: mod.forecast_heldout_linearised(Y_test, cc, HORIZON, stride=stride, return_tracks=True),
                 "moment": lambda: mod.forecast_heldout(Y_test, cc, HORIZON, stride=stride, return_tracks=True),
                 "composed": composed}
        sides = {k: sides[k] for k in names}

        def run(k):
            out[k] = sides[k]()

        for k in sides:                                         # one warm-up per side
            timed_ms(lambda: run(k), a.limit)
        ts = {k: [] for k in sides}
        for _ in range(a.repeats):                              # alternating, so that all see the same neighbours on the machine
            for k in sides:
                ts[k].append(timed_ms(lambda: run(k), a.limit))
        med = {k: statistics.median(v) for k, v in ts.items()}
        cub = out["cubature"]
        row = dict(point=point, shape=shape, T=cfg["T"], M=cfg["M"], D=D, S=S, rows=ROWS, horizon=HORIZON, stride=stride, origins=B,
                   tracks=S * B, ms_median_min_max={k: stats(v) for k, v in ts.items()},
                   cubature_launches=2 * ROWS + 1 + 2 * HORIZON + 1, horizons=[k + 1 for k in AT],
                   rmse_h={k: [out[k]["rmse_h"][i, 0] for i in AT] for k in ("cubature", "linear", "moment") if k in out},
                   ll_h={k: [out[k]["ll_h"][i, 0] for i in AT] for k in ("cubature", "linear", "moment") if k in out},
                   linear_over_cubature=round(med["linear"] / med["cubature"], 3),
                   composed_over_cubature=round(med["composed"] / med["cubature"], 3))
        if "moment" in out:
            if stride == 10:
                moment19[shape] = med["moment"]
            row["moment_over_cubature"] = round(med["moment"] / med["cubature"], 3)
            row["largest_difference_from_the_moment_fan"] = dict(cubature=float(np.max(np.abs(cub["m_fc"] - out["moment"]["m_fc"]))),
                                                                 linear=float(np.max(np.abs(out["linear"]["m_fc"] - out["moment"]["m_fc"]))))
        elif shape in moment19:
            scaled = moment19[shape] * B / 19.0
            row["moment_scaled_from_19_origins"] = dict(ms=round(scaled, 3), moment_over_cubature=round(scaled / med["cubature"], 3))
        two = out["composed"]
        row["largest_difference_from_the_composed_path"] = dict(
            m_fc=float(np.max(np.abs(cub["m_fc"] - two["m_fc"]))), S_fc=float(np.max(np.abs(cub["S_fc"] - two["S_fc"]))),
            bit_identical=bool(np.array_equal(cub["m_fc"], two["m_fc"]) and np.array_equal(cub["S_fc"], two["S_fc"])))
        row["composed_track_steps"], row["cubature_track_steps"] = int(lengths.sum()), ROWS + B * HORIZON
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not a.no_trace:
            trace[point] = kernel_trace(point, 4 * a.limit)
            print(json.dumps({point: trace[point]}), flush=True)
    fixture = fixture_fit(a.limit)
    print(json.dumps(dict(actuator_fixture=fixture)), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_forecast_cubature.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.forecast_heldout_cubature: ffvd_op_posterior_forecast_cubature_grouped (posteriors, the cubature records "
                        "launches with one record, passes of a state and a product launch per step, pooled summary)",
               baselines=dict(linear="DGPSSM.forecast_heldout_linearised of the same build",
                              moment="DGPSSM.forecast_heldout (the moment fan) of the same build; config 2 with 190 origins scaled from 19",
                              composed="one DGPSSM.filter_records_cubature call with one record per origin, Y[:o + 1] followed by h "
                                       "all-NaN rows: of the same build"),
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               points=rows, kernels=trace or None, actuator_fixture=fixture)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
