"""Linearised filtering of R held-out records in one call against the loop over the records a caller had before, of the same build, in
one process on the same GPU, with the protocol of tools/bench_forecast_linear.py (model builder, time limit and statistics of
tools/bench_moment_group.py): wall time around calls that end in a synchronisation, uploads and the posteriors included; every side
warmed up once, then measured alternately, median of --repeats runs with min-max.  No ratio is fixed in advance: the tool reports, per
shape, the R at which the call first beats the loop and the ratio at every R.

Workload: records of 200 rows, R = 1, 8, 32, 128, seeded observations, control rows and starts.
  actuator            T = 512, M = 100, D = 4, S = 10, collapsed U:
                        records  `posterior_filter_records_grouped` (posteriors, passes of a state and a product launch per step);
                        loop     `collapse_u_mean_grouped` once, then one `filter_grouped(method="linearised")` call per record.
  actuator_explicit   the same shape, explicit U shared by the chains (no q slices: one Gamma per dim, all tracks of a pass in its rows):
                        records  `kernel_pre_cal` once, `filter_records_grouped`;
                        loop     `kernel_pre_cal` once, one `filter_grouped(method="linearised")` call per record.
  config2             T = 4096, M = 512, D = 4, S = 32, collapsed U: as actuator.
The tracks of the call are compared with the loop's: over the first 30 rows against the project's floors (1e-11 + 1e-9 max|.| on means,
1e-11 + 1e-8 max|.| on covariances), and over the whole record, where the recursion amplifies the two sides' different summation orders
on some tracks (the records are noise, not data from the model); the largest differences go into the JSON.

    python tools/bench_filter_records.py [--repeats 5] [--out profiles/filter_records.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures (time per launch of the state and the product kernel, the product's flop/s against the fp64 MFMA peak of
profiles/forecast_linear.json) come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_records.py --kernel-only POINT:R

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

ROWS, HEAD = 200, 30
RECORDS = (1, 8, 32, 128)
# point -> (shape, collapsed U)
POINTS = {"actuator": ("actuator", True), "actuator_explicit": ("actuator", False), "config2": ("config2", True)}
PEAK_FP64_MFMA = 78.6e12
MOMENTS = ("m_pred", "S_pred", "m_filt", "S_filt", "cross")


def floor(key, ref):
    return 1e-11 + (1e-9 if key.startswith("m_") else 1e-8) * float(np.max(np.abs(ref)))


def data(meta, R, mod):
    """R seeded records: observations, control rows, starts around every chain's last training state"""
    rng = np.random.default_rng(100 + R)
    S, D, C = meta["S"], meta["D"], meta["C"]
    Y, ctrl = rng.standard_normal((R, ROWS, 1)), rng.standard_normal((R, ROWS, C))
    x0 = np.stack([mod._X_chains[s][-1] for s in range(S)])[:, None, :] + 0.1 * rng.standard_normal((S, R, D))
    return Y, ctrl, x0


def sides_of(mod, meta, collapsed, Y, ctrl, x0):
    """the two sides of a point as callables that return the per-track arrays (S, R, rows, ...)"""
    S, R = meta["S"], Y.shape[0]
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, Qs, em = [mod._X_chains[s] for s in range(S)], [mod.Q] * S, (lik.CC, lik.DD, lik.log_Rchols)

    def posterior():
        if collapsed:
            U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, Xs, mod.control_inputs, mod.Q)
            return list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv)
        return cmo.kernel_pre_cal(lay.Z, lay.kernel), lay.Z, lay.kernel, [lay.U] * S, None

    def records():
        if collapsed:
            return pr.posterior_filter_records_grouped(lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, x0s=x0)
        return pr.filter_records_grouped(*posterior(), x0, ctrl, Y, Qs, *em)

    def loop():
        post = posterior()
        outs = [pr.filter_grouped(*post, list(x0[:, r]), ctrl[r], 0, Y[r], Qs, *em, method="linearised") for r in range(R)]
        return {k: np.stack([o[k] for o in outs], axis=1) for k in MOMENTS + ("lpd_mix",)}
    return dict(records=records, loop=loop)


def kernel_figures(path, cfg, R, collapsed):
    """The state and the product kernel in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; for the product its
    flop/s (2 tracks D Mp^2 per launch) against the fp64 MFMA peak and the bytes of Gamma it reads per second (once per row tile)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, pick in (("state", lambda n: "mg_lrec_state_kernel" in n), ("product", lambda n: "mg_lfan_var_kernel" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    Mp = (M + 63) // 64 * 64
    if "product" in out:
        us = out["product"]["mean_launch_us"]
        units, rows_per_unit = (G * D, R) if collapsed else (D, G * R)
        flop, gam = 2.0 * G * R * D * Mp * Mp, 8.0 * units * Mp * Mp * ((rows_per_unit + 127) // 128)
        out["product"].update(tracks=G * R, flop_per_launch=flop, tflops=round(flop / (us * 1e-6) / 1e12, 3),
                              fraction_of_fp64_mfma_peak=round(flop / (us * 1e-6) / PEAK_FP64_MFMA, 4),
                              gamma_gbytes_per_second=round(gam / (us * 1e-6) / 1e9, 1))
    if "state" in out:
        out["state"].update(tracks=G * R, us_per_track=round(out["state"]["mean_launch_us"] / (G * R), 5))
    return out


def kernel_trace(point, R, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the new path at `point` with R records."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    shape, collapsed = POINTS[point]
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{point}:{R}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0], SHAPES[shape], R, collapsed) if found else dict(skipped="no kernel_stats.csv was written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default="actuator,actuator_explicit,config2")
    ap.add_argument("--records", default=",".join(str(r) for r in RECORDS))
    ap.add_argument("--trace-records", default="32,128", help="the R at which the kernels are traced")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R", help="three calls of the new path and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        point, R = a.kernel_only.split(":")
        shape, collapsed = POINTS[point]
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[shape], ROWS)
        new = sides_of(mod, meta, collapsed, *data(meta, int(R), mod))["records"]
        for _ in range(3):
            with limit(a.limit):
                f = new()
        print(json.dumps(dict(point=point, R=int(R), ll=f["ll"][:4].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace, models, crossover = [], {}, {}, {}
    counts, traced = [int(r) for r in a.records.split(",") if r], [int(r) for r in a.trace_records.split(",") if r]
    for point in [s for s in a.points.split(",") if s]:
        shape, collapsed = POINTS[point]
        cfg = SHAPES[shape]
        if shape not in models:
            with limit(a.limit):
                models[shape] = model(cfg, ROWS)
        mod, cc, _, meta = models[shape]
        for R in counts:
            sides, out = sides_of(mod, meta, collapsed, *data(meta, R, mod)), {}

            def run(k):
                out[k] = sides[k]()

            for k in sides:                                         # every side warmed up once
                timed_ms(lambda: run(k), a.limit)
            ts = {k: [] for k in sides}
            for _ in range(a.repeats):                              # alternating, so that both see the same neighbours on the machine
                for k in sides:
                    ts[k].append(timed_ms(lambda: run(k), a.limit))
            med = {k: statistics.median(v) for k, v in ts.items()}
            # the two sides add the same products in different orders, and the recursion of a filter over 200 rows of noise amplifies
            # that on some tracks: the difference is reported over the whole record, over its first HEAD rows, and as the number of
            # tracks on which the filtered means part by more than 1e-9 anywhere
            diff = {k: float(np.max(np.abs(out["records"][k] - out["loop"][k]))) for k in MOMENTS}
            head = {k: float(np.max(np.abs(out["records"][k][:, :, :HEAD] - out["loop"][k][:, :, :HEAD]))) for k in MOMENTS}
            within = all(head[k] <= floor(k, out["loop"][k][:, :, :HEAD]) for k in MOMENTS)
            apart = int(np.sum(np.max(np.abs(out["records"]["m_filt"] - out["loop"]["m_filt"]), axis=(2, 3)) > 1e-9))
            row = dict(point=point, shape=shape, collapsed_U=collapsed, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R,
                       tracks=meta["S"] * R, ms_median_min_max={k: stats(v) for k, v in ts.items()},
                       loop_over_records=round(med["loop"] / med["records"], 3), faster="records" if med["records"] < med["loop"] else "loop",
                       launch_pairs=ROWS + 1, wall_us_per_launch_pair=round(med["records"] * 1e3 / (ROWS + 1), 2),
                       loop_launches=R * (ROWS + 1), loop_wall_us_per_launch=round(med["loop"] * 1e3 / (R * (ROWS + 1)), 2),
                       largest_difference_from_the_loop=dict(whole_record=diff, first_rows=dict(head, rows=HEAD, within_the_floors=bool(within)),
                                                             tracks_with_filtered_means_apart_by_more_than_1e_9=apart),
                       ll_all=dict(records=float(out["records"]["ll_all"]), loop=float(np.mean(out["loop"]["lpd_mix"]))))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if row["faster"] == "records" and point not in crossover:
                crossover[point] = R
            if not a.no_trace and R in traced:
                trace[f"{point}:{R}"] = kernel_trace(point, R, 4 * a.limit)
                print(json.dumps({f"{point}:{R}": trace[f"{point}:{R}"]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_records.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="filter_records_grouped / posterior_filter_records_grouped: the posteriors once, passes of a state and a product "
                        "launch per step for all (chain, record) tracks",
               baseline="the loop of the same build: the posteriors once (collapse_u_mean_grouped or kernel_pre_cal), then one "
                        "filter_grouped(method='linearised') call per record",
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               first_R_at_which_the_call_beats_the_loop={p: crossover.get(p) for p in a.points.split(",") if p},
               points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
