"""Particle smoothing on the ADAPTED filter's sets of R held-out records in one call against two calls of the same build, in one process
on the same GPU, with the protocol of tools/bench_smooth_particle.py: wall time around calls that end in a synchronisation, uploads,
downloads and the posteriors included; every side warmed up once, then measured alternately, median of --repeats runs with min-max.
No time and no ratio is fixed in advance.

Workload: that of tools/bench_smooth_particle.py -- records of 200 rows, R = 1 and 8, N = 64, 256, 1024 particles (config 2: 896),
one set of draws shared by all tracks;  actuator: T = 512, M = 100, D = 4, S = 10;  config2: T = 4096, M = 512, D = 4, S = 32.
Sides:
  smooth     `posterior_smooth_adapted_records_grouped`: the adapted filter's launches with the keep kernel per step, then the
             normalisers of all rows in one launch, ONE backward launch per row, the moments;
  filter     `posterior_filter_adapted_records_grouped` of the same build on the same inputs: smooth - filter is the smoother's added
             cost;
  bootstrap  `posterior_smooth_particle_records_grouped` of the same build on the same draws: the bootstrap filter, a weights launch
             and TWO backward launches per row (omega, then its fold through the ancestors).
Reported, not asserted: ess_smooth (smallest, median) of both smoothers at every point, and at the largest N on the 200-row record of
tools/bench_filter_linear.py the standard deviation of m_smooth over --seeds seeds for both.

    python tools/bench_smooth_adapted.py [--repeats 5] [--out profiles/smooth_adapted.json] [--commit HASH] [--limit 120] [--no-trace]

The per-launch times of the new backward kernel (and of the normaliser, the keep and the moments kernels beside it) come from a trace
the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_smooth_adapted.py --kernel-only POINT:R:N

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
from bench_filter_particle import PARTICLES, POINTS, RECORDS, draws, largest_n
from bench_filter_records import ROWS, data
from bench_moment_group import SHAPES, STEPS, limit, model, stats, timed_ms
from ffvd_amd import prediction as pr

KERNELS = (("keep", "mg_psm_keep_kernel"), ("normaliser", "mg_psm_norm_kernel"), ("backward", "mg_pasm_back_kernel"),
           ("moments", "mg_psm_moments_kernel"), ("filter_weight", "mg_parec_weight_kernel"), ("filter_rows", "mg_prec_rows_kernel"),
           ("filter_product", "mg_lfan_var_kernel"))
CALLS_TRACED = 3


def sides_of(mod, meta, Y, ctrl, x0, N):
    """the three sides of a point as callables that return dicts"""
    S, D = meta["S"], meta["D"]
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, em = [mod._X_chains[s] for s in range(S)], (lik.CC, lik.DD, lik.log_Rchols)
    eps, unif = draws(N, D, 1)
    args = (lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, eps, unif)
    return dict(smooth=lambda: pr.posterior_smooth_adapted_records_grouped(*args, x0s=x0),
                filter=lambda: pr.posterior_filter_adapted_records_grouped(*args, x0s=x0),
                bootstrap=lambda: pr.posterior_smooth_particle_records_grouped(*args, x0s=x0))


def kernel_figures(path, cfg, R, N):
    """The kernels of the smoothing path in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; as an upper bound
    (columns of weight 0 are skipped) the exps per second of the backward kernel, tracks * N * N pairs per launch."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, name in KERNELS:
        hit = [r for r in rows if name in r.get("Name", "")]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3),
                            total_ms_per_call=round(total * 1e-6 / CALLS_TRACED, 3))
    V = cfg["S"] * R
    if "backward" in out:
        pairs = float(V) * N * N
        out["backward"].update(workgroups=V * ((N + 255) // 256), pairs_per_launch=pairs,
                               gexps_per_second_upper_bound=round(pairs / (out["backward"]["mean_launch_us"] * 1e-6) / 1e9, 2))
    return out


def kernel_trace(point, R, N, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the smoothing path at `point` with R records and N particles."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{point}:{R}:{N}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0], SHAPES[point], R, N) if found else dict(skipped="no kernel_stats.csv was written")


def ess_of(out):
    e = out["ess_smooth"]
    return dict(smallest=float(np.nanmin(e)), median=float(np.nanmedian(e)))


def scatter(mod, Y_test, cc, n_train, seeds, N):
    """On one record that continues the training sequence: the standard deviation of m_smooth over `seeds` seeds for both smoothers (the
    same seeds, hence the same draws), and the largest difference of their means over the seeds."""
    Yr, cr = Y_test[None], cc[n_train: n_train + len(Y_test)][None]
    runs = {k: np.stack([fn(Yr, cr, num_particles=N, seed=100 + s)["m_smooth"][:, 0] for s in range(seeds)])
            for k, fn in (("adapted", mod.smooth_records_adapted), ("bootstrap", mod.smooth_records_particle))}
    sd = {k: v.std(axis=0, ddof=1) for k, v in runs.items()}
    return dict(particles=N, seeds=seeds, sd_of_m_smooth={k: dict(largest=float(v.max()), median=float(np.median(v))) for k, v in sd.items()},
                median_sd_ratio_bootstrap_over_adapted=float(np.median(sd["bootstrap"]) / np.median(sd["adapted"])),
                largest_difference_of_the_means_over_seeds=float(np.max(np.abs(runs["adapted"].mean(axis=0) - runs["bootstrap"].mean(axis=0)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", default=",".join(str(r) for r in RECORDS))
    ap.add_argument("--particles", default=",".join(str(n) for n in PARTICLES))
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--trace", default="1:1024,8:256", help="the R:N at which the kernels are traced")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N", help="three calls of the smoothing path and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-scatter", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        point, R, N = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        new = sides_of(mod, meta, *data(meta, int(R), mod), int(N))["smooth"]
        for _ in range(CALLS_TRACED):
            with limit(a.limit):
                f = new()
        print(json.dumps(dict(point=point, R=int(R), N=int(N), smallest_ess_smooth=float(np.min(f["ess_smooth"])))))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace, scat = [], {}, {}
    counts, asked = [int(r) for r in a.records.split(",") if r], [int(n) for n in a.particles.split(",") if n]
    traced = [tuple(int(v) for v in t.split(":")) for t in a.trace.split(",") if t]
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        ns = sorted({min(n, largest_n(cfg)) for n in asked})        # (an N beyond the point's limit is run at the limit)
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        assert ROWS == STEPS
        if not a.no_scatter:
            with limit(4 * a.limit):
                scat[point] = scatter(mod, Y_test, cc, cfg["T"], a.seeds, max(ns))
            print(json.dumps({point: scat[point]}), flush=True)
        for R in counts:
            for N in ns:
                sides, out = sides_of(mod, meta, *data(meta, R, mod), N), {}

                def run(k):
                    out[k] = sides[k]()

                for k in sides:                                     # every side warmed up once
                    timed_ms(lambda: run(k), a.limit)
                ts = {k: [] for k in sides}
                for _ in range(a.repeats):                          # alternating, so that all see the same neighbours on the machine
                    for k in sides:
                        ts[k].append(timed_ms(lambda: run(k), a.limit))
                med = {k: statistics.median(v) for k, v in ts.items()}
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, tracks=meta["S"] * R,
                           ms_median_min_max={k: stats(v) for k, v in ts.items()},
                           smoother_added_ms=round(med["smooth"] - med["filter"], 3), smooth_over_filter=round(med["smooth"] / med["filter"], 3),
                           smooth_over_bootstrap_smooth=round(med["smooth"] / med["bootstrap"], 3),
                           slower_than_the_bootstrap_smoothing_call=bool(med["smooth"] > med["bootstrap"]),
                           ess_smooth=dict(adapted=ess_of(out["smooth"]), bootstrap=ess_of(out["bootstrap"])),
                           filter_keys_bit_identical=all(np.array_equal(out["smooth"][k], out["filter"][k], equal_nan=True)
                                                         for k in out["filter"] if isinstance(out["filter"][k], np.ndarray)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not a.no_trace and (R, N) in [(r, min(n, largest_n(cfg))) for r, n in traced]:
                    trace[f"{point}:{R}:{N}"] = kernel_trace(point, R, N, 4 * a.limit)
                    print(json.dumps({f"{point}:{R}:{N}": trace[f"{point}:{R}:{N}"]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_smooth_adapted.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_smooth_adapted_records_grouped: the adapted particle filter's launches with one keep launch per step, then "
                        "the normalisers of all rows in one launch, one backward launch per row for all tracks, the moments",
               baselines=dict(filter="posterior_filter_adapted_records_grouped of the same build on the same inputs: the difference is the "
                                     "smoother's added cost",
                              bootstrap="posterior_smooth_particle_records_grouped of the same build on the same draws: the bootstrap filter, "
                                        "a weights launch and two backward launches per row"),
               timing="wall time around calls that end in a synchronisation, uploads and downloads included; alternating after one warm-up "
                      "call per side",
               scatter_reported_not_asserted=scat or None, points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
