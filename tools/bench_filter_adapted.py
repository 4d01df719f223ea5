"""Fully adapted particle filtering of R held-out records in one call against the bootstrap particle filter of the same build, in one
process on the same GPU, with the protocol of tools/bench_filter_particle.py (its workload, draws and limits; model builder, time limit
and statistics of tools/bench_moment_group.py): wall time around calls that end in a synchronisation, uploads, downloads and the
posteriors included; every side warmed up once, then measured alternately, median of --repeats runs with min-max.  No time and no
ratio is fixed in advance; nothing here is asserted.

Workload: records of 200 rows, R = 1 and 8, N = 64, 256, 1024 particles (config 2: 896, the most whose rows fit the K scratch of a
pass), seeded observations, control rows and starts (those of tools/bench_filter_records.py), one set of draws shared by all tracks.
  actuator   T = 512, M = 100, D = 4, S = 10, collapsed U;   config2   T = 4096, M = 512, D = 4, S = 32, collapsed U.
Sides:
  adapted      `posterior_filter_adapted_records_grouped` (the adapted weight kernel, then the bootstrap filter's rows and product launches);
  bootstrap    `posterior_filter_particle_records_grouped` on the same draws.
Per point also: the smallest and the median ess of both filters on those draws; over --seeds further seeds of the draws the standard
deviation of ll_all and of log_evidence (mean over the tracks) of both; and from those the figure a user chooses by -- the time each
filter needs for the same standard error.  The variance of both estimates falls as 1 / N and the time of a call grows with N, so a
filter needs (its variance) x (its time) per unit of precision; `bootstrap_over_adapted_time_for_equal_se` is the ratio of the two
products at this N, above 1 where the adapted filter is the cheaper way to a given standard error.

    python tools/bench_filter_adapted.py [--repeats 5] [--out profiles/filter_adapted.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures (time per launch of the adapted weight kernel and of the bootstrap one, of the rows and the product kernel) come
from traces the tool starts itself, each in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_adapted.py --kernel-only POINT:R:N:SIDE

Every GPU step runs under a time limit of its own (an alarm whose default action ends the process); the children run under a timeout."""
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

SIDES = dict(adapted=pr.posterior_filter_adapted_records_grouped, bootstrap=pr.posterior_filter_particle_records_grouped)
KERNELS = (("adapted_weight", "mg_parec_weight_kernel"), ("bootstrap_weight", "mg_prec_weight_kernel"), ("rows", "mg_prec_rows_kernel"),
           ("product", "mg_lfan_var_kernel"))


def sides_of(mod, meta, Y, ctrl, x0, N, seed=1):
    """the two sides of a point as callables that return dicts, on the draws of `seed`"""
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, em = [mod._X_chains[s] for s in range(meta["S"])], (lik.CC, lik.DD, lik.log_Rchols)
    eps, unif = draws(N, meta["D"], seed)
    return {k: (lambda fn=fn: fn(lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, eps, unif, x0s=x0)) for k, fn in SIDES.items()}


def kernel_figures(path):
    """The kernels of a rocprofv3 kernel_stats.csv -> launches and mean duration per launch"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, word in KERNELS:
        hit = [r for r in rows if word in r.get("Name", "")]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    return out


def kernel_trace(point, R, N, side, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of one side at `point` with R records and N particles."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{point}:{R}:{N}:{side}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0]) if found else dict(skipped="no kernel_stats.csv was written")


def scatter(mod, meta, args, N, seeds, seconds):
    """sd of ll_all and of log_evidence (mean over the tracks) over `seeds` seeds of the draws, for both filters on the same draws"""
    ll, ev = {k: [] for k in SIDES}, {k: [] for k in SIDES}
    for s in range(seeds):
        sides = sides_of(mod, meta, *args, N, seed=100 + s)
        for k in SIDES:
            with limit(seconds):
                out = sides[k]()
            ll[k].append(float(out["ll_all"]))
            ev[k].append(float(np.mean(out["log_evidence"])))
    return {k: dict(seeds=seeds, ll_all_mean=float(np.mean(ll[k])), ll_all_sd=float(np.std(ll[k], ddof=1)),
                    log_evidence_mean=float(np.mean(ev[k])), log_evidence_sd=float(np.std(ev[k], ddof=1))) for k in SIDES}


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
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N:SIDE", help="three calls of one side and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--merge", nargs="*", default=None, help="JSON files of earlier runs (other --points) whose points, kernels are merged in")
    a = ap.parse_args()
    if a.kernel_only:
        point, R, N, side = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        new = sides_of(mod, meta, *data(meta, int(R), mod), int(N))[side]
        for _ in range(3):
            with limit(a.limit):
                f = new()
        print(json.dumps(dict(point=point, R=int(R), N=int(N), side=side, ll=f["ll"][:4].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace = [], {}
    for path in a.merge or []:
        with open(path) as f:
            old = json.load(f)
        rows += old.get("points") or []
        trace.update(old.get("kernels") or {})
    counts, asked = [int(r) for r in a.records.split(",") if r], [int(n) for n in a.particles.split(",") if n]
    traced = [tuple(int(v) for v in t.split(":")) for t in a.trace.split(",") if t]
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        ns = sorted({min(n, largest_n(cfg)) for n in asked})        # (an N beyond the point's limit is run at the limit)
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        assert ROWS == STEPS
        for R in counts:
            args = data(meta, R, mod)
            for N in ns:
                sides, out = sides_of(mod, meta, *args, N), {}

                def run(k):
                    out[k] = sides[k]()

                for k in sides:                                     # every side warmed up once
                    timed_ms(lambda: run(k), a.limit)
                ts = {k: [] for k in sides}
                for _ in range(a.repeats):                          # alternating, so that both see the same neighbours on the machine
                    for k in sides:
                        ts[k].append(timed_ms(lambda: run(k), a.limit))
                med = {k: statistics.median(v) for k, v in ts.items()}
                sc = scatter(mod, meta, args, N, a.seeds, a.limit) if a.seeds > 1 else None
                cost = None
                if sc:                                              # (variance) x (time): what a unit of precision costs at this N
                    cost = {w: {k: sc[k][w + "_sd"] ** 2 * med[k] for k in SIDES} for w in ("ll_all", "log_evidence")}
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, tracks=meta["S"] * R,
                           ms_median_min_max={k: stats(v) for k, v in ts.items()}, adapted_over_bootstrap=round(med["adapted"] / med["bootstrap"], 4),
                           wall_us_per_step={k: round(med[k] * 1e3 / (ROWS + 1), 2) for k in SIDES},
                           ll_all={k: float(out[k]["ll_all"]) for k in SIDES},
                           smallest_ess={k: float(np.min(out[k]["ess"])) for k in SIDES},
                           median_ess={k: float(np.median(out[k]["ess"])) for k in SIDES}, scatter_over_seeds=sc,
                           variance_times_ms=cost,
                           bootstrap_over_adapted_time_for_equal_se=None if not cost else
                           {w: (round(c["bootstrap"] / c["adapted"], 3) if c["adapted"] > 0 else None) for w, c in cost.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not a.no_trace and (R, N) in [(r, min(n, largest_n(cfg))) for r, n in traced]:
                    for side in SIDES:
                        trace[f"{point}:{R}:{N}:{side}"] = kernel_trace(point, R, N, side, 4 * a.limit)
                        print(json.dumps({f"{point}:{R}:{N}:{side}": trace[f"{point}:{R}:{N}:{side}"]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_adapted.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_filter_adapted_records_grouped: the posteriors once, passes of the adapted weight launch, the rows launch "
                        "and the product launch per step for all (chain, record) tracks; one set of draws shared by the tracks",
               baseline="posterior_filter_particle_records_grouped of the same build on the same draws",
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               equal_se="variance x time per filter at each N (the variance of both estimates falls as 1 / N); nothing is asserted",
               points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
