"""Particle filtering of R held-out records with adaptive (ESS-triggered) resampling against the bootstrap particle filter, in one
process on the same GPU, with the protocol of tools/bench_filter_particle.py (its workload, draws and limits; model builder, time limit
and statistics of tools/bench_moment_group.py): wall time around calls that end in a synchronisation, uploads, downloads and the
posteriors included; every side warmed up once, then measured alternately, median of --repeats runs with min-max.  No time and no
ratio is fixed in advance; nothing here is asserted.

Workload: records of 200 rows, R = 1 and 8, N = 64, 256, 1024 particles (config 2: 896), seeded observations, control rows and starts
(those of tools/bench_filter_records.py), one set of draws shared by all tracks.
  actuator   T = 512, M = 100, D = 4, S = 10, collapsed U;   config2   T = 4096, M = 512, D = 4, S = 32, collapsed U.
(a) Time.  Sides, all on the same draws:
  adaptive_2.0   `posterior_filter_adaptive_records_grouped(ess_threshold=2.0)`: every observed row resamples -- the bootstrap call's work;
  adaptive_0.5   the same at the default threshold;
  bootstrap      `posterior_filter_particle_records_grouped` of this build;
  parent         the same call of ANOTHER checkout (--parent ROOT, built there), served by a child process that loads that checkout's
                 package and library and answers one call per request, so that the four alternate.
`adaptive_2.0_slower_than_spread` says whether adaptive_2.0's median exceeds bootstrap's by more than bootstrap's own min-max spread.
Per point also DGPSSM.filter_records_adaptive with noise="independent": draws="device" (the seeded form) against draws="numpy".
(b) What it buys (--scatter R:N points; reported, not asserted).  Over --seeds seeds of the draws, on the tool's records as generated
and with every second row set to NaN, at thresholds 0.5 and 2.0: the share of the observed rows that resample, the standard deviation
of log_evidence (mean over the tracks) and of ll_all, the median and the smallest ess.

    python tools/bench_filter_adaptive.py [--repeats 5] [--out profiles/filter_adaptive.json] [--commit HASH] [--parent ROOT] [--no-trace]

The kernel figures (time per launch of the adaptive weight kernel and of the bootstrap one, of the rows and the product kernel) come
from traces the tool starts itself, each in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_adaptive.py --kernel-only POINT:R:N:SIDE

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

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
if "--root" in sys.argv:                                          # (the served child: another checkout's package, library and tools)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from bench_filter_particle import PARTICLES, POINTS, RECORDS, draws, largest_n
from bench_filter_records import ROWS, data
from bench_moment_group import SHAPES, STEPS, limit, model, stats, timed_ms
from ffvd_amd import prediction as pr

THRESHOLDS = (2.0, 0.5)
KERNELS = (("adaptive_weight", "mg_pess_weight_kernel"), ("bootstrap_weight", "mg_prec_weight_kernel"), ("rows", "mg_prec_rows_kernel"),
           ("product", "mg_lfan_var_kernel"))


def sides_of(mod, meta, Y, ctrl, x0, N, seed=1, bootstrap_only=False):
    """the sides of a point as callables that return dicts, on the draws of `seed`"""
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, em = [mod._X_chains[s] for s in range(meta["S"])], (lik.CC, lik.DD, lik.log_Rchols)
    eps, unif = draws(N, meta["D"], seed)
    head = (lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, eps, unif)
    out = dict(bootstrap=lambda: pr.posterior_filter_particle_records_grouped(*head, x0s=x0))
    if not bootstrap_only:
        for thr in THRESHOLDS:
            out[f"adaptive_{thr}"] = lambda thr=thr: pr.posterior_filter_adaptive_records_grouped(*head, x0s=x0, ess_threshold=thr)
    return out


def serve(seconds):
    """The child of --parent: per request line "POINT R N" one bootstrap call of this process's checkout (warmed up once per triple),
    answered with its milliseconds."""
    built, warm = {}, set()
    for line in sys.stdin:
        point, R, N = line.split()
        if point not in built:
            with limit(seconds):
                mod, _, _, meta = model(SHAPES[point], ROWS)
            built[point] = (mod, meta)
        mod, meta = built[point]
        call = sides_of(mod, meta, *data(meta, int(R), mod), int(N), bootstrap_only=True)["bootstrap"]
        if (point, R, N) not in warm:
            timed_ms(call, seconds)
            warm.add((point, R, N))
        print(json.dumps(timed_ms(call, seconds)), flush=True)
    return 0


class Parent:
    """the served child of another checkout; ms(point, R, N) -> the wall time of one bootstrap call there"""

    def __init__(self, root, seconds):
        root, env = os.path.abspath(root), dict(os.environ)
        env.pop("FFVD_LIB", None)
        self.proc = subprocess.Popen([sys.executable, HERE, "--serve", "--root", root, "--limit", str(seconds)], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, text=True, env=env, cwd=root)

    def ms(self, point, R, N):
        self.proc.stdin.write(f"{point} {R} {N}\n")
        self.proc.stdin.flush()
        line = self.proc.stdout.readline()
        if not line:
            raise RuntimeError(f"the served child of --parent ended with {self.proc.wait()}")
        return float(json.loads(line))

    def close(self):
        self.proc.stdin.close()
        self.proc.wait(timeout=60)


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
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, HERE, "--kernel-only",
               f"{point}:{R}:{N}:{side}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0]) if found else dict(skipped="no kernel_stats.csv was written")


def scatter(mod, meta, args, N, seeds, seconds):
    """(b): per workload (the records as generated; every second row NaN) and threshold, over `seeds` seeds of the draws"""
    Y, ctrl, x0 = args
    half = np.array(Y)
    half[:, 1::2] = np.nan
    out = {}
    for name, Yw in (("as_generated", Y), ("half_the_rows_nan", half)):
        res = {f"adaptive_{thr}": dict(ev=[], ll=[], ess=[], share=[]) for thr in THRESHOLDS}
        for s in range(seeds):
            sides = sides_of(mod, meta, Yw, ctrl, x0, N, seed=100 + s)
            for k, acc in res.items():
                with limit(seconds):
                    o = sides[k]()
                seen = ~np.isnan(o["lpd_joint"])
                acc["ev"].append(float(np.mean(o["log_evidence"])))
                acc["ll"].append(float(o["ll_all"]))
                acc["ess"].append(o["ess"][seen])
                acc["share"].append(float(np.mean(o["resampled"][seen] == 1)))
        out[name] = {k: dict(seeds=seeds, share_of_observed_rows_resampled=round(float(np.mean(a["share"])), 4),
                             log_evidence_mean=float(np.mean(a["ev"])), log_evidence_sd=float(np.std(a["ev"], ddof=1)),
                             ll_all_mean=float(np.mean(a["ll"])), ll_all_sd=float(np.std(a["ll"], ddof=1)),
                             median_ess=float(np.median(np.concatenate(a["ess"]))), smallest_ess=float(np.min(np.concatenate(a["ess"]))))
                     for k, a in res.items()}
    return out


def seeded_against_numpy(mod, args, N, repeats, seconds):
    """DGPSSM.filter_records_adaptive with noise="independent": the draws generated on the device against NumPy's, generation included"""
    Y, ctrl, x0 = args
    calls = {d: (lambda d=d: mod.filter_records_adaptive(Y, ctrl, num_particles=N, x0=x0, seed=1, noise="independent", draws=d))
             for d in ("device", "numpy")}
    refused = None
    for k in list(calls):
        try:
            timed_ms(calls[k], seconds)
        except ValueError as e:                                     # (NumPy draws beyond 1 GiB are refused; the device's are not)
            refused = {k: str(e)}
            del calls[k]
    ts = {k: [] for k in calls}
    for _ in range(repeats):
        for k in calls:
            ts[k].append(timed_ms(calls[k], seconds))
    return dict(ms_median_min_max={k: stats(v) for k, v in ts.items()}, refused=refused,
                device_over_numpy=round(statistics.median(ts["device"]) / statistics.median(ts["numpy"]), 4) if "numpy" in ts else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", default=",".join(str(r) for r in RECORDS))
    ap.add_argument("--particles", default=",".join(str(n) for n in PARTICLES))
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--scatter", default="8:256", help="the R:N at which (b) is measured")
    ap.add_argument("--trace", default="8:256", help="the R:N at which the kernels are traced")
    ap.add_argument("--parent", default=None, metavar="ROOT", help="a built checkout of the parent commit whose bootstrap call is the fourth side")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N:SIDE", help="three calls of one side and nothing else (for a profiler)")
    ap.add_argument("--serve", action="store_true", help="answer bootstrap calls requested on standard input (the child of --parent)")
    ap.add_argument("--root", default=None, help="with --serve: the checkout whose package, library and tools are loaded")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.serve:
        return serve(a.limit)
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
    counts, asked = [int(r) for r in a.records.split(",") if r], [int(n) for n in a.particles.split(",") if n]
    pairs = lambda text: [tuple(int(v) for v in t.split(":")) for t in text.split(",") if t]
    traced, scattered = pairs(a.trace), pairs(a.scatter)
    parent = Parent(a.parent, a.limit) if a.parent else None
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        ns = sorted({min(n, largest_n(cfg)) for n in asked})        # (an N beyond the point's limit is run at the limit)
        at = lambda picked, R, N: (R, N) in [(r, min(n, largest_n(cfg))) for r, n in picked]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        assert ROWS == STEPS
        for R in counts:
            args = data(meta, R, mod)
            for N in ns:
                sides, out = sides_of(mod, meta, *args, N), {}

                def run(k):
                    out[k] = sides[k]()

                calls = {k: (lambda k=k: timed_ms(lambda: run(k), a.limit)) for k in sides}
                if parent:
                    calls["parent"] = lambda: parent.ms(point, R, N)
                for k in calls:                                     # every side warmed up once
                    calls[k]()
                ts = {k: [] for k in calls}
                for _ in range(a.repeats):                          # alternating, so that all see the same neighbours on the machine
                    for k in calls:
                        ts[k].append(calls[k]())
                med = {k: statistics.median(v) for k, v in ts.items()}
                spread = max(ts["bootstrap"]) - min(ts["bootstrap"])
                same = all(np.array_equal(out["adaptive_2.0"][k], out["bootstrap"][k], equal_nan=True) for k in out["bootstrap"])
                seen = ~np.isnan(out["adaptive_0.5"]["lpd_joint"])
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, tracks=meta["S"] * R,
                           ms_median_min_max={k: stats(v) for k, v in ts.items()},
                           adaptive_2_over_bootstrap=round(med["adaptive_2.0"] / med["bootstrap"], 4),
                           adaptive_05_over_bootstrap=round(med["adaptive_0.5"] / med["bootstrap"], 4),
                           bootstrap_over_parent=round(med["bootstrap"] / med["parent"], 4) if parent else None,
                           bootstrap_min_max_spread_ms=round(spread, 3),
                           adaptive_2_slower_than_spread=bool(med["adaptive_2.0"] - med["bootstrap"] > spread),
                           adaptive_2_equals_bootstrap_bit_for_bit=bool(same),
                           share_of_observed_rows_resampled_at_05=round(float(np.mean(out["adaptive_0.5"]["resampled"][seen] == 1)), 4),
                           ll_all={k: float(out[k]["ll_all"]) for k in sides},
                           median_ess={k: float(np.median(out[k]["ess"])) for k in sides},
                           seeded_against_numpy=seeded_against_numpy(mod, args, N, a.repeats, a.limit),
                           what_it_buys=scatter(mod, meta, args, N, a.seeds, a.limit) if a.seeds > 1 and at(scattered, R, N) else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not a.no_trace and at(traced, R, N):
                    for side in sides:
                        trace[f"{point}:{R}:{N}:{side}"] = kernel_trace(point, R, N, side, 4 * a.limit)
                        print(json.dumps({f"{point}:{R}:{N}:{side}": trace[f"{point}:{R}:{N}:{side}"]}), flush=True)
    if parent:
        parent.close()
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_adaptive.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_filter_adaptive_records_grouped: the posteriors once, passes of the adaptive weight launch, the rows launch "
                        "and the product launch per step for all (chain, record) tracks; one set of draws shared by the tracks",
               baseline="posterior_filter_particle_records_grouped of the same build on the same draws; `parent`: the same call of the "
                        "parent commit's checkout, served by a child process and measured alternately",
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               what_it_buys="thresholds 0.5 and 2.0 over the seeds of the draws, on the records as generated and with every second row NaN; "
                            "reported, nothing is asserted",
               points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
