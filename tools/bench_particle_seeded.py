"""Particle filtering of R held-out records with the draws generated on the device against the same call with NumPy's draws, of the
same build, in one process on the same GPU: wall time around model-level calls that end in a synchronisation -- on the NumPy side the
generation of the draws, their scan and their upload count, because that is what the user pays; every side warmed up once, then
measured alternately, median of --repeats runs with min-max.  No time and no ratio is fixed in advance: with shared draws (1.6 MB at
N = 256) no gain is expected and the extra launches may show.

Workload: records of 200 rows, R = 8, N = 64, 256 and the largest N that fits (actuator 2048, config 2 896), noise "shared" and
"independent";  actuator: T = 512, M = 100, D = 4, S = 10;  config2: T = 4096, M = 512, D = 4, S = 32.
Sides:
  device  `DGPSSM.particle_records_seeded` (`ffvd_posterior_particle_seeded_records_grouped`): one fill launch per stream, no host draws;
  numpy   `DGPSSM.filter_records_particle` (`ffvd_op_posterior_filter_particle_records_grouped`): np.random.default_rng(seed) draws,
          the value scans, the upload.  Where it refuses (independent draws beyond 1 GiB) the row says so and the device side is timed
          alone.
The two sides draw different numbers (Philox against NumPy's PCG64 streams), so their outputs are not compared here: that the seeded
call equals the existing entry point on the same arrays is tests/test_gpu_particle_seeded.py's.  Reported: log_evidence (mean over
tracks) of both.

    python tools/bench_particle_seeded.py [--repeats 5] [--out profiles/particle_seeded.json] [--commit HASH] [--limit 120] [--no-trace]

The fill launch's own time and the bytes it writes per second come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_particle_seeded.py --kernel-only POINT:R:N:NOISE

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
from bench_filter_particle import POINTS, largest_n
from bench_filter_records import ROWS, data
from bench_moment_group import SHAPES, STEPS, limit, model, stats, timed_ms

NOISE = ("shared", "independent")
PARTICLES = (64, 256, 2048)
RECORDS = 8
FILL = "mg_pdraw_fill_kernel"
CALLS_TRACED = 3


def draw_doubles(cfg, R, N, noise):
    """the doubles the fill launches of a call write: eps and unif of every block (no start covariance here, so no xi0)"""
    blocks = cfg["S"] * R if noise == "independent" else 1
    return blocks * (ROWS * N * cfg["D"] + ROWS)


def sides_of(mod, Y, ctrl, x0, N, noise):
    kw = dict(x0=x0, num_particles=N, seed=7, noise=noise)
    return dict(device=lambda: mod.particle_records_seeded(Y, ctrl, **kw), numpy=lambda: mod.filter_records_particle(Y, ctrl, **kw))


def fill_figures(path, cfg, R, N, noise):
    """The fill kernel's rows of a rocprofv3 kernel_stats.csv -> launches, time per call and the bytes written per second"""
    with open(path, newline="") as f:
        hit = [r for r in csv.DictReader(f) if FILL in r.get("Name", "")]
    if not hit:
        return dict(skipped=f"no {FILL} row in the trace")
    calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
    per_call_s, nbytes = total * 1e-9 / CALLS_TRACED, 8 * draw_doubles(cfg, R, N, noise)
    return dict(kernel=hit[0]["Name"][:90], launches=calls, launches_per_call=calls // CALLS_TRACED, fill_ms_per_call=round(per_call_s * 1e3, 4),
                bytes_per_call=nbytes, gbytes_per_second=round(nbytes / per_call_s / 1e9, 2))


def kernel_trace(point, R, N, noise, seconds):
    """One child under rocprofv3 (kernel trace only): three device-side calls at `point`."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{point}:{R}:{N}:{noise}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return fill_figures(found[0], SHAPES[point], R, N, noise) if found else dict(skipped="no kernel_stats.csv was written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", type=int, default=RECORDS)
    ap.add_argument("--particles", default=",".join(str(n) for n in PARTICLES))
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N:NOISE", help="three device-side calls and nothing else (for a profiler)")
    ap.add_argument("--trace-particles", default="256,2048", help="the N at which the fill launch is traced (beyond the limit: at the limit)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    assert ROWS == STEPS
    if a.kernel_only:
        point, R, N, noise = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        run = sides_of(mod, *data(meta, int(R), mod), int(N), noise)["device"]
        for _ in range(CALLS_TRACED):
            with limit(a.limit):
                f = run()
        print(json.dumps(dict(point=point, R=int(R), N=int(N), noise=noise, mean_log_evidence=float(np.mean(f["log_evidence"])))))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    from ffvd_amd.build import source_hash

    def save():                                                     # after every row: a run that is cut short keeps what it measured
        doc = dict(tool="tools/bench_particle_seeded.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
                   new_path="DGPSSM.particle_records_seeded: ffvd_posterior_particle_seeded_records_grouped, the bootstrap filter's launches after one "
                            "fill launch per stream (eps, unif) that writes the device buffers the NumPy path uploads into",
                   baseline="DGPSSM.filter_records_particle of the same build: np.random.default_rng draws on the host, the value scans of the "
                            "Python layer and of the library, the upload",
                   timing="wall time around model-level calls that end in a synchronisation, host generation, uploads and downloads included; "
                          "alternating after one warm-up call per side",
                   points=rows)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")

    rows, R = [], a.records
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        ns = sorted({min(int(n), largest_n(cfg)) for n in a.particles.split(",") if n})          # (an N beyond the point's limit is run at the limit)
        traced = {min(int(n), largest_n(cfg)) for n in a.trace_particles.split(",") if n}
        with limit(a.limit):
            mod, cc, _, meta = model(cfg, ROWS)
        Y, ctrl, x0 = data(meta, R, mod)
        for noise in NOISE:
            for N in ns:
                sides, out, refused = sides_of(mod, Y, ctrl, x0, N, noise), {}, None

                def run(k):
                    out[k] = sides[k]()

                try:                                                # (the 1 GiB refusal comes before anything is drawn)
                    timed_ms(lambda: run("numpy"), 4 * a.limit)
                except ValueError as e:
                    refused = str(e)
                    del sides["numpy"]
                timed_ms(lambda: run("device"), a.limit)            # every side warmed up once
                ts = {k: [] for k in sides}
                for _ in range(a.repeats):                          # alternating, so that both see the same neighbours on the machine
                    for k in sides:
                        ts[k].append(timed_ms(lambda: run(k), 4 * a.limit))
                med = {k: statistics.median(v) for k, v in ts.items()}
                nd = draw_doubles(cfg, R, N, noise)
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, noise=noise, tracks=meta["S"] * R,
                           draw_bytes=8 * nd, ms_median_min_max={k: stats(v) for k, v in ts.items()},
                           mean_log_evidence={k: float(np.mean(v["log_evidence"])) for k, v in out.items()})
                if refused is None:
                    row.update(numpy_over_device=round(med["numpy"] / med["device"], 3), device_is_slower=bool(med["device"] > med["numpy"]))
                else:
                    row.update(numpy_side_refused=refused)
                if not a.no_trace and N in traced:
                    row["fill_kernel"] = kernel_trace(point, R, N, noise, 4 * a.limit)
                rows.append(row)
                print(json.dumps(row), flush=True)
                save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
