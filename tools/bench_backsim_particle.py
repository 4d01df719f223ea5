"""Particle backward simulation of R held-out records in one call against the filter and the marginal smoother of the same build, in
one process on the same GPU, with the protocol of tools/bench_smooth_particle.py: wall time around calls that end in a
synchronisation, uploads, the posteriors and the download of the trajectories included; every side warmed up once, then measured
alternately, median of --repeats runs with min-max.  No time and no ratio is fixed in advance, and none is a pass criterion.

Workload: that of tools/bench_smooth_particle.py -- records of 200 rows, one set of draws shared by all tracks;  actuator: T = 512,
M = 100, D = 4, S = 10;  config2: T = 4096, M = 512, D = 4, S = 32.  B = 16, 128, 1024 trajectories per track.
Sides:
  backsim B  `posterior_backsim_particle_records_grouped`: the filter's launches with the keep kernel per step, the weights, ONE launch
             for the backward recursions of all (track, trajectory) pairs, one for the moments;
  filter     `posterior_filter_particle_records_grouped` on the same inputs: backsim - filter is the added cost;
  smooth     `posterior_smooth_particle_records_grouped` on the same inputs: the N^2 marginal smoother.  At B ~ N the backward
             simulation evaluates as many densities as the smoother's backward kernel.
Reported beside the times: whether the filter keys are bit-identical, the largest |m_traj - m_smooth| / sqrt(diag S_smooth / B).

    python tools/bench_backsim_particle.py [--repeats 5] [--out profiles/backsim_particle.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures (time of the one backward launch and of the moments launch, density evaluations per second) come from a trace the
tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_backsim_particle.py --kernel-only POINT:R:N:B

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
from bench_filter_particle import POINTS, draws, largest_n
from bench_filter_records import ROWS, data
from bench_moment_group import SHAPES, limit, model, stats, timed_ms
from ffvd_amd import prediction as pr

TRAJECTORIES = (16, 128, 1024)
KERNELS = (("keep", "mg_psm_keep_kernel"), ("weights", "mg_psm_weights_kernel"), ("backward", "mg_pbs_kernel"),
           ("moments", "mg_pbs_moments_kernel"))


def sides_of(mod, meta, Y, ctrl, x0, N, Bs):
    S, D = meta["S"], meta["D"]
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, em = [mod._X_chains[s] for s in range(S)], (lik.CC, lik.DD, lik.log_Rchols)
    eps, unif = draws(N, D, 1)
    args = (lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, eps, unif)
    sides = dict(filter=lambda: pr.posterior_filter_particle_records_grouped(*args, x0s=x0),
                 smooth=lambda: pr.posterior_smooth_particle_records_grouped(*args, x0s=x0))
    for B in Bs:
        ub = np.random.default_rng(2000 + B).random((ROWS, B))
        sides[f"backsim_B{B}"] = lambda ub=ub: pr.posterior_backsim_particle_records_grouped(*args, ub, x0s=x0)
    return sides


def kernel_figures(path, cfg, R, N, B):
    """The kernels of the call in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; density evaluations per
    second of the backward launch (tracks * B * 199 * N in its one launch)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, name in KERNELS:
        hit = [r for r in rows if name in r.get("Name", "")]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3),
                            total_ms_per_call=round(total * 1e-6 / 3, 3))
    if "backward" in out:
        evals = float(cfg["S"] * R) * B * (ROWS - 1) * N
        out["backward"].update(workgroups=cfg["S"] * R * B, evaluations_per_launch=evals,
                               gevals_per_second=round(evals / (out["backward"]["mean_launch_us"] * 1e-6) / 1e9, 2))
    return out


def kernel_trace(point, R, N, B, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the backward simulation at `point`."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{point}:{R}:{N}:{B}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0], SHAPES[point], R, N, B) if found else dict(skipped="no kernel_stats.csv was written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", default="1,8")
    ap.add_argument("--particles", default="256,1024")
    ap.add_argument("--trajectories", default=",".join(str(b) for b in TRAJECTORIES))
    ap.add_argument("--trace", default="1:1024:1024,8:256:128", help="the R:N:B at which the kernels are traced")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N:B", help="three calls of the new path and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        point, R, N, B = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        new = sides_of(mod, meta, *data(meta, int(R), mod), int(N), [int(B)])[f"backsim_B{int(B)}"]
        for _ in range(3):
            with limit(a.limit):
                f = new()
        print(json.dumps(dict(point=point, R=int(R), N=int(N), B=int(B), indices=int(f["traj_index"].size))))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace = [], {}
    counts, asked = [int(r) for r in a.records.split(",") if r], [int(n) for n in a.particles.split(",") if n]
    Bs = [int(b) for b in a.trajectories.split(",") if b]
    traced = [tuple(int(v) for v in t.split(":")) for t in a.trace.split(",") if t]
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        ns = sorted({min(n, largest_n(cfg)) for n in asked})        # (an N beyond the point's limit is run at the limit)
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        for R in counts:
            for N in ns:
                sides, out = sides_of(mod, meta, *data(meta, R, mod), N, Bs), {}

                def run(k):
                    out[k] = sides[k]()

                for k in sides:                                     # every side warmed up once
                    timed_ms(lambda: run(k), a.limit)
                ts = {k: [] for k in sides}
                for _ in range(a.repeats):                          # alternating, so that all see the same neighbours on the machine
                    for k in sides:
                        ts[k].append(timed_ms(lambda: run(k), a.limit))
                med = {k: statistics.median(v) for k, v in ts.items()}
                sm = out["smooth"]
                sd = np.sqrt(np.diagonal(sm["S_smooth"], axis1=-2, axis2=-1))
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, tracks=meta["S"] * R,
                           ms_median_min_max={k: stats(v) for k, v in ts.items()},
                           smoother_added_ms=round(med["smooth"] - med["filter"], 3),
                           backsim_added_ms={f"B{B}": round(med[f"backsim_B{B}"] - med["filter"], 3) for B in Bs},
                           backsim_over_filter={f"B{B}": round(med[f"backsim_B{B}"] / med["filter"], 3) for B in Bs},
                           backsim_over_smooth={f"B{B}": round(med[f"backsim_B{B}"] / med["smooth"], 3) for B in Bs},
                           evaluations={f"B{B}": float(meta["S"] * R) * B * (ROWS - 1) * N for B in Bs},
                           smoother_pairs_per_kernel=float(meta["S"] * R) * (ROWS - 1) * N * N,
                           largest_m_traj_error_in_sd_over_sqrt_B={
                               f"B{B}": float(np.max((np.abs(out[f"backsim_B{B}"]["m_traj"] - sm["m_smooth"]) / (sd / np.sqrt(B)))[sd > 0.0]))
                               for B in Bs},                          # (a row whose smoothing weights sit on one particle has sd 0)
                           filter_keys_bit_identical=all(np.array_equal(out[f"backsim_B{B}"][k], out["filter"][k], equal_nan=True)
                                                         for B in Bs for k in out["filter"] if isinstance(out["filter"][k], np.ndarray)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                for r_, n_, b_ in traced:
                    if not a.no_trace and (R, N) == (r_, min(n_, largest_n(cfg))):
                        key = f"{point}:{R}:{N}:{b_}"
                        trace[key] = kernel_trace(point, R, N, b_, 4 * a.limit)
                        print(json.dumps({key: trace[key]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_backsim_particle.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_backsim_particle_records_grouped: the particle filter's launches with one keep launch per step, the "
                        "weights, one launch for the backward recursions of all (track, trajectory) pairs, the moments",
               baselines=dict(filter="posterior_filter_particle_records_grouped of the same build on the same inputs: the difference is the "
                                     "added cost of the backward simulation",
                              smooth="posterior_smooth_particle_records_grouped of the same build on the same inputs"),
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
