"""Particle filtering of R held-out records in one call against the two alternatives of the same build, in one process on the same GPU,
with the protocol of tools/bench_filter_cubature.py (model builder, time limit and statistics of tools/bench_moment_group.py): wall
time around calls that end in a synchronisation, uploads and the posteriors included; every side warmed up once, then measured
alternately, median of --repeats runs with min-max.  No time and no ratio is fixed in advance.

Workload: records of 200 rows, R = 1 and 8, N = 64, 256, 1024 particles (config 2: 896, the most whose rows fit the K scratch of a
pass), seeded observations, control rows and starts (those of tools/bench_filter_records.py), one set of draws shared by all tracks.
  actuator   T = 512, M = 100, D = 4, S = 10, collapsed U;   config2   T = 4096, M = 512, D = 4, S = 32, collapsed U.
Sides:
  particle     `posterior_filter_particle_records_grouped` (posteriors, passes of a weight, a rows and a product launch per step, N
               rows of K per track and dim);
  cubature     `posterior_filter_cubature_records_grouped` at the same R: the cost per track of the best Gaussian rule;
  host_loop    what a user could do before: `collapse_u_mean_grouped` once, then per step ONE `conditional_grouped` call on the
               particle rows of all tracks (every group evaluates every row: the call has no per-group rows), a download, weights and
               systematic resampling in NumPy, an upload with the next call.  It is linear in the steps, so it runs --loop-steps steps
               and its time is scaled by 200 / that number; the JSON says so.  Where S * S * R * N * D exceeds --loop-doubles it is
               not run.
Fit (reported, not asserted): at the largest N on the 200-row record of tools/bench_filter_linear.py at the two shapes, ll_all of the
particle filter beside ll of the three Gaussian rules, and the largest |m_filt - m_filt(rule)| of each rule against the particle filter; the
scatter of ll_all and log_evidence over --seeds seeds per N.

    python tools/bench_filter_particle.py [--repeats 5] [--out profiles/filter_particle.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures (time per launch of the weight, the rows and the product kernel, the product's flop/s against the fp64 MFMA peak, the
bytes of Gamma it reads per second) come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_particle.py --kernel-only POINT:R:N

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
from bench_filter_records import PEAK_FP64_MFMA, ROWS, data
from bench_moment_group import SHAPES, STEPS, limit, model, stats, timed_ms
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import prediction as pr

POINTS = ("actuator", "config2")
RECORDS = (1, 8)
PARTICLES = (64, 256, 1024)


def rows_of_a_pass(cfg):
    """The library's limit for a collapsed-U call (moment_group.h: K and the partials of a pass within 2^26 doubles, in whole 128-row
    tiles, (group, dim) units): the rows of K per unit, particles times records."""
    Mp = (cfg["M"] + 63) // 64 * 64
    return (1 << 26) // (cfg["S"] * cfg["D"] * (Mp + (Mp + 127) // 128)) // 128 * 128


def largest_n(cfg):
    """the most particles one record per group may have: 2048 at the actuator shape, 896 at config 2"""
    return min(rows_of_a_pass(cfg), 2048)


def draws(N, D, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ROWS, N, D)), rng.random(ROWS)


def host_step(X, mean, var, Q, eps, y, CC, DD, sd, u):
    """one step of the method in NumPy for all tracks at once: X, mean, var (V, N, D); y (V, J) (NaN = unobserved)"""
    X = X + mean + eps[None] * np.sqrt(var + Q[:, None, :])
    N = X.shape[1]
    seen = ~np.isnan(y)
    r = np.where(seen, y, 0.0)[:, None, :] - (X @ CC + DD[None, None, :])
    L = np.sum(np.where(seen[:, None, :], -0.5 * np.log(2 * np.pi * sd * sd) - 0.5 * r * r / (sd * sd), 0.0), axis=2)
    mx = L.max(axis=1, keepdims=True)
    W = np.exp(L - mx)
    cdf = np.cumsum(W, axis=1)
    lj = mx[:, 0] + np.log(cdf[:, -1] / N)
    thr = (u + np.arange(N))[None, :] / N * cdf[:, -1:]
    a = np.minimum(np.stack([np.searchsorted(cdf[v], thr[v], side="right") for v in range(X.shape[0])]), N - 1)
    keep = seen.any(axis=1)
    a = np.where(keep[:, None], a, np.arange(N)[None, :])
    return np.take_along_axis(X, a[:, :, None], axis=1), np.where(keep, lj, np.nan)


def sides_of(mod, meta, Y, ctrl, x0, N, loop_steps):
    """the three sides of a point as callables that return dicts"""
    S, R, D = meta["S"], Y.shape[0], meta["D"]
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, em = [mod._X_chains[s] for s in range(S)], (lik.CC, lik.DD, lik.log_Rchols)
    eps, unif = draws(N, D, 1)

    def particle():
        return pr.posterior_filter_particle_records_grouped(lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, eps, unif, x0s=x0)

    def cubature():
        return pr.posterior_filter_cubature_records_grouped(lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, x0s=x0)

    def host_loop():
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, Xs, mod.control_inputs, mod.Q)
        CC, DD, sd = np.asarray(lik.CC), np.asarray(lik.DD).reshape(-1), np.exp(np.asarray(lik.log_Rchols)[0])
        X = np.broadcast_to(x0[:, :, None, :], (S, R, N, D)).reshape(S * R, N, D).copy()
        Q = np.broadcast_to(np.asarray(mod.Q), (S, D))[:, None, :].repeat(R, axis=1).reshape(S * R, D)
        own = np.arange(S)[:, None, None], np.arange(S * R * N).reshape(S, R * N)[:, :, None], np.arange(D)[None, None, :]
        ev = np.zeros(S * R)
        for t in range(loop_steps):
            rows = np.concatenate((X.reshape(S, R, N, D), np.broadcast_to(ctrl[None, :, t, None, :], (S, R, N, ctrl.shape[2]))), axis=3)
            means, vars_, _, _ = cmo.conditional_grouped(list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv), rows.reshape(S * R * N, -1),
                                                         summary=False)
            X, lj = host_step(X, means[own].reshape(S * R, N, D), vars_[own].reshape(S * R, N, D), Q, eps[t], np.tile(Y[:, t], (S, 1)), CC, DD,
                              sd, unif[t])
            ev += np.nan_to_num(lj)
        return dict(log_evidence=ev.reshape(S, R))
    return dict(particle=particle, cubature=cubature, host_loop=host_loop)


def kernel_figures(path, cfg, R, N):
    """The three kernels in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; for the product its flop/s (2 rows
    Mp^2 per launch, rows = tracks * D * N) against the fp64 MFMA peak and the bytes of Gamma it reads per second (once per row tile of
    a unit); for the rows kernel the exps per second (tracks * D * N * M per launch)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, pick in (("weight", lambda n: "mg_prec_weight_kernel" in n), ("rows", lambda n: "mg_prec_rows_kernel" in n),
                      ("product", lambda n: "mg_lfan_var_kernel" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    Mp = (M + 63) // 64 * 64
    # the records of a call go in passes of as many as fit the K scratch: the figures of a launch are those of the mean pass
    rp = max(1, min(R, rows_of_a_pass(cfg) // N))
    passes = (R + rp - 1) // rp
    krows = G * R * D * N / passes
    if "product" in out:
        us = out["product"]["mean_launch_us"]
        tiles = sum((min(rp, R - r0) * N + 127) // 128 for r0 in range(0, R, rp)) / passes
        flop, gam = 2.0 * krows * Mp * Mp, 8.0 * G * D * Mp * Mp * tiles
        out["product"].update(passes=passes, records_per_pass=rp, rows_of_K=krows, rows_per_unit=krows / (G * D), flop_per_launch=flop,
                              tflops=round(flop / (us * 1e-6) / 1e12, 3), fraction_of_fp64_mfma_peak=round(flop / (us * 1e-6) / PEAK_FP64_MFMA, 4),
                              gamma_gbytes_per_launch=round(gam / 1e9, 4), gamma_gbytes_per_second=round(gam / (us * 1e-6) / 1e9, 1))
    if "rows" in out:
        us = out["rows"]["mean_launch_us"]
        out["rows"].update(workgroups=krows * ((N + 7) // 8) / N, exps_per_launch=krows * M, gexps_per_second=round(krows * M / (us * 1e-6) / 1e9, 2),
                           k_gbytes_written_per_second=round(8.0 * krows * Mp / (us * 1e-6) / 1e9, 1))
    if "weight" in out:
        out["weight"].update(workgroups=G * R / passes, particles_per_workgroup=N)
    return out


def kernel_trace(point, R, N, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the particle path at `point` with R records and N particles."""
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


def fit_and_scatter(mod, Y_test, cc, n_train, seeds, ns):
    """On one record that continues the training sequence: the three Gaussian rules beside the particle filter at the largest N of `ns`
    (seed 0), and the scatter of ll_all and log_evidence (mean over the chains) over `seeds` seeds per N."""
    Yr, cr = Y_test[None], cc[n_train: n_train + len(Y_test)][None]
    mom, lin, cub = mod.filter_heldout(Y_test, cc), mod.filter_records(Yr, cr), mod.filter_records_cubature(Yr, cr)
    big = mod.filter_records_particle(Yr, cr, num_particles=max(ns), seed=0)
    rules = dict(moment=(float(mom["ll"]), mom["m_filt"]), linearised=(float(lin["ll_all"]), lin["m_filt"][:, 0]),
                 cubature=(float(cub["ll_all"]), cub["m_filt"][:, 0]))
    out = dict(particles=max(ns), ll_all=dict(particle=float(big["ll_all"]), **{k: v[0] for k, v in rules.items()}),
               largest_m_filt_difference_from_the_particle_filter={k: float(np.max(np.abs(v[1] - big["m_filt"][:, 0]))) for k, v in rules.items()},
               smallest_ess=float(np.min(big["ess"])), median_ess=float(np.median(big["ess"])), scatter_over_seeds={})
    for N in ns:
        runs = [mod.filter_records_particle(Yr, cr, num_particles=N, seed=100 + s) for s in range(seeds)]
        ll, ev = np.array([r["ll_all"] for r in runs]), np.array([np.mean(r["log_evidence"]) for r in runs])
        out["scatter_over_seeds"][str(N)] = dict(seeds=seeds, ll_all_mean=float(ll.mean()), ll_all_sd=float(ll.std(ddof=1)),
                                                 log_evidence_mean=float(ev.mean()), log_evidence_sd=float(ev.std(ddof=1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", default=",".join(str(r) for r in RECORDS))
    ap.add_argument("--particles", default=",".join(str(n) for n in PARTICLES))
    ap.add_argument("--loop-steps", type=int, default=5, help="the steps the host loop really runs; its time is scaled to the 200 rows")
    ap.add_argument("--loop-doubles", type=int, default=1 << 24, help="the host loop is not run where S * S * R * N * D exceeds this")
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--trace", default="1:1024,8:256", help="the R:N at which the kernels are traced")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N", help="three calls of the particle path and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        point, R, N = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        new = sides_of(mod, meta, *data(meta, int(R), mod), int(N), a.loop_steps)["particle"]
        for _ in range(3):
            with limit(a.limit):
                f = new()
        print(json.dumps(dict(point=point, R=int(R), N=int(N), ll=f["ll"][:4].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, trace, fit = [], {}, {}
    counts, asked = [int(r) for r in a.records.split(",") if r], [int(n) for n in a.particles.split(",") if n]
    traced = [tuple(int(v) for v in t.split(":")) for t in a.trace.split(",") if t]
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        ns = sorted({min(n, largest_n(cfg)) for n in asked})        # (an N beyond the point's limit is run at the limit)
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        assert ROWS == STEPS
        if not a.no_fit:
            with limit(4 * a.limit):
                fit[point] = fit_and_scatter(mod, Y_test, cc, cfg["T"], a.seeds, ns)
            print(json.dumps({point: fit[point]}), flush=True)
        for R in counts:
            for N in ns:
                sides, out = sides_of(mod, meta, *data(meta, R, mod), N, a.loop_steps), {}
                heavy = meta["S"] * meta["S"] * R * N * meta["D"] > a.loop_doubles
                if heavy:                                           # (every group evaluates the rows of all: S times the work and the download)
                    del sides["host_loop"]

                def run(k):
                    out[k] = sides[k]()

                for k in sides:                                     # every side warmed up once
                    timed_ms(lambda: run(k), a.limit)
                ts = {k: [] for k in sides}
                for _ in range(a.repeats):                          # alternating, so that all see the same neighbours on the machine
                    for k in sides:
                        ts[k].append(timed_ms(lambda: run(k), a.limit))
                if not heavy:
                    ts["host_loop"] = [t * ROWS / a.loop_steps for t in ts["host_loop"]]
                med = {k: statistics.median(v) for k, v in ts.items()}
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, tracks=meta["S"] * R,
                           ms_median_min_max={k: stats(v) for k, v in ts.items()}, host_loop_steps_run=0 if heavy else a.loop_steps,
                           host_loop_scaled_by=None if heavy else round(ROWS / a.loop_steps, 3),
                           host_loop_over_particle=f"not run: its conditional_grouped call would return more than {a.loop_doubles} doubles per array"
                           if heavy else round(med["host_loop"] / med["particle"], 3),
                           particle_over_cubature=round(med["particle"] / med["cubature"], 3), fastest=min(med, key=med.get),
                           launch_triples=ROWS + 1, wall_us_per_step=round(med["particle"] * 1e3 / (ROWS + 1), 2),
                           ms_per_track=dict(particle=round(med["particle"] / (meta["S"] * R), 4), cubature=round(med["cubature"] / (meta["S"] * R), 4)),
                           ll_all=dict(particle=float(out["particle"]["ll_all"]), cubature=float(out["cubature"]["ll_all"])),
                           smallest_ess=float(np.min(out["particle"]["ess"])))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not a.no_trace and (R, N) in [(r, min(n, largest_n(cfg))) for r, n in traced]:
                    trace[f"{point}:{R}:{N}"] = kernel_trace(point, R, N, 4 * a.limit)
                    print(json.dumps({f"{point}:{R}:{N}": trace[f"{point}:{R}:{N}"]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_particle.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_filter_particle_records_grouped: the posteriors once, passes of a weight, a rows and a product launch per "
                        "step for all (chain, record) tracks, N rows of K per (track, dim); one set of draws shared by the tracks",
               baselines=dict(cubature="posterior_filter_cubature_records_grouped of the same build at the same R",
                              host_loop="collapse_u_mean_grouped once, then per step one conditional_grouped call on the particle rows of all "
                                        "tracks, weights and systematic resampling in NumPy, of the same build; it runs host_loop_steps_run "
                                        "steps and its time is scaled to the 200 rows (it is one call per step)"),
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               fit_reported_not_asserted=fit or None, points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
