"""Particle smoothing of R held-out records in one call against the two alternatives of the same build, in one process on the same GPU,
with the protocol of tools/bench_filter_particle.py: wall time around calls that end in a synchronisation, uploads and the posteriors
included; every side warmed up once, then measured alternately, median of --repeats runs with min-max.  No time and no ratio is fixed in
advance.

Workload: that of tools/bench_filter_particle.py -- records of 200 rows, R = 1 and 8, N = 64, 256, 1024 particles (config 2: 896),
one set of draws shared by all tracks;  actuator: T = 512, M = 100, D = 4, S = 10;  config2: T = 4096, M = 512, D = 4, S = 32.
Sides:
  smooth     `posterior_smooth_particle_records_grouped`: the filter's launches with the keep kernel per step, then the weights, the
             normalisers of all rows in one launch, a backward and a fold launch per row, the moments;
  filter     `posterior_filter_particle_records_grouped` of the same build on the same inputs: smooth - filter is the smoother's
             added cost;
  composed   what a user could do before: the filter with return_particles, `collapse_u_mean_grouped` once, per row ONE
             `conditional_grouped` call on the carried particles of all tracks (every group evaluates every row), and the recursion in
             NumPy.  The conditionals and the recursion are linear in the rows, so they run on --loop-rows rows and their time is
             scaled by 199 / that number (the filter call is timed whole); the JSON says so.  Where S * S * R * N * D exceeds
             --loop-doubles it is not run.
Fit (reported, not asserted): at the largest N on the 200-row record of tools/bench_filter_linear.py, the largest
|m_smooth - m_smooth(rule)| of the three Gaussian smoothers against the particle smoother, beside the same figure for the genealogy
estimate, ess_smooth (smallest, median) and the scatter of m_smooth over --seeds seeds.

    python tools/bench_smooth_particle.py [--repeats 5] [--out profiles/smooth_particle.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures (time per launch of the keep, the normaliser, the backward and the fold kernel, exps per second of the normaliser
-- one per pair -- and an upper bound for the backward kernel, which skips the columns of weight 0) come from a trace the tool starts
itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_smooth_particle.py --kernel-only POINT:R:N

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
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import prediction as pr

KERNELS = (("keep", "mg_psm_keep_kernel"), ("weights", "mg_psm_weights_kernel"), ("normaliser", "mg_psm_norm_kernel"),
           ("backward", "mg_psm_back_kernel"), ("fold", "mg_psm_fold_kernel"), ("moments", "mg_psm_moments_kernel"))


def fold(omega, a):
    w = np.zeros_like(omega)
    np.add.at(w, a, omega)
    return w


def host_row(x, mu, s, w_next, a):
    """one backward row of the recursion in NumPy for one track: x (N, D) the X^- of row t + 1, (mu, s) its transition terms"""
    q = ((x[None, :, :] - mu[:, None, :]) ** 2 / s[:, None, :]).sum(axis=2)
    lf = -0.5 * (q + np.log(s).sum(axis=1)[:, None])
    mx = lf.max(axis=0)
    c = mx + np.log(np.exp(lf - mx[None, :]).sum(axis=0))
    return fold((np.exp(lf - c[None, :]) * w_next[None, :]).sum(axis=1), a)


def sides_of(mod, meta, Y, ctrl, x0, N, loop_rows):
    """the three sides of a point as callables that return dicts"""
    S, R, D = meta["S"], Y.shape[0], meta["D"]
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, em = [mod._X_chains[s] for s in range(S)], (lik.CC, lik.DD, lik.log_Rchols)
    eps, unif = draws(N, D, 1)
    args = (lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, eps, unif)

    def smooth():
        return pr.posterior_smooth_particle_records_grouped(*args, x0s=x0)

    def filt():
        return pr.posterior_filter_particle_records_grouped(*args, x0s=x0)

    def composed_filter():
        return pr.posterior_filter_particle_records_grouped(*args, x0s=x0, return_particles=True)

    def composed_rows(f):
        """the last loop_rows backward rows of every track: the conditionals on the carried sets, then the recursion"""
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, Xs, mod.control_inputs, mod.Q)
        Q = np.broadcast_to(np.asarray(mod.Q), (S, D))
        own = np.arange(S)[:, None, None], np.arange(S * R * N).reshape(S, R * N)[:, :, None], np.arange(D)[None, None, :]
        P, A = f["particles"], f["ancestors"]
        w = np.full((S, R, N), 1.0 / N)
        for t in range(ROWS - 2, ROWS - 2 - loop_rows, -1):
            carried = np.take_along_axis(P[:, :, t], A[:, :, t, :, None].astype(np.int64), axis=2)         # X_{t+1}
            rows = np.concatenate((carried, np.broadcast_to(ctrl[None, :, t + 1, None, :], (S, R, N, ctrl.shape[2]))), axis=3)
            means, vars_, _, _ = cmo.conditional_grouped(list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv), rows.reshape(S * R * N, -1),
                                                         summary=False)
            mu, s = carried + means[own].reshape(S, R, N, D), vars_[own].reshape(S, R, N, D) + Q[:, None, None, :]
            for g in range(S):
                for r in range(R):
                    w[g, r] = host_row(P[g, r, t + 1], mu[g, r], s[g, r], w[g, r], A[g, r, t].astype(np.int64))
        return w
    return dict(smooth=smooth, filter=filt), (composed_filter, composed_rows)


def kernel_figures(path, cfg, R, N):
    """The smoother's kernels in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; exps per second of the
    normaliser (tracks * 199 * N * N pairs in its one launch) and, as an upper bound, of the backward kernel (tracks * N * N per launch)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, name in KERNELS + (("filter_weight", "mg_prec_weight_kernel"), ("filter_rows", "mg_prec_rows_kernel"), ("filter_product", "mg_lfan_var_kernel")):
        hit = [r for r in rows if name in r.get("Name", "")]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3),
                            total_ms_per_call=round(total * 1e-6 / 3, 3))
    V = cfg["S"] * R
    if "normaliser" in out:
        pairs = float(V) * (ROWS - 1) * N * N
        out["normaliser"].update(workgroups=V * (ROWS - 1) * ((N + 255) // 256), pairs_per_launch=pairs,
                                 gexps_per_second=round(pairs / (out["normaliser"]["mean_launch_us"] * 1e-6) / 1e9, 2))
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


def genealogy_mean(out):
    """m of the genealogy estimate from particles, ancestors and weights of a call with return_particles: (G, R, steps, D)"""
    P, A, W = out["particles"], out["ancestors"].astype(np.int64), out["weights"]
    G, R, n, N, D = P.shape
    m = np.zeros((G, R, n, D))
    for g in range(G):
        for r in range(R):
            w = W[g, r, n - 1] / W[g, r, n - 1].sum()
            for t in range(n - 1, -1, -1):
                if t < n - 1:
                    w = fold(w, A[g, r, t])
                m[g, r, t] = (w[:, None] * P[g, r, t]).sum(axis=0) / w.sum()
    return m


def fit_and_scatter(mod, Y_test, cc, n_train, seeds, N):
    """On one record that continues the training sequence: the three Gaussian smoothers against the particle smoother at N particles
    (seed 0), the genealogy estimate against it, and the scatter of m_smooth over `seeds` seeds."""
    Yr, cr = Y_test[None], cc[n_train: n_train + len(Y_test)][None]
    mom = mod.filter_heldout(Y_test, cc, smooth=True)
    lin, cub = mod.filter_records(Yr, cr, smooth=True), mod.filter_records_cubature(Yr, cr, smooth=True)
    big = mod.smooth_records_particle(Yr, cr, num_particles=N, seed=0, return_particles=True)
    ms = big["m_smooth"][:, 0]
    rules = dict(moment=mom["m_smooth"], linearised=lin["m_smooth"][:, 0], cubature=cub["m_smooth"][:, 0])
    runs = np.stack([mod.smooth_records_particle(Yr, cr, num_particles=N, seed=100 + s)["m_smooth"][:, 0] for s in range(seeds)])
    return dict(particles=N, largest_m_smooth_difference_from_the_particle_smoother={k: float(np.max(np.abs(v - ms))) for k, v in rules.items()},
                largest_m_smooth_difference_of_the_genealogy_estimate=float(np.max(np.abs(genealogy_mean(big)[:, 0] - ms))),
                largest_m_smooth_difference_of_the_filtered_mean=float(np.max(np.abs(big["m_filt"][:, 0] - ms))),
                smallest_ess_smooth=float(np.min(big["ess_smooth"])), median_ess_smooth=float(np.median(big["ess_smooth"])),
                scatter_of_m_smooth_over_seeds=dict(seeds=seeds, largest_sd=float(runs.std(axis=0, ddof=1).max()),
                                                    median_sd=float(np.median(runs.std(axis=0, ddof=1)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", default=",".join(str(r) for r in RECORDS))
    ap.add_argument("--particles", default=",".join(str(n) for n in PARTICLES))
    ap.add_argument("--loop-rows", type=int, default=3, help="the backward rows the composed path really runs; scaled to the 199 of a record")
    ap.add_argument("--loop-doubles", type=int, default=1 << 24, help="the composed path is not run where S * S * R * N * D exceeds this")
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--trace", default="1:1024,8:256", help="the R:N at which the kernels are traced")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R:N", help="three calls of the smoothing path and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        point, R, N = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        new = sides_of(mod, meta, *data(meta, int(R), mod), int(N), a.loop_rows)[0]["smooth"]
        for _ in range(3):
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
                fit[point] = fit_and_scatter(mod, Y_test, cc, cfg["T"], a.seeds, max(ns))
            print(json.dumps({point: fit[point]}), flush=True)
        for R in counts:
            for N in ns:
                (sides, (cfilter, crows)), out = sides_of(mod, meta, *data(meta, R, mod), N, a.loop_rows), {}
                heavy = meta["S"] * meta["S"] * R * N * meta["D"] > a.loop_doubles

                def run(k):
                    out[k] = sides[k]()

                for k in sides:                                     # every side warmed up once
                    timed_ms(lambda: run(k), a.limit)
                ts = {k: [] for k in sides}
                for _ in range(a.repeats):                          # alternating, so that all see the same neighbours on the machine
                    for k in sides:
                        ts[k].append(timed_ms(lambda: run(k), a.limit))
                if not heavy:                                       # the composed path: the filter whole, loop_rows rows scaled
                    def comp():
                        out["composed"] = cfilter()
                    t_f = [timed_ms(comp, a.limit) for _ in range(2)][-1]
                    t_r = [timed_ms(lambda: crows(out["composed"]), 4 * a.limit) for _ in range(2)][-1]
                    ts["composed"] = [t_f + t_r * (ROWS - 1) / a.loop_rows]
                med = {k: statistics.median(v) for k, v in ts.items()}
                row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, N=N, tracks=meta["S"] * R,
                           ms_median_min_max={k: stats(v) for k, v in ts.items()},
                           smoother_added_ms=round(med["smooth"] - med["filter"], 3), smooth_over_filter=round(med["smooth"] / med["filter"], 3),
                           composed_rows_run=0 if heavy else a.loop_rows, composed_rows_scaled_by=None if heavy else round((ROWS - 1) / a.loop_rows, 3),
                           composed_over_smooth=f"not run: its conditional_grouped call would return more than {a.loop_doubles} doubles per array"
                           if heavy else round(med["composed"] / med["smooth"], 3),
                           pairs_per_kernel=float(meta["S"] * R) * (ROWS - 1) * N * N,
                           smallest_ess_smooth=float(np.min(out["smooth"]["ess_smooth"])),
                           filter_keys_bit_identical=all(np.array_equal(out["smooth"][k], out["filter"][k], equal_nan=True)
                                                         for k in out["filter"] if isinstance(out["filter"][k], np.ndarray)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if not a.no_trace and (R, N) in [(r, min(n, largest_n(cfg))) for r, n in traced]:
                    trace[f"{point}:{R}:{N}"] = kernel_trace(point, R, N, 4 * a.limit)
                    print(json.dumps({f"{point}:{R}:{N}": trace[f"{point}:{R}:{N}"]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_smooth_particle.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_smooth_particle_records_grouped: the particle filter's launches with one keep launch per step, then the "
                        "weights, the normalisers of all rows in one launch, a backward and a fold launch per row for all tracks, the moments",
               baselines=dict(filter="posterior_filter_particle_records_grouped of the same build on the same inputs: the difference is the "
                                     "smoother's added cost",
                              composed="the filter with return_particles (timed whole), collapse_u_mean_grouped once, per row one "
                                       "conditional_grouped call on the carried particles of all tracks and the recursion in NumPy, of the same "
                                       "build; the rows run on composed_rows_run rows and are scaled to the 199 backward rows; one timing"),
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
