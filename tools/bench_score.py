"""CRPS, PIT and predictive quantiles on the device (`prediction.moment_score`, `prediction.particle_score`) against the vectorised
NumPy / scipy restatement of the same formulas -- the composition a user had before -- in one process, with the statistics and the
time limit of tools/bench_moment_group.py: wall time around calls that end in a synchronisation, uploads and downloads included,
one warm-up, then the median of --repeats runs with min-max.  No ratio is fixed in advance; the tool records what it finds.

Timing.  J = 1 (the actuator fixture's), D = 4, 1900 targets (190 origins x horizon 10), levels (0.05, 0.5, 0.95):
  K = 10, 32       `moment_score`: the Gaussian fans' mixtures of S chains (actuator shape, config 2);
  K = 640, 2560    `particle_score`: the actuator shape, S = 10 chains x N = 64 / 256 particles;
  K = 8192         `particle_score`: config 2, S = 32 x N = 256.
The NumPy side evaluates the K x K pair table of one target at a time (erf and exp over it), F(y), and a brentq per (target,
level).  Where 1900 targets would take more than --numpy-budget seconds it is measured on fewer targets and scaled linearly to 1900;
the row says from how many.

Kernel rates.  One child under `rocprofv3 --kernel-trace --stats` (nothing else traced) makes three `particle_score` calls at
K = 2560 (1900 targets) and three `moment_score` calls at K = 2560 (190 targets); a pair kernel's rate is K (K - 1) / 2 unordered
pair terms per target over its mean launch time.

Fit (reported, not asserted).  On the actuator fixture of the tests (400 training rows, three chains, a 40-row held-out record,
every row an origin, horizon 10) `DGPSSM.forecast_scores` of the five rules: crps_h, coverage_h and the fan's ll_h side by side.

    python tools/bench_score.py [--repeats 5] [--points K1,K2] [--out profiles/score.json] [--commit HASH]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_score.py --kernel-only 2560

Every GPU step runs under a time limit of its own (an alarm whose default action ends the process)."""
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from bench_moment_group import fixture_model, limit, stats, timed_ms

TARGETS, D, J = 1900, 4, 1
LEVELS = (0.05, 0.5, 0.95)
POINTS = {"10": ("moments", 10, 1), "32": ("moments", 32, 1), "640": ("points", 10, 64), "2560": ("points", 10, 256),
          "8192": ("points", 32, 256)}
CALLS_TRACED = 3
TRACE_TARGETS = dict(points=TARGETS, moments=190)          # targets of the traced calls (the K = 2560 moment stacks of 1900 rows are 0.8 GB)
RULES = ("moment", "linearised", "cubature", "particle", "adapted")


def stacks(kind, G, N, targets=TARGETS):
    """A fan-like stack: the groups' means wander apart with the row, the particles scatter about them."""
    rng = np.random.default_rng(17)
    CC, DD, lr = rng.standard_normal((D, J)) / 2.0, np.zeros(J), np.log(np.full(J, 0.3))
    centre = rng.standard_normal((G, targets, D)) * np.linspace(0.2, 1.0, targets)[None, :, None]
    Y = (centre[0] @ CC + 0.3 * rng.standard_normal((targets, J)))
    if kind == "moments":
        L = 0.3 * rng.standard_normal((G, targets, D, D))
        S = L @ np.swapaxes(L, -1, -2)
        return (centre, 0.5 * (S + np.swapaxes(S, -1, -2))), (CC, DD, lr), Y
    return (centre[:, :, None, :] + 0.4 * rng.standard_normal((G, targets, N, D)),), (CC, DD, lr), Y


def numpy_scores(kind, stack, em, Y, n):
    """The restatement on the first n targets: components, pair table per target, F(y), brentq per (target, level)."""
    from scipy.optimize import brentq
    from scipy.special import erf, erfc
    CC, DD, lr = em
    sd2 = np.exp(2.0 * lr)
    if kind == "moments":
        m, S = stack
        mu = np.einsum("gtd,dj->tjg", m[:, :n], CC) + DD[None, :, None]
        var = np.einsum("aj,gtab,bj->tjg", CC, S[:, :n], CC) + sd2[None, :, None]
    else:
        p = stack[0][:, :n]
        mu = np.transpose(p @ CC + DD, (1, 3, 0, 2)).reshape(n, J, -1)
        var = np.broadcast_to(sd2[None, :, None], mu.shape)
    A = lambda d, v: d * erf(d / np.sqrt(2.0 * v)) + np.sqrt(2.0 * v / np.pi) * np.exp(-d * d / (2.0 * v))
    K = mu.shape[-1]
    crps, pit, q = np.empty((n, J)), np.empty((n, J)), np.empty((n, J, len(LEVELS)))
    for t in range(n):
        for j in range(J):
            m_, v_, y = mu[t, j], var[t, j], Y[t, j]
            crps[t, j] = np.mean(A(y - m_, v_)) - np.sum(A(m_[:, None] - m_[None, :], v_[:, None] + v_[None, :])) / (2.0 * K * K)
            F = lambda x: float(np.mean(0.5 * erfc((m_ - x) / np.sqrt(2.0 * v_))))
            pit[t, j] = F(y)
            w = 8.5 * np.sqrt(np.max(v_))
            for i, lv in enumerate(LEVELS):
                q[t, j, i] = brentq(lambda x: F(x) - lv, np.min(m_) - w, np.max(m_) + w, xtol=1e-15, rtol=1e-15)
    return crps, pit, q


def device_call(kind, stack, em, Y):
    from ffvd_amd import prediction as pr
    return (pr.moment_score if kind == "moments" else pr.particle_score)(*stack, *em, Y, levels=LEVELS)


def kernel_figures(path, K):
    """The score kernels in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; the pair kernels' rate in
    unordered pair terms per second (K (K - 1) / 2 per target)."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "psc_" in r.get("Name", "")]
    out = {}
    for r in rows:
        calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
        key = r["Name"].split("psc_")[1].split("(")[0][:40]
        out[key] = dict(launches=calls, mean_launch_us=round(total / calls * 1e-3, 3), total_ms_per_call=round(total * 1e-6 / CALLS_TRACED, 3))
        if "pair_kernel" in key:
            targets = TRACE_TARGETS["moments" if "false" in key else "points"]
            out[key]["targets"] = targets
            terms = targets * J * K * (K - 1) / 2.0 * CALLS_TRACED
            out[key]["unordered_pair_terms_per_second"] = float(f"{terms / (total * 1e-9):.4g}")
    return out


def kernel_trace(K, seconds):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", str(K)]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return dict(K=K, calls_traced=CALLS_TRACED, **kernel_figures(found[0], K)) if found else dict(skipped="no kernel_stats.csv was written")


def kernel_only(K, seconds):
    """the traced child: CALLS_TRACED calls of each symbol at K components (points: 10 x K / 10; moments: K groups)"""
    for kind, G, N in (("points", 10, K // 10), ("moments", K, 1)):
        stack, em, Y = stacks(kind, G, N, TRACE_TARGETS[kind])
        for _ in range(CALLS_TRACED):
            with limit(seconds):
                device_call(kind, stack, em, Y)
    return 0


def fit(seconds):
    """crps_h, coverage_h and ll_h of the five rules on the actuator fixture (N = 256 for the particle rules, seed 7)"""
    with limit(seconds):
        mod, c, Y_test = fixture_model()
    out = {}
    for rule in RULES:
        extra = dict(num_particles=256, seed=7) if rule in ("particle", "adapted") else {}
        with limit(seconds):
            r = mod.forecast_scores(Y_test, c, 10, method=rule, levels=(0.05, 0.25, 0.5, 0.75, 0.95), **extra)
        out[rule] = dict(used=r["used"], crps_h=np.round(r["crps_h"][:, 0], 6).tolist(), ll_h=np.round(r["fan"]["ll_h"][:, 0], 6).tolist(),
                         coverage_h_90=np.round(r["coverage_h"][:, 0, 0], 4).tolist(), coverage_h_50=np.round(r["coverage_h"][:, 0, 1], 4).tolist(),
                         n_h=r["n_h"][:, 0].tolist(), crps_mean=round(r["crps_mean"], 6), coverage_90=round(float(r["coverage"][0]), 4),
                         coverage_50=round(float(r["coverage"][1]), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--numpy-budget", type=float, default=20.0, help="seconds the NumPy side may take per run before it is scaled from fewer targets")
    ap.add_argument("--kernel-only", default=None, metavar="K")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--limit", type=int, default=180, help="seconds a single GPU step may take before the process is ended")
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(int(a.kernel_only), a.limit)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows = []
    for point in [s for s in a.points.split(",") if s]:
        kind, G, N = POINTS[point]
        K = G * N
        stack, em, Y = stacks(kind, G, N)
        out = {}
        timed_ms(lambda: out.update(dev=device_call(kind, stack, em, Y)), a.limit)                  # warm-up
        dev = [timed_ms(lambda: out.update(dev=device_call(kind, stack, em, Y)), a.limit) for _ in range(a.repeats)]
        # the NumPy side: a probe of two targets sizes the run (after one untimed pass: the first call pays scipy's imports)
        numpy_scores(kind, stack, em, Y, 2)
        t0 = time.perf_counter()
        numpy_scores(kind, stack, em, Y, 2)
        per_target = (time.perf_counter() - t0) / 2.0
        n = int(min(TARGETS, max(2, a.numpy_budget / per_target)))
        ref_ts = []
        for _ in range(a.repeats if n == TARGETS and per_target * TARGETS < 2.0 else 1):
            t0 = time.perf_counter()
            ref = numpy_scores(kind, stack, em, Y, n)
            ref_ts.append((time.perf_counter() - t0) * 1e3 * TARGETS / n)
        d = out["dev"]
        err = dict(crps=float(np.max(np.abs(d["crps"][:n] - ref[0]))), pit=float(np.max(np.abs(d["pit"][:n] - ref[1]))),
                   quantiles=float(np.max(np.abs(d["quantiles"][:n] - ref[2]))))
        med = statistics.median(dev)
        row = dict(point=point, call="moment_score" if kind == "moments" else "particle_score", K=K, G=G, N=N, targets=TARGETS, J=J, D=D,
                   levels=list(LEVELS), pair_terms=float(TARGETS * J) * K * K, device_ms_median_min_max=stats(dev),
                   numpy_ms_median_min_max=stats(ref_ts), numpy_measured_on_targets=n, numpy_scaled_to_1900=n != TARGETS,
                   numpy_over_device=round(statistics.median(ref_ts) / med, 2), largest_difference=err)
        rows.append(row)
        print(json.dumps(row), flush=True)
    trace = None if a.no_trace else kernel_trace(2560, 3 * a.limit)
    print(json.dumps(dict(kernel_trace=trace)), flush=True)
    fitted = None if a.no_fit else fit(a.limit)
    print(json.dumps(dict(actuator_fixture=fitted)), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_score.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="prediction.moment_score / particle_score: ffvd_score_moments / ffvd_score_points (staging, pair kernel and finish per "
                        "pass of targets, PIT, one bisection workgroup per (target, level))",
               baseline="the vectorised NumPy / scipy restatement of the same formulas on the host (numpy_scores in the tool): the K x K pair "
                        "table of one target at a time, F(y), scipy.optimize.brentq per (target, level)",
               timing="wall time around calls that end in a synchronisation, uploads and downloads included; one warm-up, median of the "
                      "repeats; the NumPy side scaled linearly from numpy_measured_on_targets where numpy_scaled_to_1900",
               points=rows, kernel_trace=trace, actuator_fixture=fitted)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
