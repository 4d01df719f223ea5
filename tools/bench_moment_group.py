"""Moment-matched held-out evaluation against the Monte-Carlo evaluation it stands beside, in one process on the same GPU:
`DGPSSM.evaluate_heldout(method="moment")` (one `ffvd_op_posterior_moment_grouped` call with its summary) and the existing
`DGPSSM.evaluate_heldout` with 8 and with 100 rollouts per chain (`ffvd_op_posterior_rollout_grouped_summary`, which this change does
not touch).  Wall time around the calls, uploads, the posteriors and the final synchronisation included (what a caller pays); both
warmed up twice, then measured alternately, median of --repeats runs with min-max.  No ratio is fixed in advance: `faster` names the
faster side at each point.

    python tools/bench_moment_group.py [--repeats 5] [--out profiles/moment_group.json] [--commit HASH] [--limit 120]
                                       [--stats-csv FILE:SHAPE ...]

A second part measures the noise the moment method removes: ll and RMSE of the Monte-Carlo evaluation over 20 seeds at 8 and 100
rollouts per chain on the actuator fixture (tests/golden/actuator_slim.npz, 400 training rows, 40 held-out rows, three chains), next
to the single value of the moment method.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_moment_group.py --kernel-only config2

runs three moment evaluations and nothing else; --stats-csv DIR/.../*_kernel_stats.csv:config2 then adds the per-step figures of the
step kernel to the record: elements of the pair tables per second (G npair M^2 per launch) and the bytes of Gamma read over the kernel
time (G D M^2 doubles per launch).  Every GPU step runs under a time limit of its own: an alarm whose default action ends the
process, so a step that hangs inside the library ends the run and nothing more is started."""
import argparse
import csv
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ffvd_amd import synthetic
from ffvd_amd.dgp_model import DGPSSM
from ffvd_amd.kernels import SquaredExponential
from ffvd_amd.likelihoods import Gaussian

SHAPES = {
    "actuator": dict(T=512, D=4, C=1, M=100, S=10),
    "config2": dict(T=4096, D=4, C=1, M=512, S=32),
}
STEPS = 200
ROLLOUTS = (8, 100)
SEEDS = 20


class limit:
    """`with limit(seconds):` -- the process is ended (SIGALRM, default action) when the block takes longer"""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def model(cfg, steps):
    params, Y, c, meta = synthetic.make_workload(**cfg)
    D, M, P, S = meta["D"], meta["M"], meta["P"], meta["S"]
    kern = [SquaredExponential(P, ARD=True, variance=np.exp(params["logvariance"][d]), lengthscales=np.exp(params["loglengthscales"][d]))
            for d in range(D)]
    lik = Gaussian(1, D, CC=params["CC"], DD=params["DD"], RR_chol=np.exp(params["log_Rchols"]))
    rng = np.random.default_rng(5)
    cc = np.concatenate((c, rng.standard_normal((steps, meta["C"]))))
    Y_test = rng.standard_normal((steps, 1))
    X = params["X"][0]
    mod = DGPSSM(Y, [D], M, [kern], lik, QQ_chol=np.exp(0.5 * params["log_Q"]), ZZ=params["Z"], control_inputs=cc, U_ini=params["U"],
                 X_0_ini=X[0], X_train_ini=X[1:], kernel_optimization=True, U_optimization=False, U_collapse=True, Z_optimization=True,
                 case_val=4, prior_type="normal", num_chains=S)
    mod.set_X(params["X"])
    return mod, cc, Y_test, meta


def fixture_model(n_train=400, test_len=40, S=3):
    z = np.load(os.path.join(ROOT, "tests", "golden", "actuator_slim.npz"), allow_pickle=False)
    Y, c, X = z["Y"], z["control_inputs"], z["X"]
    D, M, P = X.shape[1], z["Z"].shape[0], z["Z"].shape[1]
    kern = [SquaredExponential(P, ARD=True, variance=np.exp(z["logvariance"][d]), lengthscales=np.exp(z["loglengthscales"][d]))
            for d in range(D)]
    lik = Gaussian(Y.shape[1], D, CC=z["CC"], DD=z["DD"], RR_chol=np.exp(z["log_Rchols"]))
    mod = DGPSSM(Y[:n_train], [D], M, [kern], lik, QQ_chol=np.exp(0.5 * z["log_Q"]), ZZ=z["Z"], control_inputs=c, U_ini=z["U"],
                 X_0_ini=X[0], X_train_ini=X[1:n_train + 1], kernel_optimization=True, U_optimization=False, U_collapse=True,
                 Z_optimization=True, case_val=4, prior_type="normal", num_chains=S)
    Xt = X[:n_train + 1]
    mod.set_X(np.stack([Xt + 0.05 * np.random.default_rng(40 + s).standard_normal(Xt.shape) * (s > 0) for s in range(S)]))
    return mod, c, Y[n_train:n_train + test_len]


def timed_ms(fn, seconds):
    with limit(seconds):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def step_kernel_figures(path, cfg):
    """The mg_step_kernel row of a rocprofv3 kernel_stats.csv -> per-launch time, pair-table elements and Gamma bytes per second."""
    if not os.path.exists(path):
        return None
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "mg_step_kernel" in r.get("Name", "")]
    if not rows:
        return None
    r = rows[0]
    calls, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    per_launch_s = total_ns / calls * 1e-9
    elements, gamma_bytes = G * (D * (D + 1) // 2) * M * M, G * D * M * M * 8
    return dict(kernel=r["Name"][:60], launches=calls, mean_launch_us=round(per_launch_s * 1e6, 3),
                pair_table_elements_per_launch=elements, pair_table_elements_per_second=round(elements / per_launch_s, 1),
                gamma_bytes_per_launch=gamma_bytes, gamma_gigabytes_per_second=round(gamma_bytes / per_launch_s / 1e9, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="SHAPE", help="three moment evaluations at SHAPE and nothing else (for a profiler)")
    ap.add_argument("--stats-csv", action="append", default=[], metavar="FILE:SHAPE", help="a rocprofv3 kernel_stats.csv of a --kernel-only run")
    ap.add_argument("--no-noise", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        with limit(a.limit):
            mod, cc, Y_test, meta = model(SHAPES[a.kernel_only], STEPS)
        for _ in range(3):
            with limit(a.limit):
                ev = mod.evaluate_heldout(Y_test, cc, 1, method="moment")
        print(json.dumps(dict(shape=a.kernel_only, ll=ev["ll"], rmse=ev["RMSE"])))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None                     # (no git metadata where this runs: the source hash below identifies the build)
    rows = []
    for name in [s for s in a.shapes.split(",") if s]:
        cfg = SHAPES[name]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, STEPS)
        S, D = meta["S"], meta["D"]
        for R in ROLLOUTS:
            eps = np.random.default_rng(R).standard_normal((STEPS, S, R, D))
            out = {}

            def run(moment):
                out[moment] = mod.evaluate_heldout(Y_test, cc, R, method="moment") if moment else mod.evaluate_heldout(Y_test, cc, R, eps=eps)

            for moment in (True, False, True, False):           # both sides warmed up twice
                timed_ms(lambda: run(moment), a.limit)
            tm, tr = [], []
            for _ in range(a.repeats):                          # alternating, so that both see the same neighbours on the machine
                tm.append(timed_ms(lambda: run(True), a.limit))
                tr.append(timed_ms(lambda: run(False), a.limit))
            row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=D, S=S, steps=STEPS, rollouts_per_chain=R,
                       moment_ms_median_min_max=stats(tm), rollouts_ms_median_min_max=stats(tr),
                       rollouts_over_moment=round(statistics.median(tr) / statistics.median(tm), 3),
                       faster="moment" if statistics.median(tm) < statistics.median(tr) else "rollouts",
                       ll=dict(moment=out[True]["ll"], rollouts=out[False]["ll"]), rmse=dict(moment=out[True]["RMSE"], rollouts=out[False]["RMSE"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    noise = None
    if not a.no_noise:
        with limit(a.limit):
            mod, c, Yt = fixture_model()
        with limit(a.limit):
            ev = mod.evaluate_heldout(Yt, c, 1, method="moment")
        noise = dict(fixture="tests/golden/actuator_slim.npz: 400 training rows, 40 held-out rows, 3 chains", seeds=SEEDS,
                     moment=dict(ll=ev["ll"], rmse=ev["RMSE"]), rollouts=[])
        for R in ROLLOUTS:
            lls, rmses = [], []
            for seed in range(SEEDS):
                with limit(a.limit):
                    e = mod.evaluate_heldout(Yt, c, R, seed=seed)
                lls.append(e["ll"])
                rmses.append(e["RMSE"])
            noise["rollouts"].append(dict(rollouts_per_chain=R, ll_mean=float(np.mean(lls)), ll_std=float(np.std(lls, ddof=1)),
                                          ll_min_max=[min(lls), max(lls)], rmse_mean=float(np.mean(rmses)),
                                          rmse_std=float(np.std(rmses, ddof=1)), rmse_min_max=[min(rmses), max(rmses)]))
        print(json.dumps(noise), flush=True)
    kernel = {}
    for spec in a.stats_csv:
        path, _, shape = spec.rpartition(":")
        kernel[shape] = step_kernel_figures(path, SHAPES[shape])
        print(json.dumps({shape: kernel[shape]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_moment_group.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.evaluate_heldout(method='moment'): ffvd_op_posterior_moment_grouped with its summary",
               baseline="DGPSSM.evaluate_heldout: ffvd_op_posterior_rollout_grouped_summary (untouched by the moment method)",
               timing="wall time around the call, synchronisation included; alternating after two warm-up calls per side",
               points=rows, noise=noise, step_kernel=kernel or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
