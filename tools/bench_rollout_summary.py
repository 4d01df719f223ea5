"""Held-out evaluation with the summary formed on the device against the composed path it replaces, in one process on the same GPU:
`DGPSSM.evaluate_heldout` (one `ffvd_op_posterior_rollout_grouped_summary` call: posteriors, rollouts and summary stay on the device,
no trajectory is downloaded) and `collect_samples_chains(fused=True)` with Y_test (`ffvd_op_posterior_rollout_grouped`, both
(S, R, steps, D) stacks downloaded, `predict_y_summary` in NumPy).  Wall time around the calls, uploads and downloads included (what a
caller pays); both warmed up twice, then measured alternately, median of --repeats runs with min-max.  After the timed runs one more
call of each path runs with FFVD_RG_TIMING set: the library's laps (each waits for the stream, so these calls are not timed) say
what share of a call the step launches, the summary launches and the downloads take.

    python tools/bench_rollout_summary.py [--repeats 5] [--out profiles/rollout_summary.json] [--commit HASH] [--limit 120]

Gate: at each point the new path's median must not be above the composed path's fastest run; `gate_met` says how
each point came out, nothing is tuned for it.  Every GPU step runs under a time limit of its own: an alarm whose default action ends
the process, so a step that hangs inside the library ends the run and nothing more is started.  The record names the commit
(`git rev-parse HEAD`, or --commit) and the SHA-256 of the library's sources and flags (`ffvd_amd.build.source_hash()`)."""
import argparse
import json
import os
import re
import signal
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ffvd_amd import synthetic
from ffvd_amd.dgp_model import DGPSSM
from ffvd_amd.kernels import SquaredExponential
from ffvd_amd.likelihoods import Gaussian
from ffvd_amd.prediction import predict_y_summary

SHAPES = {
    "actuator": dict(T=512, D=4, C=1, M=100, S=10),
    "config2": dict(T=4096, D=4, C=1, M=512, S=32),
}
STEPS = 200
ROLLOUTS = (8, 100)


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
    return mod, cc, Y, Y_test, meta


def timed_ms(fn, seconds):
    with limit(seconds):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def laps(fn, seconds):
    """One call with FFVD_RG_TIMING set; the library's stderr lines `who:   lap   x ms` as {lap: ms}."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.environ["FFVD_RG_TIMING"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            with limit(seconds):
                fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["FFVD_RG_TIMING"]
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    out = {}
    for m in re.finditer(r"^\S+:\s+(.+?)\s+([0-9.]+) ms$", text, flags=re.M):
        out[m.group(1)] = float(m.group(2))
    return out


def share(lap, key):
    total = sum(lap.values())
    return round(lap.get(key, 0.0) / total, 4) if total > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None                     # (no git metadata where this runs: the source hash below identifies the build)
    rows = []
    for name in a.shapes.split(","):
        cfg = SHAPES[name]
        with limit(a.limit):
            mod, cc, Y, Y_test, meta = model(cfg, STEPS)
        S, D = meta["S"], meta["D"]
        for R in ROLLOUTS:
            eps = np.random.default_rng(R).standard_normal((STEPS, S, R, D))
            out = {}

            def run(new):
                if new:
                    out[new] = mod.evaluate_heldout(Y_test, cc, R, eps=eps)
                else:
                    out[new] = mod.collect_samples_chains(R, cc, STEPS, Y_test=Y_test, Y_train=Y, eps=eps, fused=True)

            for new in (True, False, True, False):              # both sides warmed up twice
                timed_ms(lambda: run(new), a.limit)
            tns, tcs = [], []
            for _ in range(a.repeats):                          # alternating, so that both see the same neighbours on the machine
                tns.append(timed_ms(lambda: run(True), a.limit))
                tcs.append(timed_ms(lambda: run(False), a.limit))
            tn, tc = stats(tns), stats(tcs)
            lap_new, lap_old = laps(lambda: run(True), a.limit), laps(lambda: run(False), a.limit)
            t0 = time.perf_counter()
            predict_y_summary(out[False]["predict_x"].reshape(S * R, STEPS, D), out[False]["predict_x_var"].reshape(S * R, STEPS, D),
                              mod.likelihood.CC, mod.likelihood.DD, mod.likelihood.log_Rchols, Y_test)
            host_summary_ms = (time.perf_counter() - t0) * 1e3
            dy = float(np.abs(out[True]["predict_y"] - out[False]["predict_y"]).max())
            dvar = float(np.abs(out[True]["predict_y_var"] - out[False]["predict_y_var"]).max())
            row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=D, S=S, R=R, steps=STEPS, stack_megabytes=round(S * R * STEPS * D * 8 / 1e6, 2),
                       device_summary_ms=round(tn[0], 3), device_summary_min_max_ms=[round(tn[1], 3), round(tn[2], 3)],
                       composed_ms=round(tc[0], 3), composed_min_max_ms=[round(tc[1], 3), round(tc[2], 3)],
                       speedup=round(tc[0] / tn[0], 3), gate_met=bool(tn[0] <= tc[1]), host_summary_ms=round(host_summary_ms, 3),
                       laps_device_summary_ms=lap_new, laps_composed_ms=lap_old,
                       download_share_of_composed_call=share(lap_old, "results downloaded"),
                       summary_share_of_new_call=share(lap_new, "summary"),
                       max_abs_dy_vs_host=dy, max_abs_dyvar_vs_host=dvar, rmse=[out[True]["RMSE"], out[False]["RMSE"]],
                       ll=out[True]["ll"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_rollout_summary.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.evaluate_heldout: ffvd_op_posterior_rollout_grouped_summary, no trajectory downloaded",
               baseline="collect_samples_chains(fused=True) with Y_test: ffvd_op_posterior_rollout_grouped, two downloads, NumPy summary",
               gate="the new path's median must not be above the composed path's fastest run (gate_met per point)",
               laps="FFVD_RG_TIMING laps of one extra, untimed call per path; each lap waits for the stream", points=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
