"""Grouped rollouts against the loop they replace, in one process on the same GPU: one `prediction.rollout_grouped` call for G posteriors
with R rollouts each, and a Python loop of G `prediction.rollout` calls with R each (what G posteriors cost before).  Wall time around
the calls, uploads included (what a caller pays); both warmed up, median of --repeats runs.  Collapsed posteriors (q_sqrt included), as
`collect_samples_formal(rollout_mode="intent")` hands them over.

    python tools/bench_rollout_group.py [--repeats 5] [--out profiles/rollout_group.json] [--commit HASH]

The record names the commit (`git rev-parse HEAD`, or --commit) and the SHA-256 of the library's sources and flags
(`ffvd_amd.build.source_hash()`, what `libffvd_hip.so.hash` holds), which any checkout can recompute.  FFVD_RG_TIMING=1 makes the
library print where a grouped call spends its wall time (uploads, W q_sqrt, step launches, download).

Prints one line per point and writes them as JSON; exits 1 when the grouped call is not faster at some point."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ffvd_amd import synthetic
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd.kernels import SquaredExponential
from ffvd_amd.prediction import rollout, rollout_grouped

SHAPES = {
    "actuator": dict(cfg=dict(T=512, D=4, C=1, M=100, S=1), steps=200, points=[(4, 1), (32, 1), (100, 1), (10, 10)]),
    "config2": dict(cfg=dict(T=1024, D=4, C=1, M=512, S=1), steps=100, points=[(4, 1), (32, 1), (32, 8)]),
}


def posterior(cfg):
    params, Y, c, meta = synthetic.make_workload(**cfg)
    D, C = meta["D"], meta["C"]
    kern = [SquaredExponential(D + C, variance=np.exp(params["logvariance"][d]), lengthscales=np.exp(params["loglengthscales"][d]))
            for d in range(D)]
    X, Q = params["X"][0], np.exp(params["log_Q"])
    L = cmo.kernel_pre_cal(params["Z"], kern)
    U, H = cmo.collapse_u_mean_after_kernel_precalculation(L, np.concatenate((X[:-1], c), axis=1), X, params["Z"], kern, Q)
    return dict(L=L, Z=params["Z"], kern=kern, U=U, H=H, X=X, Q=Q, c=c, meta=meta)


def median_ms(fn, repeats):
    fn()
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None                     # (no git metadata where this runs: the source hash below identifies the build)
    rows, ok = [], True
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        p = posterior(sh["cfg"])
        D, C, T, steps = p["meta"]["D"], p["meta"]["C"], p["meta"]["T"], sh["steps"]
        rng = np.random.default_rng(0)
        ctrl = np.concatenate((p["c"], rng.standard_normal((steps, C))))
        for G, R in sh["points"]:
            x_lasts = [p["X"][-1] + 0.05 * rng.standard_normal(D) for _ in range(G)]
            eps = rng.standard_normal((steps, G, R, D))
            out = {}

            def grouped():
                out["g"] = rollout_grouped([p["L"]] * G, [p["Z"]] * G, [p["kern"]] * G, [p["U"]] * G, [p["H"]] * G, x_lasts, ctrl, T,
                                           steps, [p["Q"]] * G, eps)

            def loop():
                out["l"] = [rollout(p["L"], p["Z"], p["kern"], p["U"], p["H"], x_lasts[g], ctrl, T, steps, p["Q"], eps[:, g])
                            for g in range(G)]

            tg, tl = median_ms(grouped, a.repeats), median_ms(loop, a.repeats)
            dx = max(np.abs(out["g"][0][g] - out["l"][g][0]).max() for g in range(G))
            row = dict(shape=name, M=sh["cfg"]["M"], D=D, P=D + C, steps=steps, G=G, R=R, grouped_ms=round(tg[0], 3),
                       grouped_min_max_ms=[round(tg[1], 3), round(tg[2], 3)], loop_ms=round(tl[0], 3),
                       loop_min_max_ms=[round(tl[1], 3), round(tl[2], 3)], speedup=round(tl[0] / tg[0], 2),
                       grouped_us_per_step=round(tg[0] * 1e3 / steps, 2), max_abs_dx_vs_loop=float(dx))
            ok = ok and tg[0] < tl[0]
            rows.append(row)
            print(json.dumps(row), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_rollout_group.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats, gate="grouped_ms < loop_ms at every point",
               gate_passed=ok, points=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
