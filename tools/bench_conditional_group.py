"""The fused grouped conditionals against the composed path they replace, in one process on the same GPU: the transition function
f(x, c) of every chain at N inputs, by `prediction.posterior_conditional_grouped` (one `ffvd_op_posterior_conditional_grouped` call:
the S posteriors never leave the device, F is projected once per dim, the q_sqrt term runs on the matrix cores) and by the loop a
user writes today (`kernel_pre_cal`, then per chain `collapse_u_mean_after_kernel_precalculation` and
`conditional_after_kernel_precalculation(..., q_sqrt=H)`).  Wall time around the calls, uploads and downloads included (what a caller
pays); both warmed up, then measured alternately, median of --repeats runs with the spread.  The largest |mean| and |var| differences
between the two paths are recorded as well.

    python tools/bench_conditional_group.py [--repeats 5] [--out profiles/conditional_group.json] [--commit HASH] [--limit 120]

Gate: the fused median must be below the composed path's FASTEST run at every point; the tool exits 1 otherwise (the record is
written first).  Every GPU step runs under a time limit of its own: an alarm whose default action ends the process, so a step that
hangs inside the library ends the run and nothing more is started.  The record names the commit (`git rev-parse HEAD`, or --commit)
and the SHA-256 of the library's sources and flags (`ffvd_amd.build.source_hash()`).

--kernel-only SHAPE:N runs the fused call three times and nothing else: the workload of a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_conditional_group.py --kernel-only config2:1024` run, whose cg_rowsq_kernel
time gives the kernel's share of the fp64 MFMA peak from G D N M^2 flops (half the dense count: the k range is triangular)."""
import argparse
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
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import synthetic
from ffvd_amd.kernels import SquaredExponential
from ffvd_amd.prediction import posterior_conditional_grouped

SHAPES = {
    "actuator": dict(T=512, D=4, C=1, M=100, S=10),
    "config2": dict(T=4096, D=4, C=1, M=512, S=32),
}
NS = (256, 1024, 4096)


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


def workload(cfg):
    params, Y, c, meta = synthetic.make_workload(**cfg)
    D, P = meta["D"], meta["P"]
    kern = [SquaredExponential(P, variance=np.exp(params["logvariance"][d]), lengthscales=np.exp(params["loglengthscales"][d]))
            for d in range(D)]
    return params, c, meta, kern


def make_xnew(X0, c, T, N):
    """three quarters of the rows near chain 0's GP inputs, one quarter far from the data"""
    rng = np.random.default_rng(7)
    rows = np.concatenate((X0[:T], c[:T]), axis=1)
    near = N - N // 4
    pick = rng.choice(T, size=near, replace=near > T)
    return np.concatenate((rows[pick] + 0.05 * rng.standard_normal((near, rows.shape[1])),
                           3.0 * rng.standard_normal((N // 4, rows.shape[1]))))


def fused(params, c, meta, kern, Xnew):
    S = meta["S"]
    return posterior_conditional_grouped(params["Z"], kern, [params["X"][s] for s in range(S)], np.exp(params["log_Q"]), c, Xnew)


def composed(params, c, meta, kern, Xnew):
    S, T, Z, Q = meta["S"], meta["T"], params["Z"], np.exp(params["log_Q"])
    Lm = cmo.kernel_pre_cal(Z, kern)
    means, vars_ = [], []
    for s in range(S):
        X = params["X"][s]
        U, H = cmo.collapse_u_mean_after_kernel_precalculation(Lm, np.concatenate((X[:T], c[:T]), axis=1), X, Z, kern, Q)
        m, v = cmo.conditional_after_kernel_precalculation(Lm, Xnew, Z, kern, U, q_sqrt=H, white=True)
        means.append(m)
        vars_.append(v)
    return np.stack(means), np.stack(vars_)


def timed_ms(fn, seconds):
    with limit(seconds):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="SHAPE:N")
    a = ap.parse_args()
    if a.kernel_only:
        name, N = a.kernel_only.split(":")
        params, c, meta, kern = workload(SHAPES[name])
        Xnew = make_xnew(params["X"][0], c, meta["T"], int(N))
        for _ in range(3):
            with limit(a.limit):
                fused(params, c, meta, kern, Xnew)
        print(json.dumps(dict(shape=name, N=int(N), G=meta["S"], D=meta["D"], M=meta["M"],
                              useful_flops=meta["S"] * meta["D"] * int(N) * meta["M"] ** 2)))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None                     # (no git metadata where this runs: the source hash below identifies the build)
    rows = []
    for name in a.shapes.split(","):
        cfg = SHAPES[name]
        params, c, meta, kern = workload(cfg)
        for N in NS:
            Xnew = make_xnew(params["X"][0], c, meta["T"], N)
            out = {}

            def run(which):
                out[which] = (fused if which == "fused" else composed)(params, c, meta, kern, Xnew)

            for which in ("fused", "composed", "fused", "composed"):            # both sides warmed up twice
                timed_ms(lambda: run(which), a.limit)
            tfs, tcs = [], []
            for _ in range(a.repeats):                          # alternating, so that both see the same neighbours on the machine
                tfs.append(timed_ms(lambda: run("fused"), a.limit))
                tcs.append(timed_ms(lambda: run("composed"), a.limit))
            tf, tc = stats(tfs), stats(tcs)
            dm = float(np.abs(out["fused"][0] - out["composed"][0]).max())
            dv = float(np.abs(out["fused"][1] - out["composed"][1]).max())
            row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], N=N, fused_ms=round(tf[0], 3),
                       fused_min_max_ms=[round(tf[1], 3), round(tf[2], 3)], composed_ms=round(tc[0], 3),
                       composed_min_max_ms=[round(tc[1], 3), round(tc[2], 3)], speedup=round(tc[0] / tf[0], 2),
                       fused_median_below_composed_min=bool(tf[0] < tc[1]), max_abs_dmean_vs_composed=dm, max_abs_dvar_vs_composed=dv)
            rows.append(row)
            print(json.dumps(row), flush=True)
    from ffvd_amd.build import source_hash
    ok = all(r["fused_median_below_composed_min"] for r in rows)
    doc = dict(tool="tools/bench_conditional_group.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               baseline="kernel_pre_cal, then per chain collapse_u_mean_after_kernel_precalculation and "
                        "conditional_after_kernel_precalculation(q_sqrt=H): the composed path as it stands at the parent commit",
               gate="the fused median is below the composed path's fastest run at every point", gate_passed=ok, points=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
