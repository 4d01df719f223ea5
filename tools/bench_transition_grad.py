"""The linearisation against the central-difference composition it replaces, in one process on the same GPU: mean and variance of the
transition function f(x, c) of every chain at N inputs WITH their input gradients, by one
`conditionals_multi_output.conditional_grad_grouped` call and by the 2 P + 1 `conditional_grouped` calls a user writes today (the
values, then Xnew +- h e_p for every input column).  Both are given the same posteriors (one `collapse_u_mean_grouped` call, not
timed) and q_mode "reference".  `conditional_grouped` alone is timed as well: the cost of the values only.  Wall time around the
calls, uploads and downloads included (what a caller pays); all warmed up, then measured alternately, median of --repeats runs with
the spread.  The largest differences between the analytic gradients and the central differences (h = 2^-10) are recorded.

    python tools/bench_transition_grad.py [--repeats 5] [--out profiles/transition_grad.json] [--commit HASH] [--limit 120]

No gate: nobody had measured this before the first record, the ratios are reported.  Every GPU step runs under a time limit of its
own: an alarm whose default action ends the process, so a step that hangs inside the library ends the run and nothing more is
started.  The record names the commit (`git rev-parse HEAD`, or --commit) and the SHA-256 of the library's sources and flags
(`ffvd_amd.build.source_hash()`).

--kernel-only SHAPE:N runs the new call three times and nothing else: the workload of a separate
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_transition_grad.py --kernel-only config2:4096
run; --stats-csv DIR/.../*_kernel_stats.csv:config2:4096 then adds the product kernel's (tg_var_kernel) mean launch time and its share
of the fp64 MFMA peak, 2 units N Mp^2 flop over that time (units = S D with q_sqrts, Mp = M rounded up to 64), to the record."""
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
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import synthetic
from ffvd_amd.kernels import SquaredExponential

SHAPES = {
    "actuator": dict(T=512, D=4, C=1, M=100, S=10),
    "config2": dict(T=4096, D=4, C=1, M=512, S=32),
}
NS = (256, 1024, 4096)
H = 2.0 ** -10
PEAK_F64_TFLOPS = 78.6          # MI355X dense fp64 matrix peak (bench.py's figure)


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


def workload(cfg, seconds):
    """the model, and the posteriors of its S chains (formed once on the device, handed to every timed call)"""
    params, Y, c, meta = synthetic.make_workload(**cfg)
    D, P, S = meta["D"], meta["P"], meta["S"]
    kern = [SquaredExponential(P, variance=np.exp(params["logvariance"][d]), lengthscales=np.exp(params["loglengthscales"][d]))
            for d in range(D)]
    with limit(seconds):
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(params["Z"], kern, [params["X"][s] for s in range(S)], c, np.exp(params["log_Q"]))
    return dict(Z=params["Z"], kern=kern, L=list(Lm[0]), U=list(U), H=list(Hinv), X0=params["X"][0], c=c, meta=meta)


def make_xnew(X0, c, T, N):
    """three quarters of the rows near chain 0's GP inputs, one quarter far from the data"""
    rng = np.random.default_rng(7)
    rows = np.concatenate((X0[:T], c[:T]), axis=1)
    near = N - N // 4
    pick = rng.choice(T, size=near, replace=near > T)
    return np.concatenate((rows[pick] + 0.05 * rng.standard_normal((near, rows.shape[1])),
                           3.0 * rng.standard_normal((N // 4, rows.shape[1]))))


def analytic(w, Xnew):
    return cmo.conditional_grad_grouped(w["L"], w["Z"], w["kern"], w["U"], w["H"], Xnew, summary=False)


def values(w, Xnew):
    return cmo.conditional_grouped(w["L"], w["Z"], w["kern"], w["U"], w["H"], Xnew, summary=False)[:2]


def differences(w, Xnew):
    """the central-difference composition: 2 P + 1 calls"""
    mean, var = values(w, Xnew)
    P = Xnew.shape[1]
    dm, dv = np.empty(mean.shape + (P,)), np.empty(var.shape + (P,))
    for p in range(P):
        e = np.zeros(P)
        e[p] = H
        (mu, vu), (md, vd) = values(w, Xnew + e), values(w, Xnew - e)
        dm[..., p], dv[..., p] = (mu - md) / (2 * H), (vu - vd) / (2 * H)
    return dict(mean=mean, var=var, dmean=dm, dvar=dv)


def timed_ms(fn, seconds):
    with limit(seconds):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def product_kernel_figures(path, cfg, N):
    """The tg_var_kernel row of a rocprofv3 kernel_stats.csv -> mean launch time and share of the fp64 MFMA peak."""
    if not os.path.exists(path):
        return None
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "tg_var_kernel" in r.get("Name", "")]
    if not rows:
        return None
    r = rows[0]
    calls, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
    Mp, units = (cfg["M"] + 63) // 64 * 64, cfg["S"] * cfg["D"]
    flop, per_launch_s = 2.0 * units * N * Mp * Mp, total_ns / calls * 1e-9
    return dict(kernel=r["Name"][:60], launches=calls, N=N, units=units, Mp=Mp, mean_launch_ms=round(per_launch_s * 1e3, 4), flop=flop,
                tflops=round(flop / per_launch_s / 1e12, 2), fraction_of_fp64_mfma_peak=round(flop / per_launch_s / 1e12 / PEAK_F64_TFLOPS, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--shapes", default="actuator,config2")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="SHAPE:N")
    ap.add_argument("--stats-csv", action="append", default=[], metavar="FILE:SHAPE:N", help="a rocprofv3 kernel_stats.csv of a --kernel-only run")
    a = ap.parse_args()
    if a.kernel_only:
        name, N = a.kernel_only.split(":")
        w = workload(SHAPES[name], a.limit)
        Xnew = make_xnew(w["X0"], w["c"], w["meta"]["T"], int(N))
        for _ in range(3):
            with limit(a.limit):
                analytic(w, Xnew)
        print(json.dumps(dict(shape=name, N=int(N))))
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
        w = workload(cfg, a.limit)
        P = w["meta"]["P"]
        for N in NS:
            Xnew = make_xnew(w["X0"], w["c"], cfg["T"], N)
            out = {}
            runs = dict(analytic=lambda: out.__setitem__("analytic", analytic(w, Xnew)),
                        differences=lambda: out.__setitem__("differences", differences(w, Xnew)), values=lambda: values(w, Xnew))
            for which in ("analytic", "differences", "values") * 2:            # all warmed up twice
                timed_ms(runs[which], a.limit)
            ts = dict(analytic=[], differences=[], values=[])
            for _ in range(a.repeats):                          # alternating, so that all see the same neighbours on the machine
                for which in ts:
                    ts[which].append(timed_ms(runs[which], a.limit))
            ta, td, tv = stats(ts["analytic"]), stats(ts["differences"]), stats(ts["values"])
            an, fd = out["analytic"], out["differences"]
            row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=cfg["D"], P=P, S=cfg["S"], N=N, conditional_calls_replaced=2 * P + 1,
                       analytic_ms=ta[0], analytic_min_max_ms=ta[1:], differences_ms=td[0], differences_min_max_ms=td[1:],
                       values_only_ms=tv[0], values_only_min_max_ms=tv[1:], speedup_over_differences=round(td[0] / ta[0], 2),
                       cost_over_values_only=round(ta[0] / tv[0], 2),
                       max_abs_dmean_vs_differences=float(np.abs(an["dmean"] - fd["dmean"]).max()),
                       max_abs_dvar_vs_differences=float(np.abs(an["dvar"] - fd["dvar"]).max()),
                       max_abs_mean_vs_values=float(np.abs(an["mean"] - fd["mean"]).max()),
                       max_abs_var_vs_values=float(np.abs(an["var"] - fd["var"]).max()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    kernel = []
    for spec in a.stats_csv:
        path, name, N = spec.rsplit(":", 2)
        fig = product_kernel_figures(path, SHAPES[name], int(N))
        if fig is not None:
            kernel.append(dict(shape=name, **fig))
            print(json.dumps(kernel[-1]), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_transition_grad.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats, h=H,
               baseline="2 P + 1 conditional_grouped calls on the same posteriors: the values, then Xnew +- h e_p for every input column",
               gate=None, points=rows, product_kernel=kernel)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
