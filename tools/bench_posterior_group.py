"""The fused grouped posteriors + rollouts against the composed path they replace, in one process on the same GPU:
`DGPSSM.collect_samples_chains(fused=True)` (one `ffvd_op_posterior_rollout_grouped` call: the S posteriors never leave the device)
and `collect_samples_chains(fused=False)` (kernel_pre_cal, one collapse_u_mean call per chain, then rollout_grouped: L^-T, the
L_H^-T slabs and the operand stacks cross the host link).  Wall time around the calls, uploads and downloads included (what a caller
pays); both warmed up, then measured alternately, median of --repeats runs.  No ratio is required: the record says where the fused path is not faster.

    python tools/bench_posterior_group.py [--repeats 5] [--out profiles/posterior_group.json] [--commit HASH] [--limit 120]

Every GPU step (building a model, each warmed-up measurement of one path at one point) runs under a time limit of its own: an
alarm whose default action ends the process, so a step that hangs inside the library ends the run and nothing more is started.
The record names the commit (`git rev-parse HEAD`, or --commit) and the SHA-256 of the library's sources and flags
(`ffvd_amd.build.source_hash()`).  FFVD_RG_TIMING=1 makes the library print where a fused call spends its wall time."""
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
from ffvd_amd import synthetic
from ffvd_amd.dgp_model import DGPSSM
from ffvd_amd.kernels import SquaredExponential
from ffvd_amd.likelihoods import Gaussian

SHAPES = {
    "actuator": dict(T=512, D=4, C=1, M=100, S=10),
    "config2": dict(T=4096, D=4, C=1, M=512, S=32),
}
STEPS = 200
ROLLOUTS = (1, 8)


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
    cc = np.concatenate((c, np.random.default_rng(5).standard_normal((steps, meta["C"]))))
    X = params["X"][0]
    mod = DGPSSM(Y, [D], M, [kern], lik, QQ_chol=np.exp(0.5 * params["log_Q"]), ZZ=params["Z"], control_inputs=cc, U_ini=params["U"],
                 X_0_ini=X[0], X_train_ini=X[1:], kernel_optimization=True, U_optimization=False, U_collapse=True, Z_optimization=True,
                 case_val=4, prior_type="normal", num_chains=S)
    mod.set_X(params["X"])
    return mod, cc, Y, meta


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
            mod, cc, Y, meta = model(cfg, STEPS)
        S, D = meta["S"], meta["D"]
        for R in ROLLOUTS:
            eps = np.random.default_rng(R).standard_normal((STEPS, S, R, D))
            out = {}

            def run(fused):
                out[fused] = mod.collect_samples_chains(R, cc, STEPS, Y_train=Y, eps=eps, fused=fused)

            for fused in (True, False, True, False):            # both sides warmed up twice
                timed_ms(lambda: run(fused), a.limit)
            tfs, tcs = [], []
            for _ in range(a.repeats):                          # alternating, so that both see the same neighbours on the machine
                tfs.append(timed_ms(lambda: run(True), a.limit))
                tcs.append(timed_ms(lambda: run(False), a.limit))
            tf, tc = stats(tfs), stats(tcs)
            dx = float(np.abs(out[True]["predict_x"] - out[False]["predict_x"]).max())
            dv = float(np.abs(out[True]["predict_x_var"] - out[False]["predict_x_var"]).max())
            row = dict(shape=name, T=cfg["T"], M=cfg["M"], D=D, S=S, R=R, steps=STEPS, fused_ms=round(tf[0], 3),
                       fused_min_max_ms=[round(tf[1], 3), round(tf[2], 3)], composed_ms=round(tc[0], 3),
                       composed_min_max_ms=[round(tc[1], 3), round(tc[2], 3)], speedup=round(tc[0] / tf[0], 2),
                       fused_is_faster=bool(tf[0] < tc[0]), max_abs_dx_vs_composed=dx, max_abs_dvar_vs_composed=dv)
            rows.append(row)
            print(json.dumps(row), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_posterior_group.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               baseline="collect_samples_chains(fused=False): the composed path as it stands at the parent commit",
               gate="none: no ratio is set in advance; fused_is_faster says how each point came out", points=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
