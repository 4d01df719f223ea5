"""Cubature filtering of R held-out records in one call against the two alternatives of the same build, in one process on the same GPU,
with the protocol of tools/bench_filter_records.py (model builder, time limit and statistics of tools/bench_moment_group.py): wall
time around calls that end in a synchronisation, uploads and the posteriors included; every side warmed up once, then measured
alternately, median of --repeats runs with min-max.  No time and no ratio is fixed in advance.

Workload: records of 200 rows, R = 1, 8, 32, 128, seeded observations, control rows and starts (those of tools/bench_filter_records.py).
  actuator   T = 512, M = 100, D = 4, S = 10, collapsed U;   config2   T = 4096, M = 512, D = 4, S = 32, collapsed U.
Sides:
  cubature     `posterior_filter_cubature_records_grouped` (posteriors, passes of a state and a product launch per step, 2D rows of K
               per track);
  linearised   `posterior_filter_records_grouped`: what the better rule costs over the extended Kalman rule;
  moment_loop  `collapse_u_mean_grouped` once, then one `filter_grouped(method="moment")` call per record: the path of comparable
               accuracy.  It is linear in R (one call per record), so beyond --moment-records records the loop runs over the first
               --moment-records of them and its time is scaled by R / that number; the JSON says where (the differences of the
               filtered means are taken over the records the loop ran; its ll_all covers those records only).
Fit (reported, not asserted): ll, ll_joint and RMSE of the three rules on the actuator fixture (tests/golden, three chains, 40 held-out
rows) and on the 200-row record of tools/bench_filter_linear.py at the two shapes, and max|m_filt - m_filt(moment)| of the cubature and
the linearised rule side by side.

    python tools/bench_filter_cubature.py [--repeats 5] [--out profiles/filter_cubature.json] [--commit HASH] [--limit 120] [--no-trace]

The kernel figures (time per launch of the state and the product kernel, the product's flop/s against the fp64 MFMA peak, the bytes of
Gamma it reads per second, the state kernel's exps per second) come from a trace the tool starts itself, in a child process of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_filter_cubature.py --kernel-only POINT:R

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
from bench_filter_records import PEAK_FP64_MFMA, RECORDS, ROWS, data
from bench_moment_group import SHAPES, STEPS, fixture_model, limit, model, stats, timed_ms
from ffvd_amd import conditionals_multi_output as cmo
from ffvd_amd import prediction as pr

POINTS = ("actuator", "config2")
FIT = ("ll", "ll_joint", "RMSE")


def sides_of(mod, meta, Y, ctrl, x0, moment_records):
    """the three sides of a point as callables that return dicts with m_filt (S, records run, rows, D)"""
    S, R = meta["S"], Y.shape[0]
    lay, lik = mod.layers[-1], mod.likelihood
    Xs, Qs, em = [mod._X_chains[s] for s in range(S)], [mod.Q] * S, (lik.CC, lik.DD, lik.log_Rchols)
    n = min(R, moment_records)

    def cubature():
        return pr.posterior_filter_cubature_records_grouped(lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, x0s=x0)

    def linearised():
        return pr.posterior_filter_records_grouped(lay.Z, lay.kernel, Xs, mod.Q, mod.control_inputs, ctrl, Y, *em, x0s=x0)

    def moment_loop():
        U, Hinv, Lm = cmo.collapse_u_mean_grouped(lay.Z, lay.kernel, Xs, mod.control_inputs, mod.Q)
        post = (list(Lm[0]), lay.Z, lay.kernel, list(U), list(Hinv))
        outs = [pr.filter_grouped(*post, list(x0[:, r]), ctrl[r], 0, Y[r], Qs, *em, method="moment") for r in range(n)]
        return dict(m_filt=np.stack([o["m_filt"] for o in outs], axis=1), lpd_mix=np.stack([o["lpd_mix"] for o in outs]))
    return dict(cubature=cubature, linearised=linearised, moment_loop=moment_loop), n


def kernel_figures(path, cfg, R):
    """The state and the product kernel in a rocprofv3 kernel_stats.csv -> launches and mean duration per launch; for the product its
    flop/s (2 rows Mp^2 per launch, rows = tracks * D * 2D) against the fp64 MFMA peak and the bytes of Gamma it reads per second (once
    per row tile of a unit); for the state kernel the exps per second (tracks * D * 2D * M per launch)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for key, pick in (("state", lambda n: "mg_crec_state_kernel" in n), ("product", lambda n: "mg_lfan_var_kernel" in n)):
        hit = [r for r in rows if pick(r.get("Name", ""))]
        if hit:
            calls, total = sum(int(r["Calls"]) for r in hit), sum(float(r["TotalDurationNs"]) for r in hit)
            out[key] = dict(kernel=hit[0]["Name"][:90], launches=calls, mean_launch_us=round(total / calls * 1e-3, 3))
    G, D, M = cfg["S"], cfg["D"], cfg["M"]
    Mp = (M + 63) // 64 * 64
    krows = G * R * D * 2 * D
    if "product" in out:
        us = out["product"]["mean_launch_us"]
        flop, gam = 2.0 * krows * Mp * Mp, 8.0 * G * D * Mp * Mp * ((R * 2 * D + 127) // 128)
        out["product"].update(rows_of_K=krows, rows_per_unit=R * 2 * D, flop_per_launch=flop, tflops=round(flop / (us * 1e-6) / 1e12, 3),
                              fraction_of_fp64_mfma_peak=round(flop / (us * 1e-6) / PEAK_FP64_MFMA, 4),
                              gamma_gbytes_per_second=round(gam / (us * 1e-6) / 1e9, 1))
    if "state" in out:
        us = out["state"]["mean_launch_us"]
        out["state"].update(workgroups=G * R * D, exps_per_launch=krows * M, gexps_per_second=round(krows * M / (us * 1e-6) / 1e9, 2),
                            k_gbytes_written_per_second=round(8.0 * krows * Mp / (us * 1e-6) / 1e9, 1))
    return out


def kernel_trace(point, R, seconds):
    """One child under rocprofv3 (kernel trace only): three calls of the cubature path at `point` with R records."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return dict(skipped="rocprofv3 not found")
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", f"{point}:{R}"]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        if proc.returncode != 0:
            raise RuntimeError(f"the traced child ended with {proc.returncode}:\n{proc.stdout[-2000:]}{proc.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        return kernel_figures(found[0], SHAPES[point], R) if found else dict(skipped="no kernel_stats.csv was written")


def fit_of(out, record=None):
    return {k.lower(): float(out[k] if record is None else out[k][record]) for k in FIT}


def fit_three(mod, Y_test, cc, n_train):
    """ll, ll_joint, RMSE of the three rules on one record that continues the training sequence, and the filtered means against moment
    matching's"""
    mom, lin = mod.filter_heldout(Y_test, cc), mod.filter_heldout_linearised(Y_test, cc)
    cub = mod.filter_records_cubature(Y_test[None], cc[n_train: n_train + len(Y_test)][None])
    apart = dict(cubature=float(np.max(np.abs(cub["m_filt"][:, 0] - mom["m_filt"]))),
                 linearised=float(np.max(np.abs(lin["m_filt"] - mom["m_filt"]))))
    return dict(moment=fit_of(mom), linearised=fit_of(lin), cubature=fit_of(cub, 0), largest_m_filt_difference_from_moment=apart)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--records", default=",".join(str(r) for r in RECORDS))
    ap.add_argument("--moment-records", type=int, default=32, help="the most records the moment loop really runs; beyond, its time is scaled")
    ap.add_argument("--trace-records", default="1,32", help="the R at which the kernels are traced")
    ap.add_argument("--limit", type=int, default=120, help="seconds a single GPU step may take before the process is ended")
    ap.add_argument("--kernel-only", default=None, metavar="POINT:R", help="three calls of the cubature path and nothing else (for a profiler)")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        point, R = a.kernel_only.split(":")
        with limit(a.limit):
            mod, cc, _, meta = model(SHAPES[point], ROWS)
        new = sides_of(mod, meta, *data(meta, int(R), mod), a.moment_records)[0]["cubature"]
        for _ in range(3):
            with limit(a.limit):
                f = new()
        print(json.dumps(dict(point=point, R=int(R), ll=f["ll"][:4].tolist())))
        return 0
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    with limit(a.limit):
        fmod, fc, fY = fixture_model()
        fit = dict(actuator_fixture=fit_three(fmod, fY, fc, fmod.Y.shape[0]))
    print(json.dumps(fit), flush=True)
    rows, trace = [], {}
    counts, traced = [int(r) for r in a.records.split(",") if r], [int(r) for r in a.trace_records.split(",") if r]
    for point in [s for s in a.points.split(",") if s]:
        cfg = SHAPES[point]
        with limit(a.limit):
            mod, cc, Y_test, meta = model(cfg, ROWS)
        assert ROWS == STEPS
        with limit(a.limit):
            fit[point] = fit_three(mod, Y_test, cc, cfg["T"])
        print(json.dumps({point: fit[point]}), flush=True)
        for R in counts:
            (sides, n_mom), out = sides_of(mod, meta, *data(meta, R, mod), a.moment_records), {}

            def run(k):
                out[k] = sides[k]()

            for k in sides:                                         # every side warmed up once
                timed_ms(lambda: run(k), a.limit)
            ts = {k: [] for k in sides}
            for _ in range(a.repeats):                              # alternating, so that all see the same neighbours on the machine
                for k in sides:
                    ts[k].append(timed_ms(lambda: run(k), a.limit))
            ts["moment_loop"] = [t * R / n_mom for t in ts["moment_loop"]]
            med = {k: statistics.median(v) for k, v in ts.items()}
            mom = out["moment_loop"]["m_filt"]
            apart = {k: float(np.max(np.abs(out[k]["m_filt"][:, :n_mom] - mom))) for k in ("cubature", "linearised")}
            row = dict(point=point, T=cfg["T"], M=cfg["M"], D=meta["D"], S=meta["S"], rows=ROWS, R=R, tracks=meta["S"] * R,
                       ms_median_min_max={k: stats(v) for k, v in ts.items()}, moment_loop_records_run=n_mom,
                       moment_loop_scaled_by=round(R / n_mom, 3), cubature_over_linearised=round(med["cubature"] / med["linearised"], 3),
                       moment_loop_over_cubature=round(med["moment_loop"] / med["cubature"], 3),
                       fastest=min(med, key=med.get), launch_pairs=ROWS + 1,
                       wall_us_per_launch_pair=round(med["cubature"] * 1e3 / (ROWS + 1), 2),
                       largest_m_filt_difference_from_the_moment_loop=apart,
                       ll_all=dict(cubature=float(out["cubature"]["ll_all"]), linearised=float(out["linearised"]["ll_all"]),
                                   moment_loop=float(np.mean(out["moment_loop"]["lpd_mix"]))))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if not a.no_trace and R in traced:
                trace[f"{point}:{R}"] = kernel_trace(point, R, 4 * a.limit)
                print(json.dumps({f"{point}:{R}": trace[f"{point}:{R}"]}), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_filter_cubature.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="posterior_filter_cubature_records_grouped: the posteriors once, passes of a state and a product launch per step for "
                        "all (chain, record) tracks, 2D rows of K per (track, dim)",
               baselines=dict(linearised="posterior_filter_records_grouped of the same build",
                              moment_loop="collapse_u_mean_grouped once, then one filter_grouped(method='moment') call per record, of the "
                                          "same build; beyond moment_loop_records_run records its time is scaled (it is one call per record)"),
               timing="wall time around calls that end in a synchronisation; alternating after one warm-up call per side",
               fit_reported_not_asserted=fit, points=rows, kernels=trace or None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
