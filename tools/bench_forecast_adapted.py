"""Adapted particle rolling-origin forecasts in one call against the bootstrap fan of the same build and against the composed form a
user of the adapted filter had before, in one process on the same GPU, with the protocol of tools/bench_forecast_particle.py (model
builder, time limit and statistics of tools/bench_moment_group.py): wall time around calls that end in a synchronisation, the draws,
uploads, downloads and the posteriors included; every side warmed up once, then measured alternately, median of --repeats runs with
min-max.  No ratio is fixed in advance.

Workload: a record of 200 rows, horizon 10, collapsed U, stride 10 (19 origins) and stride 1 (190 origins); N = 64 / 256 / 1024 at
the actuator shape (T = 512, M = 100, D = 4, S = 10), N = 64 / 256 at config 2 (T = 4096, M = 512, D = 4, S = 32) and N = 896 -- the
largest count whose rows fit a pass there -- with 19 origins only.

  adapted    `DGPSSM.forecast_heldout_adapted`: ffvd_posterior_particle_adapted_forecast_grouped (posteriors, the adapted records
             launches with one record, passes of three launches per forecast step, pooled summary);
  bootstrap  `DGPSSM.forecast_heldout_particle` with the same seed: the same draws;
  composed   ONE `DGPSSM.filter_records_adapted` call with one record per origin, each Y[:o + 1] followed by h all-NaN rows (lengths
             o + 1 + h): B (o + h) track steps where the fan takes n + B h.  Both sides draw with noise="shared", so the composed
             form's tracks are tracks of the same law and not the same numbers (the bit identity of a track with the composed form on
             concatenated draws is what tests/test_gpu_forecast_adapted.py asserts).

On the actuator fixture of the tests (not timed): over --seeds seeds at N = 256 the standard deviation of ll_h at k = 1, 5, 10 of the
adapted and of the bootstrap fan, and per fan the largest |ll_h(N = 256) - ll_h(N = 1024)| over the horizons (both at the first seed).

    python tools/bench_forecast_adapted.py [--repeats 5] [--seeds 20] [--points P1,P2] [--out profiles/forecast_adapted.json] [--commit HASH]

Every GPU step runs under a time limit of its own (an alarm whose default action ends the process)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from bench_forecast_particle import AT, HORIZON, POINTS, ROWS, SEED
from bench_moment_group import SHAPES, fixture_model, limit, model, stats, timed_ms

FANS = ("adapted", "bootstrap")


def fixture_spread(seeds, seconds):
    """The two fans on the actuator fixture (tests/golden/actuator_slim.npz: 400 training rows, three chains, a 40-row held-out record,
    every row an origin) at N = 256 over `seeds` seeds, and at N = 1024 with the first seed."""
    with limit(seconds):
        mod, c, Y_test = fixture_model()
    fn = dict(adapted=mod.forecast_heldout_adapted, bootstrap=mod.forecast_heldout_particle)
    ll = {k: [] for k in FANS}
    for s in range(seeds):
        for k in FANS:
            with limit(seconds):
                ll[k].append(fn[k](Y_test, c, HORIZON, num_particles=256, seed=SEED + s)["ll_h"][:, 0])
    big = {}
    for k in FANS:
        with limit(seconds):
            big[k] = fn[k](Y_test, c, HORIZON, num_particles=1024, seed=SEED)["ll_h"][:, 0]
    sd = {k: np.std(np.stack(v), axis=0, ddof=1) for k, v in ll.items()}
    return dict(rows=int(Y_test.shape[0]), seeds=seeds, N=256, horizons=[k + 1 for k in AT],
                ll_h_mean={k: [float(np.mean(np.stack(v), axis=0)[i]) for i in AT] for k, v in ll.items()},
                ll_h_sd={k: [float(v[i]) for i in AT] for k, v in sd.items()},
                ll_h_sd_all_horizons={k: v.tolist() for k, v in sd.items()},
                ll_h_n1024={k: [float(v[i]) for i in AT] for k, v in big.items()},
                largest_abs_ll_h_n256_minus_n1024={k: float(np.max(np.abs(ll[k][0] - big[k]))) for k in FANS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--limit", type=int, default=180, help="seconds a single GPU step may take before the process is ended")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    rows, models = [], {}
    for point in [s for s in a.points.split(",") if s]:
        shape, stride, n = POINTS[point]
        cfg = SHAPES[shape]
        if shape not in models:
            with limit(a.limit):
                models[shape] = model(cfg, ROWS)
        mod, cc, Y_test, meta = models[shape]
        S, D = meta["S"], meta["D"]
        n_train, J = mod.Y.shape[0], Y_test.shape[1]
        origins = list(range(0, ROWS - HORIZON, stride))
        B = len(origins)
        out = {}
        # the composed form's records: record b is Y[:o + 1] followed by h all-NaN rows, its control rows those the fan reads
        Yr = np.full((B, ROWS, J), np.nan)
        for b, o in enumerate(origins):
            Yr[b, :o + 1] = Y_test[:o + 1]
        lengths = np.asarray([o + 1 + HORIZON for o in origins])
        cr = None if cc is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cc)[n_train: n_train + ROWS], (B, ROWS, np.shape(cc)[1])))
        sides = {"adapted": lambda: mod.forecast_heldout_adapted(Y_test, cc, HORIZON, stride=stride, num_particles=n, seed=SEED),
                 "bootstrap": lambda: mod.forecast_heldout_particle(Y_test, cc, HORIZON, stride=stride, num_particles=n, seed=SEED),
                 "composed": lambda: mod.filter_records_adapted(Yr, cr, lengths=lengths, num_particles=n, seed=SEED)}

        def run(k):
            out[k] = sides[k]()

        for k in sides:                                         # one warm-up per side
            timed_ms(lambda: run(k), a.limit)
        ts = {k: [] for k in sides}
        for _ in range(a.repeats):                              # alternating, so that all see the same neighbours on the machine
            for k in sides:
                ts[k].append(timed_ms(lambda: run(k), a.limit))
        med = {k: statistics.median(v) for k, v in ts.items()}
        row = dict(point=point, shape=shape, T=cfg["T"], M=cfg["M"], D=D, S=S, rows=ROWS, horizon=HORIZON, stride=stride, origins=B, N=n,
                   tracks=S * B, ms_median_min_max={k: stats(v) for k, v in ts.items()}, horizons=[k + 1 for k in AT],
                   rmse_h={k: [out[k]["rmse_h"][i, 0] for i in AT] for k in FANS}, ll_h={k: [out[k]["ll_h"][i, 0] for i in AT] for k in FANS},
                   adapted_over_bootstrap=round(med["adapted"] / med["bootstrap"], 3),
                   composed_over_adapted=round(med["composed"] / med["adapted"], 3),
                   composed_track_steps=int(lengths.sum()), adapted_track_steps=ROWS + B * HORIZON)
        rows.append(row)
        print(json.dumps(row), flush=True)
    fixture = fixture_spread(a.seeds, a.limit) if a.seeds > 1 else None
    print(json.dumps(dict(actuator_fixture=fixture)), flush=True)
    from ffvd_amd.build import source_hash
    doc = dict(tool="tools/bench_forecast_adapted.py", commit=commit, library_source_hash=source_hash(), repeats=a.repeats,
               new_path="DGPSSM.forecast_heldout_adapted: ffvd_posterior_particle_adapted_forecast_grouped (posteriors, the adapted records "
                        "launches with one record, passes of a state, a rows and a product launch per step, pooled summary)",
               baselines=dict(bootstrap="DGPSSM.forecast_heldout_particle of the same build, the same seed",
                              composed="one DGPSSM.filter_records_adapted call with one record per origin, Y[:o + 1] followed by h all-NaN "
                                       "rows: of the same build; shared draws on both sides"),
               timing="wall time around calls that end in a synchronisation, the draws included; alternating after one warm-up call per side",
               points=rows, actuator_fixture=fixture)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
