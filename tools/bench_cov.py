"""Full predictive covariance at config 2's shapes ("full covariance"): Z, kernels and chain-0 X_combine of
synthetic.make_named("c2"), N = 4096, M = 512, D = 4, through conditional_after_kernel_precalculation(full_cov=True) without and
with the posterior q_sqrt of collapse_u_mean_after_kernel_precalculation.  Prints one JSON line.

The wall time per call is dominated by copying the D N^2 8 B = 537 MB result to the host; the kernel's own time comes from a
separate `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_cov.py` run (rows cov_kernel)."""
import json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ffvd_amd import synthetic, conditionals_multi_output as cmo
from ffvd_amd.kernels import SquaredExponential


def main(reps=3):
    params, Y, c, meta = synthetic.make_named("c2")
    D, P, T = meta["D"], meta["P"], meta["T"]
    X0 = params["X"][0]
    xc = np.concatenate((X0[:-1], c[:T]), axis=1)
    Z = params["Z"]
    M, N = Z.shape[0], xc.shape[0]
    kern = [SquaredExponential(P, variance=np.exp(params["logvariance"][d]), lengthscales=np.exp(params["loglengthscales"][d]))
            for d in range(D)]
    W = cmo.kernel_pre_cal(Z, kern)
    Um, Hinv = cmo.collapse_u_mean_after_kernel_precalculation(W, xc, X0, Z, kern, np.exp(params["log_Q"]))
    out = {"N": N, "M": M, "D": D,
           # lower triangle of Sigma_d (N (N + 1) / 2 entries) at depth M (2 M with q_sqrt), 2 flops per multiply-add
           "flop_cov": float(D * N * (N + 1) * M), "flop_cov_qsqrt": float(D * N * (N + 1) * 2 * M),
           "flop_e": float(D * 2 * N * M * M)}                      # E_d = F_d q0
    for tag, q in (("plain", None), ("qsqrt", Hinv)):
        cmo.conditional_after_kernel_precalculation(W, xc, Z, kern, Um, full_cov=True, q_sqrt=q, white=True)     # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            mean, var = cmo.conditional_after_kernel_precalculation(W, xc, Z, kern, Um, full_cov=True, q_sqrt=q, white=True)
            ts.append(time.perf_counter() - t0)
        assert var.shape == (D, N, N) and np.isfinite(var).all()
        out[f"wall_ms_{tag}"] = round(1e3 * float(np.median(ts)), 2)
        del var
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
