// Rollout summaries (predict_summary.hip): the held-out predictive summary of base_model.py:330-348 over N rollouts, formed from
// the [N][steps][D] stacks predict_x / predict_var (= f_var + Q) where rg_step_kernel left them in device memory.
//   p[n][t][j]        = sum_k x[n][t][k] CC[k][j]                                   (k ascending)
//   y_mean[t][j]      = (1/N) sum_n p + DD_j                                        (:341)
//   y_var[t][j]       = (1/N) sum_n sum_k v[n][t][k] CC[k][j]^2 + s_j^2             (:342, the reference's variance)
//   y_var_total[t][j] = s_j^2 + (1/N) sum_n (p - pbar)^2                            (law of total variance over the rollouts)
//   lpd[t][j]         = log (1/N) sum_n N(y[t][j]; p + DD_j, s_j^2),  t < n_test    (Monte-Carlo predictive density)
//   lpd_gauss[t][j]   = log N(y[t][j]; y_mean[t][j], y_var_total[t][j]),  t < n_test
// Two launches.  ps_partial: a wavefront owns a chunk of PS_CHUNK rollouts and a tile of PS_TILE steps, lane = step, and walks its
// rollouts in ascending order; per (chunk, t, j) it leaves mean and M2 of p (Welford), sum v CC^2, and the running maximum and
// scaled sum of the exponents.  ps_merge: one thread per (t, j) merges the chunks in ascending order and writes the outputs.
// No atomics; the decomposition is a function of (N, steps, D, J) only: two calls are bit-identical.
// Limits (the operators return FFVD_EINVAL beyond them): D <= 32, J <= PS_MAXJ, N * steps * D < 2^31.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace ffvd {

constexpr int PS_CHUNK = 32;         // rollouts per wavefront
constexpr int PS_TILE = 64;          // steps per wavefront: one per lane
constexpr int PS_WAVES = 4;          // wavefronts (chunks) per workgroup
constexpr int PS_MAXJ = 8;           // outputs (that of the particle-Gibbs step)
constexpr int PS_FIELDS = 5;         // mean, M2, sum v CC^2, largest exponent, scaled sum of exponentials

struct PredictSummaryArgs {
    int N, steps, D, J, n_test;
    const double *x, *v;             // [N][steps][D]
    const double *CC;                // [D][J]
    const double *DD, *sd;           // [J]: offset, noise standard deviation
    const double *Y;                 // [n_test][J] or nullptr
    double *part;                    // [chunks][PS_FIELDS][steps][J]
    double *out;                     // [5][steps][J]: y_mean, y_var, y_var_total, lpd, lpd_gauss (the last two: rows t < n_test)
};

__host__ __device__ inline size_t ps_chunks(int N) { return ((size_t)N + PS_CHUNK - 1) / PS_CHUNK; }
inline size_t ps_part_doubles(int N, int steps, int J) { return ps_chunks(N) * PS_FIELDS * (size_t)steps * J; }
inline size_t ps_out_doubles(int steps, int J) { return (size_t)5 * steps * J; }

void launch_predict_summary(hipStream_t stream, const PredictSummaryArgs &a);

}  // namespace ffvd
