// Proper scores and quantiles of equal-weight Gaussian mixtures (predict_score.hip).  A target is (row t, output j); its predictive
// distribution is the mixture of K components N(mu_k, v_k), staged from the caller's stack:
//   points   mu_k = sum_d x[k][t][d] CC[d][j] (d ascending) + DD_j,  v_k = s_j^2            (one variance per output)
//   moments  mu_g = CC_j^T m[g][t] + DD_j,  v_g = CC_j^T S[g][t] CC_j + s_j^2
// With A(d, v) = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v)) = E|N(d, v)| and Phi(z) = erfc(-z / sqrt 2) / 2:
//   crps[t][j]         = (1/K) sum_k A(y - mu_k, v_k) - (1/(2 K^2)) sum_k sum_l A(mu_k - mu_l, v_k + v_l)
//   pit[t][j]          = F(y),  F(x) = (1/K) sum_k Phi((x - mu_k) / sqrt v_k)
//   quantiles[t][j][q] = the x with F(x) = levels[q]
// Launches.  psc_stage_*: one thread per (row, component) forms mu (and v, 1 / sqrt(2 v)) of every output, laid out [target][K].
// psc_pair: a workgroup owns (target, a <= b), a pair of component tiles of PSC_TILE; thread i holds component i of tile a, tile b
// is staged in LDS, and every unordered pair is evaluated once (off the diagonal doubled, on it A(0, 2 v_k) = 2 sqrt(v_k / pi));
// the workgroup's sum goes to part[target][pair].  psc_crps: one workgroup per target adds the partials and the first term and
// writes crps.  psc_pit: one workgroup per target, F(y).  psc_quantile: one workgroup per (target, level) bisects F inside
// [min mu - 8.5 max sigma, max mu + 8.5 max sigma] until the midpoint equals an end point, at most PSC_BISECT_CAP times.
// Every sum over components or partials is psc_block_sum: thread i adds the entries i, i + PSC_TILE, ... in ascending order, then
// the PSC_TILE thread sums are folded by a fixed tree.  No atomics; the decomposition is a function of (K, steps, J, Q) only, a
// target does not see the other targets or the pass size, a level does not see the other levels.  A component that is not finite
// (or whose variance is not positive) makes the outputs of its target NaN and nothing else.
// Limits (the drivers return FFVD_EINVAL beyond them): K <= PSC_MAXK, D <= 32 (points) / 8 (moments), J <= PSC_MAXJ,
// Q <= PSC_MAXQ, steps * J * K < 2^31.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace ffvd {

constexpr int PSC_TILE = 256;          // components per tile = threads per workgroup
constexpr int PSC_MAXK = 65536;
constexpr int PSC_MAXJ = 8;
constexpr int PSC_MAXQ = 16;
constexpr int PSC_MAXD_POINTS = 32;
constexpr int PSC_MAXD_MOMENTS = 8;
constexpr int PSC_BISECT_CAP = 128;    // the guarantee that a bisection ends (about 60 halvings reach neighbouring doubles)
constexpr double PSC_BRACKET = 8.5;    // Phi(-8.5) < 1e-17: below every admissible level
constexpr size_t PSC_PART_DOUBLES = (size_t)1 << 23;      // bound of the partials of one pass (64 MiB)

struct ScoreArgs {
    int K, steps, D, J, n_test, Q;
    int equal_var;                     // 1: points (v = s_j^2, var and rs are not read), 0: moments
    const double *CC, *DD, *sd;        // [D][J], [J], [J]
    const double *Y;                   // [n_test][J] or nullptr
    const double *levels;              // [Q] or nullptr
    double *mu, *var, *rs;             // [steps * J][K]: mean, variance, 1 / sqrt(2 variance)
    double *part;                      // [targets of a pass][psc_pairs(K)]
    double *crps, *pit, *quant;        // [n_test][J], [n_test][J], [steps][J][Q]; each may be nullptr
};

inline int psc_tiles(int K) { return (K + PSC_TILE - 1) / PSC_TILE; }
inline size_t psc_pairs(int K) { return (size_t)psc_tiles(K) * (psc_tiles(K) + 1) / 2; }
// targets per pass of the pair kernel: the caller's (0: automatic), bounded by PSC_PART_DOUBLES of partials
inline int psc_targets_per_pass(int K, int targets_per_pass) {
    size_t fit = PSC_PART_DOUBLES / psc_pairs(K);
    if (fit < 1) fit = 1;
    if (fit > 65535) fit = 65535;
    return targets_per_pass > 0 && (size_t)targets_per_pass < fit ? targets_per_pass : (int)fit;
}

// x: the caller's stack on the device, component k = k1 * K2 + k2 at x + k1 * stride_k1 + k2 * stride_k2, its row t at + t * stride_t
void launch_score_stage_points(hipStream_t stream, const ScoreArgs &a, const double *x, int K2, long long stride_k1, long long stride_k2,
                               long long stride_t);
// m [K][steps][D], S [K][steps][D][D]
void launch_score_stage_moments(hipStream_t stream, const ScoreArgs &a, const double *m, const double *S);
// crps of the targets [first, first + count) of the n_test * J scored ones (count <= the pass size a.part was sized for)
void launch_score_crps(hipStream_t stream, const ScoreArgs &a, int first, int count);
void launch_score_pit(hipStream_t stream, const ScoreArgs &a);
void launch_score_quantiles(hipStream_t stream, const ScoreArgs &a);

}  // namespace ffvd
