// Proper scores and quantiles of equal-weight Gaussian mixtures: the kernels of predict_score.h (method, decomposition and limits
// are described there).
#include "predict_score.h"

#include <cmath>

namespace ffvd {
namespace {

constexpr double PSC_INV_SQRT_PI = 0.56418958354775628695;

enum { PSC_SUM, PSC_MIN, PSC_MAX };

// The workgroup's reduction of one value per thread, in a fixed order (a tree over the thread index); every thread gets the result.
// red: PSC_TILE doubles of LDS, free again when the call returns to its last thread (the leading barrier covers the next call).
template <int OP>
__device__ inline double psc_block_reduce(double v, double *red) {
    const int i = threadIdx.x;
    __syncthreads();
    red[i] = v;
    __syncthreads();
    for (int s = PSC_TILE / 2; s > 0; s >>= 1) {
        if (i < s) red[i] = OP == PSC_SUM ? red[i] + red[i + s] : OP == PSC_MIN ? fmin(red[i], red[i + s]) : fmax(red[i], red[i + s]);
        __syncthreads();
    }
    return red[0];
}
__device__ inline double psc_block_sum(double v, double *red) { return psc_block_reduce<PSC_SUM>(v, red); }

// the one test of a component in the three target-level kernels: a mean or a variance that is not finite (a variance of +Inf has
// 1 / sqrt(2 v) = 0, which is finite), or a variance that is not positive, makes every output of the target NaN
__device__ inline bool psc_component_ok(double m, double v) { return isfinite(m) && isfinite(v) && v > 0.0; }

// A(d, v) with sq = sqrt(2 v)
__device__ inline double psc_abs_moment(double d, double sq) {
    const double z = d / sq;
    return d * erf(z) + sq * PSC_INV_SQRT_PI * exp(-z * z);
}

// F(x) of one target: the K-long reduction every PIT and every bisection step uses.  rs: 1 / sqrt(2 v_k) per component, or nullptr
// with rs0 for all of them.
__device__ inline double psc_cdf(double x, const double *mu, const double *rs, double rs0, int K, double *red) {
    double s = 0.0;
    for (int k = threadIdx.x; k < K; k += PSC_TILE) s += 0.5 * erfc((mu[k] - x) * (rs ? rs[k] : rs0));
    return psc_block_sum(s, red) / (double)K;
}

// ---- staging ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PSC_TILE) void psc_stage_points_kernel(ScoreArgs a, const double *x, int K2, long long stride_k1,
                                                                    long long stride_k2, long long stride_t) {
    const long long gid = (long long)blockIdx.x * PSC_TILE + threadIdx.x;
    if (gid >= (long long)a.steps * a.K) return;
    const int t = (int)(gid / a.K), k = (int)(gid % a.K);
    const double *xr = x + (k / K2) * stride_k1 + (k % K2) * stride_k2 + t * stride_t;
    for (int j = 0; j < a.J; ++j) {
        double acc = 0.0;
        for (int d = 0; d < a.D; ++d) acc += xr[d] * a.CC[d * a.J + j];
        a.mu[((size_t)t * a.J + j) * a.K + k] = acc + a.DD[j];
    }
}

__global__ __launch_bounds__(PSC_TILE) void psc_stage_moments_kernel(ScoreArgs a, const double *m, const double *S) {
    const long long gid = (long long)blockIdx.x * PSC_TILE + threadIdx.x;
    if (gid >= (long long)a.steps * a.K) return;
    const int t = (int)(gid / a.K), g = (int)(gid % a.K), D = a.D;
    const double *mr = m + ((size_t)g * a.steps + t) * D, *Sr = S + ((size_t)g * a.steps + t) * D * D;
    for (int j = 0; j < a.J; ++j) {
        double mean = 0.0, quad = 0.0;
        for (int p = 0; p < D; ++p) {
            double row = 0.0;
            for (int q = 0; q < D; ++q) row += Sr[p * D + q] * a.CC[q * a.J + j];
            mean += mr[p] * a.CC[p * a.J + j];
            quad += a.CC[p * a.J + j] * row;
        }
        const double v = quad + a.sd[j] * a.sd[j];
        const size_t at = ((size_t)t * a.J + j) * a.K + g;
        a.mu[at] = mean + a.DD[j];
        a.var[at] = v;
        a.rs[at] = 1.0 / sqrt(2.0 * v);
    }
}

// ---- CRPS: the pair kernel and its finish ---------------------------------------------------------------------------------------------
// grid: count * pairs workgroups, workgroup (target first + tl, tile pair a <= b).  EQ: every component has the variance s_j^2, so
// sqrt(2 (v_k + v_l)) = 2 s_j is one constant per output.
template <bool EQ>
__global__ __launch_bounds__(PSC_TILE) void psc_pair_kernel(ScoreArgs a, int first, int tiles, int pairs) {
    __shared__ double smu[PSC_TILE], sv[PSC_TILE], red[PSC_TILE];
    const int tl = blockIdx.x / pairs, pair = blockIdx.x % pairs;
    int ta = 0, rem = pair;
    while (rem >= tiles - ta) { rem -= tiles - ta; ++ta; }
    const int tb = ta + rem, target = first + tl, j = target % a.J, K = a.K, i = threadIdx.x;
    const double *mu = a.mu + (size_t)target * K, *var = EQ ? nullptr : a.var + (size_t)target * K;
    const int ka = ta * PSC_TILE + i, kb = tb * PSC_TILE + i, nb = min(PSC_TILE, K - tb * PSC_TILE);
    if (kb < K) {
        smu[i] = mu[kb];
        if (!EQ) sv[i] = var[kb];
    }
    __syncthreads();
    const double s = a.sd[j], inv = 0.5 / s, c = 2.0 * s * PSC_INV_SQRT_PI;
    double sum = 0.0;
    if (ka < K) {
        const double mi = mu[ka], vi = EQ ? 0.0 : var[ka];
        const bool diag = ta == tb;
        for (int l = diag ? (i & ~63) + 1 : 0; l < nb; ++l) {          // (a wavefront of a diagonal tile starts behind its first lane)
            if (!diag || l > i) {
                const double d = mi - smu[l];
                if (EQ) {
                    const double z = d * inv;
                    sum += d * erf(z) + c * exp(-z * z);
                } else {
                    sum += psc_abs_moment(d, sqrt(2.0 * (vi + sv[l])));
                }
            }
        }
        sum *= 2.0;
        if (diag) sum += EQ ? c : 2.0 * sqrt(vi) * PSC_INV_SQRT_PI;     // A(0, 2 v_k)
    }
    const double total = psc_block_sum(sum, red);
    if (i == 0) a.part[(size_t)tl * pairs + pair] = total;
}

// one workgroup per target of the pass: the first term, the partials, the non-finite check, crps
template <bool EQ>
__global__ __launch_bounds__(PSC_TILE) void psc_crps_kernel(ScoreArgs a, int first, int pairs) {
    __shared__ double red[PSC_TILE];
    const int target = first + blockIdx.x, j = target % a.J, K = a.K;
    const double *mu = a.mu + (size_t)target * K, *var = EQ ? nullptr : a.var + (size_t)target * K;
    const double y = a.Y[target], v0 = a.sd[j] * a.sd[j];
    double s = 0.0, bad = 0.0;
    for (int k = threadIdx.x; k < K; k += PSC_TILE) {
        const double m = mu[k], v = EQ ? v0 : var[k];
        if (!psc_component_ok(m, v)) bad = 1.0;
        s += psc_abs_moment(y - m, sqrt(2.0 * v));
    }
    const double term = psc_block_sum(s, red);
    double p = 0.0;
    for (int q = threadIdx.x; q < pairs; q += PSC_TILE) p += a.part[(size_t)blockIdx.x * pairs + q];
    const double pair = psc_block_sum(p, red);
    const double nbad = psc_block_sum(bad, red);
    if (threadIdx.x == 0) a.crps[target] = (nbad > 0.0 || isnan(y)) ? NAN : term / (double)K - pair / (2.0 * (double)K * (double)K);
}

// ---- PIT and quantiles ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PSC_TILE) void psc_pit_kernel(ScoreArgs a) {
    __shared__ double red[PSC_TILE];
    const int target = blockIdx.x, j = target % a.J, K = a.K;
    const double *mu = a.mu + (size_t)target * K, *rs = a.equal_var ? nullptr : a.rs + (size_t)target * K;
    const double *var = a.equal_var ? nullptr : a.var + (size_t)target * K;
    const double y = a.Y[target], v0 = a.sd[j] * a.sd[j], rs0 = 1.0 / (a.sd[j] * sqrt(2.0));
    double bad = 0.0;
    for (int k = threadIdx.x; k < K; k += PSC_TILE)
        if (!psc_component_ok(mu[k], var ? var[k] : v0)) bad = 1.0;
    const double F = psc_cdf(y, mu, rs, rs0, K, red), nbad = psc_block_sum(bad, red);
    if (threadIdx.x == 0) a.pit[target] = (nbad > 0.0 || isnan(y)) ? NAN : F;
}

// one workgroup per (target, level).  Every branch below is taken on a value all threads hold (a reduction's result), so the
// barriers inside psc_cdf are reached by the whole workgroup; the loop ends after PSC_BISECT_CAP steps whatever F returns.
__global__ __launch_bounds__(PSC_TILE) void psc_quantile_kernel(ScoreArgs a) {
    __shared__ double red[PSC_TILE];
    const int target = blockIdx.x / a.Q, j = target % a.J, K = a.K;
    const double *mu = a.mu + (size_t)target * K, *rs = a.equal_var ? nullptr : a.rs + (size_t)target * K;
    const double *var = a.equal_var ? nullptr : a.var + (size_t)target * K;
    const double p = a.levels[blockIdx.x % a.Q], v0 = a.sd[j] * a.sd[j], rs0 = 1.0 / (a.sd[j] * sqrt(2.0));
    double lo = INFINITY, hi = -INFINITY, vmax = 0.0, bad = 0.0;
    for (int k = threadIdx.x; k < K; k += PSC_TILE) {
        const double m = mu[k], v = var ? var[k] : v0;
        if (!psc_component_ok(m, v)) bad = 1.0;
        lo = fmin(lo, m); hi = fmax(hi, m); vmax = fmax(vmax, v);
    }
    lo = psc_block_reduce<PSC_MIN>(lo, red);
    hi = psc_block_reduce<PSC_MAX>(hi, red);
    vmax = psc_block_reduce<PSC_MAX>(vmax, red);
    const double nbad = psc_block_sum(bad, red);
    double x = NAN;
    if (!(nbad > 0.0)) {
        const double w = PSC_BRACKET * sqrt(vmax);
        lo -= w; hi += w;
        for (int it = 0; it < PSC_BISECT_CAP; ++it) {
            x = 0.5 * lo + 0.5 * hi;
            if (x == lo || x == hi) break;
            if (psc_cdf(x, mu, rs, rs0, K, red) < p) lo = x; else hi = x;
        }
    }
    if (threadIdx.x == 0) a.quant[blockIdx.x] = x;
}

inline unsigned psc_blocks(long long n) { return (unsigned)((n + PSC_TILE - 1) / PSC_TILE); }

}  // namespace

void launch_score_stage_points(hipStream_t stream, const ScoreArgs &a, const double *x, int K2, long long stride_k1, long long stride_k2,
                               long long stride_t) {
    psc_stage_points_kernel<<<psc_blocks((long long)a.steps * a.K), PSC_TILE, 0, stream>>>(a, x, K2, stride_k1, stride_k2, stride_t);
}

void launch_score_stage_moments(hipStream_t stream, const ScoreArgs &a, const double *m, const double *S) {
    psc_stage_moments_kernel<<<psc_blocks((long long)a.steps * a.K), PSC_TILE, 0, stream>>>(a, m, S);
}

void launch_score_crps(hipStream_t stream, const ScoreArgs &a, int first, int count) {
    const int tiles = psc_tiles(a.K), pairs = (int)psc_pairs(a.K);
    if (a.equal_var) {
        psc_pair_kernel<true><<<(unsigned)count * pairs, PSC_TILE, 0, stream>>>(a, first, tiles, pairs);
        psc_crps_kernel<true><<<count, PSC_TILE, 0, stream>>>(a, first, pairs);
    } else {
        psc_pair_kernel<false><<<(unsigned)count * pairs, PSC_TILE, 0, stream>>>(a, first, tiles, pairs);
        psc_crps_kernel<false><<<count, PSC_TILE, 0, stream>>>(a, first, pairs);
    }
}

void launch_score_pit(hipStream_t stream, const ScoreArgs &a) { psc_pit_kernel<<<a.n_test * a.J, PSC_TILE, 0, stream>>>(a); }

void launch_score_quantiles(hipStream_t stream, const ScoreArgs &a) {
    psc_quantile_kernel<<<(unsigned)a.steps * a.J * a.Q, PSC_TILE, 0, stream>>>(a);
}

}  // namespace ffvd
