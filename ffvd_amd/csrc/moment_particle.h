// Device blocks shared by the particle units (moment_particle_records.hip, _fan, _smooth, _backsim, _adapted): the one copy of every
// expression that the units must form bit for bit alike -- a fan track equals the records filter over the cut record, an unobserved
// row of the adapted filter equals the bootstrap row, the backward simulation scans as the filter does.  Every function is inlined
// into its caller and runs in a workgroup of 256 threads; none has an atomic, every sum has an order fixed by N alone.  A new particle
// unit calls these and copies nothing ("The shared particle blocks").
#pragma once
#include "moment_step.h"

namespace ffvd {
namespace {

constexpr int PARTICLE_RED = MG_MAXD * (MG_MAXD + 1) / 2; // the widest reduction: the upper triangle of a covariance

// The reductions over the workgroup: wavefront butterflies into red[wave][k], then the four wavefronts in ascending order.
template <bool MAX>
__device__ __forceinline__ double wg_op(const double x, const double y) { return MAX ? fmax(x, y) : x + y; }

template <bool MAX, int K>
__device__ __forceinline__ void wg_partials(const double (&v)[K], double (*red)[PARTICLE_RED]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = v[k];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s = wg_op<MAX>(s, __shfl_xor(s, mm));
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ double wg_sum_of(const double (*red)[PARTICLE_RED], const int k) {
    return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}
__device__ __forceinline__ double wg_max_of(const double (*red)[PARTICLE_RED], const int k) {
    return fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]));
}

// v[k] <- the sum (the maximum) over the workgroup, the same in every thread
template <int K>
__device__ __forceinline__ void wg_sum(double (&v)[K], double (*red)[PARTICLE_RED]) {
    wg_partials<false>(v, red);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wg_sum_of(red, k);
}
template <int K>
__device__ __forceinline__ void wg_max(double (&v)[K], double (*red)[PARTICLE_RED]) {
    wg_partials<true>(v, red);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wg_max_of(red, k);
}
__device__ __forceinline__ double wg_max(const double v, double (*red)[PARTICLE_RED]) {
    double a[1] = {v};
    wg_max<1>(a, red);
    return a[0];
}

// out[k] <- sum / div (the maximum), in LDS: for a kernel whose passes between the reductions are register-bound, where the uniform
// results must not live in registers
template <int K>
__device__ __forceinline__ void wg_sum_lds(const double (&v)[K], double (*red)[PARTICLE_RED], double *out, const double div) {
    wg_partials<false>(v, red);
    if (threadIdx.x < K) out[threadIdx.x] = wg_sum_of(red, threadIdx.x) / div;
    __syncthreads();
}
template <int K>
__device__ __forceinline__ void wg_max_lds(const double (&v)[K], double (*red)[PARTICLE_RED], double *out) {
    wg_partials<true>(v, red);
    if (threadIdx.x < K) out[threadIdx.x] = wg_max_of(red, threadIdx.x);
    __syncthreads();
}

// (lo, hi) and (hi, lo) of matrix o of a stack S of D x D matrices store one value: by thread 64 + k, the keeper of entry
// k = (lo <= hi) of the upper triangle stored row by row
template <int D>
__device__ __forceinline__ void particle_store_sym(double *S, const size_t o, const int lo, const int hi, const double v) {
    S[o * D * D + lo * D + hi] = v;
    S[o * D * D + hi * D + lo] = v;
}

// The start of a track (group gq, record r; vg: the track of the call): Xn[i] = x0 + L0 xi0[i], L0 the unpivoted factor of S0 in LDS
// (a pivot <= 0 gives a zero column; no S0: x0)
template <int D>
__device__ __forceinline__ void particle_start(const MomentGroupArgs &a, const MomentParticleArgs &p, const int gq, const int r,
                                               const size_t vg, double *Xn, double (*Sg)[MG_MAXD], double (*Lm)[MG_MAXD]) {
    const int tid = threadIdx.x, N = p.N;
    if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[vg * D * D + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (tid < D) {
            double pv = Sg[j][j], s = Sg[tid][j];
            for (int k = 0; k < j; ++k) { pv -= Lm[j][k] * Lm[j][k]; s -= Lm[tid][k] * Lm[j][k]; }
            double e = 0.0;
            if (pv > 0.0 && tid >= j) {
                const double q = sqrt(pv);
                e = tid == j ? q : s / q;
            }
            Lm[tid][j] = e;
        }
        __syncthreads();
    }
    const double *xi = a.S0 ? p.xi0 + (size_t)gq * p.xi0_g + (size_t)r * p.xi0_r : nullptr;
    for (int i = tid; i < N; i += 256) {
        double z[D];
#pragma unroll
        for (int c = 0; c < D; ++c) z[c] = xi ? xi[(size_t)i * D + c] : 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c <= q; ++c) s += Lm[q][c] * z[c];
            Xn[(size_t)i * D + q] = a.x_last[vg * D + q] + s;
        }
    }
}

// The transition of particle i (row `row + i` of the K blocks of group gq) in dim d, from what the rows and the product launches
// left: tmean = X + pmean, tvar = (var - qf) + Q with qf the column-tile partials in ascending tile order.  The bootstrap draw is
// tmean + eps * sqrt(tvar), formed by the caller.
template <int D>
__device__ __forceinline__ void particle_transition(const MomentLinearFanArgs &l, const int gq, const int d, const int row, const int i,
                                                    const int N, const double *X, const double *pm, const double &var, const double &Q,
                                                    double &tmean, double &tvar) {
    const double *vp = l.vpart + (size_t)(l.shared ? d : gq * D + d) * l.ntj * l.Tp + row + i;
    double qf = 0.0;
    for (int tj = 0; tj < l.ntj; ++tj) qf += vp[(size_t)tj * l.Tp];
    tmean = X[(size_t)i * D + d] + pm[(size_t)d * N + i];
    tvar = (var - qf) + Q;
}

// The emission and the row y of Y into LDS (threads < J * D; lcs: the constant of the log-density); below it the variance and the
// process noise of the track's model and group (threads < D).  The caller synchronises after them.
template <int D>
__device__ __forceinline__ void particle_stage_emission(const MomentFilterArgs &f, const double *y, double (*hs)[MG_MAXD], double *dds,
                                                        double *s2s, double *ys, double *lcs) {
    const int tid = threadIdx.x, J = f.J;
    if (tid < J * D) hs[tid / D][tid % D] = f.CC[(size_t)(tid % D) * J + tid / D];
    if (tid < J) {
        const double s2 = f.sd[tid] * f.sd[tid];
        dds[tid] = f.DD[tid];
        s2s[tid] = s2;
        lcs[tid] = -0.5 * (LOG_2PI + log(s2));
        ys[tid] = y[tid];
    }
}
template <int D>
__device__ __forceinline__ void particle_stage_noise(const MomentGroupArgs &a, const int model, const int gq, double *vard, double *Qd) {
    const int tid = threadIdx.x;
    if (tid < D) {
        vard[tid] = a.variance[(size_t)model * D + tid];
        Qd[tid] = exp(a.log_Q[(size_t)gq * D + tid]);
    }
}
// whether the staged row observes anything (NaN = unobserved); the same in every thread
__device__ __forceinline__ bool particle_any_observed(const double *ys, const int J) {
    bool any = false;
    for (int j = 0; j < J; ++j) any = any || ys[j] == ys[j];
    return any;
}
// log N(y_j; CC[:, j] . x + DD_j, sd_j^2) of one particle and one observed output j
template <int D>
__device__ __forceinline__ double particle_emit_logpdf(const int j, const double (&x)[D], const double (*hs)[MG_MAXD], const double *dds,
                                                       const double *s2s, const double *ys, const double *lcs) {
    double hm = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) hm += hs[j][d] * x[d];
    const double e = (ys[j] - hm) - dds[j];
    return lcs[j] - 0.5 * e * e / s2s[j];
}

// dst[k] <- src[0] + .. + src[k], k < N (src == dst allowed): thread c sums its chunk of PT consecutive entries, the chunk totals are
// scanned by wavefront, then across the four.  Synchronises before, and after: what every thread wrote before the call is visible.
__device__ __forceinline__ void particle_scan(const double *src, double *dst, const int N, double *wtot) {
    const int tid = threadIdx.x, PT = (N + 255) / 256, c0 = tid * PT;
    __syncthreads();
    double run = 0.0;
    for (int k = 0; k < PT; ++k)
        if (c0 + k < N) {
            run += src[c0 + k];
            dst[c0 + k] = run;
        }
    const int lane = tid & 63, wave = tid >> 6;
    double inc = run;
#pragma unroll
    for (int mm = 1; mm < 64; mm <<= 1) {
        const double up = __shfl_up(inc, mm);
        if (lane >= mm) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    double base = inc - run;                                      // the chunks before this one in its wavefront
    for (int w = 0; w < wave; ++w) base += wtot[w];
    for (int k = 0; k < PT; ++k)
        if (c0 + k < N) dst[c0 + k] += base;
    __syncthreads();
}

// an index into [0, N), whatever it held: before any address is formed from a computed or a stored index
__device__ __forceinline__ int particle_clamp(const int k, const int N) { return k < 0 ? 0 : k > N - 1 ? N - 1 : k; }

// min(#{k: cdf_k <= u}, N - 1): at most 12 rounds over integer bounds, whatever the values are; the result is clamped here
__device__ __forceinline__ int particle_search(const double *cdf, const int N, const double u) {
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid + 1;
        else hi = mid;
    }
    return particle_clamp(lo, N);
}

// The rows kernel of workgroup (slab sl of MG_PREC_SLAB particles, dim d) of a track of group gq: thread = column j, one row of Z
// against the particles of the slab.  crow: the track's control row; X: its state [N][D]; the kernel rows go to rows row0 + i of
// the unit's K block (zero beyond M), their means to pm[i].
template <int D>
__device__ __forceinline__ void particle_rows_body(const MomentGroupArgs &a, const MomentLinearFanArgs &l, const int N, const int sl,
                                                   const int d, const int gq, const double *crow, const double *X, double *pm,
                                                   const int row0) {
    constexpr int NQ = MG_PREC_SLAB;
    __shared__ double xp[NQ][MG_MAXD], xc[MAXP], il[MAXP], red[4][NQ];
    const int tid = threadIdx.x;
    const int P = a.P, M = a.M, Mp = a.Mp;
    const int model = a.n_models == 1 ? 0 : gq;
    const int i0 = sl * NQ, ni = N - i0 < NQ ? N - i0 : NQ;
    const double *lend = a.len + ((size_t)model * D + d) * P;
    if (tid < NQ * D) {
        const int i = tid / D, q = tid % D;
        xp[i][q] = i < ni ? X[(size_t)(i0 + i) * D + q] : 0.0;
    }
    if (tid >= 128 && tid < 128 + P) {
        const int q = tid - 128;
        xc[q] = q < D ? 0.0 : crow[q - D];
        il[q] = 1.0 / lend[q];
    }
    __syncthreads();

    const double *Zm = a.Z + (size_t)model * M * P;
    const double *bed = a.beta + ((size_t)gq * D + d) * Mp;
    const double var = a.variance[(size_t)model * D + d];
    double *Kr = l.K + ((size_t)(l.shared ? d : gq * D + d) * l.Tp + row0 + i0) * Mp;
    double acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
    for (int j = tid; j < Mp; j += 256) {
        const bool live = j < M;
        const double *z = Zm + (size_t)(live ? j : 0) * P;        // (a padding column reads row 0 and writes zeros)
        double zs[D], cc = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) zs[q] = z[q];
        for (int q = D; q < P; ++q) {
            const double u = (z[q] - xc[q]) * il[q];
            cc += u * u;
        }
        const double be = live ? bed[j] : 0.0, vk = live ? var : 0.0;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            if (i < ni) {
                double c = 0.0;
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    const double u = (zs[q] - xp[i][q]) * il[q];
                    c += u * u;
                }
                const double k = vk * exp(-0.5 * (c + cc));
                acc[i] += k * be;
                Kr[(size_t)i * Mp + j] = k;
            }
            __builtin_amdgcn_sched_barrier(0);                    // one particle at a time: interleaved exps cost registers
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        double s = acc[i];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s += __shfl_xor(s, mm);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (tid < ni) pm[i0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// log f without its constant.  Every rounding is spelled out (one subtraction, one product and one fused multiply-add per dim), so
// that the normaliser and the backward kernel form the same bits for the same pair and every exponent of the latter is <= 0.
template <int D, class TX, class TM, class TI>
__device__ __forceinline__ double psm_logf(const TX &x, const TM &mu, const TI &is, const double ls) {
    double q = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double u = x[d] - mu[d];
        q = __builtin_fma(u * u, is[d], q);
    }
    return -0.5 * (q + ls);
}

}  // namespace
}  // namespace ffvd
