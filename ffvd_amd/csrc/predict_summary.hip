// Rollout summaries: predictive mean, the reference's variance, the total variance over the rollouts and the held-out predictive
// log density (base_model.py:330-348 and what it lacks) as a streaming reduction over the rollouts.  predict_summary.h has the
// quantities and the shape of the two launches.
//
// Reading.  A rollout's steps * D doubles are contiguous; lane l of a wavefront takes step 64 tile + l, D contiguous doubles (16-byte
// loads when D is even: every row then starts on a 16-byte boundary), so one wavefront reads one contiguous block of 64 D doubles
// per rollout and stack.  CC, CC^2, DD and 1 / s sit in LDS (every lane reads the same word: a broadcast), the lane's Y_test row in
// registers.  Both stacks are read exactly once.
// Arithmetic.  Everything that is summed over rollouts is carried per lane and output in registers (J is a template parameter, so
// no array is indexed at run time): the mean and the centred sum of squares of p by Welford's update, sum v CC^2 as a plain sum,
// and log-sum-exp as (largest exponent m, sum of exp(e - m)) -- the sum never sees an exponent above 0, so a held-out point that is
// 40 noise standard deviations from every rollout still has a finite density.
// Merging.  Chunk c holds rollouts [32 c, 32 c + 32); ps_merge_kernel walks c upwards with the pairwise formulas
//   mean = mean_a + delta n_b / n,  M2 = M2_a + M2_b + delta^2 n_a n_b / n  (delta = mean_b - mean_a),
//   m = max(m_a, m_b),  s = s_a exp(m_a - m) + s_b exp(m_b - m).
// A NaN state (f_var + Q <= 0 in a rollout) makes the outputs of the steps it reaches NaN; no address depends on a value.
#include "predict_summary.h"
#include "kernels.h"

#include <cmath>

namespace ffvd {

namespace {
constexpr double LOG_2PI = 1.8378770664093454835606594728112;

template <int J>
__global__ __launch_bounds__(64 * PS_WAVES) void ps_partial_kernel(PredictSummaryArgs a, int ntiles) {
    __shared__ double cc[MAXP * J], cc2[MAXP * J], dd[J], isd[J];
    const int tid = threadIdx.x, N = a.N, steps = a.steps, D = a.D;
    if (tid < D * J) {
        const double c = a.CC[tid];
        cc[tid] = c;
        cc2[tid] = c * c;
    }
    if (tid < J) {
        dd[tid] = a.DD[tid];
        isd[tid] = 1.0 / a.sd[tid];
    }
    __syncthreads();
    const int tile = blockIdx.x % ntiles, lane = tid & 63, wave = tid >> 6;
    const size_t chunk = (size_t)(blockIdx.x / ntiles) * PS_WAVES + wave, n0 = chunk * PS_CHUNK;
    const int t = tile * PS_TILE + lane;
    if (n0 >= (size_t)N || t >= steps) return;
    const int nn = ((size_t)N - n0 < (size_t)PS_CHUNK) ? (int)((size_t)N - n0) : PS_CHUNK;
    const bool dens = t < a.n_test;

    double yc[J], mean[J], m2[J], sv[J], mx[J], se[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        yc[j] = dens ? a.Y[(size_t)t * J + j] - dd[j] : 0.0;
        mean[j] = m2[j] = sv[j] = se[j] = 0.0;
        mx[j] = -INFINITY;
    }
    const bool vec = (D & 1) == 0;
    for (int i = 0; i < nn; ++i) {
        const size_t row = ((n0 + i) * (size_t)steps + t) * D;
        const double *xr = a.x + row, *vr = a.v + row;
        double p[J], q[J];
#pragma unroll
        for (int j = 0; j < J; ++j) p[j] = q[j] = 0.0;
        if (vec) {
            for (int k = 0; k < D; k += 2) {
                const double2 xv = *reinterpret_cast<const double2 *>(xr + k), vv = *reinterpret_cast<const double2 *>(vr + k);
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    p[j] += xv.x * cc[k * J + j];
                    q[j] += vv.x * cc2[k * J + j];
                }
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    p[j] += xv.y * cc[(k + 1) * J + j];
                    q[j] += vv.y * cc2[(k + 1) * J + j];
                }
            }
        } else {
            for (int k = 0; k < D; ++k) {
                const double xv = xr[k], vv = vr[k];
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    p[j] += xv * cc[k * J + j];
                    q[j] += vv * cc2[k * J + j];
                }
            }
        }
        const double cnt = (double)(i + 1);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const double delta = p[j] - mean[j];
            mean[j] += delta / cnt;
            m2[j] += delta * (p[j] - mean[j]);
            sv[j] += q[j];
        }
        if (dens) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double z = (yc[j] - p[j]) * isd[j], e = -0.5 * z * z;
                if (!(e == -INFINITY)) {                      // (an exponent of -inf adds an exact zero; NaN goes through)
                    const double d = e - mx[j], w = exp(-fabs(d));
                    if (d > 0.0) { se[j] = se[j] * w + 1.0; mx[j] = e; }
                    else se[j] += w;
                }
            }
        }
    }
    const size_t SJ = (size_t)steps * J;
    double *o = a.part + chunk * PS_FIELDS * SJ + (size_t)t * J;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        o[j] = mean[j];
        o[SJ + j] = m2[j];
        o[2 * SJ + j] = sv[j];
        o[3 * SJ + j] = mx[j];
        o[4 * SJ + j] = se[j];
    }
}

__global__ __launch_bounds__(256) void ps_merge_kernel(PredictSummaryArgs a) {
    const size_t SJ = (size_t)a.steps * a.J, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= SJ) return;
    const int J = a.J, N = a.N, t = (int)(e / J), j = (int)(e % J);
    const bool dens = t < a.n_test;
    const size_t chunks = ps_chunks(N);
    double cnt = 0.0, mean = 0.0, m2 = 0.0, sv = 0.0, mx = -INFINITY, se = 0.0;
    for (size_t c = 0; c < chunks; ++c) {
        const double *q = a.part + c * PS_FIELDS * SJ + e;
        const size_t left = (size_t)N - c * PS_CHUNK;
        const double nb = (double)(left < (size_t)PS_CHUNK ? left : (size_t)PS_CHUNK), n = cnt + nb;
        const double delta = q[0] - mean;
        mean += delta * (nb / n);
        m2 = (m2 + q[SJ]) + delta * delta * (cnt * nb / n);
        cnt = n;
        sv += q[2 * SJ];
        if (dens) {
            const double mb = q[3 * SJ], sb = q[4 * SJ];
            if (!(mb == -INFINITY)) {                         // (a chunk whose exponents were all -inf adds nothing)
                const double d = mb - mx, w = exp(-fabs(d));
                if (d > 0.0) { se = se * w + sb; mx = mb; }
                else se += sb * w;
            }
        }
    }
    const double sd = a.sd[j], s2 = sd * sd, ym = mean + a.DD[j], vt = s2 + m2 / cnt;
    a.out[e] = ym;
    a.out[SJ + e] = sv / cnt + s2;
    a.out[2 * SJ + e] = vt;
    if (dens) {
        const double y = a.Y[e], r = y - ym;
        a.out[3 * SJ + e] = ((mx + log(se)) - log(cnt)) - (log(sd) + 0.5 * LOG_2PI);
        a.out[4 * SJ + e] = -0.5 * (LOG_2PI + log(vt)) - 0.5 * r * r / vt;
    }
}
}  // namespace

void launch_predict_summary(hipStream_t stream, const PredictSummaryArgs &a) {
    const int ntiles = (a.steps + PS_TILE - 1) / PS_TILE;
    const size_t groups = (ps_chunks(a.N) + PS_WAVES - 1) / PS_WAVES;
    const dim3 grid((unsigned)(groups * ntiles)), block(64 * PS_WAVES);
    switch (a.J) {
#define PS_CASE(j) case j: hipLaunchKernelGGL(ps_partial_kernel<j>, grid, block, 0, stream, a, ntiles); break;
        PS_CASE(1) PS_CASE(2) PS_CASE(3) PS_CASE(4) PS_CASE(5) PS_CASE(6) PS_CASE(7) PS_CASE(8)
#undef PS_CASE
        default: return;
    }
    const size_t SJ = (size_t)a.steps * a.J;
    hipLaunchKernelGGL(ps_merge_kernel, dim3((unsigned)((SJ + 255) / 256)), dim3(256), 0, stream, a);
}

}  // namespace ffvd
