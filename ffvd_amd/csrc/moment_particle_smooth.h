// Device helpers shared by the particle smoother (moment_particle_smooth.hip) and the particle backward simulation
// (moment_particle_backsim.hip): the workgroup reductions of 256 threads and the transition log-density without its constant.  Every
// function is inlined into its caller; the two units form the same bits for the same operands.
#pragma once
#include "moment_step.h"

namespace ffvd {
namespace {

constexpr int PSM_RED = MG_MAXD * (MG_MAXD + 1) / 2;      // the widest reduction: the upper triangle of a covariance

// v[k] <- the sum over the workgroup, the same in every thread: wavefront butterflies, then the four wavefronts in ascending order
// (the shape of the weight kernel's sums)
template <int K>
__device__ __forceinline__ void psm_sum(double (&v)[K], double (*red)[PSM_RED]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = v[k];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s += __shfl_xor(s, mm);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

__device__ __forceinline__ double psm_max(double v, double (*red)[PSM_RED]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int mm = 32; mm > 0; mm >>= 1) v = fmax(v, __shfl_xor(v, mm));
    if (lane == 0) red[wave][0] = v;
    __syncthreads();
    return fmax(fmax(red[0][0], red[1][0]), fmax(red[2][0], red[3][0]));
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
