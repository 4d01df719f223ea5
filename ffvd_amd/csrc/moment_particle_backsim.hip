// Particle backward simulation of many observed records ("Particle backward simulation"): joint smoothed
// trajectories by forward filtering / backward simulation (Godsill, Doucet & West 2004) on the equally weighted sets the particle
// filter of moment_particle_records.hip carries.  Notation of moment_particle_smooth.hip: a track of n rows, mu_t = trans_mean[t],
// s_t = trans_var[t], X^-_t = particles[t], W_t = weights[t], a_t = ancestors[t].  Trajectory b is a sequence of indices k_t into X^-_t,
// drawn with the caller's uniforms u = unif[t, b]:
//   row n-1:        cdf = the running sum of W_{n-1}, tot = cdf[N-1];  k_{n-1} = min(#{k: cdf_k <= u tot}, N - 1)
//   t = n-2 .. 0:   with x = X^-_{t+1, k_{t+1}}:  log f_i = -1/2 (sum_d (x_d - mu_{t+1,id})^2 / s_{t+1,id} + sum_d log s_{t+1,id})
//                   (psm_logf, the smoother's roundings),  p_i = exp(log f_i - max_i log f_i),  cdf = the running sum of p,
//                   i* = min(#{i: cdf_i <= u tot}, N - 1),  k_t = a_t[i*]
// The maximal term is exactly 1, so tot >= 1 and nothing divides by a sum that can vanish.  Conditional on the filter's run,
// P(k_t = k) = w_smooth[t, k] of the marginal smoother.
//
// Kernels (256 threads each; D is a template parameter, 1 .. MG_MAXD):
//   mg_pbs_prep_kernel     one launch, thread = (track, row 1 .. n - 1, particle): 1 / s and sum_d log s_d by the expressions of the
//                          smoother's kernels, once, so that the B trajectories of a track do not each take D logarithms and D
//                          divisions per particle and row (the bits are the same);
//   mg_pbs_kernel          ONE launch, workgroup = (track, trajectory), walking t = n - 1 .. 0: log f of every carried particle into LDS
//                          (thread = particle, stride 256), the workgroup maximum, p in place, the filter's scan in place and its
//                          search (particle_scan, particle_search of moment_particle.h), run by every thread on the same LDS words;
//                          the index is clamped into [0, N) before the ancestor is read and the ancestor again before the gather;
//   mg_pbs_moments_kernel  one launch, workgroup = (track, row), striding over the trajectories: their mean, centred covariance
//                          (divisor B, mirrored) and the lag-one covariance with row t + 1, centred on the two rows' own means.
// No atomics, nothing waits on another workgroup, every sum has an order fixed by N (by B in the moments) alone.
#include "moment_particle.h"

namespace ffvd {
namespace {

__device__ __forceinline__ int pbs_len(const MomentParticleBacksimArgs &q, int v) {
    const int n = q.lens ? q.lens[v % q.R] : q.steps;
    return n < 1 ? 1 : n > q.steps ? q.steps : n;
}

// Workgroup = (track, row, slab of 256 particles); rows 0 and >= n are not read by the recursion and are left alone
template <int D>
__global__ __launch_bounds__(256) void mg_pbs_prep_kernel(MomentParticleBacksimArgs q) {
    const int N = q.N, steps = q.steps, nsl = (N + 255) / 256;
    const int slab = blockIdx.x % nsl, vt = blockIdx.x / nsl, t = vt % steps, v = vt / steps;
    const int i = slab * 256 + threadIdx.x;
    if (t == 0 || t >= pbs_len(q, v) || i >= N) return;
    const size_t o = (size_t)vt * N + i;
    double ls = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double s = q.trans_var[o * D + d];
        q.inv_var[o * D + d] = 1.0 / s;
        ls += log(s);
    }
    q.log_var[o] = ls;
}

// Workgroup = (track, trajectory)
template <int D>
__global__ __launch_bounds__(256) void mg_pbs_kernel(MomentParticleBacksimArgs q) {
    __shared__ double pl[MG_PREC_MAXN], red[4][PARTICLE_RED], wtot[4];
    const int tid = threadIdx.x, N = q.N, steps = q.steps, B = q.B;
    const int b = blockIdx.x % B, v = blockIdx.x / B, n = pbs_len(q, v);
    const size_t vrow = (size_t)v * steps;
    const double *U = q.unif + (size_t)(v / q.R) * q.unif_g + (size_t)(v % q.R) * q.unif_r;
    double *out = q.trajectories + ((size_t)v * B + b) * steps * D;
    const double nan = __builtin_nan("");
    for (int e = n * D + tid; e < steps * D; e += 256) out[e] = nan;
    for (int t = n + tid; t < steps; t += 256) q.traj_index[(vrow + t) * B + b] = -1;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = 0.0;
    for (int t = n - 1; t >= 0; --t) {
        __syncthreads();                                          // the search of the row above has read pl
        if (t == n - 1) {
            const double *W = q.weights + (vrow + t) * N;
            for (int i = tid; i < N; i += 256) pl[i] = W[i];
        } else {
            const size_t o = (vrow + t + 1) * N;
            double mx = -__builtin_inf();
            for (int i = tid; i < N; i += 256) {
                double mu[D], is[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    mu[d] = q.trans_mean[(o + i) * D + d];
                    is[d] = q.inv_var[(o + i) * D + d];
                }
                const double lf = psm_logf<D>(x, mu, is, q.log_var[o + i]);
                mx = fmax(mx, lf);
                pl[i] = lf;
            }
            mx = wg_max(mx, red);
            for (int i = tid; i < N; i += 256) pl[i] = exp(pl[i] - mx);          // (this thread's own entries)
        }
        particle_scan(pl, pl, N, wtot);
        // every thread runs the same search on the same words
        int k = particle_search(pl, N, U[(size_t)t * B + b] * pl[N - 1]);
        if (t < n - 1) k = particle_clamp(q.ancestors[(vrow + t) * N + k], N);   // in [0, N) whatever the stack holds
        const double *X = q.particles + ((vrow + t) * N + k) * D;
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = X[d];
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (tid == d) out[(size_t)t * D + d] = x[d];
        if (tid == 64) q.traj_index[(vrow + t) * B + b] = k;
    }
}

// Workgroup = (track, row) of the call
template <int D>
__global__ __launch_bounds__(256) void mg_pbs_moments_kernel(MomentParticleBacksimArgs q) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double red[4][PARTICLE_RED];
    const int tid = threadIdx.x, steps = q.steps, B = q.B;
    const int t = blockIdx.x % steps, v = blockIdx.x / steps, n = pbs_len(q, v);
    const size_t row = blockIdx.x;
    const double nan = __builtin_nan("");
    if (t >= n) {
        if (tid < D) q.m_traj[row * D + tid] = nan;
        if (tid < D * D) q.S_traj[row * D * D + tid] = nan;
        if (tid >= 64 && tid < 64 + D * D) q.lag_cov[row * D * D + tid - 64] = nan;
        return;
    }
    const bool lag = t + 1 < n;                                   // (the same in every thread)
    const size_t stride = (size_t)steps * D;
    const double *X = q.trajectories + (size_t)v * B * stride + (size_t)t * D, *Xn = X + (lag ? D : 0);
    double m0[D], m1[D];
#pragma unroll
    for (int d = 0; d < D; ++d) m0[d] = m1[d] = 0.0;
    for (int b = tid; b < B; b += 256)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            m0[d] += X[b * stride + d];
            m1[d] += Xn[b * stride + d];
        }
    wg_sum<D>(m0, red);
    wg_sum<D>(m1, red);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        m0[d] /= B;
        m1[d] /= B;
    }
    double sf[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sf[k] = 0.0;
    for (int b = tid; b < B; b += 256) {
        double dx[D];
#pragma unroll
        for (int d = 0; d < D; ++d) dx[d] = X[b * stride + d] - m0[d];
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) sf[k++] += dx[lo] * dx[hi];
    }
    wg_sum<NP>(sf, red);
    // every thread holds every sum, thread k stores entry k
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (tid == d) q.m_traj[row * D + d] = m0[d];
    int k = 0;
#pragma unroll
    for (int lo = 0; lo < D; ++lo)
#pragma unroll
        for (int hi = lo; hi < D; ++hi) {
            if (tid == 64 + k) particle_store_sym<D>(q.S_traj, row, lo, hi, sf[k] / B);
            ++k;
        }
    // the lag-one covariance, one row of it (component d of x_t) at a time
#pragma unroll
    for (int d = 0; d < D; ++d) {
        double lg[D];
#pragma unroll
        for (int e = 0; e < D; ++e) lg[e] = 0.0;
        for (int b = tid; b < B; b += 256) {
            const double dx = X[b * stride + d] - m0[d];
#pragma unroll
            for (int e = 0; e < D; ++e) lg[e] += dx * (Xn[b * stride + e] - m1[e]);
        }
        wg_sum<D>(lg, red);
#pragma unroll
        for (int e = 0; e < D; ++e)
            if (tid == 128 + e) q.lag_cov[row * D * D + d * D + e] = lag ? lg[e] / B : nan;
    }
}

}  // namespace

// After launch_mg_psm_weights: 1 / s and sum log s of every row, the backward recursion of every (track, trajectory), then the moments
// of every (track, row)
void launch_mg_pbs(hipStream_t stream, const MomentParticleBacksimArgs &b) {
    const dim3 trajs((unsigned)((size_t)b.V * b.B)), rows((unsigned)((size_t)b.V * b.steps));
    // V * steps * ceil(N / 256) <= V * steps * N, which the filter's own limit G * R * steps * N * D < 2^31 keeps inside grid x
    const dim3 slabs((unsigned)((size_t)b.V * b.steps * ((b.N + 255) / 256)));
    MG_DISPATCH_D(b.D, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pbs_prep_kernel<d>), slabs, dim3(256), 0, stream, b);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pbs_kernel<d>), trajs, dim3(256), 0, stream, b);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pbs_moments_kernel<d>), rows, dim3(256), 0, stream, b);
    })
}

// The first and the last of the three launches alone (host code only: the adapted backward simulation of
// moment_particle_adapted_smooth.hip brings a recursion kernel of its own between them)
void launch_mg_pbs_prep(hipStream_t stream, const MomentParticleBacksimArgs &b) {
    const dim3 slabs((unsigned)((size_t)b.V * b.steps * ((b.N + 255) / 256)));
    MG_DISPATCH_D(b.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pbs_prep_kernel<d>), slabs, dim3(256), 0, stream, b))
}
void launch_mg_pbs_moments(hipStream_t stream, const MomentParticleBacksimArgs &b) {
    const dim3 rows((unsigned)((size_t)b.V * b.steps));
    MG_DISPATCH_D(b.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pbs_moments_kernel<d>), rows, dim3(256), 0, stream, b))
}

}  // namespace ffvd
