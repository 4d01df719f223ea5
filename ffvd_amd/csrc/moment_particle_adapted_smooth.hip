// Particle smoothing and backward simulation on the sets of the fully adapted particle filter ("Adapted particle
// smoothing").  The adapted filter of moment_particle_adapted.hip stores particles[t] = P_t, the EQUALLY WEIGHTED filtered set after
// row t, and the keep launch of moment_particle_smooth.hip after the product launch of step t stores mu_t = trans_mean[t] and
// s_t = trans_var[t], the transition moments of the set carried into row t: of P_{t-1} for t >= 1 (row 0 belongs to the start set and
// is not read here).  So p(P_{t+1,j} | P_{t,i}) = N(P_{t+1,j}; mu_{t+1,i}, diag s_{t+1,i}), particle i of row t IS carried particle i of
// row t + 1, and the recursions of the bootstrap units lose their fold through the ancestors and their emission weights:
//   marginal smoother, a track of n rows:  w_smooth[n-1, i] = 1 / N;  for t = n-2 .. 0, with x_j = P_{t+1,j}, mu_i = mu_{t+1,i}, s_i = s_{t+1,i}:
//     log f_ij by psm_logf,  c_j = max_i log f_ij + log sum_i exp(log f_ij - max)   (mg_psm_norm_kernel, unchanged),
//     w_smooth[t, i] = sum_j w_smooth[t+1, j] exp(log f_ij - c_j)                   (j ascending; every exponent is <= 0)
//   backward simulation, trajectory b with u = unif[t, b]:  k_{n-1} = min(#{k: k + 1 <= u N}, N - 1), formed by the filter's scan and
//     search on unit weights;  for t = n-2 .. 0, with x = P_{t+1, k_{t+1}}:  p_i = exp(log f_i - max_i log f_i), the filter's scan and
//     search, k_t = the searched index itself.
// Nothing is renormalised and no GP is evaluated.
//
// Kernels (256 threads each; D is a template parameter, 1 .. MG_MAXD):
//   mg_pasm_back_kernel  one launch per row t = n_max - 1 .. 0 for all tracks, workgroup = (track, slab of 256 particles i): the body of
//                        mg_psm_back_kernel (thread = i with mu_i, 1 / s_i in registers, (x_j, c_j, w_smooth[t+1, j]) staged through
//                        LDS in chunks of 256 j, a column of weight exactly 0 skipped) storing w_smooth[t] itself; the launch of a
//                        track's last row t = n - 1 fills it with 1 / N and the rows >= n with NaN;
//   mg_pabs_kernel       ONE launch, workgroup = (track, trajectory), walking t = n - 1 .. 0: mg_pbs_kernel with unit weights in the
//                        last row and without the ancestor read; the searched index is clamped into [0, N) before the gather.
// The normalisers, the moments, 1 / s and sum log s, and the moments over the trajectories are the kernels of
// moment_particle_smooth.hip and moment_particle_backsim.hip through their launchers.  No atomics, vector stores only, nothing waits on
// another workgroup, every sum has an order fixed by N alone.  The one address that depends on computed values is the gather's.
#include "moment_particle.h"

namespace ffvd {
namespace {

constexpr int PASM_CHUNK = 256;                           // rows of a staged chunk: (D + 2) * 2 KiB of LDS, 20 KiB at D = 8

template <class Q>
__device__ __forceinline__ int pasm_len(const Q &q, int v) {
    const int n = q.lens ? q.lens[v % q.R] : q.steps;
    return n < 1 ? 1 : n > q.steps ? q.steps : n;
}

// Row t.  Workgroup = (track, slab of 256 particles i of row t = carried particles of row u = t + 1)
template <int D>
__global__ __launch_bounds__(256) void mg_pasm_back_kernel(MomentParticleSmoothArgs q, const int t) {
    __shared__ double xs[PASM_CHUNK][D], cs[PASM_CHUNK], ws[PASM_CHUNK];
    const int tid = threadIdx.x, N = q.N, steps = q.steps, u = t + 1;
    const int nsl = (N + 255) / 256;
    const int slab = blockIdx.x % nsl, v = blockIdx.x / nsl, n = pasm_len(q, v);
    if (n <= t) return;                                           // (the track's own last-row launch has filled row t)
    const int i = slab * 256 + tid, ic = i < N ? i : N - 1;
    if (n == u) {                                                 // the last row: uniform; NaN at and beyond the length
        if (i >= N) return;
        const double nan = __builtin_nan("");
        q.w_smooth[((size_t)v * steps + t) * N + i] = 1.0 / (double)N;
        for (int tt = n; tt < steps; ++tt) q.w_smooth[((size_t)v * steps + tt) * N + i] = nan;
        return;
    }
    const size_t o = ((size_t)v * steps + u) * N;
    double mu[D], is[D], ls = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double s = q.trans_var[(o + ic) * D + d];
        mu[d] = q.trans_mean[(o + ic) * D + d];
        is[d] = 1.0 / s;
        ls += log(s);
    }
    double acc = 0.0;
    for (int j0 = 0; j0 < N; j0 += PASM_CHUNK) {
        const int nj = N - j0 < PASM_CHUNK ? N - j0 : PASM_CHUNK;
        __syncthreads();
        if (tid < nj) {
#pragma unroll
            for (int d = 0; d < D; ++d) xs[tid][d] = q.particles[(o + j0 + tid) * D + d];
            cs[tid] = q.cnorm[o + j0 + tid];
            ws[tid] = q.w_smooth[o + j0 + tid];
        }
        __syncthreads();
        for (int j = 0; j < nj; ++j) {
            const double w = ws[j];
            if (w != 0.0) acc = __builtin_fma(w, exp(psm_logf<D>(xs[j], mu, is, ls) - cs[j]), acc);
        }
    }
    if (i < N) q.w_smooth[((size_t)v * steps + t) * N + i] = acc;
}

// Workgroup = (track, trajectory); q.ancestors and q.weights are not read
template <int D>
__global__ __launch_bounds__(256) void mg_pabs_kernel(MomentParticleBacksimArgs q) {
    __shared__ double pl[MG_PREC_MAXN], red[4][PARTICLE_RED], wtot[4];
    const int tid = threadIdx.x, N = q.N, steps = q.steps, B = q.B;
    const int b = blockIdx.x % B, v = blockIdx.x / B, n = pasm_len(q, v);
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
            for (int i = tid; i < N; i += 256) pl[i] = 1.0;       // the filtered set is equally weighted
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
        // every thread runs the same search on the same words; the result is in [0, N) whatever they hold
        const int k = particle_clamp(particle_search(pl, N, U[(size_t)t * B + b] * pl[N - 1]), N);
        const double *X = q.particles + ((vrow + t) * N + k) * D;
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = X[d];
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (tid == d) out[(size_t)t * D + d] = x[d];
        if (tid == 64) q.traj_index[(vrow + t) * B + b] = k;
    }
}

}  // namespace

// After the filter's last pass (with the keep launch after every product launch): the normalisers of all rows, the rows
// n_max - 1 .. 0 (one launch each), the moments.  n_max: the longest record of the call (<= q.steps).  q.ancestors, q.weights and
// q.omega are not read.
void launch_mg_pasm_smooth(hipStream_t stream, const MomentParticleSmoothArgs &q, int n_max) {
    const dim3 slabs((unsigned)((size_t)q.V * ((q.N + 255) / 256)));
    launch_mg_psm_norm(stream, q, n_max);
    MG_DISPATCH_D(q.D, {
        for (int t = n_max - 1; t >= 0; --t) hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pasm_back_kernel<d>), slabs, dim3(256), 0, stream, q, t);
    })
    launch_mg_psm_moments(stream, q);
}

// After the filter's last pass: 1 / s and sum log s of every row, the backward recursion of every (track, trajectory), then the
// moments of every (track, row).  b.ancestors and b.weights are not read.
void launch_mg_pabs(hipStream_t stream, const MomentParticleBacksimArgs &b) {
    const dim3 trajs((unsigned)((size_t)b.V * b.B));
    launch_mg_pbs_prep(stream, b);
    MG_DISPATCH_D(b.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pabs_kernel<d>), trajs, dim3(256), 0, stream, b))
    launch_mg_pbs_moments(stream, b);
}

}  // namespace ffvd
