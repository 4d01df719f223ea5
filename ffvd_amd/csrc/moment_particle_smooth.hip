// Particle smoothing of many observed records ("Particle smoothing"): the marginal forward-filter /
// backward-smoother (Doucet, Godsill & Andrieu 2000) on the equally weighted sets the particle filter of moment_particle_records.hip
// carries.  Row t of a track of n rows: the filter holds the carried set X_t, forms mu_t = X_t + m(X_t, c_t) (the transition mean) and
// s_t = v(X_t, c_t) + Q (the transition variance), X^-_t = mu_t + eps[t] sqrt(s_t), weights it with W_t and carries X_{t+1} = X^-_t[a_t].
// The smoothing weights live on the stored X^-_t:
//   w_smooth[n-1] = W_{n-1} / sum W_{n-1};  for t = n-2 .. 0, with x_j = X^-_{t+1,j}, mu_i = trans_mean[t+1, i], s_i = trans_var[t+1, i]:
//   log f_ij = -1/2 (sum_d (x_jd - mu_id)^2 / s_id + sum_d log s_id)                   (the constant cancels)
//   c_j = max_i log f_ij + log sum_i exp(log f_ij - max)                               (i ascending)
//   omega_i = sum_j w_smooth[t+1, j] exp(log f_ij - c_j)                               (j ascending; every exponent is <= 0)
//   w_smooth[t, k] = sum_{i: a_t[i] = k} omega_i                                       (i ascending; no offspring: exactly 0)
//   m_smooth, S_smooth: the w-weighted mean and centred covariance of X^-_t;  ess_smooth = (sum w)^2 / sum w^2.
// Nothing is renormalised inside the recursion and no GP is evaluated: (mu, s) are what the filter's launches computed.
//
// Kernels (256 threads each; D is a template parameter, 1 .. MG_MAXD):
//   mg_psm_keep_kernel     per step and pass, between the product launch of step s and the weight launch that finishes it: thread =
//                          particle; the two parenthesised sub-expressions of the weight kernel's X^-, bit for bit, into trans_mean[s]
//                          and trans_var[s] (the state of parity s, pmean, the column-tile partials in ascending tile order);
//   mg_psm_weights_kernel  one launch, workgroup = (track, row): W_t from the stored X^- and Y by the weight kernel's expressions, and
//                          the normalised last row of the track into w_smooth; NaN at and beyond the record's length;
//   mg_psm_norm_kernel     one launch for all rows (c does not depend on the weights), workgroup = (track, row t <= n - 2, slab of 256
//                          columns j): thread = column with x_j in registers, (mu_i, 1 / s_i, sum_d log s_id) staged through LDS in chunks
//                          of 256 i; two sweeps in ascending i (the maximum without exponentials, then the sum): one exp per pair;
//   mg_psm_back_kernel     one launch per row t = n_max - 2 .. 0 for all tracks, workgroup = (track, slab of 256 carried particles i):
//                          thread = i with mu_i, 1 / s_i in registers, (x_j, c_j, w_smooth[t+1, j]) staged through LDS in chunks of 256 j;
//                          a column of weight exactly 0 adds exactly 0 and is skipped; writes omega;
//   mg_psm_fold_kernel     after it, workgroup = (track, slab of 256 k): the offspring of k are one contiguous run of the non-decreasing
//                          systematic ancestors, found by two binary searches over integer bounds; omega summed over the run;
//   mg_psm_moments_kernel  one launch, workgroup = (track, row): the reduction shape of the weight kernel.
// No atomics, nothing waits on another workgroup, every sum has an order fixed by N alone.  The addresses that depend on computed
// values are the fold's: every ancestor is clamped into [0, N) before it is compared, and the run's bounds lie in [0, N] by
// construction of the search.  A track whose length is <= t + 1 does nothing at row t.  The transition, the emission, the reductions
// and psm_logf are the blocks of moment_particle.h that the filter and the backward simulation call.
#include "moment_particle.h"

namespace ffvd {
namespace {

constexpr int PSM_CHUNK = 256;                            // rows of a staged chunk: (2 D + 1) * 2 KiB of LDS, 34 KiB at D = 8

__device__ __forceinline__ int psm_len(const MomentParticleSmoothArgs &q, int v) {
    const int n = q.lens ? q.lens[v % q.R] : q.steps;
    return n < 1 ? 1 : n > q.steps ? q.steps : n;
}

// After the product launch of step s.  a.G: the tracks of the pass; the indexing is the weight kernel's.
template <int D>
__global__ __launch_bounds__(256) void mg_psm_keep_kernel(MomentGroupArgs a, const int s, MomentRecordArgs rc, MomentLinearFanArgs l,
                                                          MomentParticleArgs p, double *tm, double *tv) {
    const int G = a.G, steps = a.steps, N = p.N;
    const int nsl = (N + 255) / 256;
    const int v = blockIdx.x / nsl, i = (blockIdx.x % nsl) * 256 + threadIdx.x;
    if (i >= N) return;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);
    const size_t vg = (size_t)gq * rc.R + r, o = ((vg * steps + s) * N + i) * D;
    const double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;
    const double *pm = p.pmean + (size_t)v * D * N;
#pragma unroll
    for (int d = 0; d < D; ++d)
        particle_transition<D>(l, gq, d, row, i, N, Xp, pm, a.variance[(size_t)model * D + d], exp(a.log_Q[(size_t)gq * D + d]), tm[o + d],
                               tv[o + d]);
}

// Workgroup = (track, row) of the call
template <int D>
__global__ __launch_bounds__(256) void mg_psm_weights_kernel(MomentFilterArgs f, MomentParticleSmoothArgs q) {
    __shared__ double Wl[MG_PREC_MAXN], red[4][PARTICLE_RED];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], lcs[MG_MAXJ];
    const int tid = threadIdx.x, N = q.N, steps = q.steps, J = f.J;
    const int t = blockIdx.x % steps, v = blockIdx.x / steps, r = v % q.R, n = psm_len(q, v);
    const size_t o = (size_t)blockIdx.x * N;
    if (t >= n) {
        const double nan = __builtin_nan("");
        for (int i = tid; i < N; i += 256) {
            q.weights[o + i] = nan;
            q.w_smooth[o + i] = nan;
        }
        return;
    }
    particle_stage_emission<D>(f, f.Y + ((size_t)r * steps + t) * J, hs, dds, s2s, ys, lcs);
    __syncthreads();
    const bool any = particle_any_observed(ys, J);
    const double *X = q.particles + o * D;
    double mx = -__builtin_inf();
    for (int i = tid; i < N; i += 256) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = X[(size_t)i * D + d];
        double L = 0.0;
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) L += particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs);
        mx = fmax(mx, L);
        Wl[i] = L;
    }
    mx = wg_max(mx, red);
    double sw[1] = {0.0};
    for (int i = tid; i < N; i += 256) {
        const double w = any ? exp(Wl[i] - mx) : 1.0;
        Wl[i] = w;
        q.weights[o + i] = w;
        sw[0] += w;
    }
    if (t != n - 1) return;
    wg_sum<1>(sw, red);
    for (int i = tid; i < N; i += 256) q.w_smooth[o + i] = Wl[i] / sw[0];
}

// Workgroup = (track, row t <= n - 2, slab of 256 columns j); c of the columns of row u = t + 1 goes to cnorm[track][u]
template <int D>
__global__ __launch_bounds__(256) void mg_psm_norm_kernel(MomentParticleSmoothArgs q) {
    __shared__ double mu[PSM_CHUNK][D], is[PSM_CHUNK][D], ls[PSM_CHUNK];
    const int tid = threadIdx.x, N = q.N, steps = q.steps;
    const int nsl = (N + 255) / 256;
    const int slab = blockIdx.x % nsl, vt = blockIdx.x / nsl, u = vt % (steps - 1) + 1, v = vt / (steps - 1);
    if (u >= psm_len(q, v)) return;
    const size_t o = ((size_t)v * steps + u) * N;
    const int j = slab * 256 + tid, jc = j < N ? j : N - 1;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = q.particles[(o + jc) * D + d];
    double mx = -__builtin_inf(), sum = 0.0;
    for (int sweep = 0; sweep < 2; ++sweep)
        for (int i0 = 0; i0 < N; i0 += PSM_CHUNK) {
            const int ni = N - i0 < PSM_CHUNK ? N - i0 : PSM_CHUNK;
            __syncthreads();
            if (tid < ni) {
                double lsum = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double s = q.trans_var[(o + i0 + tid) * D + d];
                    mu[tid][d] = q.trans_mean[(o + i0 + tid) * D + d];
                    is[tid][d] = 1.0 / s;
                    lsum += log(s);
                }
                ls[tid] = lsum;
            }
            __syncthreads();
            if (sweep == 0)
                for (int i = 0; i < ni; ++i) mx = fmax(mx, psm_logf<D>(x, mu[i], is[i], ls[i]));
            else
                for (int i = 0; i < ni; ++i) sum += exp(psm_logf<D>(x, mu[i], is[i], ls[i]) - mx);
        }
    if (j < N) q.cnorm[o + j] = mx + log(sum);
}

// Row t.  Workgroup = (track, slab of 256 carried particles i of row u = t + 1)
template <int D>
__global__ __launch_bounds__(256) void mg_psm_back_kernel(MomentParticleSmoothArgs q, const int t) {
    __shared__ double xs[PSM_CHUNK][D], cs[PSM_CHUNK], ws[PSM_CHUNK];
    const int tid = threadIdx.x, N = q.N, steps = q.steps, u = t + 1;
    const int nsl = (N + 255) / 256;
    const int slab = blockIdx.x % nsl, v = blockIdx.x / nsl;
    if (psm_len(q, v) <= u) return;
    const size_t o = ((size_t)v * steps + u) * N;
    const int i = slab * 256 + tid, ic = i < N ? i : N - 1;
    double mu[D], is[D], ls = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double s = q.trans_var[(o + ic) * D + d];
        mu[d] = q.trans_mean[(o + ic) * D + d];
        is[d] = 1.0 / s;
        ls += log(s);
    }
    double acc = 0.0;
    for (int j0 = 0; j0 < N; j0 += PSM_CHUNK) {
        const int nj = N - j0 < PSM_CHUNK ? N - j0 : PSM_CHUNK;
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
    if (i < N) q.omega[(size_t)v * N + i] = acc;
}

// Row t, after the backward kernel.  Workgroup = (track, slab of 256 particles k of row t)
__global__ __launch_bounds__(256) void mg_psm_fold_kernel(MomentParticleSmoothArgs q, const int t) {
    __shared__ int as[MG_PREC_MAXN];
    const int tid = threadIdx.x, N = q.N, steps = q.steps;
    const int nsl = (N + 255) / 256;
    const int slab = blockIdx.x % nsl, v = blockIdx.x / nsl;
    if (psm_len(q, v) <= t + 1) return;
    const size_t o = ((size_t)v * steps + t) * N;
    for (int i = tid; i < N; i += 256) as[i] = particle_clamp(q.ancestors[o + i], N);
    __syncthreads();
    const int k = slab * 256 + tid;
    if (k >= N) return;
    int lo = 0, hi = N;
    while (lo < hi) {                                             // #{i: a_i < k}: at most 12 rounds, whatever the values are
        const int mid = (lo + hi) >> 1;
        if (as[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    const int first = lo;
    hi = N;
    while (lo < hi) {                                             // #{i: a_i <= k}, from `first` on
        const int mid = (lo + hi) >> 1;
        if (as[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    const double *om = q.omega + (size_t)v * N;
    double w = 0.0;
    for (int i = first; i < lo; ++i) w += om[i];                  // 0 <= first <= lo <= N
    q.w_smooth[o + k] = w;
}

// Workgroup = (track, row) of the call
template <int D>
__global__ __launch_bounds__(256) void mg_psm_moments_kernel(MomentParticleSmoothArgs q) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double red[4][PARTICLE_RED];
    const int tid = threadIdx.x, N = q.N, steps = q.steps;
    const int t = blockIdx.x % steps, v = blockIdx.x / steps;
    const size_t row = blockIdx.x, o = row * N;
    if (t >= psm_len(q, v)) {
        const double nan = __builtin_nan("");
        if (tid < D) q.m_smooth[row * D + tid] = nan;
        if (tid < D * D) q.S_smooth[row * D * D + tid] = nan;
        if (tid == 192) q.ess_smooth[row] = nan;
        return;
    }
    const double *X = q.particles + o * D, *W = q.w_smooth + o;
    double sw[2], wm[D];
    sw[0] = sw[1] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) wm[d] = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double w = W[i];
        sw[0] += w;
        sw[1] += w * w;
#pragma unroll
        for (int d = 0; d < D; ++d) wm[d] += w * X[(size_t)i * D + d];
    }
    wg_sum<2>(sw, red);
    wg_sum<D>(wm, red);
    double ms[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ms[d] = wm[d] / sw[0];
    double sf[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sf[k] = 0.0;
    for (int i = tid; i < N; i += 256) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = X[(size_t)i * D + d] - ms[d];
        const double w = W[i];
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) sf[k++] += w * (x[lo] * x[hi]);
    }
    wg_sum<NP>(sf, red);
    // every thread holds every sum, thread k stores entry k
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (tid == d) q.m_smooth[row * D + d] = ms[d];
    int k = 0;
#pragma unroll
    for (int lo = 0; lo < D; ++lo)
#pragma unroll
        for (int hi = lo; hi < D; ++hi) {
            if (tid == 64 + k) particle_store_sym<D>(q.S_smooth, row, lo, hi, sf[k] / sw[0]);
            ++k;
        }
    if (tid == 192) q.ess_smooth[row] = sw[0] * sw[0] / sw[1];
}

}  // namespace

// a.G: the tracks of the pass (groups * rc.Rp); s < steps: the step whose product launch has been enqueued
void launch_mg_psm_keep(hipStream_t stream, const MomentGroupArgs &a, const MomentRecordArgs &rc, const MomentLinearFanArgs &l,
                        const MomentParticleArgs &p, const MomentParticleSmoothArgs &q, int s) {
    const dim3 grid((unsigned)((size_t)a.G * ((p.N + 255) / 256)));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_keep_kernel<d>), grid, dim3(256), 0, stream, a, s, rc, l, p, q.trans_mean,
                                          q.trans_var))
}

// After the filter's last pass: the weights, the normalisers of all rows, the rows n_max - 2 .. 0 (two launches each), the moments.
// n_max: the longest record of the call (<= q.steps).
void launch_mg_psm_smooth(hipStream_t stream, const MomentFilterArgs &f, const MomentParticleSmoothArgs &q, int n_max) {
    const int nsl = (q.N + 255) / 256;
    const dim3 rows((unsigned)((size_t)q.V * q.steps)), slabs((unsigned)((size_t)q.V * nsl));
    const dim3 pairs((unsigned)((size_t)q.V * (q.steps - 1) * nsl));
    MG_DISPATCH_D(q.D, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_weights_kernel<d>), rows, dim3(256), 0, stream, f, q);
        if (n_max > 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_norm_kernel<d>), pairs, dim3(256), 0, stream, q);
        for (int t = n_max - 2; t >= 0; --t) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_back_kernel<d>), slabs, dim3(256), 0, stream, q, t);
            hipLaunchKernelGGL(mg_psm_fold_kernel, slabs, dim3(256), 0, stream, q, t);
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_moments_kernel<d>), rows, dim3(256), 0, stream, q);
    })
}

// The weights kernel alone (the particle backward simulation of moment_particle_backsim.hip draws its last row from W_{n-1}); it also
// writes the last row of q.w_smooth and NaN beyond every length.
void launch_mg_psm_weights(hipStream_t stream, const MomentFilterArgs &f, const MomentParticleSmoothArgs &q) {
    const dim3 rows((unsigned)((size_t)q.V * q.steps));
    MG_DISPATCH_D(q.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_weights_kernel<d>), rows, dim3(256), 0, stream, f, q))
}

// The normalisers of all rows and the moments alone (host code only: the adapted smoother of moment_particle_adapted_smooth.hip brings
// a backward kernel of its own between them)
void launch_mg_psm_norm(hipStream_t stream, const MomentParticleSmoothArgs &q, int n_max) {
    if (n_max <= 1) return;
    const dim3 pairs((unsigned)((size_t)q.V * (q.steps - 1) * ((q.N + 255) / 256)));
    MG_DISPATCH_D(q.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_norm_kernel<d>), pairs, dim3(256), 0, stream, q))
}
void launch_mg_psm_moments(hipStream_t stream, const MomentParticleSmoothArgs &q) {
    const dim3 rows((unsigned)((size_t)q.V * q.steps));
    MG_DISPATCH_D(q.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_psm_moments_kernel<d>), rows, dim3(256), 0, stream, q))
}

}  // namespace ffvd

