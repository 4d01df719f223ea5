// Moment-matched prediction for G posteriors with SE-ARD kernels: x_t ~ N(mu, Sigma) -> mean and covariance of
// x_{t+1} = x_t + f(x_t, c_t) + process noise in closed form, re-approximated as a Gaussian.
//
// From the posterior, once per call (ops_grouped.hip puts the launches together): beta_a = W_a u_a (mg_beta_kernel) and
// Gamma_a = W_a (I - q q^T) W_a^T, so that m_a(x) = k_a(x, Z) beta_a, v_a(x) = variance_a - k_a(x, Z) Gamma_a k_a(Z, x).
// Gamma is NOT formed as W W^T - (W q)(W q)^T: where K_uu is ill-conditioned both products have entries near 1e5 and their
// difference entries near 1 (five digits lost in fp64).  With N = I - q (exact in fp64 for the entries that matter),
// E = I - q q^T = (N + N^T) - N N^T has no such cancellation, and Gamma = (W E) W^T: three products on the fp64 MFMA through
// cov.hip's product body (mg_nmat_kernel / mg_emat_kernel are the two elementwise steps).
//
// Shape of the launch.  A step of a group is cut into a FIXED set of workgroups that meet only at kernel boundaries:
//   workgroup (g, pair a <= b, slab s) owns the rows i in [16 s, 16 s + 16) of the pair's M x M table.
// Launch t (t = 0 .. steps) does, in every workgroup of group g:
//   1. (t > 0) finish step t - 1: add the slab sums of launch t - 1 in slab order and form mu_t, Sigma_t -- the same instructions
//      in the same order in every workgroup of the group; the workgroup (pair 0, slab 0) also stores them, with m_x / S_x.
//   2. (t < steps) with nu_i = z_i - [mu_t, c_t], lambda_a = 1 / l_a^2 (first D), a_i = lambda_a nu_i^x:
//        R_a = Sigma diag(lambda_a) + I, T_a = R_a^-1 Sigma, and the same with lambda_b and with lambda_a + lambda_b (R, T): three
//        D x D eliminations with partial pivoting, one thread each;
//        q^a_i = variance_a |R_a|^-1/2 exp(-nu_i^T Lambda_a^-1 nu_i / 2 + a_i^T T_a a_i / 2)      (= E[k_a(x, z_i)]);
//        Q^ab_ij = q^a_i q^b_j rho exp(delta_ij),   rho = (|R_a| |R_b| / |R|)^1/2,
//        delta_ij = a_i^T (T - T_a) a_i / 2 + b_j^T (T - T_b) b_j / 2 + a_i^T T b_j:   a D-long dot product and one expm1 per element;
//        Cov(f_a, f_b) slab sum = sum_ij beta_ai q^a_i beta_bj q^b_j (rho expm1(delta_ij) + (rho - 1))   (the centred form: at
//        Sigma = 0 every T is an exact zero, rho = 1 and each term vanishes), minus for a = b  sum_ij Gamma_ij Q^aa_ij;
//        pairs a = a also leave E[f_a] = sum_i beta_ai q^a_i and Cov(x, f_a) = T_a sum_i beta_ai q^a_i a_i of their slab.
//      -> part[t & 1].
// One launch per step for ALL groups; no atomics, nothing waits on another workgroup, nothing needs to be resident.  The
// decomposition of a group depends on (M, D) only and every sum has a fixed order: a group's results are bit-identical alone or
// among others, and run to run.
//
// |R| <= 0 or a non-finite state: NaN for that group from there on; no global address depends on a computed value.
//
// The step kernel itself is in moment_step.h: this file instantiates it as the propagation (FILTER = false), moment_filter.hip as the
// filter.  Separate translation units, so that the propagation's code does not change with the filter's.
#include "moment_step.h"

namespace ffvd {

__global__ __launch_bounds__(256) void mg_beta_kernel(int D, int M, int Mp, int w_per_group, const double *W, const double *U,
                                                      double *beta) {
    const int gd = blockIdx.x, g = gd / D, d = gd % D, i = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;
    const double *Wi = W + ((size_t)(w_per_group ? gd : d) * Mp + i) * Mp;
    const double *u = U + (size_t)g * M * D + d;
    double s = 0.0;
    for (int j = lane; j < M; j += 64) s += Wi[j] * u[(size_t)j * D];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) beta[(size_t)gd * Mp + i] = s;
}
void launch_mg_beta(hipStream_t stream, int G, int D, int M, int Mp, int w_per_group, const double *W, const double *U, double *beta) {
    hipLaunchKernelGGL(mg_beta_kernel, dim3((unsigned)(G * D), (unsigned)((M + 3) / 4)), dim3(256), 0, stream, D, M, Mp, w_per_group, W,
                       U, beta);
}

// N = I - q on the leading M x M block, zero outside (q: [nq] slots of Mp x Mp)
__global__ __launch_bounds__(256) void mg_nmat_kernel(int M, int Mp, const double *q, double *N) {
    const size_t mm = (size_t)Mp * Mp, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= mm) return;
    const int i = (int)(e / Mp), j = (int)(e % Mp);
    const size_t o = (size_t)blockIdx.y * mm + e;
    N[o] = (i < M && j < M) ? (i == j ? 1.0 : 0.0) - q[o] : 0.0;
}
// E = (N + N^T) - N N^T in place: E holds -N N^T on the leading M x M block (cov.hip), zero outside
__global__ __launch_bounds__(256) void mg_emat_kernel(int M, int Mp, const double *N, double *E) {
    const size_t mm = (size_t)Mp * Mp, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= mm) return;
    const int i = (int)(e / Mp), j = (int)(e % Mp);
    if (i >= M || j >= M) return;
    const size_t b = (size_t)blockIdx.y * mm;
    E[b + e] = (N[b + e] + N[b + (size_t)j * Mp + i]) + E[b + e];
}
void launch_mg_nmat(hipStream_t stream, int nq, int M, int Mp, const double *q, double *N) {
    hipLaunchKernelGGL(mg_nmat_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), (unsigned)nq), dim3(256), 0, stream, M, Mp, q, N);
}
void launch_mg_emat(hipStream_t stream, int nq, int M, int Mp, const double *N, double *E) {
    hipLaunchKernelGGL(mg_emat_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), (unsigned)nq), dim3(256), 0, stream, M, Mp, N, E);
}

namespace {
__global__ __launch_bounds__(256) void mg_summary_kernel(MomentSummaryArgs a) {
    const size_t SJ = (size_t)a.steps * a.J, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= SJ) return;
    const int J = a.J, D = a.D, G = a.G, t = (int)(e / J), j = (int)(e % J);
    const bool dens = t < a.n_test;
    const double sd = a.sd[j], s2n = sd * sd, dd = a.DD[j], y = dens ? a.Y[e] : 0.0;
    auto moments = [&](int g, double &m, double &s2) {
        const double *mg = a.m + ((size_t)g * a.steps + t) * D, *Sg = a.S + ((size_t)g * a.steps + t) * D * D;
        m = 0.0;
        s2 = 0.0;
        for (int k = 0; k < D; ++k) {
            const double ck = a.CC[(size_t)k * J + j];
            double row = 0.0;
            for (int l = 0; l < D; ++l) row += Sg[k * D + l] * a.CC[(size_t)l * J + j];
            m += ck * mg[k];
            s2 += ck * row;
        }
        m += dd;
        s2 += s2n;
    };
    double sm = 0.0, sq = 0.0, mx = -INFINITY;
    for (int g = 0; g < G; ++g) {                                 // ascending group order
        double m, s2;
        moments(g, m, s2);
        sm += m;
        sq += s2 + m * m;
        if (dens) {
            const double r = y - m, ex = -0.5 * (LOG_2PI + log(s2)) - 0.5 * r * r / s2;
            if (ex > mx) mx = ex;
        }
    }
    const double ym = sm / G, vt = sq / G - ym * ym;
    a.out[e] = ym;
    a.out[SJ + e] = vt;
    a.out[2 * SJ + e] = vt;
    if (dens) {
        double se = 0.0;
        for (int g = 0; g < G; ++g) {
            double m, s2;
            moments(g, m, s2);
            const double r = y - m, ex = -0.5 * (LOG_2PI + log(s2)) - 0.5 * r * r / s2;
            se += exp(ex - mx);                                   // NaN goes through; mx = -inf only when every exponent is
        }
        const double r = y - ym;
        a.out[3 * SJ + e] = (mx + log(se)) - log((double)G);
        a.out[4 * SJ + e] = -0.5 * (LOG_2PI + log(vt)) - 0.5 * r * r / vt;
    }
}

}  // namespace

void launch_mg_step(hipStream_t stream, const MomentGroupArgs &a, int t) {
    const dim3 grid((unsigned)((size_t)a.G * mg_npair(a.D) * a.NS));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_step_kernel<d, false>), grid, dim3(256), 0, stream, a, t))
}

void launch_moment_summary(hipStream_t stream, const MomentSummaryArgs &a) {
    const size_t SJ = (size_t)a.steps * a.J;
    if (SJ == 0 || a.G <= 0) return;
    hipLaunchKernelGGL(mg_summary_kernel, dim3((unsigned)((SJ + 255) / 256)), dim3(256), 0, stream, a);
}

}  // namespace ffvd
