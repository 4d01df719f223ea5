// Moment-matched prediction for G posteriors with SE-ARD kernels: x_t ~ N(mu, Sigma) -> mean and covariance of
// x_{t+1} = x_t + f(x_t, c_t) + process noise in closed form, re-approximated as a Gaussian.
//
// From the posterior, once per call (ops.hip puts the launches together): beta_a = W_a u_a (mg_beta_kernel) and
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
#include "moment_group.h"
#include "kernels.h"
#include "dev_common.h"

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
constexpr double LOG_2PI = 1.8378770664093454835606594728112;

// T = R^-1 S with R = S diag(lam) + I: Gaussian elimination with partial pivoting on the rows [R | S] (A: this thread's LDS);
// returns |R|.  S need not be positive definite (S = 0 at step 0: R = I); a zero pivot gives inf / NaN, which propagate.
template <int D>
__device__ __noinline__ double mg_solve(const double (*S)[MG_MAXD], const double *lam, double (*A)[2 * MG_MAXD], double (*T)[MG_MAXD]) {
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            A[r][c] = S[r][c] * lam[c] + (r == c ? 1.0 : 0.0);
            A[r][D + c] = S[r][c];
        }
    double det = 1.0;
    for (int k = 0; k < D; ++k) {
        int piv = k;                                             // in [k, D): an LDS row of this thread, whatever the values are
        double best = fabs(A[k][k]);
        for (int r = k + 1; r < D; ++r) {
            const double v = fabs(A[r][k]);
            if (v > best) { best = v; piv = r; }
        }
        if (piv != k) {
            for (int c = k; c < 2 * D; ++c) { const double x = A[k][c]; A[k][c] = A[piv][c]; A[piv][c] = x; }
            det = -det;
        }
        const double p = A[k][k], ip = 1.0 / p;
        det *= p;
        for (int r = k + 1; r < D; ++r) {
            const double f = A[r][k] * ip;
            for (int c = k + 1; c < 2 * D; ++c) A[r][c] -= f * A[k][c];
        }
    }
    for (int c = 0; c < D; ++c)
        for (int r = D - 1; r >= 0; --r) {
            double s = A[r][D + c];
            for (int k = r + 1; k < D; ++k) s -= A[r][k] * T[k][c];
            T[r][c] = s / A[r][r];
        }
    return det;
}

// One inducing row z for one latent dim: av = lambda nu^x, q = E[k(x, z)] (scale = variance |R_d|^-1/2), and
// de = av^T (T - T_d) av / 2, the row's share of delta.  il: 1 / lengthscales of the dim; Td, Tp: T of the dim and of the pair.
template <int D>
__device__ __forceinline__ void mg_row(const double *z, const double *xin, const double *il, int P, const double (*Td)[MG_MAXD],
                                       const double (*Tp)[MG_MAXD], double scale, double (&av)[D], double &q, double &de) {
    double c = 0.0;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        const double u = (z[p] - xin[p]) * il[p];
        c += u * u;
        av[p] = u * il[p];
    }
    for (int p = D; p < P; ++p) {
        const double u = (z[p] - xin[p]) * il[p];
        c += u * u;
    }
    double qa = 0.0, qt = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double sa = 0.0, st = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) { sa += Td[r][k] * av[k]; st += Tp[r][k] * av[k]; }
        qa += av[r] * sa;
        qt += av[r] * st;
    }
    q = scale * exp(0.5 * qa - 0.5 * c);                         // the whole exponent (never positive) before the exp
    de = 0.5 * qt - 0.5 * qa;
}

template <int D>
__global__ __launch_bounds__(256) void mg_step_kernel(MomentGroupArgs a, const int t) {
    constexpr int NP = D * (D + 1) / 2, NF = NP + D + D * D;
    __shared__ double mu[MG_MAXD], Sg[MG_MAXD][MG_MAXD], xin[MAXP], fin[NF];
    __shared__ double ils[2][MAXP], lam[3][MG_MAXD];
    __shared__ double GA[3][MG_MAXD][2 * MG_MAXD], TT[3][MG_MAXD][MG_MAXD], dets[3];
    __shared__ double tav[MG_SLAB][MG_MAXD], avs[MG_SLAB][MG_MAXD], dei[MG_SLAB], bqi[MG_SLAB], qi[MG_SLAB], rvec[MG_MAXD];
    __shared__ double red[4][2];
    const int tid = threadIdx.x;
    const int G = a.G, C = a.C, P = a.P, M = a.M, Mp = a.Mp, NS = a.NS, steps = a.steps;
    const int s = blockIdx.x % NS, gp = blockIdx.x / NS, pr = gp % NP, g = gp / NP;
    int da = 0, db = pr;                                          // pair pr -> (da <= db), row-major over the upper triangle
    while (db >= D - da) { db -= D - da; ++da; }
    db += da;
    const bool writer = (pr == 0 && s == 0);
    if (t == steps && !writer) return;
    const int model = a.n_models == 1 ? 0 : g;

    // 1. the state of this launch: (x_last, S0), or the state of launch t - 1 plus its slab sums
    if (t == 0) {
        if (tid < D) mu[tid] = a.x_last[(size_t)g * D + tid];
        if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[(size_t)g * D * D + tid] : 0.0;
    } else {
        const double *pp = a.part + ((size_t)((t - 1) & 1) * G + g) * NF * NS;
        if (tid < NF) {
            double sum = 0.0;
            for (int sl = 0; sl < NS; ++sl) sum += pp[(size_t)tid * NS + sl];          // slab order, the same in every workgroup
            fin[tid] = sum;
        }
        __syncthreads();
        const double *sp = a.state + ((size_t)((t - 1) & 1) * G + g) * (D + D * D);
        if (tid < D) mu[tid] = sp[tid] + fin[NP + tid];
        if (tid < D * D) {                                        // (r, c) and (c, r) run the same expression: exactly symmetric
            const int r = tid / D, c = tid % D, lo = r < c ? r : c, hi = r < c ? c : r;
            const int pi = lo * D - lo * (lo - 1) / 2 + (hi - lo);
            double v = sp[D + lo * D + hi] + fin[pi];
            v += fin[NP + D + hi * D + lo] + fin[NP + D + lo * D + hi];                   // Cov(x_lo, f_hi) + Cov(x_hi, f_lo)
            if (lo == hi) v += a.variance[(size_t)model * D + lo] + exp(a.log_Q[(size_t)g * D + lo]);
            Sg[r][c] = v;
        }
    }
    __syncthreads();
    if (writer) {
        double *sc = a.state + ((size_t)(t & 1) * G + g) * (D + D * D);
        if (tid < D) {
            sc[tid] = mu[tid];
            if (t > 0) a.m_x[((size_t)g * steps + (t - 1)) * D + tid] = mu[tid];
        }
        if (tid < D * D) {
            const double v = Sg[tid / D][tid % D];
            sc[D + tid] = v;
            if (t > 0) a.S_x[((size_t)g * steps + (t - 1)) * D * D + tid] = v;
        }
    }
    if (t == steps) return;

    // 2. the three eliminations of the pair
    const double *lena = a.len + ((size_t)model * D + da) * P, *lenb = a.len + ((size_t)model * D + db) * P;
    if (tid < P) {
        xin[tid] = tid < D ? mu[tid] : a.ctrl[(size_t)t * C + (tid - D)];
        const double ia = 1.0 / lena[tid], ib = 1.0 / lenb[tid];
        ils[0][tid] = ia;
        ils[1][tid] = ib;
        if (tid < D) { lam[0][tid] = ia * ia; lam[1][tid] = ib * ib; lam[2][tid] = ia * ia + ib * ib; }
    }
    __syncthreads();
    if (tid < 3) dets[tid] = mg_solve<D>(Sg, lam[tid], GA[tid], TT[tid]);
    __syncthreads();
    const double detA = dets[0], detB = dets[1], detP = dets[2];
    const bool ok = detA > 0.0 && detB > 0.0 && detP > 0.0;
    const double nan = __builtin_nan("");
    const double sca = ok ? a.variance[(size_t)model * D + da] / sqrt(detA) : nan;
    const double scb = ok ? a.variance[(size_t)model * D + db] / sqrt(detB) : nan;
    const double rho = ok ? sqrt(detA * detB / detP) : nan, rho1 = rho - 1.0;

    // 3. the slab's rows (dim a)
    const int i0 = MG_SLAB * s, ni = (M - i0 < MG_SLAB) ? M - i0 : MG_SLAB;
    const double *Zm = a.Z + (size_t)model * M * P;
    const double *bea = a.beta + ((size_t)g * D + da) * Mp, *beb = a.beta + ((size_t)g * D + db) * Mp;
    if (tid < MG_SLAB) {
        double av[D], q = 0.0, de = 0.0, be = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) av[k] = 0.0;
        if (tid < ni) {
            mg_row<D>(Zm + (size_t)(i0 + tid) * P, xin, ils[0], P, TT[0], TT[2], sca, av, q, de);
            be = bea[i0 + tid];
        }
#pragma unroll
        for (int r = 0; r < D; ++r) {
            double st = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) st += TT[2][k][r] * av[k];
            tav[tid][r] = st;
            avs[tid][r] = av[r];
        }
        dei[tid] = de;
        qi[tid] = q;
        bqi[tid] = be * q;
    }
    __syncthreads();
    double *po = a.part + ((size_t)(t & 1) * G + g) * NF * NS;
    const bool diag = da == db;
    if (diag && tid < D) {
        double r = 0.0;
        for (int i = 0; i < ni; ++i) r += bqi[i] * avs[i][tid];
        rvec[tid] = r;
    }
    if (diag && tid == 64) {
        double m = 0.0;
        for (int i = 0; i < ni; ++i) m += bqi[i];
        po[(size_t)(NP + da) * NS + s] = m;                                               // E[f_a] of the slab
    }
    __syncthreads();
    if (diag && tid < D) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) v += TT[0][tid][k] * rvec[k];
        po[(size_t)(NP + D + da * D + tid) * NS + s] = v;                                 // Cov(x, f_a) of the slab
    }

    // 4. the slab of the pair table: thread = column j
    const double *Gg = diag ? a.gam + ((size_t)(a.unit_per_group ? g : model) * D + da) * Mp * Mp + (size_t)i0 * Mp : nullptr;
    double accc = 0.0, accg = 0.0;
    for (int j = tid; j < M; j += 256) {
        double bv[D], qj, dg;
        mg_row<D>(Zm + (size_t)j * P, xin, ils[1], P, TT[1], TT[2], scb, bv, qj, dg);
        const double bqj = beb[j] * qj;
        for (int i = 0; i < ni; ++i) {
            double del = dei[i] + dg;
#pragma unroll
            for (int k = 0; k < D; ++k) del += tav[i][k] * bv[k];
            // Q_ij <= its bound means del <= -(log q_i + log q_j): an exponent beyond 700 belongs to a product q_i q_j that is zero
            const double em = expm1(del > 700.0 ? 700.0 : del);
            accc += bqi[i] * (bqj * (rho * em + rho1));
            if (diag) accg -= Gg[(size_t)i * Mp + j] * ((qi[i] * qj) * (rho * (em + 1.0)));
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int mm = 32; mm > 0; mm >>= 1) { accc += __shfl_xor(accc, mm); accg += __shfl_xor(accg, mm); }
    if (lane == 0) { red[wave][0] = accc; red[wave][1] = accg; }
    __syncthreads();
    if (tid == 0) {
        const double cs = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        const double gs = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        po[(size_t)pr * NS + s] = cs + gs;                        // Cov(f_a, f_b) of the slab (a = b: with E[v_a] - variance_a)
    }
}

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
    switch (a.D) {
#define MG_CASE(d) case d: hipLaunchKernelGGL(mg_step_kernel<d>, grid, dim3(256), 0, stream, a, t); break;
        MG_CASE(1) MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8)
#undef MG_CASE
        default: break;
    }
}

void launch_moment_summary(hipStream_t stream, const MomentSummaryArgs &a) {
    const size_t SJ = (size_t)a.steps * a.J;
    if (SJ == 0 || a.G <= 0) return;
    hipLaunchKernelGGL(mg_summary_kernel, dim3((unsigned)((SJ + 255) / 256)), dim3(256), 0, stream, a);
}

}  // namespace ffvd
