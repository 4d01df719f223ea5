// The step kernel of the moment-matched prediction and of the filter: one template, instantiated with
// FILTER = false by moment_group.hip (the propagation), with FILTER = true by moment_filter.hip (the measurement update added) and
// with FILTER = false and one MomentFanArgs by moment_fan.hip (the propagation with a track as its unit: rolling-origin forecasts).
// The instantiations live in separate translation units so that the code of the propagation does not depend on the others'.
#pragma once
#include "moment_group.h"
#include "kernels.h"
#include "dev_common.h"

namespace ffvd {
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

// The measurement update of the filter form: row t - 1 of Y against the predicted state (mu, Sg) of the launch,
// as scalar updates in ascending j -- no J x J factorisation, no pivoting.  Every workgroup of the group runs it with the same
// instructions in the same order on the same values; whether an entry is observed (y == y) is the same for every thread, so the
// barriers are met by all.  (r, c) and (c, r) of Sg run one expression.  The writer stores; the filtered state goes to state[t & 1].
template <int D>
__device__ __forceinline__ void mg_update(const MomentGroupArgs &a, const MomentFilterArgs &f, const int t, const int g, const bool writer,
                                          double *mu, double (*Sg)[MG_MAXD]) {
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], Sh[MG_MAXD];
    const int tid = threadIdx.x, J = f.J;
    if (t > 0) {
        const size_t row = (size_t)g * a.steps + (t - 1);
        if (tid < J * D) hs[tid / D][tid % D] = f.CC[(size_t)(tid % D) * J + tid / D];
        if (tid < J) {
            dds[tid] = f.DD[tid];
            s2s[tid] = f.sd[tid] * f.sd[tid];
            ys[tid] = f.Y[(size_t)(t - 1) * J + tid];
        }
        __syncthreads();
        if (writer && tid < J) {                                  // the marginal one-step densities, before any update
            const double y = ys[tid];
            double m = 0.0, s2 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double rw = 0.0;
#pragma unroll
                for (int l = 0; l < D; ++l) rw += Sg[k][l] * hs[tid][l];
                m += hs[tid][k] * mu[k];
                s2 += hs[tid][k] * rw;
            }
            m += dds[tid];
            s2 += s2s[tid];
            const double r = y - m;
            f.lpd[row * J + tid] = y != y ? __builtin_nan("") : -0.5 * (LOG_2PI + log(s2)) - 0.5 * r * r / s2;
        }
        __syncthreads();
        double lj = 0.0;
        bool any = false;
        for (int j = 0; j < J; ++j) {
            const double y = ys[j];
            if (y != y) continue;                                 // unobserved: skipped by the whole workgroup
            if (tid < D) {
                double v = 0.0;
#pragma unroll
                for (int c = 0; c < D; ++c) v += Sg[tid][c] * hs[j][c];
                Sh[tid] = v;                                      // Sigma h
            }
            __syncthreads();
            double s = 0.0, hm = 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) { s += hs[j][r] * Sh[r]; hm += hs[j][r] * mu[r]; }
            s += s2s[j];
            const double e = (y - hm) - dds[j];
            __syncthreads();
            if (tid < D) mu[tid] += Sh[tid] * e / s;
            if (tid < D * D) {
                const int r = tid / D, c = tid % D, lo = r < c ? r : c, hi = r < c ? c : r;
                Sg[r][c] -= Sh[lo] * Sh[hi] / s;
            }
            lj += -0.5 * (LOG_2PI + log(s)) - 0.5 * e * e / s;
            any = true;
            __syncthreads();
        }
        if (writer) {
            if (tid < D) f.m_filt[row * D + tid] = mu[tid];
            if (tid < D * D) f.S_filt[row * D * D + tid] = Sg[tid / D][tid % D];
            if (tid == 0) f.lpd_joint[row] = any ? lj : __builtin_nan("");
        }
    }
    if (writer) {
        double *sc = a.state + ((size_t)(t & 1) * a.G + g) * (D + D * D);
        if (tid < D) sc[tid] = mu[tid];
        if (tid < D * D) sc[D + tid] = Sg[tid / D][tid % D];
    }
}

__device__ __forceinline__ const MomentFilterArgs &mg_filter_args(const MomentFilterArgs &f) { return f; }
__device__ __forceinline__ const MomentFanArgs &mg_fan_args(const MomentFanArgs &f) { return f; }

// One launch of the propagation (FILTER = false, no further argument: the kernel as it was before the filter existed), of the
// filter (FILTER = true, one MomentFilterArgs: the measurement update and the stores of the filter are added) or of the fan
// (FILTER = false, one MomentFanArgs: the unit g of the decomposition is a track, see moment_group.h).  The fan changes WHERE a unit
// reads and writes, never an expression on the values: gq is the group whose posterior, hyper-parameters and log_Q the unit uses,
// orow the first row of its output stacks, crow its first control row; without a MomentFanArgs they are g, g * steps and 0 (and
// the existing instantiations keep the expressions they had, so that their code does not change).
template <int D, bool FILTER, class... F>
__global__ __launch_bounds__(256) void mg_step_kernel(MomentGroupArgs a, const int t, F... f) {
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
    constexpr bool FAN = !FILTER && sizeof...(F) == 1;
    int gq = g, crow = 0;
    size_t orow = 0, srow = 0;
    if constexpr (FAN) {
        const MomentFanArgs &fn = mg_fan_args(f...);
        const int b = fn.b0 + g % fn.Bp, org = fn.origin[b];        // (the table was checked on the host: 0 <= org, org + steps < n)
        gq = g / fn.Bp;
        crow = org + 1;
        orow = ((size_t)gq * fn.B + b) * steps;
        srow = (size_t)gq * fn.n + org;
    }
    const int model = a.n_models == 1 ? 0 : gq;

    // 1. the state of this launch: (x_last, S0), or the state of launch t - 1 plus its slab sums
    if (t == 0) {
        if constexpr (FAN) {                                      // the filtered state at the track's origin, where the filter left it
            if (tid < D) mu[tid] = mg_fan_args(f...).m_filt[srow * D + tid];
            if (tid < D * D) Sg[tid / D][tid % D] = mg_fan_args(f...).S_filt[srow * D * D + tid];
        } else {
            if (tid < D) mu[tid] = a.x_last[(size_t)g * D + tid];
            if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[(size_t)g * D * D + tid] : 0.0;
        }
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
            if (lo == hi) v += a.variance[(size_t)model * D + lo] + exp(a.log_Q[(size_t)gq * D + lo]);
            Sg[r][c] = v;
            if constexpr (FILTER)                                 // X = Sigma + V: Cov(x_{t-2}, x_{t-1}), Sigma the filtered one
                if (writer) mg_filter_args(f...).cross[((size_t)g * steps + (t - 1)) * D * D + tid] = sp[D + tid] + fin[NP + D + c * D + r];
        }
    }
    __syncthreads();
    if (writer) {
        double *sc = a.state + ((size_t)(t & 1) * G + g) * (D + D * D);
        if (tid < D) {
            if constexpr (!FILTER) sc[tid] = mu[tid];
            if constexpr (FAN) {
                if (t > 0) a.m_x[(orow + (t - 1)) * D + tid] = mu[tid];
            } else {
                if (t > 0) a.m_x[((size_t)g * steps + (t - 1)) * D + tid] = mu[tid];
            }
        }
        if (tid < D * D) {
            const double v = Sg[tid / D][tid % D];
            if constexpr (!FILTER) sc[D + tid] = v;
            if constexpr (FAN) {
                if (t > 0) a.S_x[(orow + (t - 1)) * D * D + tid] = v;
            } else {
                if (t > 0) a.S_x[((size_t)g * steps + (t - 1)) * D * D + tid] = v;
            }
        }
    }
    if constexpr (FILTER) mg_update<D>(a, mg_filter_args(f...), t, g, writer, mu, Sg);
    if (t == steps) return;

    // 2. the three eliminations of the pair
    const double *lena = a.len + ((size_t)model * D + da) * P, *lenb = a.len + ((size_t)model * D + db) * P;
    if (tid < P) {
        xin[tid] = tid < D ? mu[tid] : a.ctrl[(size_t)(crow + t) * C + (tid - D)];
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
    const double *bea = a.beta + ((size_t)gq * D + da) * Mp, *beb = a.beta + ((size_t)gq * D + db) * Mp;
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
    const double *Gg = diag ? a.gam + ((size_t)(a.unit_per_group ? gq : model) * D + da) * Mp * Mp + (size_t)i0 * Mp : nullptr;
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

}  // namespace
}  // namespace ffvd
