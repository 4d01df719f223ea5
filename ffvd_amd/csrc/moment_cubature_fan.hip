// Rolling-origin multi-step forecasts under the third-degree spherical cubature rule ("Cubature forecasts"): the
// propagation of moment_cubature_records.hip without a measurement update, with a TRACK (group, origin) as its unit and the indexing
// of the moment fan (moment_group.h, MomentFanArgs).  Per step, with (mu, S) the state of the track, c the control row and w = 1 / (2D):
//   S = L L^T (lower, no pivoting; a pivot <= 0 gives a zero column),  dx_i = +sqrt(D) L[:, i],  dx_{i+D} = -dx_i,  x_i = [mu + dx_i, c],
//   per dim d and point i:  k_j = variance_d exp(-sum_p (x_ip - z_jp)^2 / (2 l_dp^2)),  m_d(x_i) = sum_j k_j beta_dj,
//                           v_d(x_i) = variance_d - k^T Gamma_d k,
//   mbar = w sum_i m(x_i),  Cov(f) = w sum_i (m(x_i) - mbar)(m(x_i) - mbar)^T + diag(w sum_i v(x_i)),
//   V = w sum_{i<D} dx_i (m(x_i) - m(x_{i+D}))^T,  mu' = mu + mbar,  S' = S + Cov(f) + V + V^T + diag(Q).
// The 2D kernel rows of a (track, dim) are 2D rows of the unit's K block, so the quadratic forms of all points of all tracks of a unit
// are the diagonal of K Gamma K^T: the product kernel of the linearised forecasts, unchanged (launch_mg_lfan_var).
//
// Two launches per step for all tracks of a pass:
//   mg_cfan_state_kernel (VALU, 256 threads, workgroup = (track of the pass, dim)): finishes step t - 1 from what the previous
//     launches left (the D * 2D mean sums of msum, the column-tile partials in ascending tile order, the offsets dx of `off`) --
//     redundantly in the D workgroups of a track, the same instructions on the same values; dim 0 stores row t - 1 of the forecast and
//     the state -- factors the covariance, keeps the offsets for the next finish, then writes the 2D zero-padded kernel rows of its
//     dim into K and their 2D mean sums;
//   mg_lfan_var_kernel (moment_linear_fan.hip).
// No atomics, nothing waits on another workgroup, no address depends on a computed value (the origin table is the caller's), every
// sum has a fixed order: a track does not depend on the other rows of its tile, on the other groups or on the pass it is in.
// An eighth translation unit of the family: the code of the others does not change with it.
#include "moment_group.h"
#include "kernels.h"

namespace ffvd {
namespace {

// Launch t of h + 1.  a.G: the tracks of the pass (groups * f.Bp), a.steps: the horizon, a.state: [2][tracks][D + D * D],
// l: mg_lfan_layout with 2D rows per track, l.msum: [2][tracks][D][2D], off: [2][tracks][D][D] (dx_i = column i; step parity).
template <int D>
__global__ __launch_bounds__(256) void mg_cfan_state_kernel(MomentGroupArgs a, const int t, MomentFanArgs f, MomentLinearFanArgs l,
                                                            double *off) {
    constexpr int NQ = 2 * D;
    constexpr double W = 1.0 / NQ;
    __shared__ double mu[MG_MAXD], Sg[MG_MAXD][MG_MAXD], Vm[MG_MAXD][MG_MAXD], Lm[MG_MAXD][MG_MAXD];
    __shared__ double mp[MG_MAXD][2 * MG_MAXD], qf[MG_MAXD][2 * MG_MAXD], mbar[MG_MAXD], vbar[MG_MAXD];
    __shared__ double xp[2 * MG_MAXD][MG_MAXD], xc[MAXP], il[MAXP], red[4][2 * MG_MAXD];
    const int tid = threadIdx.x;
    const int G = a.G, C = a.C, P = a.P, M = a.M, Mp = a.Mp, steps = a.steps;
    const int d = blockIdx.x % D, v = blockIdx.x / D;
    const bool writer = d == 0;
    if (t == steps && !writer) return;
    const int bl = v % f.Bp, gq = v / f.Bp, b = f.b0 + bl, org = f.origin[b];     // (the table was checked on the host: 0 <= org, org + steps < n)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = NQ * (l.shared ? v : bl);                                     // the track's first row in the K blocks of its units
    const size_t orow = ((size_t)gq * f.B + b) * steps, srow = (size_t)gq * f.n + org;

    // 1. the state of this launch: the filtered state at the origin, or the state of launch t - 1 pushed through the cubature rule
    if (t == 0) {
        if (tid < D) mu[tid] = f.m_filt[srow * D + tid];
        if (tid < D * D) Sg[tid / D][tid % D] = f.S_filt[srow * D * D + tid];
    } else {
        const double *ms = l.msum + ((size_t)((t - 1) & 1) * G + v) * D * NQ;
        if (tid < D * NQ) mp[tid / NQ][tid % NQ] = ms[tid];
        if (tid >= 128 && tid < 128 + D * NQ) {                   // the quadratic form of (dim dd, point i): column tiles in ascending order
            const int dd = (tid - 128) / NQ, i = (tid - 128) % NQ, ku = l.shared ? dd : gq * D + dd;
            const double *vp = l.vpart + (size_t)ku * l.ntj * l.Tp + row + i;
            double sum = 0.0;
            for (int tj = 0; tj < l.ntj; ++tj) sum += vp[(size_t)tj * l.Tp];
            qf[dd][i] = sum;
        }
        __syncthreads();
        const double *sp = a.state + ((size_t)((t - 1) & 1) * G + v) * (D + D * D);
        const double *op = off + ((size_t)((t - 1) & 1) * G + v) * D * D;         // the offsets the rows of launch t - 1 were built from
        const int rr = tid / D, c = tid % D;
        if (tid < D) {                                            // mbar and the mean of the variances, points in ascending order
            const double var = a.variance[(size_t)model * D + tid];
            double sm = 0.0, sv = 0.0;
#pragma unroll
            for (int i = 0; i < NQ; ++i) { sm += mp[tid][i]; sv += var - qf[tid][i]; }
            mbar[tid] = W * sm;
            vbar[tid] = W * sv;
        }
        if (tid < D * D) {                                        // V[rr][c] = Cov(x_rr, f_c)
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) s += op[rr * D + i] * (mp[c][i] - mp[c][D + i]);
            Vm[rr][c] = W * s;
        }
        __syncthreads();
        if (tid < D) mu[tid] = sp[tid] + mbar[tid];
        if (tid < D * D) {                                        // (r, c) and (c, r) run the same expression: exactly symmetric
            const int lo = rr < c ? rr : c, hi = rr < c ? c : rr;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < NQ; ++i) s += (mp[lo][i] - mbar[lo]) * (mp[hi][i] - mbar[hi]);
            double sv = (sp[D + lo * D + hi] + W * s) + (Vm[lo][hi] + Vm[hi][lo]);
            if (lo == hi) sv += vbar[lo] + exp(a.log_Q[(size_t)gq * D + lo]);
            Sg[rr][c] = sv;
        }
    }
    __syncthreads();
    if (writer) {                                                 // the state of parity t and row t - 1 of the forecast
        double *sc = a.state + ((size_t)(t & 1) * G + v) * (D + D * D);
        if (tid < D) {
            sc[tid] = mu[tid];
            if (t > 0) a.m_x[(orow + (t - 1)) * D + tid] = mu[tid];
        }
        if (tid < D * D) {
            const double s = Sg[tid / D][tid % D];
            sc[D + tid] = s;
            if (t > 0) a.S_x[(orow + (t - 1)) * D * D + tid] = s;
        }
    }
    if (t == steps) return;

    // 2. S = L L^T, thread = row, one column per round; every thread of a round forms the pivot by the same instructions
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (tid < D) {
            double p = Sg[j][j], s = Sg[tid][j];
            for (int k = 0; k < j; ++k) { p -= Lm[j][k] * Lm[j][k]; s -= Lm[tid][k] * Lm[j][k]; }
            double e = 0.0;
            if (p > 0.0 && tid >= j) {
                const double q = sqrt(p);
                e = tid == j ? q : s / q;
            }
            Lm[tid][j] = e;
        }
        __syncthreads();
    }
    // the offsets and the points; the control columns are not spread
    const double *lend = a.len + ((size_t)model * D + d) * P;
    if (tid < D * D) {
        const int p = tid / D, i = tid % D;
        const double o = sqrt((double)D) * Lm[p][i];
        xp[i][p] = mu[p] + o;
        xp[D + i][p] = mu[p] - o;
        if (writer) off[((size_t)(t & 1) * G + v) * D * D + tid] = o;
    }
    if (tid < P) {
        xc[tid] = tid < D ? 0.0 : a.ctrl[(size_t)(org + 1 + t) * C + (tid - D)];
        il[tid] = 1.0 / lend[tid];
    }
    __syncthreads();

    // 3. the 2D kernel rows of the dim, zero beyond M, and their mean sums: thread = column j, one row of Z against all points
    const double *Zm = a.Z + (size_t)model * M * P;
    const double *bed = a.beta + ((size_t)gq * D + d) * Mp;
    const double var = a.variance[(size_t)model * D + d];
    double *Kr = l.K + ((size_t)(l.shared ? d : gq * D + d) * l.Tp + row) * Mp;
    double acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
    for (int j = tid; j < Mp; j += 256) {
        const bool live = j < M;
        const double *z = Zm + (size_t)(live ? j : 0) * P;        // (a padding column reads row 0 and writes zeros)
        double zs[D], cc = 0.0;
#pragma unroll
        for (int p = 0; p < D; ++p) zs[p] = z[p];
        for (int p = D; p < P; ++p) {
            const double u = (z[p] - xc[p]) * il[p];
            cc += u * u;
        }
        const double be = live ? bed[j] : 0.0, vk = live ? var : 0.0;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            double c = 0.0;
#pragma unroll
            for (int p = 0; p < D; ++p) {
                const double u = (zs[p] - xp[i][p]) * il[p];
                c += u * u;
            }
            const double k = vk * exp(-0.5 * (c + cc));
            acc[i] += k * be;
            Kr[(size_t)i * Mp + j] = k;
            __builtin_amdgcn_sched_barrier(0);                    // one point at a time: the 2D exps interleaved cost 256 VGPRs at D = 8
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
    if (tid < NQ)
        l.msum[(((size_t)(t & 1) * G + v) * D + d) * NQ + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace

// a.G: the tracks of the pass (groups * f.Bp); l: mg_lfan_layout of the pass with 2D rows per track and its buffers
void launch_mg_cfan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFanArgs &f, const MomentLinearFanArgs &l, double *off,
                         int t) {
    const dim3 grid((unsigned)((size_t)a.G * a.D));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_cfan_state_kernel<d>), grid, dim3(256), 0, stream, a, t, f, l, off))
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

}  // namespace ffvd
