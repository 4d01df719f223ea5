// Linearised (extended Kalman) filtering of many observed records in one call ("Filtering many records"): the
// filter of moment_linear.hip with a TRACK (group g, record r) as its unit and the launch pair of the linearised forecasts
// (moment_linear_fan.hip).  Every track is an independent filter: it runs on the posterior of its group, reads the observations, the
// control rows and the start state of its own record, and takes a measurement update (mg_update, moment_step.h) at every step.  Per
// step and (track, dim d), with x = [mu_filt, c_row]:
//   k_j = variance_d exp(-sum_p (x_p - z_jp)^2 / (2 l_dp^2)),  nu_jp = z_jp - x_p,
//   m_d = sum_j k_j beta_dj,  J_dp = (1 / l_dp^2) sum_j k_j beta_dj nu_jp (p < D),  v_d = variance_d - k^T Gamma_d k,
//   m^- = mu + m,  S^- = A S A^T + diag(v + Q),  cross = S A^T,  A = I + J.
// The tracks of a group share beta and Gamma, so the quadratic forms of all tracks of a unit are the diagonal of K Gamma K^T: the
// product kernel of the forecasts, unchanged (launch_mg_lfan_var), reads Gamma once per 128 tracks where a loop over the records
// reads it once per record.
//
// Two launches per step for all tracks of a pass:
//   mg_lrec_state_kernel (VALU, 256 threads, workgroup = (track of the pass, dim)): finishes step t - 1 from the sums the previous
//     launches left (msum, and the column-tile partials in ascending tile order), stores m_pred, S_pred and cross of row t - 1, runs
//     the measurement update with row t - 1 of its own record -- redundantly in the D workgroups of a track, the same instructions
//     on the same values; dim 0 stores -- then writes the zero-padded kernel row of its dim into K and the D + 1 sums of the mean side;
//   mg_lfan_var_kernel (moment_linear_fan.hip).
// No atomics, nothing waits on another workgroup, no address depends on a computed value, every sum has a fixed order: a track does
// not depend on the other rows of its tile, on the other groups, on the other records or on the pass it is in.
// A sixth translation unit of the family: the code of the propagation, the filters and the fans does not change with it.
#include "moment_step.h"

namespace ffvd {
namespace {

// Launch t of steps + 1.  a.G: the tracks of the pass (groups * rc.Rp), a.state: [2][tracks][D + D * D] (the FILTERED state).
template <int D>
__global__ __launch_bounds__(256) void mg_lrec_state_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentRecordArgs rc,
                                                            MomentLinearFanArgs l) {
    constexpr int NFD = D + 2;
    __shared__ double mu[MG_MAXD], Sg[MG_MAXD][MG_MAXD], Am[MG_MAXD][MG_MAXD], SA[MG_MAXD][MG_MAXD], fin[MG_MAXD * (MG_MAXD + 2)];
    __shared__ double xin[MAXP], il[MAXP], red[4][MG_MAXD + 1];
    const int tid = threadIdx.x;
    const int G = a.G, C = a.C, P = a.P, M = a.M, Mp = a.Mp, steps = a.steps;
    const int d = blockIdx.x % D, v = blockIdx.x / D;
    const bool writer = d == 0;
    if (t == steps && !writer) return;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;                     // (r < R: the host sizes the passes)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = l.shared ? v : bl;                                            // the track's row in the K blocks of its units
    const size_t vg = (size_t)gq * rc.R + r, orow = vg * steps;                   // the track of the call; its first row in the stacks

    // 1. the state of this launch: the record's start, or the filtered state of launch t - 1 pushed through its linearisation
    if (t == 0) {
        if (tid < D) mu[tid] = a.x_last[vg * D + tid];
        if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[vg * D * D + tid] : 0.0;
    } else {
        const double *ms = l.msum + ((size_t)((t - 1) & 1) * G + v) * D * (D + 1);
        if (tid < D * (D + 1)) fin[(tid / (D + 1)) * NFD + tid % (D + 1)] = ms[tid];
        if (tid >= 64 && tid < 64 + D) {                          // the quadratic form of dim dd: column tiles in ascending order
            const int dd = tid - 64, ku = l.shared ? dd : gq * D + dd;
            const double *vp = l.vpart + (size_t)ku * l.ntj * l.Tp + row;
            double sum = 0.0;
            for (int tj = 0; tj < l.ntj; ++tj) sum += vp[(size_t)tj * l.Tp];
            fin[dd * NFD + D + 1] = sum;
        }
        __syncthreads();
        const double *sp = a.state + ((size_t)((t - 1) & 1) * G + v) * (D + D * D);
        const int rr = tid / D, c = tid % D;
        if (tid < D * D) {                                        // A = I + J, row = dim of f
            const double ll = a.len[((size_t)model * D + rr) * P + c];
            Am[rr][c] = (1.0 / (ll * ll)) * fin[rr * NFD + 1 + c] + (rr == c ? 1.0 : 0.0);
        }
        if (tid < D) mu[tid] = sp[tid] + fin[tid * NFD];
        __syncthreads();
        if (tid < D * D) {                                        // S A^T = Cov(x_{t-2}, x_{t-1}), S the filtered one
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += sp[D + rr * D + k] * Am[c][k];
            SA[rr][c] = s;
            if (writer) f.cross[(orow + (t - 1)) * D * D + tid] = s;
        }
        __syncthreads();
        if (tid < D * D) {                                        // (r, c) and (c, r) run the same expression: exactly symmetric
            const int lo = rr < c ? rr : c, hi = rr < c ? c : rr;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += Am[lo][k] * SA[k][hi];
            if (lo == hi) s += (a.variance[(size_t)model * D + lo] - fin[lo * NFD + D + 1]) + exp(a.log_Q[(size_t)gq * D + lo]);
            Sg[rr][c] = s;
        }
    }
    __syncthreads();
    if (writer && t > 0) {                                        // the predicted moments of row t - 1
        if (tid < D) a.m_x[(orow + (t - 1)) * D + tid] = mu[tid];
        if (tid < D * D) a.S_x[(orow + (t - 1)) * D * D + tid] = Sg[tid / D][tid % D];
    }
    // mg_update indexes the stacks and the state by one unit g: it is handed the track of the pass (the state's index) and a copy of the
    // filter's arguments whose stacks start at the rows of the call's track minus those of the pass's, and whose Y is the record's
    {
        MomentFilterArgs fu = f;
        const size_t off = (vg - (size_t)v) * steps;              // (vg >= v: R >= Rp and r >= bl)
        fu.Y = f.Y + (size_t)r * steps * f.J;
        fu.m_filt = f.m_filt + off * D;
        fu.S_filt = f.S_filt + off * D * D;
        fu.lpd = f.lpd + off * f.J;
        fu.lpd_joint = f.lpd_joint + off;
        mg_update<D>(a, fu, t, v, writer, mu, Sg);
    }
    if (t == steps) return;

    // 2. the kernel row of the dim at x = [mu, c_row], zero beyond M, and the mean side's D + 1 sums: thread = column j
    const double *lend = a.len + ((size_t)model * D + d) * P;
    if (tid < P) {
        xin[tid] = tid < D ? mu[tid] : a.ctrl[((size_t)r * steps + t) * C + (tid - D)];
        il[tid] = 1.0 / lend[tid];
    }
    __syncthreads();
    const double *Zm = a.Z + (size_t)model * M * P;
    const double *bed = a.beta + ((size_t)gq * D + d) * Mp;
    const double var = a.variance[(size_t)model * D + d];
    double *Krow = l.K + ((size_t)(l.shared ? d : gq * D + d) * l.Tp + row) * Mp;
    double acc[D + 1];
#pragma unroll
    for (int p = 0; p <= D; ++p) acc[p] = 0.0;
    for (int j = tid; j < Mp; j += 256) {
        double k = 0.0;
        if (j < M) {
            const double *z = Zm + (size_t)j * P;
            double c = 0.0;
            for (int p = 0; p < P; ++p) {
                const double u = (z[p] - xin[p]) * il[p];
                c += u * u;
            }
            k = var * exp(-0.5 * c);
            const double kb = k * bed[j];
            acc[0] += kb;
#pragma unroll
            for (int p = 0; p < D; ++p) acc[1 + p] += kb * (z[p] - xin[p]);                // nu formed per element
        }
        Krow[j] = k;
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int p = 0; p <= D; ++p) {
        double s = acc[p];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s += __shfl_xor(s, mm);
        if (lane == 0) red[wave][p] = s;
    }
    __syncthreads();
    if (tid <= D)
        l.msum[(((size_t)(t & 1) * G + v) * D + d) * (D + 1) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void mg_lrec_spread_kernel(int R, int n, size_t total, const double *src, double *dst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) dst[e] = src[e / ((size_t)R * n) * n + e % n];
}

}  // namespace

// a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout of the pass with its buffers
void launch_mg_lrec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, int t) {
    const dim3 grid((unsigned)((size_t)a.G * a.D));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_lrec_state_kernel<d>), grid, dim3(256), 0, stream, a, t, f, rc, l))
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

void launch_mg_lrec_spread(hipStream_t stream, int G, int R, int n, const double *src, double *dst) {
    const size_t total = (size_t)G * R * n;
    if (total == 0) return;
    hipLaunchKernelGGL(mg_lrec_spread_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, R, n, total, src, dst);
}

}  // namespace ffvd
