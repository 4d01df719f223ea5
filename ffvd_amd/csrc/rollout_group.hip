// Grouped posterior rollouts: the prediction loop of collect_samples_formal (base_model.py:223-314) for G INDEPENDENT posteriors --
// one per SG-HMC sample (cases 2/3/5) or per chain -- each with its own W = L^-T stack, Z, hyper-parameters, U, q_sqrt slice, Q and
// start state.  ffvd_op_rollout advances the rollouts of ONE posterior; G posteriors were G calls, one after another.
//
// Shape of the launch.  A step of a group is cut into a FIXED set of workgroups that meet only at kernel boundaries:
//   workgroup (g, d, s, c) owns the 16 columns [16 s, 16 s + 16) of dim d's W (and of B = W q0) of group g and the chunk c of 8 rollouts
//   (of 1 when R = 1).
// Launch t (t = 0 .. steps) does, in every workgroup of group g:
//   1. (t > 0) finish step t - 1 for its 8 rollouts and ALL dims: add the slab sums of launch t - 1 in slab order, f_var = Kdiag - sum F^2
//      (+ sum E^2), x_t = x_{t-1} + f_mu + eps sqrt(f_var + Q).  Every workgroup of a group forms the same x_t with the same
//      instructions in the same order (a few hundred adds); the workgroup (d = 0, s = 0) also stores it, with predict_x / predict_var.
//   2. (t < steps) k = K_d([x_t, ctrl_t], Z_g) for the rows its columns need -- W is upper triangular: rows m < 16 (s + 1), the strict
//      lower triangle is never read -- 256 rows at a time into LDS; F = k W, E = k B for its 16 columns (16-byte loads, a row
//      segment of 128 bytes per 8 lanes); sum F^2, sum F u, sum E^2 of the slab -> part[t & 1].
// One launch per step for ALL groups; nothing waits on another workgroup, nothing needs to be resident, there is no second form.
// The decomposition of a group depends on (M, D, R) only -- not on G, not on the group's index, not on which compute units are
// free -- and every sum has a fixed order: a group's results are bit-identical alone or among others, and run to run.
//
// f_var + Q <= 0 (or NaN): sqrt gives NaN, which propagates through the following steps of that rollout (as in ffvd_op_rollout);
// no address depends on a computed value, nothing faults.
#include "rollout_group.h"
#include "kernels.h"
#include "dev_common.h"

#include <type_traits>

namespace ffvd {

__global__ __launch_bounds__(256) void rg_prep_kernel(int kind, int D, int M, int Mp, int P, const double *Z, const double *logvar,
                                                      const double *loglen, double *variance, double *len, double *Zs, double *zz) {
    __shared__ double ls[MAXP];
    const int gd = blockIdx.x, g = gd / D, tid = threadIdx.x;
    if (tid == 0) variance[gd] = exp(logvar[gd]);
    if (tid < P) {
        const double l = (kind == 0) ? exp(loglen[(size_t)gd * P + tid]) : 1.0;
        ls[tid] = l;
        len[(size_t)gd * P + tid] = l;
    }
    __syncthreads();
    const double *Zg = Z + (size_t)g * M * P;
    for (int m = tid; m < Mp; m += 256) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) {
            const double v = (m < M) ? Zg[(size_t)m * P + p] / ls[p] : 0.0;
            Zs[((size_t)gd * Mp + m) * P + p] = v;
            s += v * v;
        }
        zz[(size_t)gd * Mp + m] = s;
    }
}
void launch_rg_prep(hipStream_t stream, int kind, int G, int D, int M, int Mp, int P, const double *Z, const double *logvar,
                    const double *loglen, double *variance, double *len, double *Zs, double *zz) {
    hipLaunchKernelGGL(rg_prep_kernel, dim3(G * D), dim3(256), 0, stream, kind, D, M, Mp, P, Z, logvar, loglen, variance, len, Zs, zz);
}

// B = W q0 per (group, dim) on the matrix cores: a wavefront forms 16 rows x 64 columns; the contraction starts at the tile's first
// row (W is upper triangular) and, when q0 is upper triangular as well, ends with the tile's last column.
__global__ __launch_bounds__(256) void rg_wq_kernel(int D, int Mp, int q_upper, const double *W, const double *q0, double *B) {
    const int ncb = (Mp + 63) / 64;
    const int cb = blockIdx.x % ncb, b = blockIdx.x / ncb, g = b / D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int ti = blockIdx.y * 4 + wave;
    if (ti * 16 >= Mp) return;
    const int c0 = cb * 64, ntile = (Mp - c0) / 16 < 4 ? (Mp - c0) / 16 : 4;
    const double *Wb = W + (size_t)b * Mp * Mp, *qg = q0 + (size_t)g * Mp * Mp;
    double *Bb = B + (size_t)b * Mp * Mp;
    const int kbeg = 16 * ti, kend = q_upper ? (c0 + 64 < Mp ? c0 + 64 : Mp) : Mp;
    d4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int m0 = kbeg; m0 < kend; m0 += 4) {
        const double av = Wb[(size_t)(16 * ti + lr) * Mp + m0 + lk];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < ntile) acc[c] = mfma_f64(av, qg[(size_t)(m0 + lk) * Mp + c0 + 16 * c + lr], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < ntile) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Bb[(size_t)(16 * ti + lk + 4 * r) * Mp + c0 + 16 * c + lr] = acc[c][r];
        }
}
void launch_rg_wq(hipStream_t stream, int G, int D, int Mp, int q_upper, const double *W, const double *q0, double *B) {
    const int ncb = (Mp + 63) / 64;
    hipLaunchKernelGGL(rg_wq_kernel, dim3(G * D * ncb, ncb), dim3(256), 0, stream, D, Mp, q_upper, W, q0, B);
}

template <int KIND, int RC>
__global__ __launch_bounds__(256) void rg_step_kernel(RolloutGroupArgs a, const int t) {
    __shared__ double xraw[RC][MAXP];                                   // [x_t, ctrl_t] of the chunk's rollouts
    __shared__ double xs[RC][MAXP];                                     // the same, scaled for dim d
    __shared__ double xxs[RC];
    __shared__ __attribute__((aligned(16))) double kt[RG_MT][RC];       // K(x_t, z_m): 256 rows at a time
    __shared__ double red[4][2][RC][RG_SLAB];
    const int tid = threadIdx.x;
    const int G = a.G, R = a.R, D = a.D, C = a.C, P = a.P, M = a.M, Mp = a.Mp, NS = a.NS, steps = a.steps;
    const int s = blockIdx.x % NS, gd = blockIdx.x / NS, d = gd % D, g = gd / D;
    const int r0 = blockIdx.y * RC, nr = (R - r0 < RC) ? R - r0 : RC;
    const bool writer = (d == 0 && s == 0);
    if (t == steps && !writer) return;

    // 1. the states of this launch: x_0 = x_last, x_t = x_{t-1} + f_mu + eps sqrt(f_var + Q) from the slab sums of launch t - 1
    if (tid < RC * D) {
        const int rr = tid / D, dd = tid % D, r = r0 + rr;
        double x = 0.0;
        if (rr < nr) {
            double *xcur = a.xbuf + ((size_t)(t & 1) * G * R + (size_t)g * R + r) * D;
            if (t == 0) x = a.x_last[(size_t)g * D + dd];
            else {
                const double *xprev = a.xbuf + ((size_t)((t - 1) & 1) * G * R + (size_t)g * R + r) * D;
                const double *pp = a.part + ((((size_t)((t - 1) & 1) * G + g) * D + dd) * NS * R + r) * 4;
                double rs = 0.0, fm = 0.0, ex = 0.0;
                for (int sl = 0; sl < NS; ++sl) {                            // slab order, the same in every workgroup of the group
                    const double *q = pp + (size_t)sl * R * 4;
                    rs += q[0]; fm += q[1]; ex += q[2];
                }
                const double var = a.variance[(size_t)g * D + dd];
                double kd = var;
                if (KIND == 1) {
                    kd = 0.0;
                    for (int p = 0; p < P; ++p) {
                        const double xv = (p < D) ? xprev[p] : a.ctrl[(size_t)(t - 1) * C + (p - D)];
                        kd += (xv * xv) * var;
                    }
                }
                double vv = kd - rs;
                if (a.has_q) vv = vv + ex;
                const double v = vv + exp(a.log_Q[(size_t)g * D + dd]);
                x = (fm + xprev[dd]) + a.eps[(((size_t)(t - 1) * G + g) * R + r) * D + dd] * sqrt(v);
                if (writer) {
                    const size_t o = (((size_t)g * R + r) * steps + (t - 1)) * D + dd;
                    a.predict_x[o] = x;
                    a.predict_var[o] = v;
                }
            }
            if (writer) xcur[dd] = x;
        }
        xraw[rr][dd] = x;
    }
    if (t == steps) return;
    for (int e = tid; e < RC * C; e += 256) xraw[e / C][D + e % C] = a.ctrl[(size_t)t * C + e % C];
    __syncthreads();
    const double var = a.variance[gd];
    for (int e = tid; e < RC * P; e += 256) {
        const int rr = e / P, p = e % P;
        const double v = xraw[rr][p];
        xs[rr][p] = (KIND == 0) ? v / a.len[(size_t)gd * P + p] : v * var;
    }
    __syncthreads();
    if (tid < RC) {
        double xx = 0.0;
        if (KIND == 0)
            for (int p = 0; p < P; ++p) xx += xs[tid][p] * xs[tid][p];
        xxs[tid] = xx;
    }
    __syncthreads();

    // 2. F = k W and E = k B for this slab's 16 columns; thread = (column pair jp, part mq of 32 of the contraction)
    const int j0 = RG_SLAB * s, jp = tid & 7, mq = tid >> 3;
    const int mlimW = j0 + RG_SLAB, mlimB = a.has_q ? (a.q_upper ? mlimW : Mp) : 0, mend = mlimW > mlimB ? mlimW : mlimB;
    const double *Wd = a.W + (size_t)gd * Mp * Mp + j0 + 2 * jp;
    const double *Bd = a.has_q ? a.B + (size_t)gd * Mp * Mp + j0 + 2 * jp : nullptr;
    double accW[RC][2], accE[RC][2];
#pragma unroll
    for (int r = 0; r < RC; ++r) { accW[r][0] = accW[r][1] = 0.0; accE[r][0] = accE[r][1] = 0.0; }
    for (int m0 = 0; m0 < mend; m0 += RG_MT) {
        {
            const int m = m0 + tid;
            double dot[RC];
#pragma unroll
            for (int r = 0; r < RC; ++r) dot[r] = 0.0;
            const bool live = m < mend && m < M;
            if (live) {
                const double *zr = a.Zs + ((size_t)gd * Mp + m) * P;
                for (int p = 0; p < P; ++p) {
                    const double z = zr[p];
#pragma unroll
                    for (int r = 0; r < RC; ++r) dot[r] += xs[r][p] * z;
                }
            }
            const double zzm = live ? a.zz[(size_t)gd * Mp + m] : 0.0;
#pragma unroll
            for (int r = 0; r < RC; ++r) kt[tid][r] = live ? kernel_value<KIND>(dot[r], xxs[r], zzm, var) : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int i = 0; i < RG_MT / 32; ++i) {
            const int ml = mq + 32 * i, m = m0 + ml;
            if (m < mend) {
                double k[RC];
#pragma unroll
                for (int r = 0; r < RC; ++r) k[r] = kt[ml][r];
                if (m < mlimW) {
                    const double2 w = *reinterpret_cast<const double2 *>(Wd + (size_t)m * Mp);
#pragma unroll
                    for (int r = 0; r < RC; ++r) { accW[r][0] += k[r] * w.x; accW[r][1] += k[r] * w.y; }
                }
                if (m < mlimB) {
                    const double2 w = *reinterpret_cast<const double2 *>(Bd + (size_t)m * Mp);
#pragma unroll
                    for (int r = 0; r < RC; ++r) { accE[r][0] += k[r] * w.x; accE[r][1] += k[r] * w.y; }
                }
            }
        }
        __syncthreads();
    }
    // the 32 parts of the contraction: 8 inside a wavefront (lanes 8 apart), then the 4 wavefronts in order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < RC; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int mm = 8; mm < 64; mm <<= 1) { accW[r][c] += __shfl_xor(accW[r][c], mm); accE[r][c] += __shfl_xor(accE[r][c], mm); }
        }
    if (lane < 8) {
#pragma unroll
        for (int r = 0; r < RC; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) { red[wave][0][r][2 * jp + c] = accW[r][c]; red[wave][1][r][2 * jp + c] = accE[r][c]; }
    }
    __syncthreads();
    if (tid < RC * RG_SLAB) {
        const int rr = tid >> 4, j = tid & 15;
        const double F = ((red[0][0][rr][j] + red[1][0][rr][j]) + red[2][0][rr][j]) + red[3][0][rr][j];
        const double E = ((red[0][1][rr][j] + red[1][1][rr][j]) + red[2][1][rr][j]) + red[3][1][rr][j];
        const double uj = (j0 + j < M) ? a.f[((size_t)g * M + j0 + j) * D + d] : 0.0;
        double rs = F * F, fm = F * uj, ex = E * E;
#pragma unroll
        for (int mm = 1; mm < 16; mm <<= 1) { rs += __shfl_xor(rs, mm); fm += __shfl_xor(fm, mm); ex += __shfl_xor(ex, mm); }
        if (j == 0 && rr < nr) {
            double *pp = a.part + (((((size_t)(t & 1) * G + g) * D + d) * NS + s) * R + r0 + rr) * 4;
            pp[0] = rs; pp[1] = fm; pp[2] = ex;
        }
    }
}

void launch_rg_step(hipStream_t stream, const RolloutGroupArgs &a, int t) {
    // rollouts per workgroup: 8, or 1 for a single rollout per group (the per-sample case: no work on empty slots).  A function of R only.
    auto go = [&](auto kind, auto rc) {
        constexpr int RC = decltype(rc)::value;
        const dim3 grid(a.G * a.D * a.NS, (a.R + RC - 1) / RC);
        hipLaunchKernelGGL((rg_step_kernel<decltype(kind)::value, RC>), grid, dim3(256), 0, stream, a, t);
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I8 = std::integral_constant<int, RG_RC>;
    if (a.kind == 0) { if (a.R == 1) go(I0{}, I1{}); else go(I0{}, I8{}); }
    else { if (a.R == 1) go(I1{}, I1{}); else go(I1{}, I8{}); }
}

}  // namespace ffvd
