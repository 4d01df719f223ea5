// Linearised (extended Kalman) filtering through the GP ("Linearised filtering"): the second propagation rule
// of the filter family.  The transition is linearised at the filtered mean: with x = [mu, c_t] and, per latent dim d,
//   k_j = variance_d exp(-sum_p (x_p - z_jp)^2 / (2 l_dp^2)),  nu_jp = z_jp - x_p,
//   m_d = sum_j k_j beta_dj,  J_dp = (1 / l_dp^2) sum_j k_j beta_dj nu_jp (p < D),  v_d = variance_d - sum_i k_i (Gamma_d k)_i,
// the predicted state is mu + m, A S A^T + diag(v + Q) with A = I + J, and Cov(x_{t-1}, x_t) = S A^T.  The launch protocol, the
// measurement update (mg_update), the stores and the smoother are those of the moment-matched filter (moment_step.h,
// moment_filter.hip).  A fourth translation unit: the code of the propagation, of the filter and of the fan does not change with it.
//
// Workgroup (group g, dim d, slab s of MG_SLAB rows of Gamma_d), 256 threads.  Every workgroup forms the whole kernel row k of its
// dim in LDS (thread = column j), then its slab's D + 2 sums (moment_group.h, mg_linear_fields): the quadratic form with thread =
// column j and the slab's rows outer (coalesced reads of Gamma), reduced by wavefront shuffles and then the four wavefronts through
// LDS in fixed order; the D + 1 sums of the mean side over the slab's rows in ascending order by one thread each.  The prologue of
// launch t + 1 adds the slab sums in ascending slab order, redundantly in every workgroup of the group.  No atomics, nothing waits
// on another workgroup, every sum has a fixed order: a group's output does not depend on G or on the other groups.
#include "moment_step.h"

namespace ffvd {
namespace {

template <int D>
__global__ __launch_bounds__(256) void mg_linear_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f) {
    constexpr int NFD = D + 2, NF = D * NFD;
    __shared__ double mu[MG_MAXD], Sg[MG_MAXD][MG_MAXD], Am[MG_MAXD][MG_MAXD], SA[MG_MAXD][MG_MAXD], fin[MG_MAXD * (MG_MAXD + 2)];
    __shared__ double xin[MAXP], il[MAXP], ks[MG_LINEAR_MAXM], kbi[MG_SLAB], nui[MG_SLAB][MG_MAXD], red[4];
    const int tid = threadIdx.x;
    const int G = a.G, C = a.C, P = a.P, M = a.M, Mp = a.Mp, NS = a.NS, steps = a.steps;
    const int s = blockIdx.x % NS, gd = blockIdx.x / NS, d = gd % D, g = gd / D;
    const bool writer = (d == 0 && s == 0);
    if (t == steps && !writer) return;
    const int model = a.n_models == 1 ? 0 : g;

    // 1. the state of this launch: (x_last, S0), or the filtered state of launch t - 1 pushed through its linearisation
    if (t == 0) {
        if (tid < D) mu[tid] = a.x_last[(size_t)g * D + tid];
        if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[(size_t)g * D * D + tid] : 0.0;
    } else {
        const double *pp = a.part + ((size_t)((t - 1) & 1) * G + g) * NF * NS;
        if (tid < NF) {
            double sum = 0.0;
            for (int sl = 0; sl < NS; ++sl) sum += pp[(size_t)tid * NS + sl];              // slab order, the same in every workgroup
            fin[tid] = sum;
        }
        __syncthreads();
        const double *sp = a.state + ((size_t)((t - 1) & 1) * G + g) * (D + D * D);
        const int r = tid / D, c = tid % D;
        if (tid < D * D) {                                        // A = I + J, row = dim of f
            const double l = a.len[((size_t)model * D + r) * P + c];
            Am[r][c] = (1.0 / (l * l)) * fin[r * NFD + 1 + c] + (r == c ? 1.0 : 0.0);
        }
        if (tid < D) mu[tid] = sp[tid] + fin[tid * NFD];
        __syncthreads();
        if (tid < D * D) {                                        // S A^T = Cov(x_{t-2}, x_{t-1}), S the filtered one
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) v += sp[D + r * D + k] * Am[c][k];
            SA[r][c] = v;
            if (writer) f.cross[((size_t)g * steps + (t - 1)) * D * D + tid] = v;
        }
        __syncthreads();
        if (tid < D * D) {                                        // (r, c) and (c, r) run the same expression: exactly symmetric
            const int lo = r < c ? r : c, hi = r < c ? c : r;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) v += Am[lo][k] * SA[k][hi];
            if (lo == hi) v += (a.variance[(size_t)model * D + lo] - fin[lo * NFD + D + 1]) + exp(a.log_Q[(size_t)g * D + lo]);
            Sg[r][c] = v;
        }
    }
    __syncthreads();
    if (writer && t > 0) {                                        // the predicted moments of row t - 1
        if (tid < D) a.m_x[((size_t)g * steps + (t - 1)) * D + tid] = mu[tid];
        if (tid < D * D) a.S_x[((size_t)g * steps + (t - 1)) * D * D + tid] = Sg[tid / D][tid % D];
    }
    mg_update<D>(a, f, t, g, writer, mu, Sg);
    if (t == steps) return;

    // 2. the kernel row of the dim at x = [mu, c_t]
    const double *lend = a.len + ((size_t)model * D + d) * P;
    if (tid < P) {
        xin[tid] = tid < D ? mu[tid] : a.ctrl[(size_t)t * C + (tid - D)];
        il[tid] = 1.0 / lend[tid];
    }
    __syncthreads();
    const double *Zm = a.Z + (size_t)model * M * P;
    const double var = a.variance[(size_t)model * D + d];
    for (int j = tid; j < M; j += 256) {
        const double *z = Zm + (size_t)j * P;
        double c = 0.0;
        for (int p = 0; p < P; ++p) {
            const double u = (z[p] - xin[p]) * il[p];
            c += u * u;
        }
        ks[j] = var * exp(-0.5 * c);
    }
    __syncthreads();

    // 3. the mean side of the slab's rows: k_i beta_i and nu_ip per row, then one thread per sum, rows ascending
    const int i0 = MG_SLAB * s, ni = (M - i0 < MG_SLAB) ? M - i0 : MG_SLAB;
    const double *bed = a.beta + ((size_t)g * D + d) * Mp;
    if (tid < ni) {
        kbi[tid] = ks[i0 + tid] * bed[i0 + tid];
#pragma unroll
        for (int p = 0; p < D; ++p) nui[tid][p] = Zm[(size_t)(i0 + tid) * P + p] - xin[p];         // formed per element
    }
    __syncthreads();
    double *po = a.part + ((size_t)(t & 1) * G + g) * NF * NS + (size_t)d * NFD * NS + s;
    if (tid >= 64 && tid < 64 + D + 1) {                          // (wavefront 1: wavefront 0 ends the reduction below)
        const int p = tid - 65;
        double m = 0.0;
        for (int i = 0; i < ni; ++i) m += p < 0 ? kbi[i] : kbi[i] * nui[i][p];
        po[(size_t)(tid - 64) * NS] = m;
    }

    // 4. the slab of the quadratic form: thread = column j, the slab's rows outer
    const double *Gg = a.gam + ((size_t)(a.unit_per_group ? g : model) * D + d) * Mp * Mp + (size_t)i0 * Mp;
    double acc = 0.0;
    for (int j = tid; j < M; j += 256) {
        const double kj = ks[j];
        double gv[MG_SLAB];
#pragma unroll
        for (int i = 0; i < MG_SLAB; ++i) gv[i] = Gg[(size_t)(i < ni ? i : 0) * Mp + j];          // (row 0 again beyond the slab's end)
#pragma unroll
        for (int i = 0; i < MG_SLAB; ++i)
            if (i < ni) acc += ks[i0 + i] * (gv[i] * kj);
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int mm = 32; mm > 0; mm >>= 1) acc += __shfl_xor(acc, mm);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) po[(size_t)(D + 1) * NS] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

void launch_mg_linear_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, int t) {
    const dim3 grid((unsigned)((size_t)a.G * a.D * a.NS));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_linear_kernel<d>), grid, dim3(256), 0, stream, a, t, f))
}

}  // namespace ffvd
