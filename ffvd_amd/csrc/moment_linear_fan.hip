// Rolling-origin multi-step forecasts under the linearised (extended Kalman) rule ("Linearised forecasts"): the
// propagation of moment_linear.hip without a measurement update, with a TRACK (group, origin) as its unit and the indexing of the
// moment fan (moment_group.h, MomentFanArgs).  Per step and (track, dim d):
//   k_j = variance_d exp(-sum_p (x_p - z_jp)^2 / (2 l_dp^2)),  nu_jp = z_jp - x_p,  x = [mu, c_row],
//   m_d = sum_j k_j beta_dj,  J_dp = (1 / l_dp^2) sum_j k_j beta_dj nu_jp (p < D),  v_d = variance_d - k^T Gamma_d k,
//   mu' = mu + m,  S' = A S A^T + diag(v + Q),  A = I + J.
// The tracks of a group share beta and Gamma, so the quadratic forms of all tracks of a unit are the diagonal of K Gamma K^T with K
// (tracks x Mp) the stacked kernel rows: a dense product on v_mfma_f64_16x16x4_f64 that reads Gamma once per 128 tracks.
//
// Two launches per step for all tracks of a pass:
//   mg_lfan_state_kernel (VALU, 256 threads, workgroup = (track, dim)): finishes step t - 1 from the sums the previous launches left
//     (redundantly in the D workgroups of a track, the same instructions on the same values; dim 0 stores), then writes the
//     zero-padded kernel row of its dim into K and the D + 1 sums of the mean side;
//   mg_lfan_var_kernel (fp64 MFMA, 512 threads, workgroup = one 128 x 128 tile of T = K Gamma of one unit): tg_var_kernel's main
//     loop (gemm_rowmajor_a) and tile order, an epilogue that keeps sum_j k_nj t_nj per column tile, so T never reaches memory.
// No atomics, nothing waits on another workgroup, no address depends on a computed value (the origin table is the caller's), every
// sum has a fixed order: a track does not depend on the other rows of its tile, on the other groups or on the pass it is in.
// A fifth translation unit of the family: the code of the propagation, the filters and the moment fan does not change with it.
#include "moment_group.h"
#include "kernels.h"
#include "gemm_rowmajor.h"

namespace ffvd {
namespace {

// Launch t of h + 1.  a.G: the tracks of the pass (groups * f.Bp), a.steps: the horizon, a.state: [2][tracks][D + D * D].
template <int D>
__global__ __launch_bounds__(256) void mg_lfan_state_kernel(MomentGroupArgs a, const int t, MomentFanArgs f, MomentLinearFanArgs l) {
    constexpr int NFD = D + 2;
    __shared__ double mu[MG_MAXD], Sg[MG_MAXD][MG_MAXD], Am[MG_MAXD][MG_MAXD], SA[MG_MAXD][MG_MAXD], fin[MG_MAXD * (MG_MAXD + 2)];
    __shared__ double xin[MAXP], il[MAXP], red[4][MG_MAXD + 1];
    const int tid = threadIdx.x;
    const int G = a.G, C = a.C, P = a.P, M = a.M, Mp = a.Mp, steps = a.steps;
    const int d = blockIdx.x % D, v = blockIdx.x / D;
    const bool writer = d == 0;
    if (t == steps && !writer) return;
    const int bl = v % f.Bp, gq = v / f.Bp, b = f.b0 + bl, org = f.origin[b];     // (the table was checked on the host: 0 <= org, org + steps < n)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = l.shared ? v : bl;                                            // the track's row in the K blocks of its units
    const size_t orow = ((size_t)gq * f.B + b) * steps, srow = (size_t)gq * f.n + org;

    // 1. the state of this launch: the filtered state at the origin, or the state of launch t - 1 pushed through its linearisation
    if (t == 0) {
        if (tid < D) mu[tid] = f.m_filt[srow * D + tid];
        if (tid < D * D) Sg[tid / D][tid % D] = f.S_filt[srow * D * D + tid];
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
        const int r = tid / D, c = tid % D;
        if (tid < D * D) {                                        // A = I + J, row = dim of f
            const double ll = a.len[((size_t)model * D + r) * P + c];
            Am[r][c] = (1.0 / (ll * ll)) * fin[r * NFD + 1 + c] + (r == c ? 1.0 : 0.0);
        }
        if (tid < D) mu[tid] = sp[tid] + fin[tid * NFD];
        __syncthreads();
        if (tid < D * D) {                                        // S A^T
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += sp[D + r * D + k] * Am[c][k];
            SA[r][c] = s;
        }
        __syncthreads();
        if (tid < D * D) {                                        // (r, c) and (c, r) run the same expression: exactly symmetric
            const int lo = r < c ? r : c, hi = r < c ? c : r;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += Am[lo][k] * SA[k][hi];
            if (lo == hi) s += (a.variance[(size_t)model * D + lo] - fin[lo * NFD + D + 1]) + exp(a.log_Q[(size_t)gq * D + lo]);
            Sg[r][c] = s;
        }
    }
    __syncthreads();
    if (writer) {
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

    // 2. the kernel row of the dim at x = [mu, c_row], zero beyond M, and the mean side's D + 1 sums: thread = column j
    const double *lend = a.len + ((size_t)model * D + d) * P;
    if (tid < P) {
        xin[tid] = tid < D ? mu[tid] : a.ctrl[(size_t)(org + 1 + t) * C + (tid - D)];
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

struct LfanVarArgs {
    const double *K;                        // [units] Tp x Mp, rows beyond nr and columns beyond M are zeros
    const double *gam;                      // [units] Mp x Mp
    double *part;                           // [units][ntj][Tp]
    int Tp, Mp, nr, u0;
};

// One workgroup = one 128 x 128 tile of T = K Gamma of one unit; eight wavefronts of 64 x 32, tg_var_kernel's launch bounds, main
// loop and tile order.  Epilogue: the accumulator weighted by k_nj (read back from K, eight loads at a time), then per row the lane's
// 2 columns, the 16 lanes of a DPP row (row16_sum), the four column wavefronts through LDS in fixed order.  No atomics.
__global__ __launch_bounds__(512, 4) void mg_lfan_var_kernel(LfanVarArgs a) {
    __shared__ double As[2][AT][A_LDT];
    __shared__ double Bs[2][AT][A_LD];
    static_assert(4 * 128 <= 2 * AT * A_LDT, "the epilogue's buffer lives in the main loop's LDS");
    const int Mp = a.Mp, Tp = a.Tp, nr = a.nr;
    const int ntj = (Mp + 127) / 128, nti = (nr + 127) / 128;
    const int tj = ntj - 1 - (int)(blockIdx.x / nti), ti = blockIdx.x % nti;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const int J0 = tj * 128 + wc * 32;
    const int u = a.u0 + blockIdx.y;
    const double *Kb = a.K + (size_t)u * Tp * Mp;
    const double *gb = a.gam + (size_t)u * Mp * Mp;
    const RowMajorTile rt{ti, tj, tid, lane, wr, wc, lr, lk};
    TileAcc res = gemm_rowmajor_a(As, Bs, rt, Kb, nr, gb, Mp, Mp, 1 << 30);
    d4 (&acc)[4][2] = res.v;
    double *rs_s = &As[0][0][0];                     // [4 wc][128 rows] (the main loop ends with the workgroup synchronised)
    // w = k t, k read back from K at clamped addresses: a column beyond Mp has t = 0 exactly (the main loop zero-fills it), a row
    // beyond the pass's is never written out.  Eight loads at a time: with all 32 in flight beside the accumulator the kernel spills.
    const int col0 = J0 + lr, col1 = J0 + 16 + lr;
    const int c0 = col0 < Mp ? col0 : Mp - 1, c1 = col1 < Mp ? col1 : Mp - 1, rbase = ti * 128 + wr * 64 + lk;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int row = rbase + 16 * x + 4 * qd;
            const double *kr = Kb + (size_t)(row < Tp ? row : Tp - 1) * Mp;
            double w0 = acc[x][0][qd] * kr[c0], w1 = acc[x][1][qd] * kr[c1];
            asm volatile("" : "+v"(w0), "+v"(w1));               // (the products are formed HERE, not sunk behind the last load)
            acc[x][0][qd] = w0;
            acc[x][1][qd] = w1;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int r = wr * 64 + 16 * x + lk + 4 * qd;
            double s = acc[x][0][qd] + acc[x][1][qd];
            s = row16_sum(s);
            if (lr == 0) rs_s[wc * 128 + r] = s;
        }
    __syncthreads();
    if (tid < 128) {
        const int row = ti * 128 + tid;
        if (row < nr)
            a.part[((size_t)u * ntj + tj) * Tp + row] = ((rs_s[tid] + rs_s[128 + tid]) + rs_s[256 + tid]) + rs_s[384 + tid];
    }
}

}  // namespace

MomentLinearFanArgs mg_lfan_layout(int G, int n_models, int D, int Mp, int unit_per_group, int Bp) {
    MomentLinearFanArgs l{};
    l.shared = (!unit_per_group && n_models == 1) ? 1 : 0;
    l.units = l.shared ? D : G * D;
    l.nr = l.shared ? G * Bp : Bp;
    l.Tp = round_up(l.nr, 128);
    l.ntj = (Mp + 127) / 128;
    return l;
}

int mg_lfan_tracks_per_pass(int G, int n_models, int D, int Mp, int unit_per_group, int B) {
    const MomentLinearFanArgs one = mg_lfan_layout(G, n_models, D, Mp, unit_per_group, 1);
    long long bp = ((1LL << 31) - 1) / ((long long)G * D);                                 // grid x of the state kernel
    const long long per_row = (long long)one.units * (Mp + one.ntj);                       // K and the partials, doubles per row of a unit
    long long rows = MG_LFAN_SCRATCH_DOUBLES / per_row / 128 * 128;
    if (rows > (1LL << 30)) rows = 1LL << 30;                                              // (Tp is an int)
    const long long fit = one.shared ? rows / G : rows;
    if (fit < bp) bp = fit;
    return (int)(bp < 1 ? 1 : bp > B ? B : bp);
}

// a.G: the tracks of the pass (groups * f.Bp); l: mg_lfan_layout of the pass with its buffers
void launch_mg_lfan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFanArgs &f, const MomentLinearFanArgs &l, int t) {
    const dim3 grid((unsigned)((size_t)a.G * a.D));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_lfan_state_kernel<d>), grid, dim3(256), 0, stream, a, t, f, l))
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

void launch_mg_lfan_var(hipStream_t stream, const double *K, const double *gam, double *vpart, int Tp, int Mp, int nr, int units) {
    const int nti = (nr + 127) / 128, ntj = (Mp + 127) / 128;
    for (int u0 = 0; u0 < units; u0 += 32768) {
        const LfanVarArgs va{K, gam, vpart, Tp, Mp, nr, u0};
        hipLaunchKernelGGL(mg_lfan_var_kernel, dim3((unsigned)(nti * ntj), (unsigned)(units - u0 < 32768 ? units - u0 : 32768)),
                           dim3(512), 0, stream, va);
    }
}

}  // namespace ffvd
