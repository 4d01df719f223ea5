// Grouped GP conditionals for gfx950, fp64 (see conditional_group.h for the layouts and the launch sequence).
//
// The one new product is the q_sqrt term of the variance (conditionals_multi_output.py:369-380): per unit u = g * D + d the row sums
// of squares of E = F_{m(g),d} q_{g,d'}.  qsqrt_inflation_kernel (kernels.hip) forms them with M^2 scalar FMAs per row; here they are
// a 128 x 128-tiled product on v_mfma_f64_16x16x4_f64 with the main loop and LDS staging of proj_gemm_kernel (gemm_rowmajor_a,
// gemm_rowmajor.h) and a sum-of-squares epilogue, so E never reaches HBM.
#include "conditional_group.h"
#include "gemm_rowmajor.h"

namespace ffvd {

struct CgVarArgs {
    const double *F; size_t f_stride;       // [n_models * D] Tp x Mp
    const double *q; size_t q_stride;       // [G] or [G * D] Mp x Mp
    double *part;                           // [G * D][ntj][Tp]
    int Tp, Mp, D, n_models, q_per_dim, upper, u0;
};

// One workgroup = one 128 x 128 tile of E for one unit; eight wavefronts of 64 x 32.  With `upper` (every q slab is upper triangular)
// the k range of column tile tj ends at that tile's last column and, inside the last block, a wavefront stops at its own last column:
// the skipped terms are exact zeros, so a dense launch over the same slabs gives the same bits.
// Epilogue, fixed order: 2 columns per lane, the 16 lanes of a DPP row, the four column wavefronts through LDS.  No atomics.
__global__ __launch_bounds__(512, 4) void cg_rowsq_kernel(CgVarArgs a) {
    __shared__ double As[2][AT][A_LDT];
    __shared__ double Bs[2][AT][A_LD];
    const int ntj = (a.Mp + 127) / 128, nti = (a.Tp + 127) / 128;
    // heavy column tiles (long k range) first, as proj_gemm_kernel
    const int tj = ntj - 1 - (int)(blockIdx.x / nti), ti = blockIdx.x % nti;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const int J0 = tj * 128 + wc * 32;
    const int Mp = a.Mp, Tp = a.Tp;
    const int u = a.u0 + blockIdx.y, g = u / a.D, d = u % a.D;
    const double *Fb = a.F + (size_t)((a.n_models == 1 ? 0 : g) * a.D + d) * a.f_stride;
    const double *qb = a.q + (size_t)(a.q_per_dim ? u : g) * a.q_stride;
    const int kend = (a.upper && (tj + 1) * 128 < Mp) ? (tj + 1) * 128 : Mp;
    const RowMajorTile rt{ti, tj, tid, lane, wr, wc, lr, lk};
    TileAcc res = gemm_rowmajor_a(As, Bs, rt, Fb, Tp, qb, Mp, kend, a.upper ? (J0 + 31) / AT : (1 << 30));
    d4 (&acc)[4][2] = res.v;
    double *rs_s = &As[0][0][0];                     // [4 wc][128 rows] (the main loop ends with the workgroup synchronised)
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            double v = 0.0;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const double e = acc[x][y][qd];
                v += e * e;
            }
            v = row16_sum(v);
            if (lr == 0) rs_s[wc * 128 + wr * 64 + 16 * x + lk + 4 * qd] = v;
        }
    __syncthreads();
    if (tid < 128) {
        const int t = ti * 128 + tid;
        if (t < Tp) a.part[((size_t)u * ntj + tj) * Tp + t] = (rs_s[tid] + rs_s[128 + tid]) + (rs_s[256 + tid] + rs_s[384 + tid]);
    }
}

// Ut[(one model ? d * G + g : g * D + d)][j] = U[g][j][d], zeros for M <= j < Mp
__global__ __launch_bounds__(256) void cg_pack_ut_kernel(const double *U, int G, int D, int M, int Mp, int one_model, double *Ut) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)G * D * Mp) return;
    const int j = (int)(i % Mp);
    const size_t r = i / Mp;
    const int g = one_model ? (int)(r % G) : (int)(r / D), d = one_model ? (int)(r / G) : (int)(r % D);
    Ut[i] = j < M ? U[((size_t)g * M + j) * D + d] : 0.0;
}

struct CgFinishArgs {
    int kind, G, n_models, D, P, N, n0, nr, Tp, ng, ntj, ncols;
    const double *x, *variance, *rowsq, *part, *mbuf;
    double *mean, *var;
};
// One thread per (g, n, d) of the pass.  var = Kdiag - sum rowsq + sum extra: the arithmetic and operand order of
// conditional_finish_kernel (step_bodies.h), with the column groups and the column-tile partials added in ascending order.
__global__ __launch_bounds__(256) void cg_finish_kernel(CgFinishArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.G * a.nr * a.D) return;
    const int d = (int)(i % a.D), n = (int)((i / a.D) % a.nr), g = (int)(i / ((size_t)a.D * a.nr));
    const int md = (a.n_models == 1 ? 0 : g) * a.D + d, u = g * a.D + d;
    const size_t o = ((size_t)g * a.N + a.n0 + n) * a.D + d;
    a.mean[o] = a.mbuf[((size_t)(a.n_models == 1 ? d : u) * a.Tp + n) * a.ncols + (a.n_models == 1 ? g : 0)];
    if (!a.var) return;
    double rs = 0.0, ex = 0.0;
    for (int c = 0; c < a.ng; ++c) rs += a.rowsq[((size_t)md * a.ng + c) * a.Tp + n];
    if (a.part)
        for (int tj = 0; tj < a.ntj; ++tj) ex += a.part[((size_t)u * a.ntj + tj) * a.Tp + n];
    double kd = a.variance[md];
    if (a.kind == 1) {                                  // LinearK.Kdiag (kernels.py:278-281)
        double s = 0.0;
        for (int p = 0; p < a.P; ++p) { const double v = a.x[(size_t)(a.n0 + n) * a.P + p]; s += (v * v) * a.variance[md]; }
        kd = s;
    }
    double v = kd - rs;
    if (a.part) v = v + ex;                             // fvar + reduce_sum(square(LTA), 1)  (:380)
    a.var[o] = v;
}

__global__ __launch_bounds__(256) void cg_mixture_kernel(const double *mean, const double *var, int G, size_t ND, double *mix_mean,
                                                         double *mix_var) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ND) return;
    double sm = 0.0, sv = 0.0;
    for (int g = 0; g < G; ++g) {
        const double m = mean[(size_t)g * ND + i];
        sm += m;
        sv += var[(size_t)g * ND + i] + m * m;
    }
    const double mm = sm / (double)G;
    mix_mean[i] = mm;
    mix_var[i] = sv / (double)G - mm * mm;
}

int cg_rows_per_pass(int n_models, int D, int Mp) {
    const long long per_row = (long long)n_models * D * Mp;             // doubles of F per row of Xnew
    long long r = ((1LL << 28) / per_row) / 128 * 128;                  // 2 GiB = 2^28 doubles
    if (r < 128) r = 128;
    if (r > (1LL << 30)) r = 1LL << 30;
    return (int)r;
}

static int cg_pass_tp(int N, int rows_per_pass) { return round_up(N < rows_per_pass ? N : rows_per_pass, STRIP); }

CondGroupScratch cg_scratch_doubles(int G, int n_models, int D, int Mp, int N, int rows_per_pass, bool with_q) {
    const size_t Tp = (size_t)cg_pass_tp(N, rows_per_pass), GD = (size_t)G * D, nK = (size_t)n_models * D;
    CondGroupScratch s;
    s.F = nK * Tp * Mp;
    s.rowsq = nK * ((Mp + 511) / 512) * Tp;
    s.part = with_q ? GD * ((Mp + 127) / 128) * Tp : 0;
    s.Ut = GD * Mp;
    s.mbuf = GD * Tp;
    return s;
}

void launch_conditional_group(hipStream_t stream, const CondGroupArgs &a) {
    const int G = a.G, D = a.D, Mp = a.Mp, nm = a.n_models, GD = G * D;
    const int Tp = cg_pass_tp(a.N, a.rows_per_pass), ng = (Mp + 511) / 512, ntj = (Mp + 127) / 128, nti = (Tp + 127) / 128;
    const size_t fstride = (size_t)Tp * Mp;
    const int ncols = nm == 1 ? G : 1, ncov = nm == 1 ? D : GD;
    {
        const size_t n = (size_t)GD * Mp;
        hipLaunchKernelGGL(cg_pack_ut_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.U, G, D, a.M, Mp, nm == 1 ? 1 : 0, a.Ut);
    }
    for (int n0 = 0; n0 < a.N; n0 += a.rows_per_pass) {
        const int nr = a.N - n0 < a.rows_per_pass ? a.N - n0 : a.rows_per_pass;
        // 1. F and the row sums of F^2, once per (model, dim) (:349, :356)
        for (int m = 0; m < nm; ++m) {
            const size_t k0 = (size_t)m * D;
            ProjectArgs pa{};
            pa.kind = a.kind; pa.x = a.x + (size_t)n0 * a.P; pa.x_chain_stride = 0; pa.x_ld = a.P; pa.x_cols = a.P; pa.ctrl = nullptr;
            pa.T = nr; pa.Tp = Tp; pa.C = 0; pa.P = a.P; pa.M = a.M; pa.Mp = Mp; pa.Dl = D; pa.d_begin = 0;
            pa.hv = HyperView{a.hv.variance + k0, a.hv.len + k0 * a.P, a.hv.Zs + k0 * Mp * a.P, a.hv.zz + k0 * Mp};
            pa.W = a.W + k0 * a.w_stride; pa.w_stride = a.w_stride; pa.U = nullptr; pa.u_ld = 0; pa.b0 = 0; pa.nb = D;
            pa.F = a.F + k0 * fstride; pa.rowsq = a.rowsq + k0 * ng * Tp; pa.fmean = nullptr; pa.ng = ng;
            launch_project(stream, pa);
        }
        // 2. means: F_{m,d} against the U columns of the model's groups (:365)
        for (int c0 = 0; c0 < ncov; c0 += 32768) {
            CovArgs ca{};
            ca.mode = COV_GEN; ca.A = a.F + (size_t)c0 * fstride; ca.E = nullptr; ca.a_stride = fstride; ca.lda = Mp; ca.arows = nr; ca.K = Mp;
            ca.B = a.Ut + (size_t)c0 * ncols * Mp; ca.b_stride = (size_t)ncols * Mp; ca.ldb = Mp; ca.brows = ncols; ca.ncols = ncols;
            ca.C = a.mbuf + (size_t)c0 * Tp * ncols; ca.c_stride = (size_t)Tp * ncols; ca.ldc = ncols;
            ca.nb = ncov - c0 < 32768 ? ncov - c0 : 32768;
            launch_cov(stream, ca);
        }
        // 3. row sums of squares of E = F q, per (unit, column tile)
        const bool with_q = a.need_var && a.q;
        if (with_q)
            for (int u0 = 0; u0 < GD; u0 += 32768) {
                CgVarArgs va{a.F, fstride, a.q, (size_t)Mp * Mp, a.part, Tp, Mp, D, nm, a.q_per_dim, a.q_upper, u0};
                hipLaunchKernelGGL(cg_rowsq_kernel, dim3((unsigned)(nti * ntj), (unsigned)(GD - u0 < 32768 ? GD - u0 : 32768)), dim3(512), 0,
                                   stream, va);
            }
        // 4. mean and var of the pass's rows
        CgFinishArgs fa{a.kind, G, nm, D, a.P, a.N, n0, nr, Tp, ng, ntj, ncols, a.x, a.hv.variance, a.rowsq, with_q ? a.part : nullptr,
                        a.mbuf, a.mean, a.need_var ? a.var : nullptr};
        const size_t n = (size_t)G * nr * D;
        hipLaunchKernelGGL(cg_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fa);
    }
}

void launch_cg_mixture(hipStream_t stream, const double *mean, const double *var, int G, size_t ND, double *mix_mean, double *mix_var) {
    if (!ND) return;
    hipLaunchKernelGGL(cg_mixture_kernel, dim3((unsigned)((ND + 255) / 256)), dim3(256), 0, stream, mean, var, G, ND, mix_mean, mix_var);
}

}  // namespace ffvd
