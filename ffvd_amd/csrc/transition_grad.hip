// Input gradients of the grouped GP conditional for gfx950, fp64 (see transition_grad.h for the formulas, the layouts and the launch
// sequence).
//
// The hot path is the variance side: per unit the product T = K Gamma (N x Mp by Mp x Mp), of which only P + 1 weighted row sums are
// wanted.  It is a 128 x 128-tiled product on v_mfma_f64_16x16x4_f64 with the main loop and LDS staging of cg_rowsq_kernel
// (gemm_rowmajor_a, gemm_rowmajor.h) and an epilogue that weights each accumulator element by k_nj and contracts the tile's columns
// against [1, nu_.p], so T never reaches HBM.  The mean side is a matrix-vector product per (group, dim) with the same P + 1
// contractions: O(G D N M P) on the VALU.
#include "transition_grad.h"
#include "gemm_rowmajor.h"

namespace ffvd {

constexpr int TG_FB = 8;                    // fields reduced through LDS per round of the epilogue

struct TgVarArgs {
    const double *K; size_t k_stride;       // [n_models * D] Tp x Mp
    const double *gam; size_t g_stride;     // [units] Mp x Mp
    const double *Z;                        // [n_models][M][P]
    const double *x;                        // the pass's rows, [nr][P]
    double *part;                           // [units][ntj][P + 1][Tp]
    int Tp, Mp, M, P, D, nr, n_models, u0;
};

// One workgroup = one 128 x 128 tile of T for one unit; eight wavefronts of 64 x 32, cg_rowsq_kernel's launch bounds and tile order.
// Epilogue.  A lane holds 16 rows x 2 columns of the tile, so the P + 1 fields are formed one after the other from the weighted
// accumulator w = k t (the loop over the fields is OUTSIDE the rows): field 0 is sum_j w, field 1 + p is sum_j w (z_jp - x_np), the
// difference formed per element.  Fixed order: the lane's 2 columns, the 16 lanes of a DPP row (row16_sum), the four column
// wavefronts through LDS, TG_FB fields per round.  No atomics.
__global__ __launch_bounds__(512, 4) void tg_var_kernel(TgVarArgs a) {
    __shared__ double As[2][AT][A_LDT];
    __shared__ double Bs[2][AT][A_LD];
    static_assert(TG_FB * 4 * 128 <= 2 * AT * A_LDT && 128 * MAXP <= 2 * AT * A_LD, "the epilogue's buffers live in the main loop's LDS");
    const int ntj = (a.Mp + 127) / 128, nti = (a.Tp + 127) / 128;
    const int tj = ntj - 1 - (int)(blockIdx.x / nti), ti = blockIdx.x % nti;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const int J0 = tj * 128 + wc * 32;
    const int Mp = a.Mp, Tp = a.Tp, P = a.P, F = P + 1;
    const int u = a.u0 + blockIdx.y, d = u % a.D, m = a.n_models == 1 ? 0 : u / a.D;      // (u / D: the group or the model, the same number)
    const double *Kb = a.K + (size_t)(m * a.D + d) * a.k_stride;
    const double *gb = a.gam + (size_t)u * a.g_stride;
    const double *Zm = a.Z + (size_t)m * a.M * P;
    const RowMajorTile rt{ti, tj, tid, lane, wr, wc, lr, lk};
    TileAcc res = gemm_rowmajor_a(As, Bs, rt, Kb, Tp, gb, Mp, Mp, 1 << 30);
    d4 (&acc)[4][2] = res.v;
    double *rs_s = &As[0][0][0];                     // [TG_FB][4 wc][128 rows] (the main loop ends with the workgroup synchronised)
    double *xs = &Bs[0][0][0];                       // [128 rows][P]: the tile's rows of Xnew, zeros beyond the pass
    for (int e = tid; e < 128 * P; e += 512) {
        const int t = ti * 128 + e / P;
        xs[e] = t < a.nr ? a.x[(size_t)t * P + e % P] : 0.0;
    }
    // w = k t, k read back from the K array (zero in the padding: rows beyond the pass, columns beyond M)
    // Unconditional loads at clamped addresses: a column beyond Mp has t = 0 exactly (the main loop zero-fills it), a row beyond Tp is
    // never written out.  Eight loads at a time: with all 32 in flight beside the accumulator the kernel spills.
    const int col0 = J0 + lr, col1 = J0 + 16 + lr;
    {
        const int c0 = col0 < Mp ? col0 : Mp - 1, c1 = col1 < Mp ? col1 : Mp - 1, rbase = ti * 128 + wr * 64 + lk;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int row = rbase + 16 * x + 4 * qd;
                const double *kr = Kb + (size_t)(row < Tp ? row : Tp - 1) * Mp;
                double w0 = acc[x][0][qd] * kr[c0], w1 = acc[x][1][qd] * kr[c1];
                asm volatile("" : "+v"(w0), "+v"(w1));           // (the products are formed HERE, not sunk behind the last load)
                acc[x][0][qd] = w0;
                acc[x][1][qd] = w1;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    const bool ok0 = col0 < a.M, ok1 = col1 < a.M;
    for (int f0 = 0; f0 < F; f0 += TG_FB) {
#pragma unroll 1
        for (int fl = 0; fl < TG_FB && f0 + fl < F; ++fl) {
            const int f = f0 + fl, p = f - 1;
            const double z0 = f == 0 ? 1.0 : (ok0 ? Zm[(size_t)col0 * P + p] : 0.0);
            const double z1 = f == 0 ? 1.0 : (ok1 ? Zm[(size_t)col1 * P + p] : 0.0);
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int r = wr * 64 + 16 * x + lk + 4 * qd;
                    const double xr = f == 0 ? 0.0 : xs[r * P + p];
                    double v = acc[x][0][qd] * (z0 - xr) + acc[x][1][qd] * (z1 - xr);
                    v = row16_sum(v);
                    if (lr == 0) rs_s[(fl * 4 + wc) * 128 + r] = v;
                }
        }
        __syncthreads();
        for (int o = tid; o < TG_FB * 128; o += 512) {
            const int fl = o >> 7, r = o & 127, f = f0 + fl, t = ti * 128 + r;
            if (f < F && t < Tp)
                a.part[(((size_t)u * ntj + tj) * F + f) * Tp + t] =
                    (rs_s[(fl * 4 + 0) * 128 + r] + rs_s[(fl * 4 + 1) * 128 + r]) + (rs_s[(fl * 4 + 2) * 128 + r] + rs_s[(fl * 4 + 3) * 128 + r]);
        }
        __syncthreads();
    }
}

struct TgMeanArgs {
    const double *K; size_t k_stride;
    const double *beta, *Z, *x;             // [G * D][Mp], [n_models][M][P], the pass's rows [nr][P]
    double *msum;                           // [G * D][P + 1][Tp]
    int Tp, Mp, M, P, D, nr, n_models, nblk;
};
// One thread per (group, dim, row): sum_j k_j beta_j and sum_j k_j beta_j (z_jp - x_p), j ascending.  A workgroup serves one
// (group, dim): beta and Z are read through the scalar cache.  PM: the compile-time bound of P (8 or MAXP).
template <int PM>
__global__ __launch_bounds__(256) void tg_mean_kernel(TgMeanArgs a) {
    const int gd = (int)(blockIdx.x / a.nblk), n = (int)(blockIdx.x % a.nblk) * 256 + threadIdx.x;
    if (n >= a.nr) return;
    const int g = gd / a.D, d = gd % a.D, m = a.n_models == 1 ? 0 : g, P = a.P;
    const double *Krow = a.K + (size_t)(m * a.D + d) * a.k_stride + (size_t)n * a.Mp;
    const double *b = a.beta + (size_t)gd * a.Mp, *Zm = a.Z + (size_t)m * a.M * P;
    double xr[PM], s[PM], s0 = 0.0;
#pragma unroll
    for (int p = 0; p < PM; ++p) { xr[p] = p < P ? a.x[(size_t)n * P + p] : 0.0; s[p] = 0.0; }
    for (int j = 0; j < a.M; ++j) {
        const double w = Krow[j] * b[j];
        s0 += w;
#pragma unroll
        for (int p = 0; p < PM; ++p)
            if (p < P) s[p] += w * (Zm[(size_t)j * P + p] - xr[p]);
    }
    double *out = a.msum + (size_t)gd * (P + 1) * a.Tp + n;
    out[0] = s0;
#pragma unroll
    for (int p = 0; p < PM; ++p)
        if (p < P) out[(size_t)(1 + p) * a.Tp] = s[p];
}

struct TgFinishArgs {
    int G, n_models, D, P, N, n0, nr, Tp, ntj, unit_per_group;
    const double *variance, *len, *vpart, *msum;
    double *mean, *var, *dmean, *dvar;
};
// One thread per (g, n, d) of the pass: the column-tile partials added in ascending order, then 1 / l^2 and the factors.
__global__ __launch_bounds__(256) void tg_finish_kernel(TgFinishArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.G * a.nr * a.D) return;
    const int d = (int)(i % a.D), n = (int)((i / a.D) % a.nr), g = (int)(i / ((size_t)a.D * a.nr));
    const int md = (a.n_models == 1 ? 0 : g) * a.D + d, gd = g * a.D + d, u = a.unit_per_group ? gd : md, P = a.P, F = P + 1;
    const size_t o = ((size_t)g * a.N + a.n0 + n) * a.D + d;
    const double *ms = a.msum + (size_t)gd * F * a.Tp + n;
    a.mean[o] = ms[0];
    for (int f = 0; f < F; ++f) {
        double il2 = 0.0;
        if (f > 0) {
            const double l = a.len[(size_t)md * P + f - 1];
            il2 = 1.0 / (l * l);
            a.dmean[o * P + f - 1] = il2 * ms[(size_t)f * a.Tp];
        }
        if (!a.var) continue;
        double sv = 0.0;
        for (int tj = 0; tj < a.ntj; ++tj) sv += a.vpart[(((size_t)u * a.ntj + tj) * F + f) * a.Tp + n];
        if (f == 0) a.var[o] = a.variance[md] - sv;
        else a.dvar[o * P + f - 1] = -(2.0 * il2) * sv;
    }
}

__global__ __launch_bounds__(256) void tg_mixture_kernel(const double *mean, const double *dmean, const double *dvar, const double *mix_mean,
                                                         int G, size_t ND, int P, double *mix_dmean, double *mix_dvar) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ND * P) return;
    const size_t nd = i / P;
    const double mm = mix_mean[nd];
    double sm = 0.0, sv = 0.0;
    for (int g = 0; g < G; ++g) {
        const double dm = dmean[(size_t)g * ND * P + i];
        sm += dm;
        if (mix_dvar) sv += dvar[(size_t)g * ND * P + i] + 2.0 * (mean[(size_t)g * ND + nd] - mm) * dm;
    }
    mix_dmean[i] = sm / (double)G;
    if (mix_dvar) mix_dvar[i] = sv / (double)G;
}

static int tg_pass_tp(int N, int rows_per_pass) { return round_up(N < rows_per_pass ? N : rows_per_pass, STRIP); }

TransitionGradScratch tg_scratch_doubles(int G, int n_models, int D, int P, int Mp, int N, int rows_per_pass, int units, bool need_var) {
    const size_t Tp = (size_t)tg_pass_tp(N, rows_per_pass), F = (size_t)P + 1;
    TransitionGradScratch s;
    s.K = (size_t)n_models * D * Tp * Mp;
    s.vpart = need_var ? (size_t)units * ((Mp + 127) / 128) * F * Tp : 0;
    s.msum = (size_t)G * D * F * Tp;
    return s;
}

void launch_transition_grad(hipStream_t stream, const TransitionGradArgs &a) {
    const int G = a.G, D = a.D, P = a.P, Mp = a.Mp, nm = a.n_models, GD = G * D, units = a.unit_per_group ? GD : nm * D;
    const int Tp = tg_pass_tp(a.N, a.rows_per_pass), ntj = (Mp + 127) / 128, nti = (Tp + 127) / 128;
    const size_t kstride = (size_t)Tp * Mp;
    for (int n0 = 0; n0 < a.N; n0 += a.rows_per_pass) {
        const int nr = a.N - n0 < a.rows_per_pass ? a.N - n0 : a.rows_per_pass;
        const double *xp = a.x + (size_t)n0 * P;
        // 1. K(Xnew, Z) once per (model, dim)
        for (int m = 0; m < nm; ++m) {
            const size_t k0 = (size_t)m * D;
            ProjectArgs pa{};
            pa.kind = 0; pa.x = xp; pa.x_chain_stride = 0; pa.x_ld = P; pa.x_cols = P; pa.ctrl = nullptr;
            pa.T = nr; pa.Tp = Tp; pa.C = 0; pa.P = P; pa.M = a.M; pa.Mp = Mp; pa.Dl = D; pa.d_begin = 0;
            pa.hv = HyperView{a.hv.variance + k0, a.hv.len + k0 * P, a.hv.Zs + k0 * Mp * P, a.hv.zz + k0 * Mp};
            pa.b0 = 0; pa.nb = D; pa.F = a.K + k0 * kstride; pa.gpart = nullptr;
            launch_kfu_build(stream, pa);
        }
        // 2. the variance side: P + 1 weighted row sums of T = K Gamma per (unit, column tile)
        if (a.need_var)
            for (int u0 = 0; u0 < units; u0 += 32768) {
                TgVarArgs va{a.K, kstride, a.gam, (size_t)Mp * Mp, a.Z, xp, a.vpart, Tp, Mp, a.M, P, D, nr, nm, u0};
                hipLaunchKernelGGL(tg_var_kernel, dim3((unsigned)(nti * ntj), (unsigned)(units - u0 < 32768 ? units - u0 : 32768)), dim3(512), 0,
                                   stream, va);
            }
        // 3. the mean side
        const int nblk = (nr + 255) / 256;
        TgMeanArgs ma{a.K, kstride, a.beta, a.Z, xp, a.msum, Tp, Mp, a.M, P, D, nr, nm, nblk};
        if (P <= 8) hipLaunchKernelGGL(tg_mean_kernel<8>, dim3((unsigned)((size_t)GD * nblk)), dim3(256), 0, stream, ma);
        else hipLaunchKernelGGL(tg_mean_kernel<MAXP>, dim3((unsigned)((size_t)GD * nblk)), dim3(256), 0, stream, ma);
        // 4. values and gradients of the pass's rows
        TgFinishArgs fa{G, nm, D, P, a.N, n0, nr, Tp, ntj, a.unit_per_group, a.hv.variance, a.hv.len, a.vpart, a.msum,
                        a.mean, a.need_var ? a.var : nullptr, a.dmean, a.need_var ? a.dvar : nullptr};
        const size_t n = (size_t)G * nr * D;
        hipLaunchKernelGGL(tg_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fa);
    }
}

void launch_tg_mixture(hipStream_t stream, const double *mean, const double *dmean, const double *dvar, const double *mix_mean, int G,
                       size_t ND, int P, double *mix_dmean, double *mix_dvar) {
    if (!ND || !P) return;
    hipLaunchKernelGGL(tg_mixture_kernel, dim3((unsigned)((ND * P + 255) / 256)), dim3(256), 0, stream, mean, dmean, dvar, mix_mean, G, ND, P,
                       mix_dmean, mix_dvar);
}

}  // namespace ffvd
