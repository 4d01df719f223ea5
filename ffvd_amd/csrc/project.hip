// Projection kernels (gfx950, fp64) of the F = K_fu L^{-T} route: project_kernel forms F strip by strip with K_fu generated in
// LDS (K5b: conditionals_multi_output.py:240-242), with the per-point sums |F_t|^2 and F_t u (K8: :255, :41; K11: :48); the
// LinearK low-rank path forms those two sums through the kernel's rank P without F or K_fu (kernels.py:270-281).
// DESIGN.md section 4 describes both, section 5 has their measurements.
#include "kernels.h"
#include "dev_common.h"

namespace ffvd {

// ---------------------------------------------------------------------------------------------
// Projection:  F = K_fu * L^{-T}  (conditionals_multi_output.py:240-242), K_fu generated on the fly.
// One workgroup (8 wavefronts) = 64 rows of one (chain, latent dim) x one column group of <= 512 columns.
// ---------------------------------------------------------------------------------------------
constexpr int KC = 32;          // k-chunk (columns of K_fu produced per barrier)
constexpr int KS_LD = STRIP + 16;   // LDS row stride of the K chunk: 80 doubles => lanes l and l+16 hit different bank halves

template <int KIND, int NW>
__global__ __launch_bounds__(NW * 64) void project_kernel(ProjectArgs a) {
    constexpr int NT = NW * 64;          // threads
    constexpr int TPW = 32 / NW;         // 16-column tiles per wavefront
    __shared__ double Ks[2][KC][KS_LD];
    __shared__ double xs[MAXP][STRIP];
    __shared__ double xx[STRIP];
    __shared__ double zs[2][KC][MAXP];
    __shared__ double zzs[2][KC];
    __shared__ double part[2][NW][STRIP];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const int t0 = blockIdx.x * STRIP;
    const int g = blockIdx.y;
    const int bz = blockIdx.z;                 // index inside this pass
    const int b = a.b0 + bz;                   // global batch index
    const int s = b / a.Dl, dl = b % a.Dl, dg = a.d_begin + dl;
    const int P = a.P, Mp = a.Mp;
    const double var = a.hv.variance[dl];
    const double *Zsd = a.hv.Zs + (size_t)dl * Mp * P;
    const double *zzd = a.hv.zz + (size_t)dl * Mp;
    const double *Wd = a.W + (size_t)dl * a.w_stride;

    // ---- x rows of this strip, divided by the lengthscales (kernels_multi_output.py:170) ----
    for (int p = tid >> 6; p < P; p += NW) {
        const int t = t0 + lane;
        double v = 0.0;
        if (t < a.T) {
            v = (p < a.x_cols) ? a.x[(size_t)s * a.x_chain_stride + (size_t)t * a.x_ld + p]
                               : a.ctrl[(size_t)t * a.C + (p - a.x_cols)];
            if (KIND == 0) v = v / a.hv.len[(size_t)dl * P + p];
            else v = v * var;                                    // kernels.py:276  (X * variance) @ X2^T
        }
        xs[p][lane] = v;
    }
    const int kend = (g + 1) * 512 < Mp ? (g + 1) * 512 : Mp;
    const int nchunk = kend / KC;
    auto load_z = [&](int c, int buf) {
        if (tid < KC * P) {
            const int kk = tid / P, p = tid % P;
            zs[buf][kk][p] = Zsd[(size_t)(c * KC + kk) * P + p];
        }
        if (tid < KC) zzs[buf][tid] = zzd[c * KC + tid];
    };
    load_z(0, 0);
    __syncthreads();
    if (tid < STRIP) {
        double acc = 0.0;
        if (KIND == 0) for (int p = 0; p < P; ++p) acc += xs[p][tid] * xs[p][tid];
        xx[tid] = acc;
    }
    __syncthreads();
    auto gen = [&](int c, int buf) {
        const int row = lane;
#pragma unroll
        for (int i = 0; i < (KC * STRIP) / NT; ++i) {
            const int kk = (tid >> 6) + NW * i;
            const int kcol = c * KC + kk;
            double dot = 0.0;
            for (int p = 0; p < P; ++p) dot += xs[p][row] * zs[buf][kk][p];
            double v = kernel_value<KIND>(dot, xx[row], zzs[buf][kk], var);
            if (t0 + row >= a.T || kcol >= a.M) v = 0.0;
            Ks[buf][kk][row] = v;
        }
    };
    gen(0, 0);
    if (nchunk > 1) load_z(1, 1);
    __syncthreads();

    // ---- column tiles owned by this wavefront (snake order balances the triangular work) ----
    int c0[TPW];
    bool tv[TPW];
#pragma unroll
    for (int r = 0; r < TPW; ++r) {
        const int lt = r * NW + ((r & 1) ? NW - 1 - wave : wave);
        c0[r] = (g * 32 + lt) * 16;
        tv[r] = c0[r] < kend;
    }
    d4 acc[4][TPW];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < TPW; ++r) acc[rt][r] = (d4){0.0, 0.0, 0.0, 0.0};

    // B fragments (rows of L^{-T}) are prefetched one k-step ahead straight from L2 into registers.
    // L^{-T} is upper triangular: a 16-column tile starting at c0 only needs rows k < c0 + 16.
    // uniform row base (scalar registers) + 32-bit per-lane offset: lets the load use the saddr form
    int boff[TPW];
#pragma unroll
    for (int r = 0; r < TPW; ++r) boff[r] = lk * Mp + c0[r] + lr;
    auto loadB = [&](int kglob, double(&bv)[TPW]) {
        const double *Wk = Wd + (size_t)kglob * Mp;
#pragma unroll
        for (int r = 0; r < TPW; ++r)
            bv[r] = (tv[r] && kglob < c0[r] + 16) ? Wk[boff[r]] : 0.0;
    };
    // SIMD partners (waves w and w+4) alternate roles inside a chunk: one generates the next K_fu chunk on the
    // VALU while the other feeds the matrix pipe, instead of all eight waves doing the same phase in lockstep.
    const bool gen_first = ((wave >> 2) & 1) == 0;
    double bcur[TPW], bnxt[TPW];
    loadB(0, bcur);
    for (int c = 0; c < nchunk; ++c) {
        const int buf = c & 1;
        if (c + 2 < nchunk) load_z(c + 2, buf);        // zs[buf] was consumed by gen(c) before the last barrier
        if (gen_first && c + 1 < nchunk) gen(c + 1, buf ^ 1);   // zs[buf^1] was loaded one iteration ago
        double af[4], afn[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) af[rt] = Ks[buf][lk][16 * rt + lr];
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            const int kglob = c * KC + 4 * ks;
            if (kglob + 4 < kend) loadB(kglob + 4, bnxt);
            if (ks + 1 < KC / 4) {
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) afn[rt] = Ks[buf][4 * (ks + 1) + lk][16 * rt + lr];
            }
#pragma unroll
            for (int r = 0; r < TPW; ++r) {
                if (tv[r] && kglob < c0[r] + 16) {
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) acc[rt][r] = mfma_f64(af[rt], bcur[r], acc[rt][r]);
                }
            }
#pragma unroll
            for (int r = 0; r < TPW; ++r) bcur[r] = bnxt[r];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) af[rt] = afn[rt];
        }
        if (!gen_first && c + 1 < nchunk) gen(c + 1, buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue ----
    if (a.F) {
        double *Fb = a.F + ((size_t)bz * a.Tp + t0) * Mp;
#pragma unroll
        for (int r = 0; r < TPW; ++r) {
            if (!tv[r]) continue;
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    Fb[(size_t)(16 * rt + lk + 4 * q) * Mp + c0[r] + lr] = acc[rt][r][q];
        }
    }
    if (a.rowsq || a.fmean) {
        double uc[TPW];
#pragma unroll
        for (int r = 0; r < TPW; ++r) {
            const int col = c0[r] + lr;
            uc[r] = (a.fmean && tv[r] && col < a.M) ? a.U[(size_t)col * a.u_ld + dg] : 0.0;
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double sq = 0.0, fm = 0.0;
#pragma unroll
                for (int r = 0; r < TPW; ++r) {
                    const double v = tv[r] ? acc[rt][r][q] : 0.0;
                    sq += v * v;
                    fm += v * uc[r];
                }
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    sq += __shfl_xor(sq, m);
                    fm += __shfl_xor(fm, m);
                }
                if (lr == 0) {
                    part[0][wave][16 * rt + lk + 4 * q] = sq;
                    part[1][wave][16 * rt + lk + 4 * q] = fm;
                }
            }
        __syncthreads();
        if (tid < STRIP) {
            double sq = 0.0, fm = 0.0;
            for (int w = 0; w < NW; ++w) { sq += part[0][w][tid]; fm += part[1][w][tid]; }
            const size_t o = ((size_t)b * a.ng + g) * a.Tp + t0 + tid;
            if (a.rowsq) a.rowsq[o] = sq;
            if (a.fmean) a.fmean[o] = fm;
        }
    }
}

void launch_project(hipStream_t stream, const ProjectArgs &a) {
    dim3 grid(a.Tp / STRIP, a.ng, a.nb);
    // 16 wavefronts per workgroup (4 per SIMD, 2 column tiles each) measured 4.1-4.2 ms against 4.6-4.7 ms for
    // 8 wavefronts with 4 tiles each on config 2: one fp64 MFMA wavefront fills at most half a SIMD's matrix pipe.
    if (a.kind == 0) hipLaunchKernelGGL((project_kernel<0, 16>), grid, dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((project_kernel<1, 16>), grid, dim3(1024), 0, stream, a);
}

// ---------------------------------------------------------------------------------------------
// LinearK, explicit-U branch, forward only: the projection through the kernel's rank.  K_fu = sigma^2 X Z^T (kernels.py:276) has
// rank P = D + C, so F = K_fu L^-T = sigma^2 X C with C = Z^T L^-T (P x Mp), and what the branch reads of F
// (conditionals_multi_output.py:44-52, dgp_model.py:346-351) are two forms per row:
//     fmean_t = F_t u = sigma^2 x_t . v,   v = C u (P);       sum_j F_tj^2 = sigma^4 x_t^T G x_t,   G = C C^T (P x P).
// T M^2 -> T P^2 flops per unit (BASELINE configs[4]: 0.50 ms of projection -> two launches of a few microseconds).  Same values as
// the M-wide route up to summation order; C, v, G are bounded by construction (C C^T = Z^T K^-1 Z), so nothing cancels.
// C comes out of the K_uu chain itself: its launch carries ONE 64-row extension block holding Z^T (kuu_build_kernel, zt_rows) instead
// of the M identity rows that become L^-T -- extension rows X end as X L^-T.  linear_gv: partial sums of G and v per (dim, 64 columns);
// linear_rows: one thread per row t, every workgroup first adds the partials.
// ---------------------------------------------------------------------------------------------
constexpr int LRP = 32;             // bound on P for this path (register arrays; <= 64 rows of one extra block); larger P takes project_kernel
__global__ __launch_bounds__(256) void linear_gv_kernel(const double *Crows, size_t c_stride, const double *U, int u_ld, int d_begin,
                                                        int M, int Mp, int P, double *part /*[Dl][nblk][P*P + P]*/) {
    __shared__ double cs[LRP][64];                       // C[:, this block of 64 columns]
    const int jb = blockIdx.x, dl = blockIdx.y, tid = threadIdx.x, nblk = gridDim.x;
    const double *C = Crows + (size_t)dl * c_stride;     // row p at C + p * Mp: C = Z^T L^-T out of the K_uu chain's launch
    for (int e = tid; e < P * 64; e += 256) cs[e >> 6][e & 63] = C[(size_t)(e >> 6) * Mp + jb * 64 + (e & 63)];
    __syncthreads();
    double *o = part + ((size_t)dl * nblk + jb) * ((size_t)P * P + P);
    for (int e = tid; e < P * P + P; e += 256) {
        double v = 0.0;
        if (e < P * P) {
            const double *a = cs[e / P], *b = cs[e % P];
#pragma unroll 8
            for (int c = 0; c < 64; ++c) v = fma(a[c], b[c], v);
        } else {
            const double *a = cs[e - P * P];
            for (int c = 0; c < 64; ++c) {
                const int jj = jb * 64 + c;
                const double u = (jj < M) ? U[(size_t)jj * u_ld + d_begin + dl] : 0.0;
                v = fma(a[c], u, v);
            }
        }
        o[e] = v;
    }
}
__global__ __launch_bounds__(256) void linear_rows_kernel(ProjectArgs a, const double *part, int nblk) {
    extern __shared__ double gv[];                       // G [P][P] | v [P]
    const int bz = blockIdx.y, b = a.b0 + bz, s = b / a.Dl, dl = b % a.Dl, tid = threadIdx.x, P = a.P;
    const int ne = P * P + P;
    for (int e = tid; e < ne; e += 256) {
        double v = 0.0;
        for (int k = 0; k < nblk; ++k) v += part[((size_t)dl * nblk + k) * ne + e];
        gv[e] = v;
    }
    __syncthreads();
    const int t = blockIdx.x * 256 + tid;
    if (t >= a.Tp) return;
    double rs = 0.0, fm = 0.0;
    if (t < a.T) {
        double x[LRP];
        const double *xr = a.x + (size_t)s * a.x_chain_stride + (size_t)t * a.x_ld;
#pragma unroll
        for (int p = 0; p < LRP; ++p) {
            x[p] = 0.0;
            if (p < a.x_cols) x[p] = xr[p];
            else if (p < P) x[p] = a.ctrl[(size_t)t * a.C + (p - a.x_cols)];
        }
        double q = 0.0, m = 0.0;
#pragma unroll
        for (int p = 0; p < LRP; ++p) {
            if (p < P) {
                double y = 0.0;
#pragma unroll
                for (int r = 0; r < LRP; ++r)
                    if (r < P) y = fma(gv[p * P + r], x[r], y);
                q = fma(x[p], y, q);
                m = fma(x[p], gv[P * P + p], m);
            }
        }
        const double var = a.hv.variance[dl];
        rs = var * var * q;
        fm = var * m;
    }
    const size_t o = (size_t)b * a.Tp + t;              // one column group (ng = 1 for this path)
    if (a.rowsq) a.rowsq[o] = rs;
    if (a.fmean) a.fmean[o] = fm;
}
bool linear_lowrank_supported(int kind, int P) { return kind == 1 && P <= LRP; }
size_t linear_lowrank_doubles(int Mp, int Dl, int P) { return (size_t)Dl * (Mp / 64) * ((size_t)P * P + P); }
void launch_linear_lowrank(hipStream_t stream, const ProjectArgs &a, double *part) {
    const int nblk = a.Mp / 64;
    if (a.b0 == 0)          // G, v depend on the dim only: once per iteration (the first pass)
        hipLaunchKernelGGL(linear_gv_kernel, dim3(nblk, a.Dl), dim3(256), 0, stream, a.W, a.w_stride, a.U, a.u_ld, a.d_begin, a.M, a.Mp,
                           a.P, part);
    hipLaunchKernelGGL(linear_rows_kernel, dim3((a.Tp + 255) / 256, a.nb), dim3(256), ((size_t)a.P * a.P + a.P) * sizeof(double), stream, a,
                       part, nblk);
}

}  // namespace ffvd
