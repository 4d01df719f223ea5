// Full predictive covariance of the GP conditional and the joint posterior draw (gfx950 / CDNA4, fp64).
//
//   conditional(..., full_cov=True)  (conditionals_multi_output.py:73-120 -> base_conditional :6-70), per latent dim d, white=True:
//     Sigma_d = K_d(Xnew, Xnew) - F_d F_d^T (+ E_d E_d^T),   F_d = K_d(Xnew, Z) L_d^-T  (N x M),   E_d = F_d q0
//   get_rand((mean, var), eps, full_cov=True)  (utils.py:4-11):  out[:, d] = mean[:, d] + chol(Sigma_d + jitter I) eps[:, d]
//
// One NT product body on v_mfma_f64_16x16x4_f64 serves both products: a 128 x 128 output tile per workgroup, eight wavefronts of
// 64 x 32, both operands stored k-contiguous over the OUTPUT rows (F as launch_project writes it), so both are transposed on their
// way into LDS (the A chunk of grad.hip's gemm_rowmajor_a, here for both sides), register-staged one 16-deep chunk ahead.
//   COV_SYM: C_d = seed_d - [F_d | E_d] [F_d | -E_d]^T, lower-triangular tiles only, every element (i > j) stored at (i, j) and at
//            (j, i) from the same register: the result is exactly symmetric.  seed_d = K_d(x_i, x_j) is formed in the epilogue from
//            Xnew and the hyper-parameters, with the arithmetic of kernel_matrix_kernel (kernels.hip); it never goes to HBM.  The
//            diagonal is copied from the per-point variance of the same call (conditional_finish) when one is passed: where the
//            posterior variance is a cancellation (LinearK: var ~ 1e-6 K_ii) two roundings of the same sum would differ in its
//            leading digits, and full_cov=True must agree with full_cov=False on the diagonal.
//   COV_GEN: C_d = A_d B^T with one B for every d (E_d = F_d q0, B = q0^T), every tile, no seed.
// DESIGN.md section 4 ("full covariance") has the layout, the flop count and the measured times.
#include "kernels.h"
#include "dev_common.h"

namespace ffvd {

constexpr int CT = 128;                 // output tile
constexpr int CK = 16;                  // k-chunk
constexpr int C_LDT = CT + 17;          // row stride of a transposed chunk in LDS (odd, = 1 mod 4: the transposed stores of 16 lanes
                                        // hit 32 different banks; grad.hip A_LDT)

__device__ __forceinline__ void cov_tile_of(int idx, int &ti, int &tj) {      // idx -> (ti >= tj), row-major over the lower triangle
    int t = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
    while ((t + 1) * (t + 2) / 2 <= idx) ++t;
    while (t * (t + 1) / 2 > idx) --t;
    ti = t;
    tj = idx - t * (t + 1) / 2;
}

__global__ __launch_bounds__(512, 4) void cov_kernel(CovArgs a) {
    __shared__ double lds[2 * 2 * CK * C_LDT];
    double (*As)[CK][C_LDT] = reinterpret_cast<double (*)[CK][C_LDT]>(lds);
    double (*Bs)[CK][C_LDT] = reinterpret_cast<double (*)[CK][C_LDT]>(lds + 2 * CK * C_LDT);
    const int d = blockIdx.y;
    int ti, tj;
    if (a.mode == COV_SYM) cov_tile_of(blockIdx.x, ti, tj);
    else { const int ntj = (a.ncols + CT - 1) / CT; ti = blockIdx.x / ntj; tj = blockIdx.x % ntj; }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const double *Ad = a.A + (size_t)d * a.a_stride;
    const double *Ed = a.E ? a.E + (size_t)d * a.a_stride : nullptr;         // COV_SYM: second half of the depth
    const double *Bd = a.B ? a.B + (size_t)d * a.b_stride : nullptr;         // COV_GEN: right operand rows
    const int K = a.K;
    const int nchunk = (a.mode == COV_SYM && Ed ? 2 * K : K) / CK;
    const int nhalf = K / CK;

    // thread -> (row il of the tile, 4 consecutive k of the chunk)
    const int il = tid >> 2, kseg = 4 * (tid & 3);
    const int arow = ti * CT + il, brow = tj * CT + il;
    const bool okA = arow < a.arows;
    const bool okB = brow < (a.mode == COV_SYM ? a.arows : a.brows);
    const double *Arow = Ad + (size_t)(okA ? arow : 0) * a.lda + kseg;
    const double *Erow_a = Ed ? Ed + (size_t)(okA ? arow : 0) * a.lda + kseg : nullptr;
    const double *Brow = (a.mode == COV_SYM) ? Ad + (size_t)(okB ? brow : 0) * a.lda + kseg
                                             : Bd + (size_t)(okB ? brow : 0) * a.ldb + kseg;
    const double *Erow_b = Ed ? Ed + (size_t)(okB ? brow : 0) * a.lda + kseg : nullptr;
    d2 ra[2], rb[2];
    bool neg = false;                   // the chunk in registers belongs to the E half: its B side enters with a minus sign
    auto load = [&](int c) {
        const bool second = c >= nhalf;
        const double *pa = second ? Erow_a + (size_t)(c - nhalf) * CK : Arow + (size_t)c * CK;
        const double *pb = second ? Erow_b + (size_t)(c - nhalf) * CK : Brow + (size_t)c * CK;
        ra[0] = *reinterpret_cast<const d2 *>(pa);
        ra[1] = *reinterpret_cast<const d2 *>(pa + 2);
        rb[0] = *reinterpret_cast<const d2 *>(pb);
        rb[1] = *reinterpret_cast<const d2 *>(pb + 2);
        neg = second;
    };
    auto store = [&](int buf) {
        const double sb = neg ? -1.0 : 1.0;
        As[buf][kseg + 0][il] = okA ? ra[0].x : 0.0;
        As[buf][kseg + 1][il] = okA ? ra[0].y : 0.0;
        As[buf][kseg + 2][il] = okA ? ra[1].x : 0.0;
        As[buf][kseg + 3][il] = okA ? ra[1].y : 0.0;
        Bs[buf][kseg + 0][il] = okB ? sb * rb[0].x : 0.0;
        Bs[buf][kseg + 1][il] = okB ? sb * rb[0].y : 0.0;
        Bs[buf][kseg + 2][il] = okB ? sb * rb[1].x : 0.0;
        Bs[buf][kseg + 3][il] = okB ? sb * rb[1].y : 0.0;
    };
    d4 acc[4][2];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    // a wavefront whose 64 rows or 32 columns lie wholly outside the output (ragged last tiles) skips the MFMAs
    const int nrow_out = a.mode == COV_SYM ? a.N : a.arows, ncol_out = a.mode == COV_SYM ? a.N : a.ncols;
    const bool live = ti * CT + wr * 64 < nrow_out && tj * CT + wc * 32 < ncol_out &&
                      !(a.mode == COV_SYM && ti == tj && wr * 64 + 63 < wc * 32);      // (diagonal tile: wholly above it)
    load(0);
    store(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunk) load(c + 1);
        if (live) {
#pragma unroll
            for (int ks = 0; ks < CK / 4; ++ks) {
                double af[4], bf[2];
#pragma unroll
                for (int x = 0; x < 4; ++x) af[x] = As[buf][4 * ks + lk][wr * 64 + 16 * x + lr];
#pragma unroll
                for (int y = 0; y < 2; ++y) bf[y] = Bs[buf][4 * ks + lk][wc * 32 + 16 * y + lr];
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
            }
        }
        if (c + 1 < nchunk) store(buf ^ 1);
        __syncthreads();
    }

    const int I0 = ti * CT + wr * 64, J0 = tj * CT + wc * 32;
    double *Cd = a.C + (size_t)d * a.c_stride;
    if (a.mode == COV_GEN) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = I0 + 16 * x + lk + 4 * q;
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const int j = J0 + 16 * y + lr;
                    if (i < a.arows && j < a.ncols) Cd[(size_t)i * a.ldc + j] = acc[x][y][q];
                }
            }
        return;
    }

    // ---- COV_SYM epilogue: the tile's row and column inputs in LDS (the chunk buffers are free), p-major ----
    const int P = a.P;
    double *xr = lds, *xc = lds + MAXP * CT, *xxr = lds + 2 * MAXP * CT, *xxc = xxr + CT;
    const double var = a.variance[d];
    const double *lend = a.len + (size_t)d * P;
    if (tid < 2 * CT) {
        const int side = tid >> 7, r = tid & (CT - 1);
        const int row = (side ? tj : ti) * CT + r;
        double *dst = side ? xc : xr;
        double s = 0.0;
        for (int p = 0; p < P; ++p) {
            const double v = row < a.N ? a.x[(size_t)row * P + p] : 0.0;
            double u;
            if (a.kind == 0) { u = v / lend[p]; s += u * u; }                   // kernel_matrix_kernel: a = x_p / l_p, xx += a * a
            else u = side ? v : v * var;                                         // LinearK: (x_i * variance) . x_j
            dst[p * CT + r] = u;
        }
        (side ? xxc : xxr)[r] = s;
    }
    __syncthreads();
    double xxj[2];
#pragma unroll
    for (int y = 0; y < 2; ++y) xxj[y] = xxc[wc * 32 + 16 * y + lr];
    const bool diag_tile = ti == tj;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ilr = wr * 64 + 16 * x + lk + 4 * q, i = ti * CT + ilr;
            const double xxi = xxr[ilr];
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const int j = J0 + 16 * y + lr;
                if (i >= a.N || j >= a.N || (diag_tile && j > i)) continue;
                double dot = 0.0;
                const int jl = wc * 32 + 16 * y + lr;
                for (int p = 0; p < P; ++p) dot += xr[p * CT + ilr] * xc[p * CT + jl];
                const double seed = a.kind == 0 ? kernel_value<0>(dot, xxi, xxj[y], var) : dot;
                const double v = (j == i && a.diag) ? a.diag[(size_t)i * a.nb + d] : seed - acc[x][y][q];
                Cd[(size_t)i * a.ldc + j] = v;
                if (j != i) Cd[(size_t)j * a.ldc + i] = v;
            }
        }
}

void launch_cov(hipStream_t stream, const CovArgs &a) {
    if (a.nb <= 0) return;
    unsigned ntiles;
    if (a.mode == COV_SYM) {
        if (a.N <= 0) return;
        const unsigned nt = (unsigned)((a.N + CT - 1) / CT);
        ntiles = nt * (nt + 1) / 2;
    } else {
        if (a.arows <= 0 || a.ncols <= 0) return;
        ntiles = (unsigned)(((a.arows + CT - 1) / CT) * ((a.ncols + CT - 1) / CT));
    }
    hipLaunchKernelGGL(cov_kernel, dim3(ntiles, (unsigned)a.nb), dim3(512), 0, stream, a);
}

// out[d][n] = sum_j E[d][n][j]^2 for n < N: the q_sqrt term of the per-point variance from E itself (one wavefront per row, fixed
// shuffle tree).  qsqrt_inflation forms the same sums from F and q0 on the VALU: 1.95 ms at N = 4096, M = 512, D = 4 against the
// covariance kernel's 1.4 ms.
__global__ __launch_bounds__(256) void row_sumsq_kernel(const double *E, size_t e_stride, int ld, int K, int N, size_t out_stride,
                                                        double *out) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), d = blockIdx.y, lane = threadIdx.x & 63;
    if (n >= N) return;
    const double *En = E + (size_t)d * e_stride + (size_t)n * ld;
    double s = 0.0;
    for (int j = lane; j < K; j += 64) s += En[j] * En[j];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) out[(size_t)d * out_stride + n] = s;
}
void launch_row_sumsq(hipStream_t stream, const double *E, size_t e_stride, int ld, int K, int N, int D, size_t out_stride,
                      double *out) {
    if (N <= 0 || D <= 0) return;
    hipLaunchKernelGGL(row_sumsq_kernel, dim3((unsigned)((N + 3) / 4), (unsigned)D), dim3(256), 0, stream, E, e_stride, ld, K, N,
                       out_stride, out);
}

// out[i][d] = mean[i][d] + sum_{j <= i} L_d[i][j] eps[j][d]: one wavefront per (i, d), its lanes over j, the 64 partial sums added by
// a fixed shuffle tree.  Only the lower triangle of L is read (the Cholesky leaves the upper one as it found it).
__global__ __launch_bounds__(256) void tril_matvec_kernel(const double *L, size_t l_stride, int ld, int N, int D,
                                                          const double *mean, const double *eps, double *out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), d = blockIdx.y, lane = threadIdx.x & 63;
    if (i >= N) return;
    const double *Li = L + (size_t)d * l_stride + (size_t)i * ld;
    double s = 0.0;
    for (int j = lane; j <= i; j += 64) s += Li[j] * eps[(size_t)j * D + d];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) out[(size_t)i * D + d] = mean[(size_t)i * D + d] + s;
}
void launch_tril_matvec(hipStream_t stream, const double *L, size_t l_stride, int ld, int N, int D, const double *mean,
                        const double *eps, double *out) {
    if (N <= 0 || D <= 0) return;
    hipLaunchKernelGGL(tril_matvec_kernel, dim3((unsigned)((N + 3) / 4), (unsigned)D), dim3(256), 0, stream, L, l_stride, ld, N, D,
                       mean, eps, out);
}

}  // namespace ffvd
