// The small kernels around the three big families of the FFVD ELBO hot path (gfx950 / MI355X, fp64): utilities, hyper-parameter
// preparation, the K_uu / K_fu / operator kernel-matrix builders, the reductions that turn factors and per-point sums into the
// terms of the bound, the skinny-product wrappers, the elementwise operators, the nll assembly, and the per-step kernels of
// rollouts and particle-Gibbs sweeps.  Cholesky is in potrf.hip / potrf_flow.hip, the projection in project.hip, the Gram
// kernel in gram.hip.
//
// Reference arithmetic restated here (TensorFlow op call sites):
//   K1/K2  kernels_multi_output.py:163-182,246-247 (SE), kernels.py:270-281 (LinearK)
//   K9/K10 conditionals_multi_output.py:253-254  logdet H, b H^{-1} b^T (from the factor: h_finish_kernel)
//   K8     conditionals_multi_output.py:255, :41 per-point explained variance
//   K11    conditionals_multi_output.py:48       GP mean A^T u
//   K12/13 likelihoods.py:76-111, dgp_model.py:105-143,248-297,326-359
//
// Every M x M matrix is padded to Mp = multiple of 64 with an identity block, T to a multiple of 64 with zero rows of K_fu,
// so no kernel has edge handling along M or T.  DESIGN.md section 3 has the layout, section 4 the kernels.
#include "kernels.h"
#include "dev_common.h"
#define FFVD_STEP_TRACE_OWNER
#include "step_bodies.h"
#if defined(FFVD_STEP_TRACE)
extern "C" int ffvd_debug_step_spans(unsigned long long *out) {      // [64 steps][4 kernels][first workgroup's start, a late end]
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ffvd::step_span), sizeof(unsigned long long) * 64 * 4 * 2);
}
extern "C" int ffvd_debug_step_trace(long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ffvd::step_trace_buf), sizeof(long long) * 4096 * 8);
}
#endif
#include <type_traits>
#include <cstdlib>

namespace ffvd {

__device__ __forceinline__ double block_sum_256(double v, double *scratch /*[256]*/) {
    const int tid = threadIdx.x;
    scratch[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) scratch[tid] += scratch[tid + s];
        __syncthreads();
    }
    double r = scratch[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------
// small utilities
// ---------------------------------------------------------------------------------------------
__global__ void fill_kernel(double *p, size_t n, double v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}
// Diagnostic (schedule tests, FFVD_DEBUG_SIDE_DELAY_US / FFVD_DEBUG_MAIN_DELAY_US): one wavefront that occupies its stream for `us`
// microseconds of the 100 MHz wall clock and touches no memory.
__global__ void spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
void launch_spin(hipStream_t stream, int us) {
    if (us > 0) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, stream, (long long)us * 100);
}
void launch_fill(hipStream_t stream, double *p, size_t n, double v) {
    if (n == 0) return;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(256), 0, stream, p, n, v);
}

// ---------------------------------------------------------------------------------------------
// hyper-parameter preparation: variance = exp(logvariance) (kernels_multi_output.py:157),
// lengthscales = exp(loglengthscales) (:161), Zs = Z / lengthscales (:170), zz = reduce_sum(square(Zs)) (:171)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_hypers_kernel(int kind, const double *Z, int M, int Mp, int P, int d_begin,
                                                          const double *logvar, const double *loglen,
                                                          double *variance, double *len, double *Zs, double *zz,
                                                          int32_t *info, int ninfo) {
    __shared__ double ls[MAXP];
    const int dl = blockIdx.x, dg = d_begin + dl, tid = threadIdx.x;
    if (info && dl == 0)                             // re-arm the factorisation flags of this iteration
        for (int i = tid; i < ninfo; i += 256) info[i] = 0;
    if (tid == 0) variance[dl] = exp(logvar[dg]);
    if (tid < P) {
        double l = (kind == 0) ? exp(loglen[(size_t)dg * P + tid]) : 1.0;
        ls[tid] = l;
        len[(size_t)dl * P + tid] = l;
    }
    __syncthreads();
    for (int m = tid; m < Mp; m += 256) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) {
            double v = (m < M) ? Z[(size_t)m * P + p] / ls[p] : 0.0;
            Zs[((size_t)dl * Mp + m) * P + p] = v;
            s += v * v;
        }
        zz[(size_t)dl * Mp + m] = s;
    }
}
void launch_prep_hypers(hipStream_t stream, int kind, const double *Z, int M, int Mp, int P, int Dl, int d_begin,
                        const double *logvar, const double *loglen, double *variance, double *len,
                        double *Zs, double *zz, int32_t *info, int ninfo) {
    hipLaunchKernelGGL(prep_hypers_kernel, dim3(Dl), dim3(256), 0, stream, kind, Z, M, Mp, P, d_begin, logvar,
                       loglen, variance, len, Zs, zz, info, ninfo);
}

// One workgroup = KUU_ROWS rows x 256 consecutive columns.  The 256 rows z_j are staged once through LDS with coalesced loads
// (row stride P | 1 doubles: conflict-free reads whatever P) and reused for every row i, whose z_i is a scalar operand.  The
// first version (one output per thread, 256 per workgroup, operands from global) was bound by the dispatch of its tiny
// workgroups: 147 us for the 16 matrices of config 5 (32768 workgroups), 12 us for the 4 of config 2.
// The row operands z_i (and |z_i|^2) go through LDS too and the inner product runs over a compile-time PM >= P with zero padding
// (same terms in the same order, then zeros): with a run-time P the p loop was not unrolled and read z_i[p] from global memory
// with a wait per iteration -- 19 us for the 4 matrices of config 2, 37-46 us for the 16 of config 5 (P = 17), for a few
// microseconds of arithmetic.
constexpr int KUU_ROWS = 16;
template <int PM>
__global__ __launch_bounds__(256) void kuu_build_kernel(int kind, HyperView hv, int M, int Mp, int P, double jitter,
                                                        double *A, double *Kcopy, int zt_rows, double *zero, int nzero) {
    extern __shared__ double zs_lds[];                    // [256][P | 1] | zi [KUU_ROWS][PM] | zzi [KUU_ROWS]
    const int dl = blockIdx.z, tid = threadIdx.x;
    // the progress words of the dataflow Cholesky that follows on the same stream (launch_kuu_build, flow_words): one launch less
    if (zero && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = tid; i < nzero; i += 256) zero[i] = 0.0;
    const int ncc = (Mp + 255) / 256;                     // column chunks per row
    const int i0 = (int)(blockIdx.x / ncc) * KUU_ROWS, j0 = (int)(blockIdx.x % ncc) * 256;
    const int j = j0 + tid;
    double *slab = A + (size_t)dl * 2 * Mp * Mp;
    if (blockIdx.y == 1) {   // extra rows: identity, becomes L^{-T}
        if (zt_rows) {       // ... or (LinearK through its rank) ONE 64-row block holding Z^T, which becomes C = Z^T L^-T: rows >= P zero
            if (j < Mp && i0 < NB)
                for (int r = 0; r < KUU_ROWS; ++r) {
                    const int i = i0 + r;
                    slab[(size_t)Mp * Mp + (size_t)i * Mp + j] = (i < P) ? hv.Zs[((size_t)dl * Mp + j) * P + i] : 0.0;
                }
            return;
        }
        if (j < Mp)
            for (int r = 0; r < KUU_ROWS && i0 + r < Mp; ++r) slab[(size_t)Mp * Mp + (size_t)(i0 + r) * Mp + j] = (i0 + r == j) ? 1.0 : 0.0;
        return;
    }
    const int ld = P | 1;
    {
        const int nrow = (j0 + 256 <= Mp) ? 256 : Mp - j0;
        const double *zsrc = hv.Zs + ((size_t)dl * Mp + j0) * P;
        int r = tid / P, c = tid % P;                     // element e = tid + 256 k  <->  (r, c), advanced without divisions
        const int dr = 256 / P, dc = 256 % P;
        for (int e = tid; e < nrow * P; e += 256) {
            zs_lds[r * ld + c] = zsrc[e];
            r += dr; c += dc;
            if (c >= P) { c -= P; ++r; }
        }
    }
    double *zi_lds = zs_lds + (size_t)256 * ld, *zzi_lds = zi_lds + KUU_ROWS * PM;
    for (int e = tid; e < KUU_ROWS * PM; e += 256) {
        const int rr = e / PM, pp = e % PM, i = i0 + rr;
        zi_lds[e] = (pp < P && i < Mp) ? hv.Zs[((size_t)dl * Mp + i) * P + pp] : 0.0;
    }
    if (tid < KUU_ROWS) zzi_lds[tid] = (kind == 0 && i0 + tid < Mp) ? hv.zz[(size_t)dl * Mp + i0 + tid] : 0.0;
    __syncthreads();
    if (j >= Mp) return;
    double zl[PM];
#pragma unroll
    for (int p = 0; p < PM; ++p) zl[p] = (p < P) ? zs_lds[(size_t)tid * ld + p] : 0.0;
    const double var = hv.variance[dl];
    const double zzj = (kind == 0 && j < M) ? hv.zz[(size_t)dl * Mp + j] : 0.0;
    for (int r = 0; r < KUU_ROWS && i0 + r < Mp; ++r) {
        const int i = i0 + r;
        double v;
        if (i >= M || j >= M) {
            v = (i == j) ? 1.0 : 0.0;
        } else {
            const double *zi = zi_lds + r * PM;
            double dot = 0.0;
            if (kind == 0) {
#pragma unroll
                for (int p = 0; p < PM; ++p) dot += zi[p] * zl[p];
                v = kernel_value<0>(dot, zzi_lds[r], zzj, var);
            } else {
#pragma unroll
                for (int p = 0; p < PM; ++p) dot += (zi[p] * var) * zl[p];
                v = dot;
            }
            if (i == j) v += jitter;   // conditionals_multi_output.py:108,159
        }
        const size_t idx = (size_t)i * Mp + j;
        slab[idx] = v;
        if (Kcopy) Kcopy[(size_t)dl * Mp * Mp + idx] = v;     // the factorisation overwrites `slab` in place
    }
}
void launch_kuu_build(hipStream_t stream, int kind, HyperView hv, int M, int Mp, int P, int Dl, double jitter, double *A,
                      double *Kcopy, bool zt_rows, double *flow_words) {
    // (what potrf_flow_clear zeroes for Dl matrices)
    const int nzero = flow_words ? (int)(potrf_flow_words(Dl) / 2) : 0;
    const int ncc = (Mp + 255) / 256, nrg = (Mp + KUU_ROWS - 1) / KUU_ROWS;
    dim3 grid((unsigned)(ncc * nrg), 2, Dl);
    if (P <= 8)
        hipLaunchKernelGGL(kuu_build_kernel<8>, grid, dim3(256), ((size_t)256 * (P | 1) + KUU_ROWS * 9) * sizeof(double), stream, kind, hv, M,
                           Mp, P, jitter, A, Kcopy, zt_rows ? 1 : 0, flow_words, nzero);
    else
        hipLaunchKernelGGL(kuu_build_kernel<MAXP>, grid, dim3(256), ((size_t)256 * (P | 1) + KUU_ROWS * (MAXP + 1)) * sizeof(double), stream,
                           kind, hv, M, Mp, P, jitter, A, Kcopy, zt_rows ? 1 : 0, flow_words, nzero);
}

// out[dl][i][j] = in[dl][j][i] for Dl square Mp x Mp matrices (L^-T -> L^-1)
__global__ __launch_bounds__(256) void transpose_kernel(const double *in, size_t in_stride, double *out, size_t out_stride,
                                                        int Mp) {
    __shared__ double t[64][65];
    const int dl = blockIdx.z, bi = blockIdx.y * 64, bj = blockIdx.x * 64, tid = threadIdx.x;
    const double *I = in + (size_t)dl * in_stride;
    double *O = out + (size_t)dl * out_stride;
    for (int r = tid >> 6; r < 64; r += 4) t[r][tid & 63] = I[(size_t)(bi + r) * Mp + bj + (tid & 63)];
    __syncthreads();
    for (int r = tid >> 6; r < 64; r += 4) O[(size_t)(bj + r) * Mp + bi + (tid & 63)] = t[tid & 63][r];
}
void launch_transpose(hipStream_t stream, const double *in, size_t in_stride, double *out, size_t out_stride, int Mp,
                      int Dl) {
    hipLaunchKernelGGL(transpose_kernel, dim3(Mp / 64, Mp / 64, Dl), dim3(256), 0, stream, in, in_stride, out,
                       out_stride, Mp);
}

// K_fu materialised (only the K_uu + K_uf K_fu / Q route needs it in HBM): out[bz][t][m] = K_d(x_t, Z_m),
// zero for t >= T or m >= M.  64 x 64 tile per workgroup; thread (tid & 63) owns a column, 16 rows.
// SMALLP (P <= 8): x / l is kept row-major and zero-padded to 8 components in LDS, so a row is four 16-byte
// broadcast reads and the dot product eight unconditional FMAs (with a run-time `p < P` test the compiler emits one
// LDS round trip and one scalar branch per component: 0.55 instead of 0.40 ms for the 2 GiB of config 2).
// NQ > 0: the SMALLP form with 2 NQ components (P = 5: six FMAs and three reads per element instead of eight and four -- the
// build is bound by its fp64 VALU work as much as by the write); NQ = 0: the general form.
template <int KIND, int NQ, bool NT>
__global__ __launch_bounds__(256) void kfu_build_kernel(ProjectArgs a) {
    kfu_build_body<KIND, NQ, NT>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}


__global__ __launch_bounds__(256) void brow_finish_kernel(const double *gpart, int nblk, int Mp, int Dl, int d_begin, int b0,
                                                          const double *log_Q, double yn_over_batch, double *H, size_t h_stride, int brow) {
    const int m = blockIdx.x * 256 + threadIdx.x, bz = blockIdx.y;
    if (m >= Mp) return;
    const double *g = gpart + (size_t)bz * nblk * Mp + m;
    double acc = 0.0;
    for (int k0 = 0; k0 < nblk; k0 += 8) {      // eight independent loads in flight, one fixed summation order
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (k0 + k < nblk) ? g[(size_t)(k0 + k) * Mp] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += v[k];
    }
    const int dg = d_begin + (b0 + bz) % Dl;
    H[(size_t)bz * h_stride + (size_t)brow * Mp + m] = acc * (yn_over_batch / exp(log_Q[dg]));
}
void launch_brow_finish(hipStream_t stream, const double *gpart, int nblk, int Mp, int Dl, int d_begin, int b0, int nb,
                        const double *log_Q, double yn_over_batch, double *H, size_t h_stride, int brow) {
    hipLaunchKernelGGL(brow_finish_kernel, dim3((Mp + 255) / 256, nb), dim3(256), 0, stream, gpart, nblk, Mp, Dl, d_begin, b0, log_Q,
                       yn_over_batch, H, h_stride, brow);
}
template <bool NT>
static void launch_kfu_build_nt(hipStream_t stream, const ProjectArgs &a) {
    dim3 grid(a.Tp / 64, a.Mp / 64, a.nb);
    if (a.P <= 8) {
        const int nq = (a.P + 1) / 2;
        if (a.kind == 0) {
            if (nq <= 2) hipLaunchKernelGGL((kfu_build_kernel<0, 2, NT>), grid, dim3(256), 0, stream, a);
            else if (nq == 3) hipLaunchKernelGGL((kfu_build_kernel<0, 3, NT>), grid, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((kfu_build_kernel<0, 4, NT>), grid, dim3(256), 0, stream, a);
        } else hipLaunchKernelGGL((kfu_build_kernel<1, 4, NT>), grid, dim3(256), 0, stream, a);
    } else {
        if (a.kind == 0) hipLaunchKernelGGL((kfu_build_kernel<0, 0, NT>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((kfu_build_kernel<1, 0, NT>), grid, dim3(256), 0, stream, a);
    }
}
template <int KIND, int NQ, int MW>
__global__ __launch_bounds__(256) void kfu_build_t_kernel(ProjectArgs a, int ldt) {
    kfu_build_t_body<KIND, NQ, MW>(a, ldt, blockIdx.x, blockIdx.y, blockIdx.z);
}
// K(x, Z) of a step, transposed: a.F receives KT[nb][Mp][ldt] (ldt >= a.Tp) -- the skinny product's coalesced A operand.  A step has
// few rows: tiles of 64 rows x 16 inducing points (4 per wavefront) put its 128 x 512 x 4 values on 256 workgroups instead of 64.
void launch_kfu_build_t(hipStream_t stream, const ProjectArgs &a, int ldt) {
    constexpr int MW = 4;
    dim3 grid(a.Tp / 64, a.Mp / (4 * MW), a.nb);
    if (a.P <= 8) {
        const int nq = (a.P + 1) / 2;
        if (a.kind == 0) {
            if (nq <= 2) hipLaunchKernelGGL((kfu_build_t_kernel<0, 2, MW>), grid, dim3(256), 0, stream, a, ldt);
            else if (nq == 3) hipLaunchKernelGGL((kfu_build_t_kernel<0, 3, MW>), grid, dim3(256), 0, stream, a, ldt);
            else hipLaunchKernelGGL((kfu_build_t_kernel<0, 4, MW>), grid, dim3(256), 0, stream, a, ldt);
        } else hipLaunchKernelGGL((kfu_build_t_kernel<1, 4, MW>), grid, dim3(256), 0, stream, a, ldt);
    } else {
        if (a.kind == 0) hipLaunchKernelGGL((kfu_build_t_kernel<0, 0, MW>), grid, dim3(256), 0, stream, a, ldt);
        else hipLaunchKernelGGL((kfu_build_t_kernel<1, 0, MW>), grid, dim3(256), 0, stream, a, ldt);
    }
}
void launch_kfu_build(hipStream_t stream, const ProjectArgs &a) {
    // streaming stores for outputs of 1 GB and more (nothing of them survives in a cache until the Gram kernel reads it)
    const bool nt = (size_t)a.nb * a.Tp * a.Mp * sizeof(double) >= ((size_t)1 << 30);
    if (nt) launch_kfu_build_nt<true>(stream, a);
    else launch_kfu_build_nt<false>(stream, a);
}

// Operator-API kernel matrix (one kernel, arbitrary N, N2; no padding).
__global__ __launch_bounds__(256) void kernel_matrix_kernel(int kind, const double *X, int N, const double *X2, int N2,
                                                            int P, double logvar, const double *loglen, double jitter,
                                                            int same, double *out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)N * N2) return;
    const int i = (int)(idx / N2), j = (int)(idx % N2);
    const double var = exp(logvar);
    const double *xi = X + (size_t)i * P, *zj = X2 + (size_t)j * P;
    double v;
    if (kind == 0) {
        double dot = 0.0, xx = 0.0, zz = 0.0;
        for (int p = 0; p < P; ++p) {
            double l = exp(loglen[p]);
            double a = xi[p] / l, b = zj[p] / l;
            dot += a * b; xx += a * a; zz += b * b;
        }
        v = kernel_value<0>(dot, xx, zz, var);
    } else {
        double dot = 0.0;
        for (int p = 0; p < P; ++p) dot += (xi[p] * var) * zj[p];
        v = dot;
    }
    if (same && i == j) v += jitter;
    out[idx] = v;
}
void launch_kernel_matrix(hipStream_t stream, int kind, const double *X, int N, const double *X2, int N2, int P,
                          double logvar, const double *loglen_dev, double jitter, int same, double *out) {
    size_t n = (size_t)N * N2;
    if (n == 0) return;
    hipLaunchKernelGGL(kernel_matrix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, kind, X, N, X2,
                       N2, P, logvar, loglen_dev, jitter, same, out);
}
__global__ void kernel_diag_kernel(int kind, const double *X, int N, int P, double logvar, double *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double var = exp(logvar);
    if (kind == 0) { out[i] = var; return; }                     // kernels_multi_output.py:199-200
    double s = 0.0;
    for (int p = 0; p < P; ++p) { double x = X[(size_t)i * P + p]; s += (x * x) * var; }   // kernels.py:278-281
    out[i] = s;
}
void launch_kernel_diag(hipStream_t stream, int kind, const double *X, int N, int P, double logvar, double *out) {
    if (N == 0) return;
    hipLaunchKernelGGL(kernel_diag_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, kind, X, N, P, logvar, out);
}

// ---------------------------------------------------------------------------------------------
// logdet(H) = 2 sum log diag(L_H)  (tf.linalg.logdet, :253);  b H^{-1} b^T = |L_H^{-1} b|^2 (:254)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void h_finish_kernel(const double *H, int Mp, size_t h_stride, double *hterms, int yrow) {
    __shared__ double scratch[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *Hb = H + (size_t)b * h_stride;
    double ld = 0.0, qd = 0.0;
    for (int i = tid; i < Mp; i += 256) {
        ld += log(Hb[(size_t)i * Mp + i]);
        const double y = Hb[(size_t)yrow * Mp + i];
        qd += y * y;
    }
    ld = block_sum_256(ld, scratch);
    qd = block_sum_256(qd, scratch);
    if (tid == 0) { hterms[2 * b] = 2.0 * ld; hterms[2 * b + 1] = qd; }
}
void launch_h_finish(hipStream_t stream, const double *H, int Mp, size_t h_stride, int nb, double *hterms, int yrow) {
    hipLaunchKernelGGL(h_finish_kernel, dim3(nb), dim3(256), 0, stream, H, Mp, h_stride, hterms, yrow > 0 ? yrow : Mp);
}

// ---------------------------------------------------------------------------------------------
// Per-chain streaming reductions (likelihoods.py:76-111; dgp_model.py:250-252,283-284,346-351)
// chain_terms[s] = { lik quadratic sum, transition quadratic sum, trace sum, prior_x_0 }
// ---------------------------------------------------------------------------------------------
constexpr int CR_SPLIT = 8;     // workgroups per chain (four times as many from 8 latent dims on: a row's terms are a loop over the dims)
static int chain_reduce_split(int Dl) { return Dl >= 8 ? 4 * CR_SPLIT : CR_SPLIT; }
__global__ __launch_bounds__(256) void chain_reduce_kernel(ReduceArgs a, double *partial /*[S][nsplit][4]*/, const int nsplit) {
    __shared__ double scratch[256];
    const int s = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    const int T = a.T, D = a.D;
    const double *Xs = a.X + (size_t)s * (T + 1) * D;
    double lik = 0.0, xq = 0.0, tr = 0.0;
    for (int t = part * 256 + tid; t < T; t += 256 * nsplit) {
        if (a.shared_terms) {
            for (int j = 0; j < a.Ydim; ++j) {
                double ym = 0.0;
                for (int d = 0; d < D; ++d) ym += Xs[(size_t)(t + 1) * D + d] * a.CC[(size_t)d * a.Ydim + j];   // :76-79
                ym += a.DD[j];
                const double R = exp(a.log_Rchols[j]);          // Rchols[0] = first row (dgp_model.py:250)
                const double r = (a.Y[(size_t)t * a.Ydim + j] - ym) / R;
                lik += -0.5 * (r * r);
            }
        }
        double xsq = 0.0;
        if (a.kind == 1) {                                       // LinearK.Kdiag (kernels.py:278-281), per unit variance
            const double *xr = a.xk + (size_t)s * a.xk_chain_stride + (size_t)t * a.xk_ld;
            for (int p = 0; p < a.xk_cols; ++p) xsq += xr[p] * xr[p];
            for (int p = 0; p < a.C; ++p) { double x = a.ctrl[(size_t)t * a.C + p]; xsq += x * x; }
        }
        for (int dl = 0; dl < a.Dl; ++dl) {
            const int dg = a.d_begin + dl;
            const double Q = exp(a.log_Q[dg]);
            const double sq = sqrt(Q);                           // Q ** 0.5 (dgp_model.py:284,351)
            const size_t bb = ((size_t)s * a.Dl + dl) * a.ng;
            double rs = 0.0, fm = 0.0;
            for (int g = 0; g < a.ng; ++g) {
                if (a.rowsq) rs += a.rowsq[(bb + g) * a.Tp + t];
                if (a.branch == 0) fm += a.fmean[(bb + g) * a.Tp + t];
            }
            const double kdiag = (a.kind == 0) ? a.variance[dl] : xsq * a.variance[dl];
            tr += -0.5 * ((kdiag - rs) / Q);                     // conditionals_multi_output.py:255 / dgp_model.py:348
            const double x1 = Xs[(size_t)(t + 1) * D + dg], x0 = Xs[(size_t)t * D + dg];
            double r;
            if (a.branch == 1) r = (x1 - x0) / sq;               // dgp_model.py:283-284
            else r = (x1 - (fm + x0)) / sq;                      // dgp_model.py:346,351
            xq += -0.5 * (r * r);
        }
    }
    lik = block_sum_256(lik, scratch);
    xq = block_sum_256(xq, scratch);
    tr = block_sum_256(tr, scratch);
    if (tid == 0) {
        double *o = partial + ((size_t)s * nsplit + part) * 4;
        o[0] = lik; o[1] = xq; o[2] = tr;
    }
}
__global__ void chain_combine_kernel(ReduceArgs a, const double *partial, const int nsplit) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    double lik = 0.0, xq = 0.0, tr = 0.0;
    for (int p = 0; p < nsplit; ++p) {
        const double *o = partial + ((size_t)s * nsplit + p) * 4;
        lik += o[0]; xq += o[1]; tr += o[2];
    }
    const double *Xs = a.X + (size_t)s * (a.T + 1) * a.D;
    double px0 = 0.0;
    for (int d = 0; d < a.D; ++d) px0 += Xs[d] * Xs[d];
    double *o = a.chain_terms + (size_t)s * 8;
    o[0] = lik; o[1] = xq; o[2] = tr; o[3] = a.skip_x0 ? 0.0 : -px0 / 2.0;     // prior_x_0 dgp_model.py:252
    bool bad = false;
    for (int i = 0; i < a.ninfo; ++i) bad = bad || a.info[i] != 0;
    if (bad) o[0] = o[1] = o[2] = __longlong_as_double(0x7ff8000000000000LL);
}
void launch_chain_reduce(hipStream_t stream, const ReduceArgs &a, double *partial) {
    const int nsplit = chain_reduce_split(a.Dl);
    hipLaunchKernelGGL(chain_reduce_kernel, dim3(a.S, nsplit), dim3(256), 0, stream, a, partial, nsplit);
    hipLaunchKernelGGL(chain_combine_kernel, dim3((a.S + 63) / 64), dim3(64), 0, stream, a, partial, nsplit);
}

// conditional() outputs (conditionals_multi_output.py:41,48,120): mean N x D, var N x D
// One output (n, d) per group of 16 lanes: the lanes share the partial-sum groups (the skinny products of the step loops leave
// Mp / 16 of them per array) and add them by a shuffle tree -- a thread walking 96 dependent loads per output took 18 us.
__global__ __launch_bounds__(256) void conditional_finish_kernel(int kind, const double *x, int N, int P, const double *variance,
                                          const double *rowsq, const double *fmean, int ng, int Tp, int D,
                                          double *mean, double *var, const double *extra /*[D][extra_ng][Tp] or null*/,
                                          int extra_ng) {
    conditional_finish_body(blockIdx.x, kind, x, N, P, variance, rowsq, fmean, ng, Tp, D, mean, var, extra, extra_ng);
}
void launch_conditional_finish(hipStream_t stream, int kind, const double *x, int N, int P, const double *variance,
                               const double *rowsq, const double *fmean, int ng, int Tp, int D, double *mean,
                               double *var, const double *extra, int extra_ng) {
    if (N * D == 0) return;
    hipLaunchKernelGGL(conditional_finish_kernel, dim3((N * D * 16 + 255) / 256), dim3(256), 0, stream, kind, x, N, P,
                       variance, rowsq, fmean, ng, Tp, D, mean, var, extra, extra_ng);
}

// Skinny product for the step loops (rollouts, particle Gibbs: at most a few hundred rows per latent dim and step):
//   C[b] (rows x N) = A[b] (rows x K) * B (K x N),   optionally  sq[b][slab][r] = sum_{n in slab} C[r][n]^2,
//                                                                dot[b][slab][r] = sum_{n in slab} C[r][n] u[b][n].
// One workgroup = 32 rows x 16 columns, its four wavefronts a quarter of the k range each (operands straight from L2, no
// LDS staging: 64 MFMAs per wavefront at K = 512), partial tiles added through LDS in fixed order.  N / 16 x rows / 32 x nb
// workgroups instead of the handful of 128 x 128 tiles the projection GEMM cuts such a product into: 50 -> 7 us per step at 32 rows.
// `upper`: B[k][n] = 0 for k > n (L^-T), the k range of a slab ends at its last column.
__global__ __launch_bounds__(256) void skinny_gemm_kernel(SkinnyArgs a) {
    skinny_body(a, blockIdx.x, blockIdx.y, blockIdx.z);
}
// Same product from a 1-D grid for nb <= 8 units: workgroup id i runs on XCD i % 8 (round-robin dispatch), unit u owns the XCDs
// x with x % nb == u and deals its (slab, row group) pairs over them, so a unit's A rows and B slabs are fetched into one or two L2s
// instead of all eight.  The arithmetic of a workgroup does not depend on where it runs.
__global__ __launch_bounds__(256) void skinny_gemm_xcd_kernel(SkinnyArgs a, int nbx, int nby) {
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int u = xcd % a.nb, j = xcd / a.nb, cnt = (8 - u + a.nb - 1) / a.nb;
    const int widx = k * cnt + j;
    if (widx >= nbx * nby) return;
    // a CU takes slots k and k + 32 of its XCD (two workgroups per CU, 32 CUs; HW_ID stamps, profiles/r05_step_trace.txt): every other
    // block of 32 slots walks the slabs backwards, so that a long triangular slab (up to K / 16 k blocks) shares its CU's MFMA pipes
    // with a short one.  The choice depends on the row group only: (slab, row group) pairs are still covered once each.
    const int by = widx / nbx, rev = ((by * nbx) / (32 * cnt)) & 1;
    const int bx = widx % nbx;
    skinny_body(a, rev ? nbx - 1 - bx : bx, by, u);
}
// rows <= Tp (a multiple of 32) rows of A exist; N, K multiples of 16.
void launch_skinny_gemm(hipStream_t stream, const double *A, size_t a_stride, int lda, const double *B, size_t b_stride, int ldb,
                        int upper, int rows, int K, int N, int nb, int Tp, double *C, size_t c_stride, int ldc,
                        const double *u, size_t u_stride, double *sq, double *dot, const double *B2, size_t b2_stride, int ldb2,
                        int N2, double *sq2, int a_trans, int upper2) {
    if (rows <= 0 || nb <= 0) return;
    SkinnyArgs a{A, a_stride, lda, B, b_stride, ldb, upper, rows, K, N, nb, Tp, C, c_stride, ldc, u, u_stride, sq, dot,
                 B2, b2_stride, ldb2, B2 ? N2 : 0, sq2, a_trans, B2 ? upper2 : 0};
    const int nbx = N / 16 + (B2 ? N2 / 16 : 0), nby = (rows + 31) / 32;
    static const bool flat = !(getenv("FFVD_SKINNY_GRID3D") && atoi(getenv("FFVD_SKINNY_GRID3D")));
    if (flat && nb <= 8) {
        const int slots = (nbx * nby + 8 / nb - 1) / (8 / nb);       // per XCD: the unit with the fewest XCDs has 8 / nb of them
        hipLaunchKernelGGL(skinny_gemm_xcd_kernel, dim3(8 * slots), dim3(256), 0, stream, a, nbx, nby);
    } else
        hipLaunchKernelGGL(skinny_gemm_kernel, dim3(nbx, nby, nb), dim3(256), 0, stream, a);
}

// out[b][i] = sum_j W[b][i][j] * y[b][j]   (posterior mean of the whitened inducing outputs: L_H^-T (L_H^-1 b))
__global__ __launch_bounds__(256) void matvec_kernel(const double *W, size_t w_stride, const double *y, size_t y_stride,
                                                     int Mp, double *out, int out_ld, int out_bs, int M, int w_mod) {
    __shared__ double ys[2048];
    const int b = blockIdx.y, tid = threadIdx.x;
    const double *Wb = W + (size_t)(w_mod > 0 ? b % w_mod : b) * w_stride, *yb = y + (size_t)b * y_stride;
    for (int j0 = 0; j0 < Mp; j0 += 2048) {     // Mp <= 2048 per tile of y
        for (int j = tid; j < 2048 && j0 + j < Mp; j += 256) ys[j] = yb[j0 + j];
        __syncthreads();
        const int i = blockIdx.x * 256 + tid;
        if (i < M) {
            double acc = (j0 == 0) ? 0.0 : out[(size_t)i * out_ld + (size_t)b * out_bs];
            const int jn = (Mp - j0 < 2048) ? Mp - j0 : 2048;
            for (int j = 0; j < jn; ++j) acc += Wb[(size_t)i * Mp + j0 + j] * ys[j];
            out[(size_t)i * out_ld + (size_t)b * out_bs] = acc;
        }
        __syncthreads();
    }
}
void launch_matvec(hipStream_t stream, const double *W, size_t w_stride, const double *y, size_t y_stride, int Mp,
                   double *out, int out_ld, int out_bs, int M, int batch, int w_mod) {
    hipLaunchKernelGGL(matvec_kernel, dim3((M + 255) / 256, batch), dim3(256), 0, stream, W, w_stride, y, y_stride, Mp, out,
                       out_ld, out_bs, M, w_mod);
}

// extra[b][n] = sum_j ( sum_m F[b][n][m] * Qs[m][j] )^2   -- the q_sqrt variance inflation of
// base_conditional_after_kernel_precalculation (conditionals_multi_output.py:371-380) with LTA^T = F q_sqrt.
__global__ __launch_bounds__(256) void qsqrt_inflation_kernel(const double *F, size_t f_stride, int Tp, int Mp, int M,
                                                              const double *Qs /*M x M*/, double *extra) {
    __shared__ double fr[2048];
    __shared__ double scratch[256];
    const int n = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const double *Fr = F + (size_t)b * f_stride + (size_t)n * Mp;
    for (int m = tid; m < M; m += 256) fr[m] = Fr[m];
    __syncthreads();
    double acc = 0.0;
    for (int j = tid; j < M; j += 256) {
        double v = 0.0;
        for (int m = 0; m < M; ++m) v += fr[m] * Qs[(size_t)m * M + j];
        acc += v * v;
    }
    acc = block_sum_256(acc, scratch);
    if (tid == 0) extra[(size_t)b * Tp + n] = acc;
}
void launch_qsqrt_inflation(hipStream_t stream, const double *F, size_t f_stride, int Tp, int Mp, int M, const double *Qs,
                            double *extra, int N, int batch) {
    if (N == 0) return;
    hipLaunchKernelGGL(qsqrt_inflation_kernel, dim3(N, batch), dim3(256), 0, stream, F, f_stride, Tp, Mp, M, Qs, extra);
}

// Operator-API elementwise kernels (likelihoods.py:76-79, 89-111; utils.py:11)
__global__ void predict_mean_kernel(const double *X, int N, int D, const double *CC, const double *DD, int J, double *out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * J) return;
    const int n = idx / J, j = idx % J;
    double v = 0.0;
    for (int d = 0; d < D; ++d) v += X[(size_t)n * D + d] * CC[(size_t)d * J + j];     // tf.matmul(X_end, CC)
    out[idx] = v + DD[j];                                                              // + DD
}
// mode 0: logdensity_norm_diag (N outputs), mode 1: logdensity_norm_diag_nonvec (N x J outputs)
__global__ void logdensity_kernel(int mode, const double *y, const double *ymean, const double *R, int N, int J, double *out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == 1) {
        if (idx >= N * J) return;
        const int j = idx % J;
        const double r = (y[idx] - ymean[idx]) / R[j];
        out[idx] = -0.5 * (r * r) + (-log(R[j]));
        return;
    }
    if (idx >= N) return;
    double e = 0.0, lr = 0.0;
    for (int j = 0; j < J; ++j) {
        const double r = (y[(size_t)idx * J + j] - ymean[(size_t)idx * J + j]) / R[j];
        e += r * r;
        lr += log(R[j]);
    }
    out[idx] = -0.5 * e + (-lr);
}
__global__ void get_rand_kernel(const double *mean, const double *var, const double *eps, size_t n, double *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mean[i] + eps[i] * sqrt(var[i]);
}
void launch_predict_mean(hipStream_t stream, const double *X, int N, int D, const double *CC, const double *DD, int J,
                         double *out) {
    if (N * J == 0) return;
    hipLaunchKernelGGL(predict_mean_kernel, dim3((N * J + 255) / 256), dim3(256), 0, stream, X, N, D, CC, DD, J, out);
}
void launch_logdensity(hipStream_t stream, int mode, const double *y, const double *ymean, const double *R, int N, int J,
                       double *out) {
    const int n = mode == 1 ? N * J : N;
    if (n == 0) return;
    hipLaunchKernelGGL(logdensity_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, mode, y, ymean, R, N, J, out);
}
void launch_get_rand(hipStream_t stream, const double *mean, const double *var, const double *eps, size_t n, double *out) {
    if (n == 0) return;
    hipLaunchKernelGGL(get_rand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mean, var, eps, n, out);
}

// ---------------------------------------------------------------------------------------------
// Priors + nll assembly (dgp_model.py:105-143, 259-297, 326-334)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void finalize_kernel(FinalizeArgs a) {
    __shared__ double scratch[4][10];
    if (a.prior_sums) {               // formed earlier in the iteration by the same code (prior_sums_kernel): the same bits
        double sm[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) sm[i] = a.prior_sums[i];
        finalize_assemble<256>(a, scratch, sm);
    } else finalize_body<256>(a, scratch);
}
__global__ __launch_bounds__(256) void prior_sums_kernel(FinalizeArgs a, double *out) {
    __shared__ double scratch[4][10];
    double sm[10];
    finalize_priors<256>(a, scratch, sm);
#pragma unroll
    for (int i = 0; i < 10; ++i)
        if ((int)threadIdx.x == i) out[i] = sm[i];
}
void launch_prior_sums(hipStream_t stream, const FinalizeArgs &a, double *out) {
    hipLaunchKernelGGL(prior_sums_kernel, dim3(1), dim3(256), 0, stream, a, out);
}
void launch_finalize(hipStream_t stream, const FinalizeArgs &a) {
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, stream, a);
}

// One step of the posterior rollout (collect_samples_formal, base_model.py:304-314) for R rollouts side by side:
//   x_next = x + f_mu + eps * sqrt(f_var + Q);  predict_x[r][t] = x_next;  predict_var[r][t] = f_var + Q;
// and the GP input row of the next step, xc[r] = [x_next, control_inputs[t + 1]].
// The conditional() epilogue inside a step-loop kernel, bit for bit what conditional_finish_kernel computes: 16 lanes per (row n,
// dim d) sum the partials strided, an xor-butterfly combines them; every lane returns the sums (call with ALL lanes of the 16 active).
__global__ __launch_bounds__(256) void rollout_finish_update_kernel(FinishIn f, const double *log_Q, const double *eps_t,
                                                                    const double *ctrl_next, int R, int C, int t, int steps,
                                                                    const double *x_in, double *x_out, double *predict_x,
                                                                    double *predict_var) {
    rollout_finish_update_body(blockIdx.x, f, log_Q, eps_t, ctrl_next, R, C, t, steps, x_in, x_out, predict_x, predict_var);
}
void launch_rollout_finish_update(hipStream_t stream, int kind, const double *variance, const double *rowsq, const double *fmean,
                                  int ng, int Tp, const double *extra, int extra_ng, const double *log_Q, const double *eps_t,
                                  const double *ctrl_next, int R, int D, int C, int t, int steps, const double *x_in, double *x_out,
                                  double *predict_x, double *predict_var) {
    if (R * D == 0) return;
    FinishIn f{kind, D + C, ng, Tp, D, extra_ng, variance, rowsq, fmean, extra};
    hipLaunchKernelGGL(rollout_finish_update_kernel, dim3((R * D * 16 + 255) / 256), dim3(256), 0, stream, f, log_Q, eps_t, ctrl_next, R,
                       C, t, steps, x_in, x_out, predict_x, predict_var);
}

__global__ void rollout_update_kernel(const double *mean, const double *var, const double *log_Q, const double *eps_t,
                                      const double *ctrl_next, int R, int D, int C, int t, int steps, double *xc,
                                      double *predict_x, double *predict_var) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int P = D + C;
    if (idx >= R * P) return;
    const int r = idx / P, p = idx % P;
    if (p < D) {
        const double v = var[r * D + p] + exp(log_Q[p]);
        const double xn = (mean[r * D + p] + xc[idx]) + eps_t[r * D + p] * sqrt(v);
        const size_t o = ((size_t)r * steps + t) * D + p;
        predict_x[o] = xn;
        predict_var[o] = v;
        xc[idx] = xn;
    } else if (ctrl_next) {
        xc[idx] = ctrl_next[p - D];
    }
}
void launch_rollout_update(hipStream_t stream, const double *mean, const double *var, const double *log_Q,
                           const double *eps_t, const double *ctrl_next, int R, int D, int C, int t, int steps, double *xc,
                           double *predict_x, double *predict_var) {
    const int n = R * (D + C);
    if (n == 0) return;
    hipLaunchKernelGGL(rollout_update_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, mean, var, log_Q, eps_t,
                       ctrl_next, R, D, C, t, steps, xc, predict_x, predict_var);
}

// One workgroup: thread i < R propagates particle i and forms its log weight, thread R the reference's; the softmax
// CDF is summed sequentially in index order (as the oracle's cumsum) by one thread; then every thread i < R finds its
// ancestor by binary search and gathers.
__global__ __launch_bounds__(PG_MAXN) void pg_step_kernel(const double *mean, const double *var, const double *log_Q,
                                                          const double *eps_t, const double *unif_t, const double *y_t,
                                                          const double *x_ref_next, const double *CC, const double *DD,
                                                          const double *Rch, const double *ctrl_next, int R, int D, int C,
                                                          int Ydim, double *xc, double *cand, double *parts_next,
                                                          int32_t *idx_out) {
    pg_step_body<0>(mean, var, log_Q, eps_t, unif_t, y_t, x_ref_next, CC, DD, Rch, ctrl_next, R, D, C, Ydim, xc, cand, parts_next, idx_out);
}
void launch_pg_step(hipStream_t stream, const double *mean, const double *var, const double *log_Q, const double *eps_t,
                    const double *unif_t, const double *y_t, const double *x_ref_next, const double *CC, const double *DD,
                    const double *Rch, const double *ctrl_next, int R, int D, int C, int Ydim, double *xc, double *cand,
                    double *parts_next, int32_t *idx_out) {
    int threads = 64;
    while (threads < R + 1) threads <<= 1;
    hipLaunchKernelGGL(pg_step_kernel, dim3(1), dim3(threads), 0, stream, mean, var, log_Q, eps_t, unif_t, y_t, x_ref_next,
                       CC, DD, Rch, ctrl_next, R, D, C, Ydim, xc, cand, parts_next, idx_out);
}

}  // namespace ffvd
