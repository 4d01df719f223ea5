// Grouped collapsed posteriors: U_mean and L_H^-T of collapse_u_mean_after_kernel_precalculation (conditionals_multi_output.py:206-227,
// called at base_model.py:243-256) for G groups -- one per chain or per SG-HMC sample -- without the host in between.  The
// factorisations are the ELBO's batch launches over units b = g * D + d (ops_grouped.hip puts them together); the kernels here move their
// results from the factorisation slabs (Mp = M rounded up to 64) into the operands of the grouped rollout loop (rollout_group.h:
// Mp16 = M rounded up to 16, exact zeros in the padding and below the diagonal) or into packed result arrays.
// Pure data movement: every output element is written by exactly one thread from at most one input element, so the results are
// bit-identical run to run and independent of the launch shape.
#include "posterior_group.h"
#include "kernels.h"

namespace ffvd {

int pg_groups_per_pass(int G, int D, int Tp, int Mp) {
    const size_t per_group = (size_t)D * Tp * Mp;                        // doubles of F
    size_t n = (((size_t)2 << 30) / sizeof(double)) / per_group;
    const size_t by_grid = (size_t)32768 / (size_t)D;                    // units of a pass are a grid dimension of the batch launches
    if (n > by_grid) n = by_grid;
    if (n > (size_t)G) n = (size_t)G;
    return n < 1 ? 1 : (int)n;
}

__global__ __launch_bounds__(256) void pg_stage_x_kernel(const double *Xs, int G, int T, int D, double *Xt) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, GD = (size_t)G * D;
    if (e >= (size_t)(T + 1) * GD) return;
    const size_t t = e / GD, gd = e % GD, g = gd / D, d = gd % D;
    Xt[e] = Xs[(g * (size_t)(T + 1) + t) * D + d];
}
void launch_pg_stage_x(hipStream_t stream, const double *Xs, int G, int T, int D, double *Xt) {
    const size_t n = (size_t)(T + 1) * G * D;
    hipLaunchKernelGGL(pg_stage_x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, Xs, G, T, D, Xt);
}

// VEC: ld even -- a thread moves two neighbouring columns (16 bytes in, 16 bytes out); otherwise one.
template <bool VEC>
__global__ __launch_bounds__(256) void pg_pack_kernel(const double *src, size_t src_stride, int src_ld, int row0, int src_mod,
                                                      int src_step, int M, int upper_only, double *dst, int rows, int ld,
                                                      unsigned blocks_per_matrix) {
    const unsigned n = blockIdx.x / blocks_per_matrix, blk = blockIdx.x % blocks_per_matrix;
    const int per_row = VEC ? ld / 2 : ld;
    const size_t e = (size_t)blk * 256 + threadIdx.x;
    if (e >= (size_t)rows * per_row) return;
    const int i = (int)(e / per_row), j = (int)(e % per_row) * (VEC ? 2 : 1);
    const double *S = src + (size_t)((n % (unsigned)src_mod) * (unsigned)src_step) * src_stride + (size_t)(row0 + i) * src_ld;
    double *O = dst + ((size_t)n * rows + i) * ld + j;
    if (VEC) {
        double2 v = make_double2(0.0, 0.0);
        // live: row i < M and a column of the pair inside the block (and, upper_only, on or right of the diagonal)
        if (i < M && j < M && (!upper_only || j + 1 >= i)) {
            v = *reinterpret_cast<const double2 *>(S + j);              // j even, src_ld even: j + 1 < src_ld
            if (j + 1 >= M) v.y = 0.0;
            if (upper_only && j < i) v.x = 0.0;
        }
        *reinterpret_cast<double2 *>(O) = v;
    } else {
        *O = (i < M && j < M && (!upper_only || j >= i)) ? S[j] : 0.0;
    }
}
void launch_pg_pack(hipStream_t stream, const double *src, size_t src_stride, int src_ld, int row0, int src_mod, int src_step,
                    int M, int upper_only, double *dst, int rows, int ld, int count) {
    if (count <= 0) return;
    const bool vec = (ld % 2 == 0);
    const size_t per_matrix = (size_t)rows * (vec ? ld / 2 : ld);
    const unsigned bpm = (unsigned)((per_matrix + 255) / 256);
    const dim3 grid((unsigned)((size_t)bpm * count));
    if (vec)
        hipLaunchKernelGGL(pg_pack_kernel<true>, grid, dim3(256), 0, stream, src, src_stride, src_ld, row0, src_mod, src_step, M,
                           upper_only, dst, rows, ld, bpm);
    else
        hipLaunchKernelGGL(pg_pack_kernel<false>, grid, dim3(256), 0, stream, src, src_stride, src_ld, row0, src_mod, src_step, M,
                           upper_only, dst, rows, ld, bpm);
}

__global__ __launch_bounds__(256) void pg_unpack_u_kernel(const double *u, int ng, int D, int M, double *f) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, MD = (size_t)M * D;
    if (e >= (size_t)ng * MD) return;
    const size_t gl = e / MD, r = e % MD, i = r / D, d = r % D;
    f[e] = u[(gl * D + d) * M + i];
}
void launch_pg_unpack_u(hipStream_t stream, const double *u, int ng, int D, int M, double *f) {
    const size_t n = (size_t)ng * M * D;
    hipLaunchKernelGGL(pg_unpack_u_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, u, ng, D, M, f);
}

__global__ __launch_bounds__(256) void pg_x_last_kernel(const double *Xs, int G, int T, int D, double *x_last) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)G * D) return;
    const size_t g = e / D, d = e % D;
    x_last[e] = Xs[(g * (size_t)(T + 1) + T) * D + d];
}
void launch_pg_x_last(hipStream_t stream, const double *Xs, int G, int T, int D, double *x_last) {
    const size_t n = (size_t)G * D;
    hipLaunchKernelGGL(pg_x_last_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, Xs, G, T, D, x_last);
}

}  // namespace ffvd
