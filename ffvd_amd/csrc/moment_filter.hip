// Filtering and smoothing of an observed sequence through the GP ("Filtering and smoothing"): the step kernel
// of the moment-matched prediction (moment_step.h) instantiated with the measurement update, and the RTS pass over the stored stacks.
#include "moment_step.h"

namespace ffvd {
namespace {

// The RTS pass of one group: [S^- | X^T] of index i + 1 in LDS, one thread eliminates (partial pivoting: the pivot row is an LDS row in
// [k, D) whatever the values are) and substitutes back, thread (r, c) forms the products
__global__ __launch_bounds__(64) void mg_smooth_kernel(MomentSmoothArgs a) {
    __shared__ double A[MG_MAXD][2 * MG_MAXD], JT[MG_MAXD][MG_MAXD], Wk[MG_MAXD][MG_MAXD], Dl[MG_MAXD][MG_MAXD], Ss[MG_MAXD][MG_MAXD];
    __shared__ double ms[MG_MAXD], dm[MG_MAXD];
    const int tid = threadIdx.x, g = blockIdx.x, D = a.D, n = a.steps, DD2 = D * D;
    const int r = tid / D, c = tid % D, lo = r < c ? r : c, hi = r < c ? c : r;
    const size_t base = (size_t)g * n;
    if (tid < D) {
        const double v = a.m_filt[(base + n - 1) * D + tid];
        ms[tid] = v;
        a.m_smooth[(base + n - 1) * D + tid] = v;
    }
    if (tid < DD2) {
        const double v = a.S_filt[(base + n - 1) * DD2 + tid];
        Ss[r][c] = v;
        a.S_smooth[(base + n - 1) * DD2 + tid] = v;
    }
    __syncthreads();
    for (int i = n - 2; i >= 0; --i) {
        const double *Sp = a.S_pred + (base + i + 1) * DD2, *X = a.cross + (base + i + 1) * DD2;
        if (tid < DD2) {
            const double sp = Sp[tid];
            A[r][c] = sp;
            A[r][D + c] = X[c * D + r];                           // X^T: J^T = (S^-)^-1 X^T, S^- symmetric
            Dl[r][c] = Ss[r][c] - sp;
        }
        if (tid < D) dm[tid] = ms[tid] - a.m_pred[(base + i + 1) * D + tid];
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < D; ++k) {
                int piv = k;
                double best = fabs(A[k][k]);
                for (int q = k + 1; q < D; ++q) {
                    const double v = fabs(A[q][k]);
                    if (v > best) { best = v; piv = q; }
                }
                if (piv != k)
                    for (int q = k; q < 2 * D; ++q) { const double x = A[k][q]; A[k][q] = A[piv][q]; A[piv][q] = x; }
                const double ip = 1.0 / A[k][k];
                for (int q = k + 1; q < D; ++q) {
                    const double fq = A[q][k] * ip;
                    for (int w = k + 1; w < 2 * D; ++w) A[q][w] -= fq * A[k][w];
                }
            }
            for (int w = 0; w < D; ++w)
                for (int q = D - 1; q >= 0; --q) {
                    double s = A[q][D + w];
                    for (int k = q + 1; k < D; ++k) s -= A[q][k] * JT[k][w];
                    JT[q][w] = s / A[q][q];
                }
        }
        __syncthreads();
        double mn = 0.0;
        if (tid < DD2) {                                          // W = J (S^s - S^-)
            double v = 0.0;
            for (int k = 0; k < D; ++k) v += JT[k][r] * Dl[k][c];
            Wk[r][c] = v;
        }
        if (tid < D) {
            double v = 0.0;
            for (int k = 0; k < D; ++k) v += JT[k][tid] * dm[k];
            mn = a.m_filt[(base + i) * D + tid] + v;
        }
        __syncthreads();
        if (tid < DD2) {                                          // (r, c) and (c, r) run the same expression
            double v = 0.0;
            for (int k = 0; k < D; ++k) v += Wk[lo][k] * JT[k][hi];
            v = a.S_filt[(base + i) * DD2 + lo * D + hi] + v;
            Ss[r][c] = v;
            a.S_smooth[(base + i) * DD2 + tid] = v;
        }
        if (tid < D) {
            ms[tid] = mn;
            a.m_smooth[(base + i) * D + tid] = mn;
        }
        __syncthreads();
    }
}

}  // namespace

void launch_mg_filter_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, int t) {
    const dim3 grid((unsigned)((size_t)a.G * mg_npair(a.D) * a.NS));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_step_kernel<d, true, MomentFilterArgs>), grid, dim3(256), 0, stream, a, t, f))
}

void launch_mg_smooth(hipStream_t stream, const MomentSmoothArgs &a) {
    if (a.G <= 0 || a.steps <= 0) return;
    hipLaunchKernelGGL(mg_smooth_kernel, dim3((unsigned)a.G), dim3(64), 0, stream, a);
}

}  // namespace ffvd
