// Grouped GP conditionals (conditional_group.hip): mean and variance of the transition function f(x, c) of G posteriors at N common
// inputs, conditional_after_kernel_precalculation (conditionals_multi_output.py:306-387, white=True, full_cov=False) for every group
// in one launch sequence.  The operators ffvd_op_conditional_grouped / ffvd_op_posterior_conditional_grouped (ops_grouped.hip) stage the
// operands and call launch_conditional_group.
//
// Layouts (Mp = M rounded up to 64, Tp = the rows of a pass rounded up to 64):
//   F     [n_models * D][Tp][Mp]   F_{m,d} = K_d(Xnew, Z_m) L_{m,d}^-T, k-contiguous rows, zeros beyond the pass's rows and beyond M;
//                                  projected ONCE per (model, dim), not per group
//   q     [G] or [G * D] slabs of Mp x Mp (q_per_dim), zero padding; q_upper: every slab's strict lower triangle is exact zeros
//   Ut    [D][G][Mp] (one model) or [G * D][1][Mp] (a model per group): column d of U_g, zero padded -- the right operand of the mean
//   part  [G * D][ceil(Mp / 128)][Tp]   row sums of squares of E = F q per (unit, column tile); E itself never reaches memory
// Launches per pass: launch_project per model (F, row sums of F^2), launch_cov(COV_GEN) (means), the variance product, the finish.
// A group's results depend on (N, M, the pass size) and its own operands only: never on G or on the other groups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels.h"

namespace ffvd {

// rows of Xnew per pass: the largest multiple of 128 whose F (n_models * D * rows * Mp doubles) is at most 2 GiB, at least 128.
// A function of the shapes alone.
int cg_rows_per_pass(int n_models, int D, int Mp);

struct CondGroupArgs {
    int kind, G, n_models, M, Mp, P, D, N;
    int rows_per_pass;          // > 0
    HyperView hv;               // [n_models * D] (launch_rg_prep's layout)
    const double *W;            // [n_models * D] slabs: L^-T (Mp x Mp, upper triangular), slab stride w_stride
    size_t w_stride;
    const double *U;            // [G][M][D]
    const double *q;            // null (no third variance term) or the q slabs
    int q_per_dim, q_upper;
    const double *x;            // [N][P]
    int need_var;
    double *F, *rowsq, *part, *Ut, *mbuf;      // scratch: cg_scratch_doubles()
    double *mean, *var;         // [G][N][D] (var may be null without need_var)
};
struct CondGroupScratch { size_t F, rowsq, part, Ut, mbuf; };
CondGroupScratch cg_scratch_doubles(int G, int n_models, int D, int Mp, int N, int rows_per_pass, bool with_q);
void launch_conditional_group(hipStream_t stream, const CondGroupArgs &a);
// mix_mean = (sum_g mean_g) / G,  mix_var = (sum_g (var_g + mean_g^2)) / G - mix_mean^2, g ascending; [N][D]
void launch_cg_mixture(hipStream_t stream, const double *mean, const double *var, int G, size_t ND, double *mix_mean, double *mix_var);

}  // namespace ffvd
