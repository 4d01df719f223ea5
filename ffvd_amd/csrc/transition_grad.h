// Linearisation of the learned transition (transition_grad.hip): mean and variance of the GP increment f(x, c) of G posteriors at N
// common inputs TOGETHER WITH their gradients with respect to all P = D + C input columns, SE-ARD kernels, white = True,
// full_cov = False (conditional_after_kernel_precalculation, conditionals_multi_output.py:306-387, differentiated).  With
// k_j = K_d(x, z_j), nu_jp = z_jp - x_p, beta = W_d u_{g,d}, Gamma = W_d (I - q q^T) W_d^T (the moment family's staging) and t = Gamma k:
//   mean     = sum_j k_j beta_j                         var      = variance_d - sum_j k_j t_j
//   dmean_p  = (1 / l_dp^2) sum_j k_j beta_j nu_jp      dvar_p   = -(2 / l_dp^2) sum_j k_j t_j nu_jp
// The operators ffvd_op_conditional_grad_grouped / ffvd_op_posterior_conditional_grad_grouped (ops_grouped.hip) stage the operands and
// call launch_transition_grad.  DESIGN.md section 9, "Linearisation".
//
// Layouts (Mp = M rounded up to 64, Tp = the rows of a pass rounded up to 64, F = P + 1 fields: the plain sum, then one per column p):
//   K      [n_models * D][Tp][Mp]       K_d(Xnew, Z_m) row-major (launch_kfu_build), zeros beyond the pass's rows and beyond M
//   gam    [units][Mp][Mp]              unit = (group, dim) with q_sqrts (unit_per_group), (model, dim) without
//   beta   [G * D][Mp]
//   vpart  [units][ceil(Mp / 128)][F][Tp]   per column tile: sum_j k t and sum_j k t nu_p; T = K Gamma itself never reaches memory
//   msum   [G * D][F][Tp]                   sum_j k beta and sum_j k beta nu_p
// Launches per pass: launch_kfu_build per model, the variance product (tg_var_kernel), the mean sums, the finish.
// Every sum is local to a row and has a fixed order: a group's results do not depend on G or on the other groups, a row's results
// not on N, on the other rows or on the pass size.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels.h"

namespace ffvd {

struct TransitionGradArgs {
    int G, n_models, M, Mp, P, D, N;
    int rows_per_pass;          // > 0
    int unit_per_group;         // gam per (group, dim) (1) or per (model, dim) (0)
    int need_var;               // the variance side runs
    HyperView hv;               // [n_models * D] (launch_rg_prep's layout)
    const double *Z;            // [n_models][M][P], the inducing inputs as given
    const double *beta, *gam;
    const double *x;            // [N][P]
    double *K, *vpart, *msum;   // scratch: tg_scratch_doubles()
    double *mean, *var;         // [G][N][D]; var and dvar may be null without need_var
    double *dmean, *dvar;       // [G][N][D][P]
};
struct TransitionGradScratch { size_t K, vpart, msum; };
TransitionGradScratch tg_scratch_doubles(int G, int n_models, int D, int P, int Mp, int N, int rows_per_pass, int units, bool need_var);
void launch_transition_grad(hipStream_t stream, const TransitionGradArgs &a);
// mix_dmean = (sum_g dmean_g) / G,  mix_dvar = (sum_g (dvar_g + 2 (mean_g - mix_mean) dmean_g)) / G, g ascending; [N][D][P].
// mix_dvar (and with it dvar) may be null.
void launch_tg_mixture(hipStream_t stream, const double *mean, const double *dmean, const double *dvar, const double *mix_mean, int G,
                       size_t ND, int P, double *mix_dmean, double *mix_dvar);

}  // namespace ffvd
