// Grouped posterior rollouts (rollout_group.hip): G independent posteriors, each with its own W = L^-T stack, Z, hyper-parameters,
// U, q_sqrt slice and start state, advanced R rollouts each by ONE launch per step over all groups.
//
// Limits (ffvd_op_rollout_grouped returns FFVD_EINVAL beyond them): M <= 2048, P = D + C <= 32 (those of ffvd_op_rollout), and
//   G * D * Mp * Mp <= 2^29 doubles (4 GiB per stack: W and, with q_sqrt, W q_sqrt), Mp = M rounded up to 16;
//   G * R <= 2^20;  ceil(R / 8) <= 65535 (grid y);  G * D * (Mp / 16) < 2^31 (grid x).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace ffvd {

constexpr int RG_SLAB = 16;          // columns of W (and W q_sqrt) per workgroup
constexpr int RG_RC = 8;             // rollouts per workgroup (grid y walks the chunks of RG_RC rollouts)
constexpr int RG_MT = 256;           // rows of K(x, Z) staged in LDS at a time

struct RolloutGroupArgs {
    int kind, G, R, D, C, P, M, Mp, NS, steps;
    int has_q, q_upper;
    const double *W;         // [G][D][Mp][Mp]   upper triangular, zero padded
    const double *B;         // [G][D][Mp][Mp]   W q0 (has_q)
    const double *Zs;        // [G][D][Mp][P]    Z / lengthscales (Z for LinearK), zero padded rows
    const double *zz;        // [G][D][Mp]       |Zs row|^2
    const double *variance;  // [G][D]
    const double *len;       // [G][D][P]        lengthscales (1 for LinearK)
    const double *f;         // [G][M][D]
    const double *x_last;    // [G][D]
    const double *log_Q;     // [G][D]
    const double *ctrl;      // [steps][C] or nullptr
    const double *eps;       // [steps][G][R][D]
    double *part;            // [2][G][D][NS][R][4]: sum F^2, sum F u, sum E^2 of a slab (step parity)
    double *xbuf;            // [2][G][R][D]: the states (step parity)
    double *predict_x, *predict_var;   // [G][R][steps][D]
};

// variance / lengthscales / scaled Z / |z|^2 of every (group, dim): launch_prep_hypers' arithmetic, one launch for all groups
void launch_rg_prep(hipStream_t stream, int kind, int G, int D, int M, int Mp, int P, const double *Z, const double *logvar,
                    const double *loglen, double *variance, double *len, double *Zs, double *zz);
// B[b] = W[b] q0[b / D] for the G * D matrices (W upper triangular; q_upper: q0 too, then B is)
void launch_rg_wq(hipStream_t stream, int G, int D, int Mp, int q_upper, const double *W, const double *q0, double *B);
// launch t of steps + 1: finishes step t - 1 (t > 0) and forms the slab sums of step t (t < steps)
void launch_rg_step(hipStream_t stream, const RolloutGroupArgs &a, int t);

}  // namespace ffvd
