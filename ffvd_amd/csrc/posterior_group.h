// Grouped collapsed posteriors (posterior_group.hip): the kernels that hand G posteriors from the factorisation slabs to the grouped
// rollout loop (rollout_group.hip) or to packed result arrays without a trip through the host.  The factorisations themselves are
// the ELBO's batch machinery (kernels.h: launch_kuu_build, launch_project, launch_gram, launch_potrf_ext, launch_matvec); the
// operators ffvd_op_posterior_grouped / ffvd_op_posterior_rollout_grouped (ops_grouped.hip) put the launches together.
//
// Slab layouts read here (Mp = M rounded up to 64, ld Mp):
//   K_uu slab of (model, dim): 2 Mp rows, rows [Mp, 2 Mp) = L^-T after launch_potrf_ext (upper triangular, identity padding);
//   H slab of (group, dim):    2 Mp + 64 rows, rows [0, Mp) H -> L_H, rows [Mp, 2 Mp) identity -> L_H^-T, row 2 Mp b -> L_H^-1 b.
// Limits (the operators return FFVD_EINVAL beyond them): M <= 2048, P <= 32, T >= 1, n_models 1 or G; the fused form also those of
// rollout_group.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace ffvd {

// groups per pass: the largest count whose F = K_fu L^-T (D * Tp * Mp doubles per group) is at most 2 GiB and whose units fit one
// grid dimension, at least 1, at most G.  A function of the shapes alone.
int pg_groups_per_pass(int G, int D, int Tp, int Mp);

// Xt[t][g * D + d] = Xs[g][t][d], t <= T: the G trajectories as ONE chain of G * D dims -- with it a single launch_gram serves
// units whose Q differs per group (log_Q[g * D + d]), which its [D]-indexed log_Q cannot do for [S][T+1][D]
void launch_pg_stage_x(hipStream_t stream, const double *Xs, int G, int T, int D, double *Xt);

// dst[n] (rows x ld, n < count) <- the leading M x M block of rows [row0, row0 + M) of source slab (n % src_mod) * src_step
// (slabs of src_stride doubles, ld src_ld); everything outside the block is written as an exact zero and, with upper_only, so is the
// strict lower triangle.  16-byte loads and stores when ld is even (src_ld, src_stride are: multiples of 64).
void launch_pg_pack(hipStream_t stream, const double *src, size_t src_stride, int src_ld, int row0, int src_mod, int src_step,
                    int M, int upper_only, double *dst, int rows, int ld, int count);

// f[g0 + gl][i][d] = u[gl * D + d][i] (the matvec output of a pass of ng groups, rows of M), i < M
void launch_pg_unpack_u(hipStream_t stream, const double *u, int ng, int D, int M, double *f /* at group g0 */);
// x_last[g][d] = Xs[g][T][d]
void launch_pg_x_last(hipStream_t stream, const double *Xs, int G, int T, int D, double *x_last);

}  // namespace ffvd
