// Moment-matched prediction (moment_group.hip): a Gaussian state x_t ~ N(mu, Sigma) of each of G posteriors is pushed through
// x_{t+1} = x_t + f(x_t, c_t) + process noise in closed form (SE-ARD kernels only; Girard et al. 2003, the PILCO propagation) and
// re-approximated as a Gaussian: one launch per step for all groups, no sampling.  DESIGN.md section 9 has the formulas.
//
// Limits (the operators return FFVD_EINVAL beyond them): SE kernel, D <= MG_MAXD, D <= P <= 32, M <= 2048, n_models 1 or G,
//   G * D * Mp * Mp <= 2^29 doubles (the W E and Gamma stacks), Mp = M rounded up to 64;  G * npair * NS < 2^31 (grid x),
//   npair = D (D + 1) / 2, NS = ceil(M / MG_SLAB);  G * steps * D * D < 2^31.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace ffvd {

constexpr int MG_SLAB = 16;          // rows i of the pair tables per workgroup
constexpr int MG_MAXD = 8;           // latent dims (the D x D elimination runs in one thread)

// The launchers' dispatch on D: the statement with `d` a constant expression equal to D, for D = 1 .. MG_MAXD (nothing beyond: the
// operators have returned FFVD_EINVAL).  MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<d>), ...))
#define MG_DISPATCH_D_CASE(n, ...)                                                                                                  \
    case n: {                                                                                                                       \
        constexpr int d = n;                                                                                                        \
        __VA_ARGS__;                                                                                                                \
        break;                                                                                                                      \
    }
#define MG_DISPATCH_D(D, ...)                                                                                                       \
    switch (D) {                                                                                                                    \
        MG_DISPATCH_D_CASE(1, __VA_ARGS__) MG_DISPATCH_D_CASE(2, __VA_ARGS__) MG_DISPATCH_D_CASE(3, __VA_ARGS__)                    \
        MG_DISPATCH_D_CASE(4, __VA_ARGS__) MG_DISPATCH_D_CASE(5, __VA_ARGS__) MG_DISPATCH_D_CASE(6, __VA_ARGS__)                    \
        MG_DISPATCH_D_CASE(7, __VA_ARGS__) MG_DISPATCH_D_CASE(8, __VA_ARGS__)                                                       \
        default: break;                                                                                                             \
    }
static_assert(MG_MAXD == 8, "MG_DISPATCH_D lists the cases 1 .. MG_MAXD");

__host__ __device__ inline int mg_npair(int D) { return D * (D + 1) / 2; }
__host__ __device__ inline int mg_fields(int D) { return mg_npair(D) + D + D * D; }     // Cov(f) pairs, E[f], Cov(x, f)

struct MomentGroupArgs {
    int G, n_models, D, C, P, M, Mp, NS, steps;
    int unit_per_group;      // beta is always per (group, dim); Gamma per (group, dim) (1) or per (model, dim) of a shared model (0)
    const double *Z;         // [n_models][M][P]
    const double *variance;  // [n_models][D]
    const double *len;       // [n_models][D][P]   lengthscales
    const double *beta;      // [G][D][Mp]         W u
    const double *gam;       // [units][Mp][Mp]    Gamma = W (I - q q^T) W^T, entries (i, j < M) are read
    const double *x_last;    // [G][D]
    const double *S0;        // [G][D][D] or nullptr (zeros)
    const double *log_Q;     // [G][D]
    const double *ctrl;      // [steps][C] or nullptr
    double *part;            // [2][G][fields][NS]: slab sums of a step (step parity)
    double *state;           // [2][G][D + D * D]: mu, Sigma (step parity)
    double *m_x;             // [G][steps][D]
    double *S_x;             // [G][steps][D][D]
};

// beta[(g * D + d) * Mp + i] = sum_{j < M} W[unit(g, d)][i][j] U[g][j][d], i < M; unit = g * D + d (w_per_group) or d
void launch_mg_beta(hipStream_t stream, int G, int D, int M, int Mp, int w_per_group, const double *W, const double *U, double *beta);
// N = I - q and E = (N + N^T) - N N^T (in place over -N N^T) for nq slots of Mp x Mp: I - q q^T without its cancellation
void launch_mg_nmat(hipStream_t stream, int nq, int M, int Mp, const double *q, double *N);
void launch_mg_emat(hipStream_t stream, int nq, int M, int Mp, const double *N, double *E);
// launch t of steps + 1: finishes step t - 1 (t > 0) and forms the slab sums of step t (t < steps)
void launch_mg_step(hipStream_t stream, const MomentGroupArgs &a, int t);

// Filtering ("Filtering and smoothing"): the same launch with a measurement update between "finish step t - 1"
// and "form the slabs of step t".  The state after step i emits row i of Y (y = CC^T x + DD + noise, diagonal noise sd_j); a NaN entry
// of Y is unobserved.  The update is a sequence of scalar updates in ascending j, run redundantly by every workgroup of the group (the
// same instructions in the same order, as the finish of the step); only the writer workgroup stores.  MomentGroupArgs::m_x / S_x are
// the PREDICTED moments m^-_i, S^-_i in this form; state[] holds the FILTERED state.
constexpr int MG_MAXJ = 8;           // outputs of the emission
struct MomentFilterArgs {
    int J;
    const double *CC;                // [D][J]
    const double *DD, *sd;           // [J]
    const double *Y;                 // [steps][J], NaN = unobserved
    double *m_filt, *S_filt;         // [G][steps][D], [G][steps][D][D]: after the update with row i
    double *cross;                   // [G][steps][D][D]: Cov(x_{i-1}, x_i | y_{0:i-1}), row = component of x_{i-1}
    double *lpd;                     // [G][steps][J]: log N(y_ij; .) under the predicted state, NaN where unobserved
    double *lpd_joint;               // [G][steps]: joint log density of the observed entries of row i, NaN where there is none
};
void launch_mg_filter_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, int t);

// Linearised filtering (moment_linear.hip; DESIGN.md section 9, "Linearised filtering"): the filter's launch sequence, arguments,
// update and stores with the extended Kalman rule in place of moment matching.  With A = I + J, J the Jacobian of the posterior mean
// of f at [mu, c_t] (state columns) and v its variance there: m^- = mu + m, S^- = A S A^T + diag(v + Q), cross = S A^T.
// Workgroup (group, dim, slab of MG_SLAB rows of Gamma_dim): grid x = G * D * NS (below the moment step's G * npair * NS).
// part is [2][G][D][D + 2][NS]: per dim the slab sums of k_i beta_i, of k_i beta_i nu_ip (p < D) and of k_i (Gamma k)_i.
constexpr int MG_LINEAR_MAXM = 2048; // the kernel row of a dim lives in LDS (the family's limit on M)
__host__ __device__ inline int mg_linear_fields(int D) { return D * (D + 2); }
void launch_mg_linear_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, int t);

// RTS pass over the stored stacks, one workgroup per group, i = steps - 2 .. 0:  J_i = X_{i+1} (S^-_{i+1})^-1 (pivoted elimination),
// m^s_i = m_i + J_i (m^s_{i+1} - m^-_{i+1}),  S^s_i = S_i + J_i (S^s_{i+1} - S^-_{i+1}) J_i^T (exactly symmetric); the last row is the
// filtered one bit for bit.  Every sum has a fixed order.
struct MomentSmoothArgs {
    int G, D, steps;
    const double *m_pred, *S_pred, *m_filt, *S_filt, *cross;
    double *m_smooth, *S_smooth;     // [G][steps][D], [G][steps][D][D]
};
void launch_mg_smooth(hipStream_t stream, const MomentSmoothArgs &a);

// Rolling-origin forecasts (moment_fan.hip; DESIGN.md section 9, "Rolling-origin forecasts"): the propagation's launch with a TRACK as
// its unit of work.  Track v = g * Bp + b of a pass is (group g, origin b0 + b of the origin table): it reads beta, Gamma, the
// hyper-parameters and log_Q of its group, starts from row origin[b0 + b] of the filter's stacks (launch 0, no gather pass), reads
// control row origin[b0 + b] + 1 + t at launch t, and launch t + 1 writes row t of its forecast.  In this form MomentGroupArgs::G is
// the number of tracks of the pass (part and state are per track), steps the horizon h, ctrl the rows the filter read, and m_x / S_x
// the forecast stacks [G][B][h][D], [G][B][h][D][D]; x_last and S0 are not read.
// Limits: a pass holds at most Bp tracks per group with G * Bp * npair * NS < 2^31 (grid x) and 2 * G * Bp * fields * NS <=
//   MG_FAN_PART_DOUBLES (the slab sums of its tracks: 128 MiB);  G * B * h * D * D < 2^31.
constexpr long long MG_FAN_PART_DOUBLES = 1LL << 24;
struct MomentFanArgs {
    int B, Bp, b0, n;                // origins of the call; tracks per group of this pass; its first origin; rows of the filter's stacks
    const int *origin;               // [B], ascending, every origin + h < n (checked on the host)
    const double *m_filt, *S_filt;   // [groups][n][D], [groups][n][D][D]
};
// the largest number of tracks per group of a pass (at least 1) for G groups and B origins
int mg_fan_tracks_per_pass(int G, int D, int NS, int B);
void launch_mg_fan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFanArgs &f, int t);

// Linearised forecasts (moment_linear_fan.hip; DESIGN.md section 9, "Linearised forecasts"): the fan's tracks and indexing with the
// extended Kalman rule of moment_linear.hip and no measurement update.  Two launches per step for all tracks of a pass: the state
// kernel (workgroup (track, dim): finishes step t - 1, writes the kernel row of its dim into K and the D + 1 sums of the mean side)
// and the product kernel (one 128 x 128 tile of T = K Gamma of a unit on the fp64 MFMA; only sum_j k_nj t_nj per column tile is kept).
// A unit is (group, dim) with rows = the group's tracks of the pass, or -- one model shared by the groups and no q slices, where
// Gamma is per dim -- (dim) with rows = all tracks of the pass (`shared`); Gamma of unit u is slot u of MomentGroupArgs::gam either way.
// MomentGroupArgs as for the moment fan; `part` is not read, `state` is [2][tracks][D + D * D].
// Limits: a pass holds at most Bp tracks per group with G * Bp * D < 2^31 (grid x) and K plus the partials within
//   MG_LFAN_SCRATCH_DOUBLES (512 MiB; one track per group is always tried).
constexpr long long MG_LFAN_SCRATCH_DOUBLES = 1LL << 26;
struct MomentLinearFanArgs {
    int shared, units, Tp, nr, ntj;  // nr: live rows per unit of this pass; Tp: rows of a K block (a multiple of 128); ntj = ceil(Mp / 128)
    double *K;                       // [units][Tp][Mp]: kernel rows, zero beyond M
    double *vpart;                   // [units][ntj][Tp]: column-tile partials of k^T Gamma k
    double *msum;                    // [2][tracks][D][D + 1]: sum_j k_j beta_j, sum_j k_j beta_j nu_jp (step parity)
};
// the layout (without buffers) of a pass of Bp tracks per group
MomentLinearFanArgs mg_lfan_layout(int G, int n_models, int D, int Mp, int unit_per_group, int Bp);
int mg_lfan_tracks_per_pass(int G, int n_models, int D, int Mp, int unit_per_group, int B);
// launch t of h + 1: the state kernel, then (t < h) the product kernel
void launch_mg_lfan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFanArgs &f, const MomentLinearFanArgs &l, int t);

// the product kernel's launches alone: per unit u < units the column-tile partials of diag(K_u Gamma_u K_u^T), rows < nr
void launch_mg_lfan_var(hipStream_t stream, const double *K, const double *gam, double *vpart, int Tp, int Mp, int nr, int units);

// Linearised filtering of many records (moment_linear_records.hip; DESIGN.md section 9, "Filtering many records"): R observed records
// through G posteriors, a TRACK (group g, record r) = one independent linearised filter of moment_linear.hip.  The launch pair, the
// unit layout, K, the partials and the mean sums are those of the linearised forecasts (MomentLinearFanArgs, the product kernel
// unchanged); the state kernel adds the filter's stores and mg_update with row t - 1 of the track's own record.  Track v = g * Rp + b
// of a pass is record r = r0 + b; its rows in every stack are those of the global track g * R + r.
// In this form MomentGroupArgs::G is the number of tracks of the pass (state and msum are per track of the pass), steps the rows of a
// record, x_last [G][R][D], S0 [G][R][D][D] or nullptr, ctrl [R][steps][C], m_x / S_x the predicted stacks [G][R][steps]...; `part`
// is not read.  MomentFilterArgs: Y [R][steps][J], every stack [G][R][steps]...
// Limits: those of the linearised forecasts with records for origins (mg_lfan_tracks_per_pass);  G * R * steps * D * D < 2^31.
struct MomentRecordArgs {
    int R, Rp, r0;                   // records of the call; records per group of this pass; its first record
};
// launch t of steps + 1: the state kernel, then (t < steps) the product kernel
void launch_mg_lrec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, int t);
// dst[g][r][:] = src[g][:] (n doubles per group): the start of every record of a group where the caller gave one per group
void launch_mg_lrec_spread(hipStream_t stream, int G, int R, int n, const double *src, double *dst);

// Cubature filtering of many records (moment_cubature_records.hip; DESIGN.md section 9, "Cubature filtering"): the tracks, passes,
// stacks and update of the linearised records filter with the third-degree spherical cubature rule as the propagation.  A track brings
// 2D points per step, mu +- sqrt(D) (column i of the Cholesky factor of S) with the control columns not spread, hence 2D kernel rows per
// (track, dim): rows 2D * (track row) + i of the unit's K block.  MomentLinearFanArgs is mg_lfan_layout with Bp = 2D * (records per
// group of the pass); msum is [2][tracks][D][2D] (the mean at every point) and `off` [2][tracks][D][D] (the offsets of a step, kept
// for the finish of that step; step parity).  The product kernel runs unchanged.
// Limits: those of the linearised records with 2D rows per track (mg_crec_records_per_pass).
constexpr int mg_crec_rows(int D) { return 2 * D; }
int mg_crec_records_per_pass(int G, int n_models, int D, int Mp, int unit_per_group, int R);
// launch t of steps + 1: the state kernel, then (t < steps) the product kernel
void launch_mg_crec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, double *off, int t);

// Particle filtering of many records (moment_particle_records.hip; DESIGN.md section 9, "Particle filtering"): the tracks, passes and
// stacks of the linearised records filter with a bootstrap particle filter of N particles per track as the propagation and the update
// (no Gaussian projection, no `cross`, no smoother).  A track brings N kernel rows per (track, dim): rows N * (track row) + i of the
// unit's K block.  MomentLinearFanArgs is mg_lfan_layout with Bp = N * (records per group of the pass); msum is not read.  The draws
// are the caller's: eps [..][steps][N][D], unif [..][steps] and xi0 [..][N][D] (read only with S0) are indexed through a group and a
// record stride in doubles, each of which may be 0 (common random numbers).  The product kernel runs unchanged.
// Limits: MG_PREC_MINN <= N <= MG_PREC_MAXN; N <= mg_prec_max_particles (one track per group fits K); G * Rp * D * ceil(N / slab) < 2^31.
constexpr int MG_PREC_MINN = 2, MG_PREC_MAXN = 2048;
constexpr int MG_PREC_SLAB = 8;      // particles per workgroup of the rows kernel
struct MomentParticleArgs {
    int N;
    const double *eps;
    long long eps_g, eps_r;
    const double *unif;
    long long unif_g, unif_r;
    const double *xi0;               // nullptr without S0
    long long xi0_g, xi0_r;
    double *xstate;                  // [2][tracks][N][D]: the particles (step parity)
    double *pmean;                   // [tracks][D][N]: the conditional mean at every particle
    double *ess;                     // [G][R][steps]
    double *particles;               // [G][R][steps][N][D] (the X^-) or nullptr
    int *ancestors;                  // [G][R][steps][N] or nullptr
};
long long mg_prec_max_particles(int G, int n_models, int D, int Mp, int unit_per_group);
int mg_prec_records_per_pass(int G, int n_models, int D, int Mp, int unit_per_group, int R, int N);
// launch t of steps + 1: the weight kernel, then (t < steps) the rows kernel and the product kernel
void launch_mg_prec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, const MomentParticleArgs &p, int t);
// the rows kernel's launch of step t < steps alone (host code only: for the units that bring a weight kernel of their own)
void launch_mg_prec_rows(hipStream_t stream, const MomentGroupArgs &a, const MomentRecordArgs &rc, const MomentLinearFanArgs &l,
                         const MomentParticleArgs &p, int t);

// Fully adapted particle filtering of many records (moment_particle_adapted.hip; DESIGN.md section 9, "Adapted particle filtering"):
// the tracks, passes, stacks, draws and limits of the particle filter above with the optimal proposal: the parents are weighted by
// p(y_t | parent) before anything is drawn, resampled, and the children are drawn from p(x_t | parent, y_t).  Its weight kernel
// replaces the bootstrap one; the rows kernel and the product kernel run unchanged.  In this form MomentParticleArgs::particles is
// the equally weighted FILTERED set after the row (X_{t+1}, not X^-) and ancestors[t, i] indexes the set carried INTO row t.
// Between the weighting and the draw only the parents' transition mean and variance are kept.
struct MomentParticleAdaptedArgs {
    double *mu, *sv;                 // [tracks][N][D]: X_t + mean and v + Q of the row in flight (trans_mean, trans_var of the smoother)
};
// launch t of steps + 1: the adapted weight kernel, then (t < steps) the rows kernel and the product kernel
void launch_mg_parec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                          const MomentLinearFanArgs &l, const MomentParticleArgs &p, const MomentParticleAdaptedArgs &q, int t);

// Particle filtering of many records with adaptive resampling (moment_particle_adaptive.hip; DESIGN.md section 9, "Adaptive
// resampling"): the tracks, passes, stacks, draws and limits of the bootstrap particle filter above carrying a weighted set, which is
// resampled only on the rows whose effective sample size falls below ess_threshold * N (unif of the other rows is not read).  Its
// weight kernel replaces the bootstrap one; the rows kernel and the product kernel run unchanged.  MomentParticleArgs::particles is
// the X^- and (particles[t], weights[t]) the filtering approximation after row t.
struct MomentParticleEssArgs {
    double *logw;                    // [tracks][N]: the carried log-weights, largest entry 0 (written by the launch at t = 0)
    double ess_threshold;            // finite, >= 0
    double *weights;                 // [G][R][steps][N]: the normalised weights after the row, or nullptr
    int *resampled;                  // [G][R][steps]: 1 where the row resampled
};
// launch t of steps + 1: the adaptive weight kernel, then (t < steps) the rows kernel and the product kernel
void launch_mg_pess_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, const MomentParticleArgs &p, const MomentParticleEssArgs &q, int t);

// Particle smoothing of many records (moment_particle_smooth.hip; DESIGN.md section 9, "Particle smoothing"): the marginal
// forward-filter / backward-smoother on the sets the particle filter above carries.  The driver keeps the filter's device stacks
// `particles` and `ancestors`, launches the keep kernel after the product launch of every step (trans_mean, trans_var: the two
// parenthesised sub-expressions of the weight kernel's X^-) and, after the last pass, the smoother over all V = G * R tracks of the
// call: the weights, the normalisers c of all rows in one launch, the rows n_max - 2 .. 0 (omega, then its fold through the
// ancestors), the moments.  No GP evaluation, no draws.
// Limits: the particle filter's.  The stacks take (3 D + 3) N doubles and N ints per track row, omega N doubles per track.
struct MomentParticleSmoothArgs {
    int V, R, steps, N, D;           // V = G * R tracks, track v is record v % R
    const int *lens;                 // [R]: rows of every record, or nullptr (every record has `steps` rows)
    const double *particles;         // [V][steps][N][D]: the filter's X^-
    const int *ancestors;            // [V][steps][N]
    double *trans_mean, *trans_var;  // [V][steps][N][D]
    double *weights, *w_smooth;      // [V][steps][N]: W_t; the smoothing weights on the X^-_t; NaN at and beyond a record's length
    double *cnorm;                   // [V][steps][N]: c of the columns of row u at [u], u >= 1
    double *omega;                   // [V][N]: the backward sums of the row in flight
    double *m_smooth, *S_smooth;     // [V][steps][D], [V][steps][D][D]
    double *ess_smooth;              // [V][steps]
};
// after launch_mg_prec_step(.., s), s < steps, and before launch_mg_prec_step(.., s + 1)
void launch_mg_psm_keep(hipStream_t stream, const MomentGroupArgs &a, const MomentRecordArgs &rc, const MomentLinearFanArgs &l,
                        const MomentParticleArgs &p, const MomentParticleSmoothArgs &q, int s);
// after the last pass; n_max: the longest record of the call
void launch_mg_psm_smooth(hipStream_t stream, const MomentFilterArgs &f, const MomentParticleSmoothArgs &q, int n_max);
// the weights kernel of the smoother alone: q.weights, the last row of q.w_smooth (NaN at and beyond a record's length in both)
void launch_mg_psm_weights(hipStream_t stream, const MomentFilterArgs &f, const MomentParticleSmoothArgs &q);

// Particle backward simulation (moment_particle_backsim.hip; DESIGN.md section 9, "Particle backward simulation"): B joint trajectories
// per track by forward filtering / backward simulation (Godsill, Doucet & West 2004) on the stacks the smoother's keep launch and its
// weights kernel store.  One launch walks t = n - 1 .. 0 for every (track, trajectory), one more forms the moments over the
// trajectories.  No GP evaluation; the uniforms are the caller's, [..][steps][B] through a group and a record stride in doubles, each
// of which may be 0.
// Limits: the particle filter's; 1 <= B <= MG_PBS_MAXB; V * B < 2^31 (grid x).  The stacks are the smoother's without cnorm and
// omega, plus (D + 1) N doubles per track row for 1 / s and sum log s; trajectories take B * D doubles and B ints per track row.
constexpr int MG_PBS_MAXB = 4096;
struct MomentParticleBacksimArgs {
    int V, R, steps, N, D, B;        // V = G * R tracks, track v is record v % R of group v / R
    const int *lens;                 // [R] or nullptr
    const double *particles;         // [V][steps][N][D]
    const int *ancestors;            // [V][steps][N]
    const double *trans_mean, *trans_var;  // [V][steps][N][D]
    const double *weights;           // [V][steps][N]
    double *inv_var, *log_var;       // [V][steps][N][D], [V][steps][N]: 1 / s and sum_d log s_d of the rows 1 .. n - 1
    const double *unif;              // the uniforms of (g, r) at unif + g * unif_g + r * unif_r, [steps][B]
    long long unif_g, unif_r;
    int *traj_index;                 // [V][steps][B]: k_t, -1 at and beyond a record's length
    double *trajectories;            // [V][B][steps][D]: X^-_{t, k_t}, NaN at and beyond a record's length
    double *m_traj, *S_traj;         // [V][steps][D], [V][steps][D][D]
    double *lag_cov;                 // [V][steps][D][D]: row index = component of x_t; NaN at row n - 1
};
// after launch_mg_psm_weights
void launch_mg_pbs(hipStream_t stream, const MomentParticleBacksimArgs &b);

// Particle smoothing and backward simulation on the ADAPTED filter's sets (moment_particle_adapted_smooth.hip; DESIGN.md section 9,
// "Adapted particle smoothing").  particles[t] is the equally weighted filtered set after row t and (trans_mean, trans_var)[t + 1],
// kept by launch_mg_psm_keep after the product launch of step t + 1, are the transition moments of exactly those particles: no fold
// through the ancestors, no emission weights, a uniform last row.  The structs are the bootstrap units' with `ancestors`, `weights`
// and `omega` not read (nullptr).  The normalisers, the moments, 1 / s and sum log s and the trajectory moments are the bootstrap
// units' kernels through the launchers below; the backward kernel (one launch per row) and the recursion kernel are the unit's own.
// Limits: the bootstrap smoother's and backward simulation's.
void launch_mg_psm_norm(hipStream_t stream, const MomentParticleSmoothArgs &q, int n_max);       // mg_psm_norm_kernel alone (n_max > 1)
void launch_mg_psm_moments(hipStream_t stream, const MomentParticleSmoothArgs &q);               // mg_psm_moments_kernel alone
void launch_mg_pbs_prep(hipStream_t stream, const MomentParticleBacksimArgs &b);                 // mg_pbs_prep_kernel alone
void launch_mg_pbs_moments(hipStream_t stream, const MomentParticleBacksimArgs &b);              // mg_pbs_moments_kernel alone
// after the adapted filter's last pass; n_max: the longest record of the call
void launch_mg_pasm_smooth(hipStream_t stream, const MomentParticleSmoothArgs &q, int n_max);
void launch_mg_pabs(hipStream_t stream, const MomentParticleBacksimArgs &b);

// Cubature forecasts (moment_cubature_fan.hip; DESIGN.md section 9, "Cubature forecasts"): the fan's tracks and indexing (MomentFanArgs)
// with the cubature rule above and no measurement update.  MomentGroupArgs as for the linearised forecasts; MomentLinearFanArgs is
// mg_lfan_layout with Bp = 2D * (tracks per group of the pass), msum [2][tracks][D][2D], `off` [2][tracks][D][D].  The product kernel
// runs unchanged.
// Limits: those of the cubature records with origins for records (mg_crec_records_per_pass);  G * B * h * D * D < 2^31.
// launch t of h + 1: the state kernel, then (t < h) the product kernel
void launch_mg_cfan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFanArgs &f, const MomentLinearFanArgs &l, double *off,
                         int t);

// Particle forecasts (moment_particle_fan.hip; DESIGN.md section 9, "Particle forecasts"): the fan's tracks and indexing (MomentFanArgs)
// with the particle propagation above and no weighting or resampling.  A track starts from the particles the filter carries after
// the row of its origin: `particles` and `ancestors` are the filter's device stacks of the one record, [groups][n][N][D] and
// [groups][n][N].  MomentGroupArgs as for the linearised forecasts (`state` is not read); MomentFilterArgs gives the emission and the
// record's Y [n][J] (its output stacks are not touched); MomentLinearFanArgs is mg_lfan_layout with Bp = N * (tracks per group of the
// pass), msum is not read.  The forecast draws eps_fc [..][h][N][D] are indexed through a group and an origin stride in doubles, each
// of which may be 0 (common random numbers).  The product kernel runs unchanged.
// Limits: those of the particle records with origins for records (mg_prec_records_per_pass);  G * B * h * N * D < 2^31.
struct MomentParticleFanArgs {
    int N;
    const double *eps_fc;
    long long eps_g, eps_b;
    const double *particles;         // [groups][n][N][D]: the X^- of the filter
    const int *ancestors;            // [groups][n][N]
    double *xstate;                  // [2][tracks][N][D]: the particles (step parity)
    double *pmean;                   // [tracks][D][N]: the conditional mean at every particle
    double *lpd_fc;                  // [G][B][h][J]: log mean_i N(y; .) per output, NaN where the target is unobserved
    double *fc_particles;            // [G][B][h][N][D] or nullptr
};
// launch t of h + 1: the state kernel, then (t < h) the rows kernel and the product kernel
void launch_mg_pfan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentFanArgs &fn,
                         const MomentLinearFanArgs &l, const MomentParticleFanArgs &p, int t);

// Adapted particle forecasts (moment_particle_adapted_fan.hip; DESIGN.md section 9, "Adapted particle forecasts"): the tracks, passes,
// buffers, draws and limits of the particle forecasts above on the sets of the ADAPTED filter.  `particles` is that filter's device
// stack, the equally weighted filtered set after every row, and a track starts from a straight copy of it (`ancestors` is not read).
// The rows of the forecast are the adapted filter's Rao-Blackwellised m_pred / S_pred / lpd expressions; the set is advanced as that
// filter advances it over a row with nothing observed.  The product kernel runs unchanged.
// launch t of h + 1: the state kernel, then (t < h) the rows kernel and the product kernel
void launch_mg_pafan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentFanArgs &fn,
                          const MomentLinearFanArgs &l, const MomentParticleFanArgs &p, int t);

struct MomentSummaryArgs {
    int G, steps, D, J, n_test;
    const double *m, *S;             // [G][steps][D], [G][steps][D][D]
    const double *CC;                // [D][J]
    const double *DD, *sd;           // [J]
    const double *Y;                 // [n_test][J] or nullptr
    double *out;                     // [5][steps][J]: y_mean, y_var (= y_var_total), y_var_total, lpd, lpd_gauss (rows t < n_test)
};
void launch_moment_summary(hipStream_t stream, const MomentSummaryArgs &a);

}  // namespace ffvd
