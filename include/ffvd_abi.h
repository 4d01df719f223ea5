/*
 * ffvd_abi.h -- C ABI of the MI355X-native FFVD ELBO engine (libffvd_hip.so).
 *
 * The reference (xuhuifan/FFVD) has no FFI: its "model/ELBO callable" is the
 * TensorFlow tensor `DGPSSM.nll` (vfegpssm/dgp_model.py:248-297) evaluated by
 * `session.run` (vfegpssm/base_model.py:952-989).  This header is the boundary
 * a maintainer binds instead (ctypes stub in INTEGRATION.md): plain pointers
 * and sizes, row-major contiguous fp64 arrays, no torch / numpy types.
 *
 * Conventions
 *   - status: 0 = OK, <0 usage/runtime error, >0 numerical error (FFVD_ENOTPD);
 *     the message is retrievable with ffvd_last_error(); nothing aborts or throws.
 *   - a handle = one device + one HIP stream + all device workspace (allocated in
 *     ffvd_create, nothing is allocated on the hot path).  Not thread-safe;
 *     distinct handles are independent.
 *   - pointer arguments are HOST pointers unless the call has an `on_device`
 *     flag / FFVD_PARAMS_ON_DEVICE, in which case they are device pointers used
 *     in place (zero copy).  Caller owns every buffer it passes in.
 *   - calls that write host outputs synchronise the handle's stream; the
 *     `_async` forms only enqueue.
 */
#ifndef FFVD_ABI_H
#define FFVD_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFVD_OK        0
#define FFVD_EINVAL   (-1)   /* bad shape / null pointer / unsupported option */
#define FFVD_ENOMEM   (-2)   /* device or host allocation failed */
#define FFVD_EDEVICE  (-3)   /* HIP runtime error (message in ffvd_last_error) */
#define FFVD_ENOTPD     1    /* Cholesky met a non-positive pivot (which matrix/pivot: ffvd_last_error) */

#define FFVD_F64  0   /* everything in fp64 (the reference's dtype: every variable is tf.float64, dgp_model.py:64-69) */
/* fp32 CONTRACTIONS (BASELINE configs[3]; SURVEY 7 "Conditioning"): K_fu (conditionals_multi_output.py:240) and the two
 * T x M x M products F = K_fu L^-T (:242), F^T F (:246) in fp32 on v_mfma_f32_32x32x2_f32; K_uu, every M x M
 * factorisation and solve (:159-166, :253-254), H from the moment it leaves the matrix cores, delta^T F (:247-248) and
 * the sum of F^2 in the trace term (:255) in fp64.  All inputs and outputs of the ABI stay fp64.  Collapsed branch,
 * FFVD_ROUTE_REFERENCE (the Gram route's error is eps * cond(K_uu): unusable in fp32).
 * Measured against the fp64 oracle: every term and the nll within 1e-5 absolute (worst case 5.5e-6 with M = 1100 inducing
 * points for T = 1400; 2e-7 relative on the nll at T=16384, M=2048) -- tests/test_gpu_f32c.py.
 * With grad = 1 the backward pass forms its T x M x M product K_fu Gamma in fp32 as well (Gamma rounded once; dl/dK_fu is never
 * stored, the reductions run in fp64): gradients within 1e-3 (X) / 1e-2 (Z, kernel hyper-parameters) of the largest entry of each
 * array, measured 9e-5 / 3.5e-3 -- what one fp32 product of K_fu with Gamma ~ alpha |L^-T|^2 gives; config 4 trains with it. */
#define FFVD_F32C 1

#define FFVD_KERNEL_SE      0   /* kernels_multi_output.py:140-247 SquaredExponential (ARD) */
#define FFVD_KERNEL_LINEAR  1   /* kernels.py:250-281 LinearK, one scalar variance per latent dim */

#define FFVD_BRANCH_A 0   /* explicit U:  dgp_model.py:289-297 (regularizer :337-359, conditional) */
#define FFVD_BRANCH_B 1   /* collapsed U: dgp_model.py:267-288 (kernel_pre_cal + collapse_after_kernel_precalculation) */

#define FFVD_PRIOR_UNIFORM 0    /* Layer.prior_Z dgp_model.py:106-107 */
#define FFVD_PRIOR_NORMAL  1    /* dgp_model.py:108-109 */

/* How the collapsed bound (branch B) is evaluated.  Both are the same algebra:
 *   REFERENCE: F = K_fu L^-T, H = F^T F / Q + I, exactly the reference's op order (conditionals_multi_output.py:242-255)
 *   GRAM     : log|H| = log|K_uu + K_uf K_fu / Q| - log|K_uu|, b^T H^-1 b = g^T (K_uu + K_uf K_fu / Q)^-1 g / Q^2,
 *              sum_t |F_t|^2 = tr(K_uu^-1 K_uf K_fu); about half the flops, K_fu L^-T is never formed.
 *              Rounding differs: nll agrees with REFERENCE to ~1e-9 relative on the benchmark workloads.   */
#define FFVD_ROUTE_REFERENCE 0
#define FFVD_ROUTE_GRAM      1

#define FFVD_PARAMS_ON_DEVICE 1u

/* indices into the 8-double term vector written by ffvd_elbo*()               */
#define FFVD_TERM_PART_PRIOR   0   /* nll_part_prior            dgp_model.py:286/296 */
#define FFVD_TERM_LOG_LIK      1   /* nll_log_likelihood        dgp_model.py:264     */
#define FFVD_TERM_X_PRIOR_Q    2   /* x_t_prior_Q               dgp_model.py:283/294 */
#define FFVD_TERM_TRACE        3   /* nll_reg_trace_inverse_Q_B dgp_model.py:275/292 */
#define FFVD_TERM_LATER1       4   /* later_term1 (branch B)    dgp_model.py:275     */
#define FFVD_TERM_LATER2       5   /* later_term2 (branch B)    dgp_model.py:275     */
#define FFVD_TERM_NLL          6   /* nll                       dgp_model.py:288/297 */
#define FFVD_TERM_COUNT        7   /* number of chains the sums cover (for the mean after an all-reduce) */

typedef struct ffvd_handle ffvd_handle;

typedef struct ffvd_config {
    int32_t T;            /* transitions = len(Y_train); X has T+1 rows            */
    int32_t D;            /* latent dim x_dims[-1] (columns of X)                  */
    int32_t C;            /* control-input dim; GP input dim P = D + C (models.py:51) */
    int32_t M;            /* inducing points                                        */
    int32_t S_local;      /* latent trajectories (posterior samples/chains) this handle evaluates */
    int32_t Ydim;         /* observation dim                                        */
    int32_t d_begin;      /* first latent dim this handle evaluates (shard D: BASELINE config 5) */
    int32_t d_count;      /* number of latent dims evaluated; 0 = all D             */
    int32_t shared_terms; /* 1: also add the terms not tied to a latent dim (likelihood, prior_Z, prior_x_0, hyper prior) */
    int32_t dtype;        /* FFVD_F64 or FFVD_F32C                                  */
    int32_t kernel_kind;  /* FFVD_KERNEL_*                                          */
    int32_t branch;       /* FFVD_BRANCH_*                                          */
    int32_t prior_type;   /* FFVD_PRIOR_*                                           */
    int32_t device_id;    /* HIP device ordinal                                     */
    int32_t chains_per_pass; /* chains whose T x M projections are resident at once; 0 = auto */
    int32_t route;        /* FFVD_ROUTE_*  (branch B only)                          */
    int32_t grad;         /* 1: also allocate the backward-pass workspace (ffvd_elbo_grad) */
    int32_t T_total;      /* > 0: this handle holds a T-SHARD -- rows [t_begin, t_begin + T) of a job with T_total
                           * transitions (its X has T + 1 rows starting at global row t_begin); see ffvd_elbo_tshard */
    int32_t t_begin;      /* first global transition of the shard (T_total > 0)     */
    int32_t reserved;
    double  jitter;       /* 1e-5: conditionals_multi_output.py:108,159             */
} ffvd_config;

/* All arrays fp64, row-major, contiguous. */
typedef struct ffvd_params {
    const double *X;               /* S_local x (T+1) x D   Layer.X        dgp_model.py:56-64 */
    const double *Z;               /* M x P                 Layer.Z        dgp_model.py:67    */
    const double *U;               /* M x D (branch A; NULL allowed in B)  dgp_model.py:66    */
    const double *logvariance;     /* D                     kernels_multi_output.py:156       */
    const double *loglengthscales; /* D x P (SE; NULL for LINEAR)  kernels_multi_output.py:160 */
    const double *log_Q;           /* D                     dgp_model.py:182                  */
    const double *CC;              /* D x Ydim              likelihoods.py:19                 */
    const double *DD;              /* Ydim                  likelihoods.py:23                 */
    const double *log_Rchols;      /* Ydim x Ydim           likelihoods.py:54                 */
} ffvd_params;

/* ---- lifetime ----------------------------------------------------------- */
int  ffvd_create(const ffvd_config *cfg, ffvd_handle **out);
int  ffvd_destroy(ffvd_handle *h);
/* message of the most recent failure on `h` (or of the last failed ffvd_create / handle-less op when h == NULL) */
const char *ffvd_last_error(const ffvd_handle *h);
int  ffvd_sync(ffvd_handle *h);
/* How often a synchronous call on this handle (ffvd_elbo, ffvd_elbo_grad, ffvd_adam_step, ffvd_sghmc_step) re-ran its iteration
 * because the one-launch Cholesky gave up on a bounded wait (info = -1): the iteration is then enqueued once more, in process,
 * with the launch-per-column Cholesky, the call returns FFVD_OK and ffvd_last_error holds a warning; only a second failure is
 * FFVD_EDEVICE.  Collective calls do not retry (the other ranks have moved on); instead the failure is made COLLECTIVE: the
 * finalize kernel turns the rank's seven partial sums into NaN whenever one of its factorisation flags is non-zero (bad pivot or
 * abandoned launch), so after the all-reduce EVERY rank sees non-finite sums, returns an error (FFVD_EDEVICE on the rank that
 * stalled, FFVD_ENOTPD elsewhere) and leaves its parameters untouched.  ffvd_tshard_finish (no collective after it) retries. */
int  ffvd_stall_recoveries(const ffvd_handle *h);
/* A stall is remembered: after a recovery the handle's synchronous calls stay on the schedule that has no inter-workgroup waits
 * (multi-kernel iteration, launch-per-column Cholesky) for this many further calls -- 16 after the first recovery -- and then try
 * the fast path again; a probe that stalls again doubles the hold (up to 1024 calls), a clean one resets it.  A co-tenant that keeps
 * compute units busy therefore costs one bounded wait per hold instead of one per call (the reference's only failure mode is an
 * error surfaced at session.run, dgp_model.py:320-324; here the call returns FFVD_OK either way).  ffvd_schedule_name names the
 * state while it lasts.  Collective calls neither retry nor consult the hold. */
int  ffvd_stall_hold(const ffvd_handle *h);
/* Non-zero when the handle evaluates its iteration (and, with grad = 1, the backward pass) as ONE kernel launch: the collapsed-U
 * branch with SquaredExponential kernels in fp64 at the reference's own experiment size (FFVD_Main.py:356-369: M <= 128,
 * P = D + C <= 8, every role's workgroup resident at once; ffvd_amd/csrc/tiny.hip).  The value is the wavefronts per workgroup
 * (4 or 8).  The arithmetic is the reference's op order (F = K_fu L^-T, H = I + F^T F / Q, conditionals_multi_output.py:230-257)
 * whatever cfg.route says.  FFVD_NO_TINY=1 in the environment keeps the multi-kernel schedule. */
int  ffvd_single_launch(const ffvd_handle *h);
/* One line naming the launch schedule the handle's iteration runs (decided from the configuration in ONE place, plan_schedule in
 * abi.hip; "INVALID" if its consistency check ever fails -- the ELBO entry points then return FFVD_EINVAL instead of a wrong
 * number).  Diagnostics: FFVD_DEBUG_SIDE_DELAY_US / FFVD_DEBUG_MAIN_DELAY_US = n (read at ffvd_create) put a spin kernel of n
 * microseconds at the head of the side / main stream at every fork; results must be bit-identical with and without. */
const char *ffvd_schedule_name(const ffvd_handle *h);
/* bytes of device workspace owned by the handle */
int64_t ffvd_workspace_bytes(const ffvd_handle *h);

/* ---- data and parameters (resident copies owned by the handle) ------------ */
/* Y: T x Ydim observations (base_model.py:14); control_inputs: at least T x C rows, the first T are used (dgp_model.py:255). */
int  ffvd_set_data(ffvd_handle *h, const double *Y, const double *control_inputs, int on_device);
int  ffvd_set_params(ffvd_handle *h, const ffvd_params *p, int on_device);

/* ---- the hot path ---------------------------------------------------------- */
/*
 * One ELBO iteration = DGPSSM.nll and its component tensors (dgp_model.py:248-297) for the
 * S_local trajectories of this handle.  p == NULL: use the resident parameters.  Otherwise p is
 * uploaded first (host pointers) or used in place (flags & FFVD_PARAMS_ON_DEVICE).
 * out_terms[0..6] = SUMS over the local chains of the per-chain terms, out_terms[7] = chain count
 * (so that an all-reduce(sum) over ranks followed by a division yields the mean);
 * out_nll = out_terms[6] / out_terms[7] (mean nll over the local chains).
 */
int  ffvd_elbo(ffvd_handle *h, const ffvd_params *p, uint32_t flags, double out_terms[8], double *out_nll);
/* enqueue only; the 8 doubles are written to device memory `out_terms_dev` (e.g. the buffer a
 * collective library all-reduces).  ffvd_sync() or a later synchronous call reports numerical errors. */
int  ffvd_elbo_async(ffvd_handle *h, double *out_terms_dev);
/* Gradient of the mean-over-chains nll w.r.t. every parameter (what the reference gets from tf.gradients(nll, vars),
 * base_model.py:148, and AdamOptimizer.minimize(nll), dgp_model.py:303-305).  Needs a handle created with
 * grad = 1: either branch with either kernel (collapsed branch: either route in fp64; FFVD_F32C with the SE kernel only)
 * (LinearK: the loglengthscales gradient is identically zero -- the kernel has none).  Host output pointers with
 * the shapes of ffvd_params; any of them may be NULL.  S_total = number of chains of the whole job (the divisor of
 * the mean).  Sharded jobs: every output is this handle's ADDITIVE share of the whole-job gradient -- entries of
 * dims it does not own are zero, prior gradients are weighted S_local / S_total (and the shared ones only added
 * where shared_terms = 1) -- so summing the shared-parameter gradients over ranks gives the whole-job gradient; X
 * gradients are complete per rank for chain shards and must be summed too for latent-dim shards. */
typedef struct ffvd_grads {
    double *X;               /* S_local x (T+1) x D */
    double *Z;               /* M x P               */
    double *logvariance;     /* D                   */
    double *loglengthscales; /* D x P               */
    double *log_Q;           /* D                   */
    double *CC;              /* D x Ydim            */
    double *DD;              /* Ydim                */
    double *log_Rchols;      /* Ydim x Ydim         */
    double *U;               /* M x D: explicit-U branch; zeros in the collapsed branch (U integrated out) */
} ffvd_grads;
int  ffvd_elbo_grad(ffvd_handle *h, const ffvd_params *p, uint32_t flags, int S_total, double out_terms[8],
                    double *out_nll, const ffvd_grads *g);
/* ---- optimiser / sampler steps -------------------------------------------------
 * ffvd_adam_step: one train_hypers iteration (base_model.py:944-950) entirely on the device: forward + backward on
 * the resident parameters, then tf.compat.v1.train.AdamOptimizer's update (dgp_model.py:303-305; TensorFlow is not
 * vendored by the reference -- the published rule is  lr_t = lr sqrt(1-b2^t)/(1-b1^t),  m = b1 m + (1-b1) g,
 * v = b2 v + (1-b2) g^2,  theta -= lr_t m / (sqrt(v) + eps);  TF defaults b1 = 0.9, b2 = 0.999, eps = 1e-8;
 * lr = 0.003 * 0.95^(1/1000), base_model.py:190) applied in one fused launch to the arrays selected by train_mask.
 * out_terms / out_nll describe the parameters BEFORE the update.  Needs grad = 1, all latent dims on the handle and a handle
 * that is not one rank of a multi-rank communicator (those use ffvd_adam_step_allreduce below);
 * a failed factorisation returns FFVD_ENOTPD and leaves the parameters untouched.  The handle keeps m, v and t;
 * ffvd_optimizer_reset zeroes them.  ffvd_get_params copies the resident parameters to host arrays (NULL = skip). */
#define FFVD_TRAIN_X 1u
#define FFVD_TRAIN_Z 2u
#define FFVD_TRAIN_LOGVARIANCE 4u
#define FFVD_TRAIN_LOGLENGTHSCALES 8u
#define FFVD_TRAIN_LOG_Q 16u
#define FFVD_TRAIN_CC 32u
#define FFVD_TRAIN_DD 64u
#define FFVD_TRAIN_LOG_RCHOLS 128u
#define FFVD_TRAIN_U 256u            /* explicit-U branch only; ignored where U is integrated out */
#define FFVD_TRAIN_ALL 511u
int  ffvd_adam_step(ffvd_handle *h, double lr, double beta1, double beta2, double eps, uint32_t train_mask,
                    double out_terms[8], double *out_nll);
int  ffvd_optimizer_reset(ffvd_handle *h);
int  ffvd_get_params(ffvd_handle *h, const ffvd_params *out_host);
/* overwrite some of the bound parameter arrays from host memory (NULL members are kept): what feeding a stored
 * SG-HMC window sample through feed_dict does in train_hypers (base_model.py:948-949). */
int  ffvd_update_params(ffvd_handle *h, const ffvd_params *p_host);
/* One burn_in_op (burn_in != 0) or sample_op (0) of BaseModel.generate_update_step (base_model.py:143-179) on the
 * device: forward + backward on the resident parameters, then the SG-HMC update of the arrays in sample_mask
 * (FFVD_TRAIN_* bits; X is never sampled, dgp_model.py:213-244) with X_N = T + 1 (dgp_model.py:203).  The handle keeps
 * xi, g, g2 (ones) and p (zeros) per array.  noise: host arrays of standard-normal draws (base_model.py:169) for
 * the sampled arrays, other members ignored.  out_terms / out_nll: the nll before the update. */
int  ffvd_sghmc_step(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in,
                     const ffvd_params *noise_host, double out_terms[8], double *out_nll);
/* ---- sharded training step, device resident (the multi-GPU counterpart of adam.minimize(nll), dgp_model.py:303-305 /
 * train_hypers, base_model.py:944-950, and of burn_in_op / sample_op, base_model.py:143-179) ---------------------------------
 * Every rank runs forward + backward on its shard with S_total (the job's chain count) as the divisor of the mean, which
 * leaves its ADDITIVE share of the job's gradient in ONE device block  [8 term sums | dZ | dlogvariance dloglengthscales
 * dlog_Q dCC dDD dlog_Rchols | dU | dX]  (every segment on a 256-byte boundary; the gradient arrays of ffvd_elbo_grad ARE
 * these segments, nothing is packed).  ONE ncclAllReduce(sum) of the block -- without dX for chain shards, whose rows of X
 * are their own; with it for latent-dim shards, where every rank holds a partial sum for all chains -- then the fused
 * update reads the reduced block.  No gradient crosses PCIe.  out_terms = whole-job sums (out_terms[7] = chains counted),
 * out_nll = their mean, both for the parameters BEFORE the update.  A failed factorisation on any rank makes the sums
 * non-finite on every rank: all return FFVD_ENOTPD and all leave their parameters untouched, so the replicas stay equal.
 * The Adam moments / SG-HMC state live on the handle as for ffvd_adam_step / ffvd_sghmc_step; SG-HMC noise must be the same
 * on every rank (the shared parameters are replicated).  rccl_comm = NULL: the handle's own communicator (ffvd_comm_init).
 * Once a handle belongs to a communicator of more than one rank, plain ffvd_adam_step / ffvd_sghmc_step refuse it
 * (FFVD_EINVAL): they would silently train on the local share only.
 * Three-step form for hosts that carry the exchange themselves (tests: two ranks on ONE GPU over gloo; MPI):
 *   ffvd_train_local(h, S_total)           forward + backward + the 8 sums into the block (enqueue only)
 *   ffvd_train_exchange_count / _ptr       doubles that take part in the exchange / device pointer of the block
 *   ffvd_train_exchange_get / _set         copy the block to / from the host (synchronise)
 *   ffvd_adam_apply / ffvd_sghmc_apply     info + finiteness check, then the update from the block                      */
int  ffvd_adam_step_allreduce(ffvd_handle *h, void *rccl_comm, int S_total, double lr, double beta1, double beta2, double eps,
                              uint32_t train_mask, double out_terms[8], double *out_nll);
int  ffvd_sghmc_step_allreduce(ffvd_handle *h, void *rccl_comm, int S_total, double epsilon, double mdecay,
                               uint32_t sample_mask, int burn_in, const ffvd_params *noise_host, double out_terms[8],
                               double *out_nll);
int  ffvd_train_local(ffvd_handle *h, int S_total);
int64_t ffvd_train_exchange_count(const ffvd_handle *h);
void *ffvd_train_exchange_ptr(ffvd_handle *h);
int  ffvd_train_exchange_get(ffvd_handle *h, double *host_out);
int  ffvd_train_exchange_set(ffvd_handle *h, const double *host_in);
int  ffvd_adam_apply(ffvd_handle *h, double lr, double beta1, double beta2, double eps, uint32_t train_mask,
                     double out_terms[8], double *out_nll);
int  ffvd_sghmc_apply(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in,
                      const ffvd_params *noise_host, double out_terms[8], double *out_nll);

/* ---- multi-GPU: one process per GPU, ONE exchange step ------------------------------------------
 * The reference is single-process (no collective call sites); this build shards chains or latent
 * dims over ranks and all-reduces the 8 partial sums with RCCL over xGMI.  librccl is bound at run time (the copy already
 * mapped in the process, else $FFVD_RCCL_LIB, else the system library); without it these calls return FFVD_EDEVICE.
 *   ffvd_comm_unique_id   rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other ranks by
 *                         any means the host has (file, socket, MPI, a torch.distributed store ...).
 *   ffvd_comm_init        every rank: ncclCommInitRank on the handle's device; the handle owns the communicator
 *                         (ffvd_comm_destroy / ffvd_destroy release it).  Collective: all ranks must call it.
 *   ffvd_elbo_allreduce   one ELBO iteration of this rank's shard + ncclAllReduce(sum, 8 doubles) on the handle's stream
 *                         + one copy back.  rccl_comm: a caller-owned ncclComm_t, or NULL = the handle's own.  out_terms =
 *                         whole-job sums, out_terms[7] = whole-job chain count (only handles with shared_terms = 1 count
 *                         their chains, so latent-dim shards count each chain once), out_nll = out_terms[6] / out_terms[7].  A failed factorisation on this
 *                         rank -> FFVD_ENOTPD with the matrix/pivot; on another rank -> FFVD_ENOTPD (NaN in the sums).
 *   ffvd_elbo_allreduce_async   enqueue only; sums land in out_terms_dev (NULL = the handle's result block).
 *   ffvd_allreduce_sum_async    in-place ncclAllReduce(sum) of `count` doubles at device pointer buf_dev on the handle's
 *                         stream (shared-parameter gradients of a sharded training step; Gram tiles of a T-shard). */
#define FFVD_COMM_ID_BYTES 128
int  ffvd_comm_unique_id(void *id_out /* FFVD_COMM_ID_BYTES */);
int  ffvd_comm_init(ffvd_handle *h, int world, int rank, const void *id /* FFVD_COMM_ID_BYTES */);
int  ffvd_comm_destroy(ffvd_handle *h);
void *ffvd_comm_get(ffvd_handle *h);   /* the handle's ncclComm_t or NULL */
int  ffvd_elbo_allreduce(ffvd_handle *h, void *rccl_comm, double out_terms[8], double *out_nll);
int  ffvd_elbo_allreduce_async(ffvd_handle *h, void *rccl_comm, double *out_terms_dev);
int  ffvd_allreduce_sum_async(ffvd_handle *h, void *rccl_comm, double *buf_dev, int64_t count);
/* the same for a HOST array (staged through a device buffer the handle keeps); synchronises */
int  ffvd_allreduce_sum(ffvd_handle *h, void *rccl_comm, double *buf_host, int64_t count);

/* ---- T-shard fallback (SURVEY 8e last bullet, section 5 "long-context"): when chains x latent dims < ranks ---------
 * T is a pure reduction axis of the collapsed bound: the Gram matrices K_uf K_fu (M x M per unit) and the rows
 * delta^T K_fu, the likelihood and transition sums are all sums over t.  A T-shard handle (cfg.T = rows of the shard,
 * cfg.T_total, cfg.t_begin; FFVD_BRANCH_B, FFVD_ROUTE_GRAM, FFVD_F64; X = rows t_begin .. t_begin + T of
 * every chain, Y / control_inputs = the shard's rows) evaluates its rows' share; ONE all-reduce(sum) of the raw Gram
 * tiles + the per-chain partial sums (S_local * D * (M_p + 1) * M_p + 8 S_local doubles, M_p = M rounded up to 64)
 * follows, and EVERY rank finishes the same factorisations on the reduced sums, so every rank holds the whole-job
 * terms (out_terms[7] = S_local).  ffvd_elbo_tshard = local part + ncclAllReduce on the handle's stream + finish.
 * The three-step form lets a host carry the buffer itself (tests: two ranks on one GPU over gloo). */
int  ffvd_elbo_tshard(ffvd_handle *h, void *rccl_comm, double out_terms[8], double *out_nll);
int  ffvd_tshard_local(ffvd_handle *h);                       /* enqueue this shard's partial sums               */
int64_t ffvd_tshard_count(const ffvd_handle *h);              /* doubles in the exchange buffer                   */
int  ffvd_tshard_get(ffvd_handle *h, double *host_out);       /* copy the exchange buffer to the host (synchronises) */
int  ffvd_tshard_set(ffvd_handle *h, const double *host_in);  /* ... and the reduced sums back                    */
int  ffvd_tshard_finish(ffvd_handle *h, double out_terms[8], double *out_nll);
/* Gradient of a T-sharded job (cfg.grad = 1, every latent dim on the handle).  After the exchange of the raw tiles every shard
 * holds the job's A = K_uu + K_uf K_fu / Q, its factor, u and Gamma, so the backward pass needs no further operand from the other
 * shards: its K_fu side (the T x M product and its reductions, dgp_model.py:261-288 differentiated) runs over the shard's own rows
 * and is ADDITIVE over shards like the likelihood and transition sums; the M x M side (K_uu chain rule, tr(A^-1 G), u^T G u, the
 * priors) is identical on every shard and counted on the first (t_begin == 0) only.  ffvd_tshard_finish_grad = finish + backward
 * pass (divisor S_total, every 1 / T the job's T_total); it leaves the block [8 term sums (first shard; zero elsewhere) | dZ |
 * dlogvariance | dloglengthscales | dlog_Q | dCC | dDD | dlog_Rchols] at ffvd_train_exchange_ptr, ffvd_train_exchange_count
 * doubles: ONE all-reduce(sum) of it (ffvd_allreduce_sum_async, or ffvd_train_exchange_get / _set through the host) completes
 * the gradient and the terms on every rank; ffvd_tshard_grad_fetch then copies it out.  dX covers the shard's OWN T + 1 rows and
 * does not take part in the exchange: the row two neighbouring shards share (the last of one, the first of the next) receives a
 * part from each, which the caller adds.  ffvd_elbo_tshard_grad = all of it with the two native RCCL all-reduces. */
int  ffvd_tshard_finish_grad(ffvd_handle *h, int S_total, double out_terms[8], double *out_nll);
int  ffvd_tshard_grad_fetch(ffvd_handle *h, double out_terms[8], const ffvd_grads *gout);
int  ffvd_elbo_tshard_grad(ffvd_handle *h, void *rccl_comm, int S_total, double out_terms[8], double *out_nll,
                           const ffvd_grads *gout);
/* Optimiser step of a T-sharded job (the reference trains every variable with one AdamOptimizer, dgp_model.py:303-305).  Call after
 * ffvd_tshard_grad_fetch / ffvd_elbo_tshard_grad: the exchanged block already holds the job's shared-parameter gradients, identical
 * on every shard.  `dX_rows` = the shard's own S_local x (T + 1) x D rows of dX AFTER the caller has added the neighbouring shards'
 * parts of the first and the last row (host memory; ffvd_amd/distributed.py exchanges them with one small all-reduce).  The fused
 * Adam update then runs over every array of `train_mask`; shared parameters and both copies of a boundary row receive identical
 * gradients and carry identical state, so the shards stay in step without a broadcast.  out_terms = the job's 8 sums. */
int  ffvd_tshard_adam_apply(ffvd_handle *h, const double *dX_rows, double lr, double beta1, double beta2, double eps,
                            uint32_t train_mask, double out_terms[8], double *out_nll);
/* ... and the SG-HMC update (burn_in_op / sample_op, base_model.py:143-179) of a T-sharded job from the same exchanged block: X is
 * never an SG-HMC variable, so no rows travel; `noise` must be identical on every shard; X_N of the step size is the JOB's row
 * count (T_total + 1). */
int  ffvd_tshard_sghmc_apply(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in,
                             const ffvd_params *noise, double out_terms[8], double *out_nll);

/* the handle's HIP stream (a hipStream_t), so that a collective library or another framework can order its work after
 * ffvd_elbo_async without a host synchronisation (e.g. torch.cuda.ExternalStream around the RCCL all-reduce). */
void *ffvd_get_stream(ffvd_handle *h);
/* after a synchronous ffvd_elbo: per-chain nll values (S_local doubles, host) */
int  ffvd_chain_nll(ffvd_handle *h, double *out_nll_per_chain);
/* timing helper for benchmarks: run `iters` back-to-back ffvd_elbo_async on the resident inputs,
 * bracketed by HIP events on the handle's stream; returns total milliseconds. */
int  ffvd_time_elbo(ffvd_handle *h, int iters, float *out_ms);
/* HIP-event timing of each stage of one iteration (ms): [0] K_uu build+Cholesky+inverse,
 * [1] K_fu projection (F = K_fu L^-T), [2] Gram H = F^T F, [3] Cholesky(H)+solve, [4] reductions. */
int  ffvd_profile_stages(ffvd_handle *h, float out_ms[8]);
/* live stage timing: while enabled, every ffvd_elbo* records HIP events on the handle's stream around the
 * stages above; ffvd_stage_times() synchronises, returns the accumulated milliseconds and the number of timed
 * intervals (= kernel-launch groups) per stage since the last read, and resets the accumulators. */
int  ffvd_stage_timing(ffvd_handle *h, int enable);
int  ffvd_stage_times(ffvd_handle *h, double out_ms[8], int32_t out_launches[8]);

/* ---- operator-level entry points (host pointers in/out; they allocate temporaries) ----------
 * These mirror the reference's pure functions so that parity tests read like calls of the reference. */

/* kernel.K(X, X2) / kernel.K(X) (X2 == NULL) for ONE kernel: kernels_multi_output.py:202-214, kernels.py:270-276.
 * jitter is added to the diagonal when X2 == NULL. out: N x N2. */
int  ffvd_op_kernel_matrix(int kind, const double *X, int N, const double *X2, int N2, int P,
                           double logvariance, const double *loglengthscales, double jitter, double *out);
/* kernel.Kdiag(X): kernels_multi_output.py:199-200, kernels.py:278-281. out: N. */
int  ffvd_op_kernel_diag(int kind, const double *X, int N, int P, double logvariance, double *out);
/* batched lower Cholesky of `batch` n x n SPD matrices (tf.linalg.cholesky, conditionals_multi_output.py:28,162).
 * Only the lower triangle of A is read (entries above the diagonal are ignored, NaN included); L comes back with an exactly zero
 * strict upper triangle. A and L may alias. info (may be NULL) [b] = 0 or 1 + index of the first pivot that is not positive (NaN
 * included). Returns FFVD_ENOTPD if any info != 0; the message names the first such matrix. */
int  ffvd_op_cholesky(const double *A, int n, int batch, double *L, int32_t *info);
/* The whitened triangular solve of base_conditional: A = Lm^-1 Kmn = tf.linalg.triangular_solve(Lm, Kmn, lower=True)
 * (conditionals_multi_output.py:34, conditionals.py:30).  L: n x n lower triangular (entries above the diagonal are ignored),
 * B: n x m, X: n x m = L^-1 B.  Runs the wavefront-level blocked substitution of the Cholesky panel step on its own. */
int  ffvd_op_trsm(const double *L, int n, const double *B, int m, double *X);
/* kernel_pre_cal (conditionals_multi_output.py:124-169): for D kernels returns the stack of L_d^{-T} (D x M x M, upper). */
int  ffvd_op_kernel_pre_cal(int kind, const double *Z, int M, int P, int D, const double *logvariance,
                            const double *loglengthscales, double jitter, double *Lm_inverse_seq);
/* collapse_after_kernel_precalculation (conditionals_multi_output.py:230-257).
 * X_combine: T x P, X: (T+1) x D, Q: D.  out3 = (-term1/Y_N, -term2/Y_N, -trace/Y_N). */
int  ffvd_op_collapse(int kind, const double *Lm_inverse_seq, const double *X_combine, const double *X,
                      const double *Z, int T, int M, int P, int D, const double *logvariance,
                      const double *loglengthscales, const double *Q, double batch_size, double Y_N, double out3[3]);
/* conditional(Xnew, Z, kern, f, white=True, full_cov=False) (conditionals_multi_output.py:73-120 -> base_conditional :6-70).
 * Xnew: N x P, f: M x D.  mean, var: N x D. */
int  ffvd_op_conditional(int kind, const double *Xnew, int N, const double *Z, int M, int P, int D,
                         const double *logvariance, const double *loglengthscales, const double *f,
                         double jitter, double *mean, double *var);

/* collapse_u_mean_after_kernel_precalculation (conditionals_multi_output.py:206-227): posterior mean of the whitened
 * inducing outputs U_mean (M x D, = H_d^-1 b_d per column) and the stack L_{H_d}^{-T} (D x M x M, upper). */
int  ffvd_op_collapse_u_mean(int kind, const double *Lm_inverse_seq, const double *X_combine, const double *X,
                             const double *Z, int T, int M, int P, int D, const double *logvariance,
                             const double *loglengthscales, const double *Q, double *U_mean, double *H_inv_sqrt);
/* conditional_after_kernel_precalculation(..., white=True, full_cov=False) (conditionals_multi_output.py:306-387).
 * q_sqrt: NULL, or the M x M slice d = 0 of the D x M x M stack -- the reference hands the whole stack to every
 * dim and `[:, :, 0]` (:322) keeps slice 0 for all of them; the caller passes that slice. */
int  ffvd_op_conditional_precalc(int kind, const double *Lm_inverse_seq, const double *Xnew, int N, const double *Z,
                                 int M, int P, int D, const double *logvariance, const double *loglengthscales,
                                 const double *f, const double *q_sqrt, double *mean, double *var);
/* conditional(Xnew, Z, kern, f, full_cov=..., q_sqrt=..., white=True) (conditionals_multi_output.py:73-120 -> base_conditional
 * :6-70), per latent dim d with F_d = K_d(Xnew, Z) L_d^-T (N x M) and L_d = chol(K_d(Z, Z) + jitter I):
 *   mean: N x D, the same values as ffvd_op_conditional.
 *   full_cov = 0: var N x D, var[:, d] = Kdiag_d(Xnew) - sum_j F_d[:, j]^2 (+ sum_j E_d[:, j]^2 with q_sqrt).
 *   full_cov = 1: var D x N x N (GPflow's R x N x N layout), var[d] = K_d(Xnew, Xnew) - F_d F_d^T (+ E_d E_d^T with q_sqrt),
 *                 exactly symmetric.  The reference's final stacking (`[:, :, 0]` and a transpose, :120) is written for N x 1
 *                 blocks and does not return a covariance for N x N ones: not reproduced.
 * q_sqrt: NULL, or the M x M slice 0 of the D x M x M stack, used as given (no triangle mask): E_d = F_d q_sqrt for EVERY d -- the
 * convention of ffvd_op_conditional_precalc (the reference hands the whole stack to every dim and keeps index 0).  A 2-D (M x D)
 * q_sqrt is the slice diag(q_sqrt[:, 0]) (built by the caller).  M <= 2048 when q_sqrt is given.
 * Returns FFVD_EINVAL (before any device work) on a null pointer, N < 0, full_cov not 0 / 1, M > 2048 with q_sqrt. */
int  ffvd_op_conditional_cov(int kind, const double *Xnew, int N, const double *Z, int M, int P, int D,
                             const double *logvariance, const double *loglengthscales, const double *f, const double *q_sqrt,
                             int full_cov, double jitter, double *mean, double *var);
/* conditional_after_kernel_precalculation(..., full_cov=..., q_sqrt=..., white=True) (conditionals_multi_output.py:306-387): as
 * ffvd_op_conditional_cov with the caller's stack Lm_inverse_seq = L_d^-T (D x M x M) instead of the factorisation. */
int  ffvd_op_conditional_precalc_cov(int kind, const double *Lm_inverse_seq, const double *Xnew, int N, const double *Z, int M,
                                     int P, int D, const double *logvariance, const double *loglengthscales, const double *f,
                                     const double *q_sqrt, int full_cov, double *mean, double *var);
/* get_rand((mean, var), eps, full_cov=True) (utils.py:4-11): the joint draw out[:, d] = mean[:, d] + L_d eps[:, d],
 * L_d = chol(var[d] + jitter I).  mean, eps, out: N x D; var: D x N x N (ffvd_op_conditional_cov, full_cov = 1).  The DGP code the
 * reference derives get_rand from uses jitter 1e-7.  A var[d] + jitter I that is not positive definite returns FFVD_ENOTPD; the
 * message names the dim and the pivot. */
int  ffvd_op_get_rand_full_cov(const double *mean, const double *var, const double *eps, int N, int D, double jitter, double *out);
/* Gaussian.predict_mean(X_end) = X_end @ CC + DD (likelihoods.py:76-79). X_end: N x D, out: N x Ydim. */
int  ffvd_op_predict_mean(const double *X_end, int N, int D, const double *CC, const double *DD, int Ydim, double *out);
/* logdensity_norm_diag (nonvec = 0, out: N; likelihoods.py:96-111) / logdensity_norm_diag_nonvec (nonvec = 1,
 * out: N x J; likelihoods.py:89-93).  y, ymean: N x J; Rchols: J.  No log(2 pi) constants, as in the reference. */
int  ffvd_op_logdensity_norm_diag(int nonvec, const double *y, const double *ymean, const double *Rchols, int N, int J,
                                  double *out);
/* get_rand (utils.py:11, diagonal case) with the standard-normal draw injected: out = mean + eps * sqrt(var). */
int  ffvd_op_get_rand(const double *mean, const double *var, const double *eps, int64_t n, double *out);

/* One Adam update of a flat host array (in place: theta, m, v), t = 1-based step count; same rule as ffvd_adam_step. */
int  ffvd_op_adam_step(double *theta, const double *grad, double *m, double *v, int64_t n, double lr, double beta1,
                       double beta2, double eps, int64_t t);
/* One SG-HMC update, BaseModel.generate_update_step base_model.py:143-179, of a flat host array (in place):
 * state xi, g, g2 (initialised to ones by the reference) and momentum p (zeros); noise = the standard-normal draw of
 * :169 (injected); epsilon, mdecay as DGPSSM(epsilon=0.01, mdecay=0.05) dgp_model.py:161; X_N = number of training
 * rows (:164).  burn_in != 0 = burn_in_op (xi, g, g2, theta, p move), 0 = sample_op (theta, p only).  Every
 * right-hand side reads the state from before the call. */
int  ffvd_op_sghmc_step(double *theta, const double *grad, double *xi, double *g, double *g2, double *p,
                        const double *noise, int64_t n, double epsilon, double mdecay, double X_N, int burn_in);

/* The ffvd_op_* entry points keep their device temporaries and their stream in a per-thread cache between calls (a rollout call
 * made ~27 allocations around its step loop: 2.7 ms of host work per call).  ffvd_op_release_cache frees what the calling thread's
 * cache holds; the cache also trims itself beyond 256 blocks / 8 GiB.  A host that runs ffvd_op_* calls on short-lived threads
 * calls it before a thread exits (nothing is freed at thread exit: the HIP runtime may already be shutting down then). */
int  ffvd_op_release_cache(void);

/* The prediction loop of collect_samples_formal (base_model.py:288-314) for R posterior rollouts advanced side by
 * side on the device: per step, conditional_after_kernel_precalculation at the R current states (:300, q_sqrt = the
 * d = 0 slice or NULL as in ffvd_op_conditional_precalc), then x_next = x + f_mu + eps * sqrt(f_var + Q) (:304-306).
 * x_last: D (= layers[-1].X[-1], :226); ctrl: steps x C, row t = control_inputs[Y_train.shape[0] + t] (:293), NULL when
 * C = 0; f = U_val: M x D; eps: steps x R x D standard-normal draws (injected); outputs R x steps x D:
 * predict_x (:313) and predict_var = f_var + Q (:314).
 * M <= 2048, P = D + C <= 32.  Lm_inverse_seq must be upper triangular, as ffvd_op_kernel_pre_cal returns it: the step products skip
 * its strict lower triangle without reading it (and that of W q_sqrt when the q_sqrt slice is upper triangular, which is checked).
 * Which form runs: the resident-operand loop when R <= 32 (R <= 64 with FFVD_STEP_LOOP=2), M <= 512, D <= 8 and P <= 8; otherwise
 * per-step launches, the skinny step product for R <= 512 and the tiled projection beyond. */
int  ffvd_op_rollout(int kind, const double *Lm_inverse_seq, const double *Z, int M, int P, int D,
                     const double *logvariance, const double *loglengthscales, const double *f, const double *q_sqrt,
                     const double *x_last, int R, const double *ctrl, int C, int steps, const double *log_Q,
                     const double *eps, double *predict_x, double *predict_var);
/* How many ffvd_op_rollout calls of this process completed on the per-step launches because the resident-operand loop (the default
 * up to 32 rollouts, up to 64 with FFVD_STEP_LOOP=2; M <= 512) gave up on a bounded wait -- its workgroups must all be resident, a
 * co-tenant can prevent that.  The two forms agree to 1e-9 but not bit for bit: a seeded rollout is bit-reproducible only while this
 * counter stands still (or with FFVD_STEP_LOOP=0, which always takes the launches).  The call that fell back also leaves a warning
 * in ffvd_last_error(NULL). */
int  ffvd_op_rollout_fallbacks(void);

/* The same prediction loop (base_model.py:223-314) for G INDEPENDENT posteriors in one call: one per SG-HMC sample of cases 2/3/5 (every
 * sample num_i has its own hyper-parameters, :223-240) or one per chain.  Group g has its own Lm_inverse_seq, Z, hyper-parameters,
 * f = U_val, q_sqrt slice, x_last and log_Q; kind, M, P, D, C, R, steps and ctrl are common.  Per step, group, rollout and dim the
 * arithmetic is that of ffvd_op_rollout.  The big operands are handed over as POINTER TABLES, so that nothing is packed on the host:
 * Lm_inverse_seqs: G * D pointers (entry g * D + d -> the M x M matrix of group g, dim d), q_sqrts: G pointers (entry g -> the M x M
 * d = 0 slice of group g's stack, it inflates every dim: SURVEY a14) or NULL for all groups; each matrix goes straight into its slot of
 * the padded device stack.  The other arrays are packed, row-major, group outermost: Zs G x M x P;
 * logvariances G x D; loglengthscales G x D x P (NULL for LinearK); fs G x M x D; x_lasts G x D; log_Qs G x D; ctrl steps x C (NULL when C = 0);
 * eps steps x G x R x D; outputs predict_x and predict_var = f_var + Q, each G x R x steps x D.
 * Every Lm_inverse_seq must be upper triangular, as ffvd_op_kernel_pre_cal returns it: the step products skip its strict lower triangle
 * without reading it (and that of W q_sqrt when every group's q_sqrt slice is upper triangular, which is checked).
 * Determinism: a step is one launch over a fixed set of workgroups per group that depends on (M, D, R) only; nothing waits on another
 * workgroup, no workgroup needs to be resident with another, there is no second form and no fallback.  Group g's outputs are
 * bit-identical whether it is computed alone (G = 1) or among any other groups, from run to run, and whatever else the GPU is doing.
 * f_var + Q <= 0 gives NaN from that step of that rollout on, as in ffvd_op_rollout; nothing faults.
 * Limits: M <= 2048, P = D + C <= 32, G * D * Mp^2 <= 2^29 (Mp = M rounded up to 16: 4 GiB per operand stack), G * R <= 2^20,
 * R <= 524280; FFVD_EINVAL beyond them, before any device work.  G = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_rollout_grouped(int kind, int G, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                             const double *logvariances, const double *loglengthscales, const double *fs,
                             const double *const *q_sqrts, const double *x_lasts, int R, const double *ctrl, int C, int steps,
                             const double *log_Qs, const double *eps, double *predict_x, double *predict_var);

/* The collapsed posterior of G groups in one call: per group what ffvd_op_kernel_pre_cal (conditionals_multi_output.py:124-169) and
 * ffvd_op_collapse_u_mean (:206-227) compute one after the other, as base_model.py:243-256 calls them -- one group per chain of a
 * trained model (n_models = 1: Z and the hyper-parameters are shared, so is W = L^-T) or per SG-HMC sample (n_models = G: every group
 * has its own).  Units b = g * D + d run through the ELBO's batch launches; the K_uu slabs, the zeroed H slabs with their identity
 * rows, F and L_H^-T never leave the device, and there is no host synchronisation before the factorisation flags are read (once).
 * Packed, row-major, group outermost: Zs n_models x M x P; logvariances n_models x D; loglengthscales n_models x D x P (NULL for
 * LinearK); Xs G x (T+1) x D; ctrl_fit T x C (NULL when C = 0), common to the groups; log_Qs G x D (log Q: :215 divides by exp of it).
 * Outputs: U_means G x M x D; H_inv_sqrts G x D x M x M (L_H^-T, :222) or NULL; Lm_inverse n_models x D x M x M (L^-T) or NULL.
 * groups_per_pass: F = K_fu L^-T takes D * Tp * Mp doubles per group (Tp, Mp: T, M rounded up to 64) and is reused between passes of
 * that many groups; 0 = the largest count whose F is at most 2 GiB (at least 1), a function of the shapes alone.
 * Determinism: two identical calls give bit-identical outputs (fixed summation orders, no atomics on results).  A group's posterior
 * is NOT promised to be independent of G or groups_per_pass: the batch launches choose their shape from the number of units.
 * Errors: a non-positive pivot gives FFVD_ENOTPD and ffvd_last_error names the group, the latent dim and the matrix (K_uu + jitter*I
 * or H); a one-launch Cholesky that gave up on a bounded wait is re-run with the launch-per-column variant (a warning says so).  No
 * output is written on failure.
 * Limits: M <= 2048, P = D + C <= 32, T >= 1, n_models 1 or G; FFVD_EINVAL beyond them, before any device call.  G = 0: FFVD_OK,
 * nothing is touched. */
int  ffvd_op_posterior_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                               const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                               const double *log_Qs, double jitter, int groups_per_pass, double *Lm_inverse, double *U_means,
                               double *H_inv_sqrts);

/* ffvd_op_posterior_grouped followed by ffvd_op_rollout_grouped (base_model.py:243-314 per group: posterior, then R rollouts of
 * `steps` steps from the last row of the group's X) WITHOUT the posteriors leaving the device: W, the d = 0 slice of L_H^-T (it
 * inflates every dim), f = U_mean and x_last are written into the rollout loop's operands by device kernels -- padding
 * and strict lower triangles as exact zeros -- and the loop's own launches follow unchanged.  Only the inputs above, ctrl_roll
 * steps x C (NULL when C = 0), eps steps x G x R x D and the results predict_x, predict_var = f_var + Q (G x R x steps x D) and,
 * optionally, U_means (G x M x D) cross the host link.  The flags are read before the first step is enqueued; errors as above.
 * Limits: those of ffvd_op_posterior_grouped and of ffvd_op_rollout_grouped.  G = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_posterior_rollout_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                       const double *logvariances, const double *loglengthscales, const double *Xs,
                                       const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                       int groups_per_pass, int R, const double *ctrl_roll, int steps, const double *eps,
                                       double *predict_x, double *predict_var, double *U_means);

/* The held-out predictive summary of base_model.py:330-348 over N rollouts, and what it lacks: the total variance and the predictive
 * log density.  predict_x, predict_var (= f_var + Q, :311): N x steps x D, as the rollout operators return them (G x R x steps x D is
 * N = G * R); CC D x J, DD J (the emission, :341); noise_std J: s_j > 0, the standard deviation of the emission noise of output j
 * (the Python layer passes exp(log_Rchols[0, :]), the row the likelihood uses); Y_test n_test x J (NULL when n_test = 0), the
 * held-out observations of steps t < n_test.  With p[n][t][j] = sum_k predict_x[n][t][k] CC[k][j] (k ascending):
 *   y_mean[t][j]      = (1/N) sum_n p + DD_j                                          (:341)
 *   y_var[t][j]       = (1/N) sum_n sum_k predict_var[n][t][k] CC[k][j]^2 + s_j^2     (:342: the mean of the one-step variances)
 *   y_var_total[t][j] = s_j^2 + (1/N) sum_n (p - pbar)^2     (law of total variance: the noise plus the spread of the rollouts; from
 *                       centred sums -- Welford per chunk of 32 rollouts, (count, mean, M2) merged pairwise -- never E[p^2] - E[p]^2)
 *   lpd[t][j]         = log (1/N) sum_n N(Y_test[t][j]; p + DD_j, s_j^2)              (the largest exponent is subtracted before summing)
 *   lpd_gauss[t][j]   = log N(Y_test[t][j]; y_mean[t][j], y_var_total[t][j])
 * y_mean, y_var, y_var_total: steps x J; lpd, lpd_gauss: n_test x J; each output may be NULL, at least one must not be.  Per-output
 * marginals only: no joint density over the J outputs.
 * Determinism: a wavefront owns 32 rollouts and 64 steps and sums in ascending rollout order, a second launch merges the chunks in
 * ascending order; no atomics.  The decomposition depends on (N, steps, D, J) only: two calls are bit-identical.
 * Limits: 1 <= D <= 32, 1 <= J <= 8, 0 <= n_test <= steps, N * steps * D < 2^31, every s_j finite and positive, Y_test given when
 * n_test > 0 or an lpd output is requested; FFVD_EINVAL otherwise, before any device call.  N = 0 or steps = 0: FFVD_OK, nothing is
 * touched. */
int  ffvd_op_rollout_summary(const double *predict_x, const double *predict_var, int N, int steps, int D, const double *CC,
                             const double *DD, const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean,
                             double *y_var, double *y_var_total, double *lpd, double *lpd_gauss);

/* ffvd_op_rollout_grouped with the summary of ffvd_op_rollout_summary (base_model.py:330-348) over all N = G * R rollouts, formed on
 * the device stacks the step launches wrote, before any download.  The arguments of ffvd_op_rollout_grouped, then those of the
 * summary.  predict_x / predict_var may each be NULL: that stack is then not downloaded, and the summary does not depend on it.
 * The stacks are bit-identical to ffvd_op_rollout_grouped's, the summary to ffvd_op_rollout_summary's on those stacks.
 * Limits: those of both.  G = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_rollout_grouped_summary(int kind, int G, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                                     const double *logvariances, const double *loglengthscales, const double *fs,
                                     const double *const *q_sqrts, const double *x_lasts, int R, const double *ctrl, int C, int steps,
                                     const double *log_Qs, const double *eps, double *predict_x, double *predict_var,
                                     const double *CC, const double *DD, const double *noise_std, int J, const double *Y_test,
                                     int n_test, double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss);

/* ffvd_op_posterior_rollout_grouped with the summary of ffvd_op_rollout_summary (base_model.py:330-348) in the same way: posteriors,
 * rollouts and summary without anything but the inputs and the steps x J results crossing the host link when predict_x, predict_var
 * and U_means are NULL. */
int  ffvd_op_posterior_rollout_grouped_summary(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                               const double *logvariances, const double *loglengthscales, const double *Xs,
                                               const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                               int groups_per_pass, int R, const double *ctrl_roll, int steps, const double *eps,
                                               double *predict_x, double *predict_var, double *U_means, const double *CC,
                                               const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                                               double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss);

/* The posterior transition function f(x, c) of G groups at N common inputs: conditional_after_kernel_precalculation
 * (conditionals_multi_output.py:306-387, white=True, full_cov=False) for every group in one launch sequence.  Group g uses model
 * m(g) (n_models = 1: Z, the hyper-parameters and W = L^-T are shared; n_models = G: own).  With F_{m,d} = K_d(Xnew, Z_m) W_{m,d}
 * (:349), projected once per (model, dim):
 *   means[g][n][d] = sum_j F_{m(g),d}[n][j] U_g[j][d]                                                      (:365)
 *   vars[g][n][d]  = Kdiag_d(x_n) - sum_j F_{m(g),d}[n][j]^2 + sum_j (F_{m(g),d} q_{g,d'})[n][j]^2         (:356, :369-380)
 * q_mode 0 ("reference"): d' = 0, slice 0 of the group's L_H^-T stack inflates every dim (the stack is handed to every dim at :317,
 * `[:, :, 0]` at :322 keeps slice 0) and q_sqrts holds G pointers; q_mode 1 ("intent"): d' = d, G * D pointers, entry
 * g * D + d.  q_sqrts = NULL: no third term (explicit U, SG-HMC samples of U).  The pooled posterior is the equal-weight mixture,
 * summed over g in ascending order: mix_mean = (sum_g mean_g) / G, mix_var = (sum_g (var_g + mean_g^2)) / G - mix_mean^2.
 * Lm_inverse_seqs: n_models * D pointers, entry m * D + d -> M x M, upper triangular; every matrix goes from the caller's memory
 * into its slot of a padded device stack.  Zs n_models x M x P; logvariances n_models x D; loglengthscales n_models x D x P (NULL
 * for LinearK); fs G x M x D; Xnew N x P.  Outputs: means, vars G x N x D, either may be NULL; mix_mean, mix_var N x D, both or
 * neither; at least one output overall.
 * The third term is a 128 x 128-tiled fp64-MFMA product whose epilogue keeps only row sums of squares.  When every q slice is upper
 * triangular (checked on the host) the k range of a column tile ends at its last column; a dense slice takes the full range and, where
 * its strict lower triangle is zero, gives the same bits.
 * rows_per_pass: F takes n_models * D * rows * Mp doubles (Mp: M rounded up to 64) and is reused between passes over the rows of
 * Xnew; 0 = the largest multiple of 128 whose F is at most 2 GiB, a function of the shapes alone; a positive value forces the size.
 * Determinism: two identical calls are bit-identical; a group's means / vars do not depend on G or on the other groups, nor on the
 * pass size (fixed summation orders, no atomics).
 * Limits: M <= 2048, D <= P <= 32, n_models 1 or G, N >= 0, q_mode 0 or 1, rows_per_pass >= 0, G * D <= 2^24, G * D * Mp^2 <= 2^29
 * doubles (the q stack), G * N * D < 2^31; FFVD_EINVAL beyond them, before any device call.  G = 0 or N = 0: FFVD_OK, nothing is
 * touched. */
int  ffvd_op_conditional_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                 int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                 const double *const *q_sqrts, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                 double *means, double *vars, double *mix_mean, double *mix_var);

/* ffvd_op_posterior_grouped (kernel_pre_cal :124-169 and collapse_u_mean_after_kernel_precalculation :206-227, as base_model.py:243-256
 * calls them) followed by ffvd_op_conditional_grouped (:306-387) WITHOUT the posteriors leaving the device: W is read where the K_uu
 * chain left it, f = U_mean where the matvec left it, and the q slices (q_mode 0: slice 0 of each group, q_mode 1: all D) are packed
 * by a device kernel with exact zeros in the padding and the strict lower triangle, so the triangular k cut holds by construction.
 * Up the host link go the inputs; down come the factorisation flags, once, and the requested outputs (U_means G x M x D optional).
 * Errors, stall recovery, "no output written on failure" and determinism: as ffvd_op_posterior_grouped.
 * Limits: those of ffvd_op_posterior_grouped and of ffvd_op_conditional_grouped.  G = 0 or N = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_posterior_conditional_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                           const double *logvariances, const double *loglengthscales, const double *Xs,
                                           const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                           int groups_per_pass, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                           double *means, double *vars, double *mix_mean, double *mix_var, double *U_means);

/* Linearisation of the transition function: ffvd_op_conditional_grouped's mean and variance TOGETHER WITH their gradients with respect
 * to the rows of Xnew, all P = D + C columns (the first D give d/dx, the last C give d/dc).  SE-ARD kernels only (FFVD_EINVAL for
 * LinearK: its Jacobian is constant).  conditional_after_kernel_precalculation (conditionals_multi_output.py:306-387, white=True,
 * full_cov=False) written with the posterior terms of ffvd_op_moment_grouped, beta = W_d u_{g,d} and Gamma = W_d (I - q q^T) W_d^T
 * (q: slice 0 of the group's stack for q_mode 0, slice d for q_mode 1; q_sqrts = NULL: W_d W_d^T), and differentiated: with
 * k_j = variance_d exp(-sum_p (x_p - z_jp)^2 / (2 l_dp^2)) (:349's K(Xnew, Z)), nu_jp = z_jp - x_p and t = Gamma k,
 *   means[g][n][d]     = sum_j k_j beta_j                              (:365)
 *   vars[g][n][d]      = variance_d - sum_j k_j t_j                    (:356, :369-380)
 *   dmeans[g][n][d][p] =  (1 / l_dp^2) sum_j k_j beta_j nu_jp
 *   dvars[g][n][d][p]  = -(2 / l_dp^2) sum_j k_j t_j nu_jp
 * The mixture keeps ffvd_op_conditional_grouped's mix_mean / mix_var; its gradients in centred form, g ascending:
 *   mix_dmean = (sum_g dmean_g) / G,   mix_dvar = (sum_g (dvar_g + 2 (mean_g - mix_mean) dmean_g)) / G.
 * The local linear model of x' = x + f(x, c) at row n is A = I + dmeans[g][n][:, :D], B = dmeans[g][n][:, D:].
 * Arguments as ffvd_op_conditional_grouped.  Outputs: means, vars G x N x D; dmeans, dvars G x N x D x P; mix_mean, mix_var N x D;
 * mix_dmean, mix_dvar N x D x P.  Any may be NULL, at least one must be given; mix_mean and mix_var both or neither; mixture gradients
 * only together with the mixture values.  The variance side (Gamma and the product below) is skipped when none of vars, dvars,
 * mix_var, mix_dvar is asked for.
 * K(Xnew, Z) is built once per (model, dim) and pass.  The variance side is a 128 x 128-tiled fp64-MFMA product T = K Gamma per unit --
 * (group, dim) with q_sqrts, (model, dim) without -- whose epilogue keeps P + 1 weighted row sums per column tile; T never reaches memory.
 * rows_per_pass: as ffvd_op_conditional_grouped (K takes n_models * D * rows * Mp doubles).
 * Determinism: two identical calls are bit-identical; a group's outputs do not depend on G or on the other groups, a row's outputs
 * not on N, on the other rows or on the pass size (fixed summation orders, no atomics).
 * Limits: those of ffvd_op_conditional_grouped and G * D * N * P < 2^31; FFVD_EINVAL beyond them, before any device call.  G = 0 or
 * N = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_conditional_grad_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                      int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                      const double *const *q_sqrts, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                      double *means, double *vars, double *dmeans, double *dvars, double *mix_mean, double *mix_var,
                                      double *mix_dmean, double *mix_dvar);

/* ffvd_op_posterior_grouped (kernel_pre_cal :124-169 and collapse_u_mean_after_kernel_precalculation :206-227, as base_model.py:243-256
 * calls them) followed by ffvd_op_conditional_grad_grouped WITHOUT the posteriors leaving the device, as
 * ffvd_op_posterior_conditional_grouped: W is packed from the K_uu slabs, f = U_mean where the matvec left it, the q slices are packed
 * by a device kernel.  Errors, stall recovery, "no output written on failure" and determinism: as ffvd_op_posterior_grouped.
 * Limits: those of ffvd_op_posterior_grouped and of ffvd_op_conditional_grad_grouped.  G = 0 or N = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_posterior_conditional_grad_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                const double *logvariances, const double *loglengthscales, const double *Xs,
                                                const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                int groups_per_pass, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                                double *means, double *vars, double *dmeans, double *dvars, double *mix_mean,
                                                double *mix_var, double *mix_dmean, double *mix_dvar, double *U_means);

/* Moment-matched prediction: the Gaussian state x_t ~ N(mu, Sigma) of each of G posteriors is pushed through
 * x_{t+1} = x_t + f(x_t, ctrl_t) + N(0, Q) in closed form and re-approximated as a Gaussian (Girard et al. 2003; the propagation of
 * PILCO); one launch per step for all groups, nothing is sampled.  SE-ARD kernels only.  The posterior is that of
 * ffvd_op_conditional_grouped, with the same arguments: m_a(x) = k_a(x, Z) beta_a, v_a(x) = variance_a - k_a(x, Z) Gamma_a k_a(Z, x),
 * beta_a = W_a u_a, Gamma_a = W_a (I - q q^T) W_a^T (q_sqrts = NULL: W_a W_a^T); q_mode 0 ("reference"): q is slice 0 of the group's
 * stack for every dim (G pointers; what the rollouts use), q_mode 1 ("intent"): slice a (G * D pointers, entry g * D + a).
 * Per step, with nu_i = z_i - [mu ; ctrl_t], lambda_a the first D entries of 1 / lengthscales_a^2 and R_a = Sigma diag(lambda_a) + I:
 *   E[f_a]        = sum_i beta_ai q^a_i,  q^a_i = variance_a |R_a|^-1/2 exp(-nu_i^xT (Sigma + Lambda_a^xx)^-1 nu_i^x / 2 - (control part) / 2)
 *   Cov(f_a, f_b) = sum_ij beta_ai beta_bj (Q^ab_ij - q^a_i q^b_j),  a = b: + variance_a - sum_ij Gamma_a,ij Q^aa_ij, where
 *   Q^ab_ij       = variance_a variance_b |R|^-1/2 exp(-nu_i^T Lambda_a^-1 nu_i / 2 - nu_j^T Lambda_b^-1 nu_j / 2 + (a_i + b_j)^T T (a_i + b_j) / 2),
 *                   R = Sigma diag(lambda_a + lambda_b) + I, T = R^-1 Sigma, a_i = lambda_a nu_i^x, b_j = lambda_b nu_j^x
 *   Cov(x, f_a)   = Sigma (Sigma + Lambda_a^xx)^-1 sum_i beta_ai q^a_i nu_i^x  (column a of V)
 *   mu' = mu + E[f],  Sigma' = Sigma + Cov(f) + V + V^T + diag(Q)  (stored exactly symmetric)
 * The D x D systems are solved by Gaussian elimination with partial pivoting (Sigma = 0 is allowed); |R| <= 0 or a non-finite state
 * gives NaN for that group from that step on, nothing faults.
 * x_lasts G x D (start means); S0s NULL (zeros) or G x D x D (start covariances, symmetric); ctrl steps x C (NULL when C = 0);
 * log_Qs G x D.  Outputs m_x G x steps x D, S_x G x steps x D x D (the state AFTER step t at index t); either may be NULL when a
 * summary is requested.  The trailing block is that of ffvd_op_rollout_grouped_summary; it is requested by giving any of its
 * arguments.  Per output j over the G groups (equal weights, ascending order), m_gj = CC_j^T mu_g + DD_j, s2_gj = CC_j^T Sigma_g CC_j
 * + s_j^2:  y_mean = mean_g m,  y_var_total = mean_g (s2 + m^2) - y_mean^2,  y_var = y_var_total (this method has no other variance),
 * lpd = log (1/G) sum_g N(y; m_g, s2_g) (largest exponent subtracted),  lpd_gauss = log N(y; y_mean, y_var_total).
 * Determinism: the decomposition of a group depends on (M, D) only, sums have fixed orders, no atomics: two calls are bit-identical
 * and a group's m_x / S_x do not depend on G or the other groups.
 * Limits: SE kernel, D <= 8, P = D + C <= 32, M <= 2048, J <= 8, n_models 1 or G, q_mode 0 or 1, G * D <= 2^24, G * D * Mp^2 <= 2^29
 * doubles (Mp: M rounded up to 64), G * steps * D * D < 2^31; FFVD_EINVAL beyond them, before any device call.  G = 0 or steps = 0:
 * FFVD_OK, nothing is touched. */
int  ffvd_op_moment_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                            const double *logvariances, const double *loglengthscales, const double *fs,
                            const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                            int C, int steps, const double *log_Qs, double *m_x, double *S_x, const double *CC, const double *DD,
                            const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean, double *y_var,
                            double *y_var_total, double *lpd, double *lpd_gauss);

/* ffvd_op_posterior_grouped followed by ffvd_op_moment_grouped WITHOUT the posteriors leaving the device (as
 * ffvd_op_posterior_rollout_grouped does for the rollouts): W is packed from the K_uu slabs, f = U_mean is read where the matvec left
 * it, the q slices are packed with exact zeros in the padding and the strict lower triangle, the start means are Xs[g][T].  ctrl_fit
 * T x C feeds the posterior, ctrl_roll steps x C the propagation.  U_means G x M x D optional.
 * Limits: those of ffvd_op_posterior_grouped and of ffvd_op_moment_grouped.  G = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_posterior_moment_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                      const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                      const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *S0s,
                                      const double *ctrl_roll, int steps, double *m_x, double *S_x, double *U_means, const double *CC,
                                      const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                                      double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss);

/* Gaussian filtering and RTS smoothing of an observed sequence through the GP by moment matching (assumed-density filtering;
 * Deisenroth et al. 2012): ffvd_op_moment_grouped -- same arguments up to log_Qs, same posterior, same step -- with a measurement
 * update after every step.  The state after step i emits row i of Y_obs (steps x J): y = CC^T x + DD + N(0, diag(noise_std^2));
 * a NaN entry of Y_obs is unobserved (an all-NaN row is a pure prediction step: trailing all-NaN rows forecast); an infinity is
 * rejected.  Per group, from N(x_lasts[g], S0s[g]), for i = 0 .. steps - 1:
 *   predict:  m^-_i = mu + E[f],  S^-_i = Sigma + Cov(f) + V + V^T + diag(Q)  (the step of ffvd_op_moment_grouped from the filtered
 *             state of index i - 1),  X_i = Sigma + V = Cov(x_{i-1}, x_i | y_{0:i-1})  (row: component of x_{i-1});
 *   density:  lpd[g][i][j] = log N(y_ij; CC_j^T m^-_i + DD_j, CC_j^T S^-_i CC_j + s_j^2)  (marginal, before any update),
 *             lpd_joint[g][i] = joint log density of the observed entries of row i;  NaN where the entry / the whole row is unobserved;
 *   update:   exact, as scalar updates in ascending j over the observed entries: with h = CC_j, s = h^T Sigma h + s_j^2,
 *             e = y_ij - h^T mu - DD_j:  mu += Sigma h e / s,  Sigma -= (Sigma h)(Sigma h)^T / s  (no J x J factorisation; the terms
 *             -(log 2 pi + log s) / 2 - e^2 / (2 s) add up to lpd_joint).  A row without an observed entry leaves m_filt = m_pred and
 *             S_filt = S_pred bit for bit.
 * Smoothing (only when m_smooth or S_smooth is given; the start state is not smoothed): the last row is the filtered one bit for bit,
 * then for i = steps - 2 .. 0:  J_i = X_{i+1} (S^-_{i+1})^-1 (Gaussian elimination with partial pivoting),
 *   m^s_i = m_i + J_i (m^s_{i+1} - m^-_{i+1}),  S^s_i = S_i + J_i (S^s_{i+1} - S^-_{i+1}) J_i^T.
 * Outputs, each may be NULL: m_pred, m_filt, m_smooth G x steps x D;  S_pred, S_filt, cross, S_smooth G x steps x D x D (every
 * covariance exactly symmetric);  lpd G x steps x J;  lpd_joint G x steps;  and the pooled ONE-STEP summary y_mean, y_var_total, lpd_mix,
 * lpd_gauss, each steps x J: the summary of ffvd_op_moment_grouped applied to the predicted stacks with Y_obs (NaN densities where
 * an entry is unobserved).  It pools the groups with EQUAL weights, as everywhere in this library: the chains are NOT re-weighted by
 * their likelihoods.  Determinism as ffvd_op_moment_grouped: two calls are bit-identical, a group does not depend on the others.
 * Limits: those of ffvd_op_moment_grouped, 1 <= J <= 8, steps >= 0, at least one output; FFVD_EINVAL beyond them, before any device
 * call.  G = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_filter_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                            const double *logvariances, const double *loglengthscales, const double *fs,
                            const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                            int C, int steps, const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                            const double *Y_obs, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                            double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total,
                            double *lpd_mix, double *lpd_gauss);

/* ffvd_op_posterior_grouped followed by ffvd_op_filter_grouped WITHOUT the posteriors leaving the device (as
 * ffvd_op_posterior_moment_grouped).  x0s G x D: the start means, NULL: Xs[g][T] (the record continues the training sequence).
 * Limits: those of ffvd_op_posterior_grouped and of ffvd_op_filter_grouped. */
int  ffvd_op_posterior_filter_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                      const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                      const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s,
                                      const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                      const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                      double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                      double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                      double *U_means);

/* Linearised (extended Kalman) filtering and RTS smoothing through the GP: ffvd_op_filter_grouped -- same arguments, same outputs,
 * same timing convention, same measurement update, densities, smoother and pooled summary -- with the transition linearised at the
 * filtered mean instead of moment-matched (GP-EKF; Deisenroth et al. 2012 compare the two).  With (mu, S) the filtered state before
 * step t, x = [mu, c_t], beta_d = W_d u_d and Gamma_d = W_d (I - q q^T) W_d^T of the group, per latent dim d:
 *   k_j = variance_d exp(-1/2 sum_p (x_p - z_jp)^2 / l_dp^2),   nu_jp = z_jp - x_p,
 *   m_d = sum_j k_j beta_dj,
 *   J_dp = (1 / l_dp^2) sum_j k_j beta_dj nu_jp   for the D state columns p < D only,
 *   v_d = variance_d - sum_i k_i (sum_j Gamma_d,ij k_j),
 * and with A = I + J:
 *   predict:  m^-_t = mu + m,  S^-_t = A S A^T + diag(v + Q)  (one expression for (lo, hi), mirrored: exactly symmetric),
 *             cross_t = S A^T = Cov(x_{t-1}, x_t | y_{0:t-1})  (row: component of x_{t-1}).
 * From S = 0 the first predicted state is the GP conditional at [x_lasts, c_0]: m^- - x_lasts its mean, diag(S^-) - Q its variance,
 * off-diagonal entries exact zeros.  Cheaper than moment matching (one exp per inducing point and one quadratic form per (group,
 * dim) against a D (D + 1) / 2-pair table), and first-order where that is exact for the Gaussian: the mean ignores the curvature
 * of f under S.  Determinism and limits as ffvd_op_filter_grouped; SE kernel only (FFVD_EINVAL with a message that says so). */
int  ffvd_op_filter_linear_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                   int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                   const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                   const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                   const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred, double *m_filt,
                                   double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth,
                                   double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss);

/* ffvd_op_posterior_grouped followed by ffvd_op_filter_linear_grouped WITHOUT the posteriors leaving the device: the arguments of
 * ffvd_op_posterior_filter_grouped, the rule of ffvd_op_filter_linear_grouped. */
int  ffvd_op_posterior_filter_linear_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                             const double *logvariances, const double *loglengthscales, const double *Xs,
                                             const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                             int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                             const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                             const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                             double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                             double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                             double *lpd_gauss, double *U_means);

/* Linearised filtering (and RTS smoothing) of R observed records in one call: ffvd_op_filter_linear_grouped -- its rule, measurement
 * update, densities and smoother -- with a TRACK (group g, record r) as the unit.  Every track is an independent filter: it runs on
 * the posterior of group g, reads the observations Y_obs[r] (steps x J, NaN = unobserved; a shorter record is padded with all-NaN
 * rows, which are prediction steps), the control rows ctrl[r] (steps x C) and starts from N(x_lasts[g][r], S0s[g][r]).  The
 * argument list of ffvd_op_filter_linear_grouped with: R records; x_lasts G x R x D; S0s G x R x D x D or NULL (zeros); ctrl
 * R x steps x C; Y_obs R x steps x J; records_per_pass (0: automatic; otherwise at most that many records advance together).
 * beta and Gamma are prepared once per call; the tracks of a pass advance in one launch pair per step, and the quadratic forms of
 * all tracks that share a Gamma are one dense product on the fp64 matrix cores (the product of ffvd_op_forecast_linear_grouped), so
 * Gamma is read once per 128 tracks.  A track does not depend on the other groups, the other records, their order or
 * records_per_pass (bit for bit); against ffvd_op_filter_linear_grouped on the same record it agrees to rounding, not bit for bit
 * (the quadratic form and the mean sums are added in another order).
 * Outputs, each may be NULL (at least one is needed): m_pred .. S_smooth as ffvd_op_filter_linear_grouped with G x R x steps in
 * place of G x steps; the pooled one-step summary over the groups (equal weights) per record and row, each R x steps x J: y_mean,
 * y_var_total, lpd_mix, lpd_gauss.
 * Limits: those of ffvd_op_filter_linear_grouped, R >= 0, records_per_pass >= 0, G * R * steps * D * D < 2^31, G * R * D < 2^31;
 * FFVD_EINVAL beyond them, before any device call; SE kernel only (FFVD_EINVAL with a message that says so).  G = 0, R = 0 or
 * steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_filter_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                    int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                    const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                    const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                    const double *noise_std, int J, const double *Y_obs, int records_per_pass, double *m_pred,
                                    double *S_pred, double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                    double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                    double *lpd_gauss);

/* ffvd_op_posterior_grouped followed by ffvd_op_filter_records_grouped WITHOUT the posteriors leaving the device: the arguments of
 * ffvd_op_posterior_filter_linear_grouped with R, x0s G x R x D (NULL: every record of group g starts at Xs[g][T]), S0s
 * G x R x D x D or NULL, ctrl_roll R x steps x C, Y_obs R x steps x J and records_per_pass; the outputs of
 * ffvd_op_filter_records_grouped and U_means. */
int  ffvd_op_posterior_filter_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                              const double *logvariances, const double *loglengthscales, const double *Xs,
                                              const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                              int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                              const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                              const double *noise_std, int J, const double *Y_obs, int records_per_pass, double *m_pred,
                                              double *S_pred, double *m_filt, double *S_filt, double *cross, double *lpd,
                                              double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean,
                                              double *y_var_total, double *lpd_mix, double *lpd_gauss, double *U_means);

/* Cubature (sigma-point) filtering of R observed records in one call: ffvd_op_filter_records_grouped -- its tracks, timing, emission,
 * measurement update, densities, smoother, pooled summary, passes and argument list -- with the third-degree spherical cubature rule
 * (Arasaratnam & Haykin 2009) as the propagation in place of the extended Kalman rule.  Per step, with (mu, S) the filtered state,
 * c the record's control row and w = 1 / (2D): L the lower Cholesky factor of S without pivoting (a pivot <= 0 gives a zero column:
 * S = 0 and a rank-deficient S are allowed); offsets dx_i = +sqrt(D) (column i of L), dx_{i+D} = -dx_i; points x_i = [mu + dx_i, c]
 * (the control columns are not spread); m(x_i), v(x_i) the mean and variance of the GP conditional there;
 *   mbar = w sum_i m(x_i),  Cov(f) = w sum_i (m(x_i) - mbar)(m(x_i) - mbar)^T + diag(w sum_i v(x_i)),  V = w sum_i dx_i (m(x_i) - mbar)^T,
 *   m_pred = mu + mbar,  S_pred = S + Cov(f) + V + V^T + diag(Q),  cross = S + V.
 * Its difference from moment matching is second order in S where the extended Kalman rule's is first order.  The 2D kernel rows of
 * every (track, dim) are rows of the same dense product on the fp64 matrix cores, so Gamma is still read once per 128 rows.  Every
 * covariance is exactly symmetric; from S = 0 the step is the conditional at [mu, c] and cross is exact zeros; a track does not depend
 * on the other groups, the other records, their order or records_per_pass (bit for bit).
 * Arguments, outputs and limits: those of ffvd_op_filter_records_grouped (x_lasts G x R x D, G * R * steps * D * D < 2^31); SE kernel
 * only (FFVD_EINVAL with a message that says so).  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_filter_cubature_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                             int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                             const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                             const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                             const double *DD, const double *noise_std, int J, const double *Y_obs,
                                             int records_per_pass, double *m_pred, double *S_pred, double *m_filt, double *S_filt,
                                             double *cross, double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth,
                                             double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss);

/* ffvd_op_posterior_grouped followed by ffvd_op_filter_cubature_records_grouped WITHOUT the posteriors leaving the device: the
 * arguments and outputs of ffvd_op_posterior_filter_records_grouped. */
int  ffvd_op_posterior_filter_cubature_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                       const double *logvariances, const double *loglengthscales, const double *Xs,
                                                       const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                       int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                       const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                       const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                       double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                                                       double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth,
                                                       double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                                       double *U_means);

/* Bootstrap particle filtering of R observed records in one call: the tracks, passes, timing (the state after step i emits row i of
 * Y_obs), emission, NaN = unobserved convention, staging and q_mode of ffvd_op_filter_records_grouped with N particles per track in
 * place of one Gaussian.  Every random draw is the caller's (ffvd_particle_seeded_records_grouped generates them on the device from
 * a seed instead): eps (standard normal, steps x N x D per track), unif (in [0, 1), steps per track) and xi0 (standard normal, N x D per track; needed exactly when S0s is given) are read through a group
 * and a record stride in doubles, each 0 (shared: common random numbers) or the stride of a contiguous [G or 1][R or 1][...] array.
 * Per track:
 *   start      X_0i = x_last + L0 xi0_i, L0 the lower Cholesky factor of S0 without pivoting (a pivot <= 0 gives a zero column);
 *              S0s NULL: every particle starts at x_last
 *   propagate  with (m_i, v_i) the mean and variance of the GP conditional of the group at [X_ti, c_t]:
 *              X^-_i = X_ti + m_i + eps[t, i] sqrt(v_i + Q) per dim
 *   moments    m_pred[t] = sum_i X^-_i / N,  S_pred[t] = sum_i (X^-_i - m_pred)(X^-_i - m_pred)^T / N (centred, exactly symmetric)
 *   densities  l_ij = log N(y_tj; CC[:, j] . X^-_i + DD_j, noise_std_j^2);  lpd[t, j] = log(sum_i exp l_ij / N), NaN where y_tj is NaN;
 *              L_i = sum over the observed j of l_ij;  lpd_joint[t] = log(sum_i exp L_i / N), NaN for a row with nothing observed
 *   filtered   W_i = exp(L_i - max L);  m_filt[t], S_filt[t]: the W-weighted mean and centred covariance;  ess[t] = (sum W)^2 / sum W^2;
 *              a row with nothing observed: W = 1, m_filt = m_pred and S_filt = S_pred bit for bit, ess = N
 *   resample   systematic, one uniform per track and step, only for a row with an observed entry: cdf_k = W_0 + .. + W_k,
 *              a_i = min(#{k: cdf_k <= (unif[t] + i) / N cdf_{N-1}}, N - 1), X_{t+1,i} = X^-_{a_i}; otherwise a_i = i.  The index is
 *              clamped into [0, N) before it addresses anything, whatever the weights are.  No adaptive resampling.
 *              (ffvd_particle_adaptive_records_grouped resamples only below an ESS threshold.)
 * log_evidence (G x R) is the sum of lpd_joint over the rows that have an observation: the SMC estimate of log p(y) of that record
 * under that group.  Pooled over the groups with equal weights (R x steps x J): y_mean, y_var_total and lpd_gauss as
 * ffvd_op_filter_records_grouped on (m_pred, S_pred); lpd_mix = log mean_g exp(lpd[g]), the density of the mixture of all G * N
 * particles' emissions.  There is no smoother and no cross-covariance in this call (the particle smoother is
 * ffvd_particle_smooth_records_grouped).
 * Outputs, each of which may be NULL: m_pred, m_filt (G x R x steps x D), S_pred, S_filt (.. x D x D), lpd (.. x J), lpd_joint, ess
 * (G x R x steps), the pooled four, log_evidence, particles (G x R x steps x N x D: the X^-) and ancestors (G x R x steps x N).
 * The kernel rows of all particles of all tracks that share a Gamma are one dense product on the fp64 matrix cores (the product of
 * ffvd_op_forecast_linear_grouped, N rows of K per track and dim).  A track does not depend on the other groups, the other records,
 * their order or records_per_pass (bit for bit).
 * Limits: those of ffvd_op_filter_records_grouped; 2 <= N <= 2048; G * R * steps * N * D < 2^31; the N kernel rows of one record per
 * group must fit the scratch of a pass (FFVD_EINVAL with a message that names the largest N that fits); SE kernel only.
 * G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_filter_particle_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                             int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                             const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                             const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                             const double *DD, const double *noise_std, int J, const double *Y_obs,
                                             int records_per_pass, int N, const double *eps, long long eps_stride_g,
                                             long long eps_stride_r, const double *unif, long long unif_stride_g,
                                             long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                             double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                             double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                             double *ess, double *log_evidence, double *particles, int *ancestors);

/* ffvd_op_posterior_grouped followed by ffvd_op_filter_particle_records_grouped WITHOUT the posteriors leaving the device: the model
 * and start arguments of ffvd_op_posterior_filter_records_grouped (x0s NULL: every record of group g starts at the last row of
 * Xs[g]), the particle arguments and outputs of the call above. */
int  ffvd_op_posterior_filter_particle_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                       const double *logvariances, const double *loglengthscales, const double *Xs,
                                                       const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                       int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                       const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                       const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                       int N, const double *eps, long long eps_stride_g, long long eps_stride_r,
                                                       const double *unif, long long unif_stride_g, long long unif_stride_r,
                                                       const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                                       double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                                       double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                                       double *lpd_gauss, double *ess, double *log_evidence, double *particles,
                                                       int *ancestors, double *U_means);

/* Fully adapted particle filtering of R observed records in one call: ffvd_op_filter_particle_records_grouped with the optimal
 * proposal in place of the bootstrap one (the fully adapted auxiliary particle filter of Pitt & Shephard 1999).  Given the parent
 * the transition is Gaussian with a diagonal covariance and the emission is linear-Gaussian, so p(y_t | parent) and
 * p(x_t | parent, y_t) are closed forms: the parents are weighted by how well they predict y_t before anything is drawn, resampled,
 * and the children are drawn from the optimal proposal; the new set is equally weighted.  The argument list, the tracks, passes,
 * timing, NaN convention, staging, q_mode, the caller's draws with their strides and the limits are those of
 * ffvd_op_filter_particle_records_grouped.  Per track, with X_t the equally weighted set carried into row t (X_0: that call's
 * start, bit for bit) and (mean_i, v_i) the GP conditional of the group at [X_ti, c_t]:
 *   parents    mu_i = X_ti + mean_i,  s_i = v_i + Q  (per dim: trans_mean and trans_var of ffvd_particle_smooth_records_grouped)
 *   moments    m_pred[t] = sum_i mu_i / N,  S_pred[t] = sum_i (mu_i - m_pred)(mu_i - m_pred)^T / N + diag(sum_i s_i / N): the moments
 *              of the mixture (1/N) sum_i N(mu_i, diag s_i); no draw enters (exactly symmetric)
 *   densities  lpd[t, j] = log mean_i N(y_tj; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + noise_std_j^2), NaN where y_tj is NaN
 *   update     per particle from (m, P) = (mu_i, diag s_i) and L_i = 0, exact scalar updates over the observed j in ascending order:
 *              h = P c_j, sig2 = c_j . h + noise_std_j^2, r = y_tj - (c_j . m + DD_j), L_i += -1/2 (log 2 pi + log sig2 + r^2 / sig2),
 *              m += h (r / sig2), P_ab -= h_a h_b / sig2  ->  mt_i, P_i;  lpd_joint[t] = log mean_i exp L_i, NaN for a row with nothing
 *              observed
 *   filtered   W_i = exp(L_i - max L);  ess[t] = (sum W)^2 / sum W^2;  m_filt[t] = sum W mt / sum W,
 *              S_filt[t] = sum W (P_i + (mt_i - m_filt)(mt_i - m_filt)^T) / sum W (exactly symmetric)
 *   resample   the PARENTS, by ffvd_op_filter_particle_records_grouped's systematic rule with unif[t] (index clamped into [0, N)): a_i
 *   draw       X_{t+1,i} = mt_{a_i} + L_{a_i} eps[t, i], L the lower Cholesky factor of P without pivoting (a pivot <= 0 gives a zero
 *              column)
 *   a row with nothing observed: X_{t+1,i} = X_ti + mean_i + eps[t, i] sqrt(v_i + Q) (that call's expression), a_i = i, W = 1,
 *              ess = N, m_filt = m_pred and S_filt = S_pred bit for bit; a record that is all NaN returns that call's particles bit
 *              for bit
 * The outputs have that call's names and shapes with two differences: particles[t] is X_{t+1}, the equally weighted FILTERED set
 * after row t (not X^-), and ancestors[t, i] indexes the set carried INTO row t.  log_evidence stays the unbiased SMC estimate; the
 * pooled arrays are formed as in that call (y_mean, y_var_total, lpd_gauss from (m_pred, S_pred); lpd_mix from lpd).  Three launches
 * per step as that call: only the per-track weight kernel differs.  Smoothing and backward simulation on the adapted sets are
 * ffvd_particle_adapted_smooth_records_grouped and ffvd_particle_adapted_backsim_records_grouped; there is no forecast on them.
 * Limits: those of ffvd_op_filter_particle_records_grouped.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is
 * touched. */
int  ffvd_particle_adapted_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                           int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                           const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                           const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                           const double *DD, const double *noise_std, int J, const double *Y_obs,
                                           int records_per_pass, int N, const double *eps, long long eps_stride_g,
                                           long long eps_stride_r, const double *unif, long long unif_stride_g,
                                           long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                           double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                           double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                           double *ess, double *log_evidence, double *particles, int *ancestors);

/* ffvd_op_posterior_grouped followed by ffvd_particle_adapted_records_grouped WITHOUT the posteriors leaving the device: the
 * argument list of ffvd_op_posterior_filter_particle_records_grouped, the method and outputs of the call above. */
int  ffvd_posterior_particle_adapted_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                     const double *logvariances, const double *loglengthscales, const double *Xs,
                                                     const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                     int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                     const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                     const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                     int N, const double *eps, long long eps_stride_g, long long eps_stride_r,
                                                     const double *unif, long long unif_stride_g, long long unif_stride_r,
                                                     const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                                     double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                                     double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                                     double *lpd_gauss, double *ess, double *log_evidence, double *particles,
                                                     int *ancestors, double *U_means);

/* ffvd_op_filter_particle_records_grouped followed by the marginal particle smoother (forward filter / backward smoother of Doucet,
 * Godsill & Andrieu 2000) of every (group, record) track, on the equally weighted sets the filter carries.  The arguments and the
 * filter outputs are those of ffvd_op_filter_particle_records_grouped, bit for bit; no GP is evaluated beyond the filter's and no
 * draw is added: the result is a deterministic function of the filter's run.  lengths (R ints, each in [1, steps]; NULL: every record
 * has `steps` rows) gives the rows n of every record: the recursion of a track starts at its row n - 1, and the new outputs are NaN at
 * and beyond it.  Per track, with X_t the set carried into row t (X_0 the start set), c_t the control row and (m, v) the GP conditional:
 *   kept       trans_mean[t] = X_t + m(X_t, c_t),  trans_var[t] = v(X_t, c_t) + Q: the two terms of the filter's
 *              X^-_t = trans_mean[t] + eps[t] sqrt(trans_var[t]), bit for bit (computed through every row of the call)
 *   weights    weights[t] = W_t of the filter: exp(L_i - max L), L_i the sum of l_ij over the observed j in ascending j; 1 for a row
 *              with nothing observed
 *   last row   w_smooth[n-1] = W_{n-1} / sum W_{n-1}
 *   backward   for t = n-2 .. 0, with x_j = X^-_{t+1,j}, mu_i = trans_mean[t+1, i], s_i = trans_var[t+1, i]:
 *              log f_ij = -1/2 sum_d ((x_jd - mu_id)^2 / s_id + log s_id)
 *              c_j = max_i log f_ij + log sum_i exp(log f_ij - max)                       (i ascending)
 *              omega_i = sum_j w_smooth[t+1, j] exp(log f_ij - c_j)                       (j ascending, every exponent <= 0)
 *              w_smooth[t, k] = sum of omega_i over the i with ancestors[t, i] = k        (i ascending; no offspring: exactly 0)
 *              nothing is renormalised inside the recursion
 *   moments    m_smooth[t] = sum_k w_k X^-_tk / sum_k w_k;  S_smooth[t]: the w-weighted centred covariance, exactly symmetric;
 *              ess_smooth[t] = (sum w)^2 / sum w^2
 * New outputs, each of which may be NULL: m_smooth (G x R x steps x D), S_smooth (.. x D x D), ess_smooth (G x R x steps), w_smooth and
 * weights (G x R x steps x N), trans_mean and trans_var (G x R x steps x N x D).  A record of one row returns its filtered row.  Every
 * sum has an order fixed by N alone: a track does not depend on the other groups, the other records, their order or records_per_pass
 * (bit for bit).  The device holds (3 D + 3) N doubles and N ints per track row beside the filter's buffers (FFVD_ENOMEM if they cannot
 * be had).  Limits: those of ffvd_op_filter_particle_records_grouped.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_particle_smooth_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                          int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                          const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                          const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                          const double *DD, const double *noise_std, int J, const double *Y_obs,
                                          int records_per_pass, int N, const double *eps, long long eps_stride_g,
                                          long long eps_stride_r, const double *unif, long long unif_stride_g,
                                          long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                          double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                          double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                          double *ess, double *log_evidence, double *particles, int *ancestors, const int *lengths,
                                          double *m_smooth, double *S_smooth, double *ess_smooth, double *w_smooth, double *weights,
                                          double *trans_mean, double *trans_var);

/* ffvd_op_posterior_grouped followed by ffvd_particle_smooth_records_grouped WITHOUT the posteriors leaving the device: the
 * arguments of ffvd_op_posterior_filter_particle_records_grouped, then lengths and the new outputs of the call above; U_means stays
 * last. */
int  ffvd_posterior_particle_smooth_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                    const double *logvariances, const double *loglengthscales, const double *Xs,
                                                    const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                    int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                    const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                    const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                    int N, const double *eps, long long eps_stride_g, long long eps_stride_r,
                                                    const double *unif, long long unif_stride_g, long long unif_stride_r,
                                                    const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                                    double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                                    double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                                    double *lpd_gauss, double *ess, double *log_evidence, double *particles,
                                                    int *ancestors, const int *lengths, double *m_smooth, double *S_smooth,
                                                    double *ess_smooth, double *w_smooth, double *weights, double *trans_mean,
                                                    double *trans_var, double *U_means);

/* ffvd_op_filter_particle_records_grouped followed by the backward simulation of B joint smoothed trajectories per (group, record)
 * track (forward filtering / backward simulation, Godsill, Doucet & West 2004) on the equally weighted sets the filter carries.  The
 * arguments up to and including `lengths` and the filter outputs are those of ffvd_particle_smooth_records_grouped, bit for bit; no
 * GP is evaluated beyond the filter's.  The uniforms are the caller's: unif_bs, a block of steps x B per track, each in [0, 1),
 * indexed through a group and a record stride in doubles (0 = shared, otherwise the stride of a contiguous array).  Per track of n
 * rows and trajectory b, with u = unif_bs[t, b] and the notation of the smoothing call:
 *   row n-1    cdf = the running sum of W_{n-1} in index order, tot = cdf[N-1];  k_{n-1} = min(#{k: cdf_k <= u tot}, N - 1)
 *   backward   for t = n-2 .. 0, with x = X^-_{t+1, k_{t+1}}, mu_i = trans_mean[t+1, i], s_i = trans_var[t+1, i]:
 *              log f_i = -1/2 sum_d ((x_d - mu_id)^2 / s_id + log s_id),  p_i = exp(log f_i - max_i log f_i)    (tot >= 1 always)
 *              cdf = the running sum of p in index order;  i* = min(#{i: cdf_i <= u tot}, N - 1);  k_t = ancestors[t, i*]
 *              every index is clamped into [0, N) before it addresses anything
 *   outputs    traj_index[t, b] = k_t (-1 at and beyond n);  trajectories[b, t, :] = X^-_{t, k_t}, a gather, bit for bit;
 *              m_traj[t]: the mean over b;  S_traj[t]: the centred covariance with divisor B, exactly symmetric;
 *              lag_cov[t] = (1 / B) sum_b (x_t^b - m_traj[t]) (x_{t+1}^b - m_traj[t+1])^T, row index = component of x_t, not
 *              symmetric, NaN at t = n - 1
 * Conditional on the filter's run P(k_t = k) = w_smooth[t, k] of ffvd_particle_smooth_records_grouped.  Outputs, each of which may be
 * NULL: trajectories (G x R x B x steps x D), traj_index (G x R x steps x B), m_traj (G x R x steps x D), S_traj and lag_cov
 * (.. x D x D), then weights, trans_mean and trans_var of the smoothing call (the stacks the recursion reads); all NaN at and beyond
 * a record's length; a record of one row draws from its filtered weights.  Trajectory b depends on column b of unif_bs alone, a
 * track does not depend on the other groups, the other records, their order or records_per_pass (bit for bit).  The device holds
 * (4 D + 3) N doubles and N ints per track row beside the filter's buffers, and B D doubles and B ints per track row for the
 * trajectories (FFVD_ENOMEM if they cannot be had).  Limits: those of ffvd_op_filter_particle_records_grouped; 1 <= B <= 4096;
 * G * R * B < 2^31.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_particle_backsim_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                           int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                           const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                           const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                           const double *DD, const double *noise_std, int J, const double *Y_obs,
                                           int records_per_pass, int N, const double *eps, long long eps_stride_g,
                                           long long eps_stride_r, const double *unif, long long unif_stride_g,
                                           long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                           double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                           double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                           double *ess, double *log_evidence, double *particles, int *ancestors, const int *lengths,
                                           int B, const double *unif_bs, long long unif_bs_stride_g, long long unif_bs_stride_r,
                                           double *trajectories, int *traj_index, double *m_traj, double *S_traj, double *lag_cov,
                                           double *weights, double *trans_mean, double *trans_var);

/* ffvd_op_posterior_grouped followed by ffvd_particle_backsim_records_grouped WITHOUT the posteriors leaving the device: the
 * arguments of ffvd_op_posterior_filter_particle_records_grouped, then lengths, B, unif_bs with its strides and the new outputs of
 * the call above; U_means stays last. */
int  ffvd_posterior_particle_backsim_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                     const double *logvariances, const double *loglengthscales, const double *Xs,
                                                     const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                     int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                     const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                     const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                     int N, const double *eps, long long eps_stride_g, long long eps_stride_r,
                                                     const double *unif, long long unif_stride_g, long long unif_stride_r,
                                                     const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                                     double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                                     double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                                     double *lpd_gauss, double *ess, double *log_evidence, double *particles,
                                                     int *ancestors, const int *lengths, int B, const double *unif_bs,
                                                     long long unif_bs_stride_g, long long unif_bs_stride_r, double *trajectories,
                                                     int *traj_index, double *m_traj, double *S_traj, double *lag_cov, double *weights,
                                                     double *trans_mean, double *trans_var, double *U_means);

/* ffvd_particle_adapted_records_grouped followed by the marginal particle smoother of every (group, record) track on the ADAPTED
 * sets.  The arguments are those of ffvd_particle_smooth_records_grouped without `weights` (the filtered sets are equally weighted);
 * the filter outputs are those of ffvd_particle_adapted_records_grouped, bit for bit (the same draws); no GP is evaluated beyond the
 * filter's and no draw is added.  Per track of n = lengths[r] rows, with P_t = particles[t] the equally weighted filtered set after
 * row t:
 *   kept       trans_mean[t], trans_var[t] = (mu, s) of that call for the set carried into row t: for t >= 1 the transition moments
 *              of P_{t-1}, particle by particle (row 0 belongs to the start set and is not read by the recursion)
 *   last row   w_smooth[n-1, i] = 1 / N
 *   backward   for t = n-2 .. 0, with x_j = P_{t+1,j}, mu_i = trans_mean[t+1, i], s_i = trans_var[t+1, i]:
 *              log f_ij, c_j as in ffvd_particle_smooth_records_grouped
 *              w_smooth[t, i] = sum_j w_smooth[t+1, j] exp(log f_ij - c_j)                (j ascending, every exponent <= 0)
 *              no fold through the ancestors, no emission weight, nothing is renormalised
 *   moments    m_smooth[t], S_smooth[t] (exactly symmetric), ess_smooth[t] from (w_smooth[t], P_t) as in that call
 * A record of one row returns the plain mean and covariance of P_0: the unweighted particle estimate, not the Rao-Blackwellised
 * m_filt / S_filt.  An all-NaN record returns ffvd_particle_smooth_records_grouped's new outputs bit for bit.  Outputs, each of which
 * may be NULL, NaN at and beyond a record's length: m_smooth, S_smooth, ess_smooth, w_smooth, trans_mean, trans_var with that call's
 * shapes.  A track does not depend on the other groups, the other records, their order or records_per_pass (bit for bit).  The
 * device holds (3 D + 2) N doubles and N ints per track row beside the filter's buffers (FFVD_ENOMEM if they cannot be had).
 * Limits: those of ffvd_op_filter_particle_records_grouped.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_particle_adapted_smooth_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs,
                                                  int M, int P, int D, const double *logvariances, const double *loglengthscales,
                                                  const double *fs, const double *const *q_sqrts, int q_mode, int R,
                                                  const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps,
                                                  const double *log_Qs, const double *CC, const double *DD, const double *noise_std,
                                                  int J, const double *Y_obs, int records_per_pass, int N, const double *eps,
                                                  long long eps_stride_g, long long eps_stride_r, const double *unif,
                                                  long long unif_stride_g, long long unif_stride_r, const double *xi0,
                                                  long long xi0_stride_g, long long xi0_stride_r, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                  double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                  double *log_evidence, double *particles, int *ancestors, const int *lengths,
                                                  double *m_smooth, double *S_smooth, double *ess_smooth, double *w_smooth,
                                                  double *trans_mean, double *trans_var);

/* ffvd_op_posterior_grouped followed by ffvd_particle_adapted_smooth_records_grouped WITHOUT the posteriors leaving the device: the
 * arguments of ffvd_posterior_particle_smooth_records_grouped without `weights`; U_means stays last. */
int  ffvd_posterior_particle_adapted_smooth_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                            const double *logvariances, const double *loglengthscales,
                                                            const double *Xs, const double *ctrl_fit, int C, int T,
                                                            const double *log_Qs, double jitter, int groups_per_pass, int q_mode,
                                                            int R, const double *x0s, const double *S0s, const double *ctrl_roll,
                                                            int steps, const double *CC, const double *DD, const double *noise_std,
                                                            int J, const double *Y_obs, int records_per_pass, int N, const double *eps,
                                                            long long eps_stride_g, long long eps_stride_r, const double *unif,
                                                            long long unif_stride_g, long long unif_stride_r, const double *xi0,
                                                            long long xi0_stride_g, long long xi0_stride_r, double *m_pred,
                                                            double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                                            double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                                            double *lpd_gauss, double *ess, double *log_evidence, double *particles,
                                                            int *ancestors, const int *lengths, double *m_smooth, double *S_smooth,
                                                            double *ess_smooth, double *w_smooth, double *trans_mean,
                                                            double *trans_var, double *U_means);

/* ffvd_particle_adapted_records_grouped followed by the backward simulation of B joint smoothed trajectories per (group, record)
 * track on the ADAPTED sets.  The arguments are those of ffvd_particle_backsim_records_grouped without `weights`; the filter outputs
 * are those of ffvd_particle_adapted_records_grouped, bit for bit.  Per track of n rows and trajectory b, with u = unif_bs[t, b] and
 * the notation of ffvd_particle_adapted_smooth_records_grouped:
 *   row n-1    k_{n-1} = min(#{k: k + 1 <= u N}, N - 1): the filter's scan and search on unit weights
 *   backward   for t = n-2 .. 0, with x = P_{t+1, k_{t+1}}:  p_i = exp(log f_i - max_i log f_i), cdf = the running sum of p in index
 *              order, k_t = min(#{i: cdf_i <= u tot}, N - 1): the searched index itself, no ancestor indirection; clamped into
 *              [0, N) before it addresses anything
 *   outputs    traj_index, trajectories[b, t, :] = P_{t, k_t} (a gather, bit for bit), m_traj, S_traj, lag_cov as in
 *              ffvd_particle_backsim_records_grouped; then trans_mean and trans_var
 * Conditional on the filter's run P(k_t = k) = w_smooth[t, k] of ffvd_particle_adapted_smooth_records_grouped.  An all-NaN record
 * returns ffvd_particle_backsim_records_grouped's traj_index and trajectories for the same unif_bs, bit for bit.  Limits: those of
 * ffvd_particle_backsim_records_grouped.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_particle_adapted_backsim_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs,
                                                   int M, int P, int D, const double *logvariances, const double *loglengthscales,
                                                   const double *fs, const double *const *q_sqrts, int q_mode, int R,
                                                   const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps,
                                                   const double *log_Qs, const double *CC, const double *DD, const double *noise_std,
                                                   int J, const double *Y_obs, int records_per_pass, int N, const double *eps,
                                                   long long eps_stride_g, long long eps_stride_r, const double *unif,
                                                   long long unif_stride_g, long long unif_stride_r, const double *xi0,
                                                   long long xi0_stride_g, long long xi0_stride_r, double *m_pred, double *S_pred,
                                                   double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                   double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                   double *log_evidence, double *particles, int *ancestors, const int *lengths, int B,
                                                   const double *unif_bs, long long unif_bs_stride_g, long long unif_bs_stride_r,
                                                   double *trajectories, int *traj_index, double *m_traj, double *S_traj,
                                                   double *lag_cov, double *trans_mean, double *trans_var);

/* ffvd_op_posterior_grouped followed by ffvd_particle_adapted_backsim_records_grouped WITHOUT the posteriors leaving the device: the
 * arguments of ffvd_posterior_particle_backsim_records_grouped without `weights`; U_means stays last. */
int  ffvd_posterior_particle_adapted_backsim_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                             const double *logvariances, const double *loglengthscales,
                                                             const double *Xs, const double *ctrl_fit, int C, int T,
                                                             const double *log_Qs, double jitter, int groups_per_pass, int q_mode,
                                                             int R, const double *x0s, const double *S0s, const double *ctrl_roll,
                                                             int steps, const double *CC, const double *DD, const double *noise_std,
                                                             int J, const double *Y_obs, int records_per_pass, int N,
                                                             const double *eps, long long eps_stride_g, long long eps_stride_r,
                                                             const double *unif, long long unif_stride_g, long long unif_stride_r,
                                                             const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                                             double *m_pred, double *S_pred, double *m_filt, double *S_filt,
                                                             double *lpd, double *lpd_joint, double *y_mean, double *y_var_total,
                                                             double *lpd_mix, double *lpd_gauss, double *ess, double *log_evidence,
                                                             double *particles, int *ancestors, const int *lengths, int B,
                                                             const double *unif_bs, long long unif_bs_stride_g,
                                                             long long unif_bs_stride_r, double *trajectories, int *traj_index,
                                                             double *m_traj, double *S_traj, double *lag_cov, double *trans_mean,
                                                             double *trans_var, double *U_means);

/* Seeded draws generated on the device (Philox4x32-10, Salmon et al. 2011): the draws of every particle call above as a pure function
 * of (seed, stream, group, record, element).  noise: 0 shared (one block for every track), 1 per record (one per record, shared by
 * the groups), 2 independent (one per (group, record)).  A block of a stream is laid out as the calls above read it -- eps
 * [steps][N][D], unif [steps], xi0 [N][D], unif_bs [steps][B] -- and is generated in pairs of consecutive elements: pair p of the
 * block of (g, r) is the Philox block of counter (p, g, r, stream) under the key (seed & 0xffffffff, seed >> 32), with g and r 0
 * where the mode shares the axis and stream 0 eps, 1 unif, 2 xi0, 3 unif_bs.  From its words w0..w3, k1 = (w0 >> 5) 2^26 + (w1 >> 6)
 * and k2 = (w2 >> 5) 2^26 + (w3 >> 6); the uniform streams hold k1 2^-53 and k2 2^-53 (exact, in [0, 1)); the normal streams hold
 * rho cos(2 pi u2) and rho sin(2 pi u2) with u1 = (k1 + 1) 2^-53, u2 = k2 2^-53, rho = sqrt(-2 ln u1) (finite, |z| < 8.58); the second
 * element of the last pair of an odd block is dropped.  So a block does not depend on G, R or steps (a shorter call's draws are a
 * prefix of a longer one's), nor on records_per_pass.
 *
 * ffvd_particle_draws returns the arrays a seeded call uses, generated on the device and downloaded; each output may be NULL.  Shapes:
 * lead x block with lead = (), (R) or (G x R) for noise 0, 1, 2.  B may be 0 when unif_bs is NULL.  Limits: those of
 * ffvd_op_filter_particle_records_grouped (2 <= N <= 2048, 1 <= D <= 8, G * R * steps * N * D < 2^31), 0 <= B <= 4096,
 * G * R * B < 2^31.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_particle_draws(unsigned long long seed, int noise, int G, int R, int steps, int N, int D, int B, double *eps, double *unif,
                         double *xi0, double *unif_bs);

/* The six particle calls of many records with seeded draws: rule 0 bootstrap / 1 fully adapted, stage 0 filter / 1 marginal smoother /
 * 2 backward simulation, then the arguments of ffvd_particle_backsim_records_grouped with `seed, noise` in place of the nine draw
 * arguments eps .. xi0_stride_r, without unif_bs and its strides, and with the smoother's m_smooth, S_smooth, ess_smooth, w_smooth
 * added at the end.  The draws never exist on the host: one launch per stream fills the device buffers the calls above upload into,
 * and nothing is scanned.  CONTRACT: every output is, bit for bit, that of the existing entry point of the (rule, stage) called with
 * the arrays of ffvd_particle_draws(seed, noise, ..) and the strides of the mode ((0, 0), (0, block) or (R block, block)).  Outputs
 * the (rule, stage) does not produce must be NULL -- at stage 0 lengths, trajectories .. w_smooth; at stage 1 trajectories .. lag_cov;
 * at stage 2 m_smooth .. w_smooth; under rule 1 weights -- else FFVD_EINVAL with a message that names them; B is read at stage 2
 * only.  A bad rule, stage or noise is FFVD_EINVAL.  Limits and the zero sizes: those of the entry point selected. */
int  ffvd_particle_seeded_records_grouped(int rule, int stage, int kind, int G, int n_models, const double *const *Lm_inverse_seqs,
                                          const double *Zs, int M, int P, int D, const double *logvariances,
                                          const double *loglengthscales, const double *fs, const double *const *q_sqrts, int q_mode,
                                          int R, const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps,
                                          const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                                          const double *Y_obs, int records_per_pass, int N, unsigned long long seed, int noise,
                                          double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                          double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                          double *ess, double *log_evidence, double *particles, int *ancestors, const int *lengths,
                                          int B, double *trajectories, int *traj_index, double *m_traj, double *S_traj,
                                          double *lag_cov, double *weights, double *trans_mean, double *trans_var, double *m_smooth,
                                          double *S_smooth, double *ess_smooth, double *w_smooth);

/* ffvd_op_posterior_grouped followed by ffvd_particle_seeded_records_grouped WITHOUT the posteriors leaving the device: rule, stage,
 * the arguments of ffvd_posterior_particle_backsim_records_grouped changed as above; U_means stays last. */
int  ffvd_posterior_particle_seeded_records_grouped(int rule, int stage, int kind, int G, int n_models, const double *Zs, int M, int P,
                                                    int D, const double *logvariances, const double *loglengthscales,
                                                    const double *Xs, const double *ctrl_fit, int C, int T, const double *log_Qs,
                                                    double jitter, int groups_per_pass, int q_mode, int R, const double *x0s,
                                                    const double *S0s, const double *ctrl_roll, int steps, const double *CC,
                                                    const double *DD, const double *noise_std, int J, const double *Y_obs,
                                                    int records_per_pass, int N, unsigned long long seed, int noise, double *m_pred,
                                                    double *S_pred, double *m_filt, double *S_filt, double *lpd, double *lpd_joint,
                                                    double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                                    double *ess, double *log_evidence, double *particles, int *ancestors,
                                                    const int *lengths, int B, double *trajectories, int *traj_index, double *m_traj,
                                                    double *S_traj, double *lag_cov, double *weights, double *trans_mean,
                                                    double *trans_var, double *m_smooth, double *S_smooth, double *ess_smooth,
                                                    double *w_smooth, double *U_means);

/* ffvd_op_filter_particle_records_grouped with ADAPTIVE (ESS-triggered) resampling: the track carries a WEIGHTED set and resamples only
 * on the rows whose effective sample size falls below ess_threshold * N.  The arguments are that call's with `ess_threshold` behind
 * xi0_stride_r and with `weights` and `resampled` behind `ancestors`; the draws, their layouts and their indexing are that call's
 * (unif[t] is not read on a row that does not resample).  Per track, with X the particles and a the log-weights carried into row t
 * (largest entry exactly 0; a = 0 at the start), e_i = exp(a_i) and A = sum_i e_i:
 *   propagate  X^-_i = X_i + m_i + eps[t, i] sqrt(v_i + Q)  (that call's expression)
 *   moments    m_pred[t] = sum_i e_i X^-_i / A,  S_pred[t] = sum_i e_i (X^-_i - m_pred)(X^-_i - m_pred)^T / A (exactly symmetric)
 *   densities  l_ij that call's emission log-density;  lpd[t, j] = max_i (a_i + l_ij) + log(sum_i exp(a_i + l_ij - max) / A), NaN where
 *              y_tj is NaN;  b_i = a_i + sum_{j observed} l_ij;  lpd_joint[t] = max b + log(sum_i exp(b_i - max b) / A)
 *   filtered   W_i = exp(b_i - max b);  m_filt[t], S_filt[t]: the W-weighted mean and centred covariance;  ess[t] = (sum W)^2 / sum W^2;
 *              weights[t, i] = W_i / sum W
 *   decide     ess[t] < ess_threshold N: that call's systematic resampling with unif[t] (ancestors[t], index clamped into [0, N)),
 *              then a = 0 and resampled[t] = 1;  otherwise ancestors[t, i] = i, the X^- are carried, a_i = b_i - max b, resampled[t] = 0
 *   a row with nothing observed: the propagation alone; m_filt = m_pred and S_filt = S_pred bit for bit, lpd and lpd_joint NaN,
 *              ess[t] = A^2 / sum_i e_i^2, weights[t, i] = e_i / A, ancestors[t, i] = i, a kept, resampled[t] = 0
 * particles[t] is X^- as in that call, so (particles[t], weights[t]) is the filtering approximation after every row.  log_evidence,
 * the sum of lpd_joint over the observed rows, is the unbiased SMC estimate whether or not a row resamples.  ess_threshold must be
 * finite and >= 0 (FFVD_EINVAL otherwise): 0 never resamples (sequential importance sampling), any value > 1 resamples every observed
 * row.  CONTRACT: with ess_threshold > 1 every output the two calls share is ffvd_op_filter_particle_records_grouped's, bit for bit.
 * New outputs, each may be NULL: weights G x R x steps x N, resampled G x R x steps (int).  Three launches per step as that call: only
 * the per-track weight kernel differs.  Smoothing, backward simulation and forecasts on the weighted sets are not built.
 * Limits: those of ffvd_op_filter_particle_records_grouped.  G = 0, R = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_particle_adaptive_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                            int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                            const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                            const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                            const double *DD, const double *noise_std, int J, const double *Y_obs,
                                            int records_per_pass, int N, const double *eps, long long eps_stride_g,
                                            long long eps_stride_r, const double *unif, long long unif_stride_g,
                                            long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                            double ess_threshold, double *m_pred, double *S_pred, double *m_filt, double *S_filt,
                                            double *lpd, double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                            double *lpd_gauss, double *ess, double *log_evidence, double *particles, int *ancestors,
                                            double *weights, int *resampled);

/* ffvd_op_posterior_grouped followed by ffvd_particle_adaptive_records_grouped WITHOUT the posteriors leaving the device: the
 * argument list of ffvd_op_posterior_filter_particle_records_grouped changed as above (U_means stays last), the method and outputs of
 * the call above. */
int  ffvd_posterior_particle_adaptive_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                      const double *logvariances, const double *loglengthscales, const double *Xs,
                                                      const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                      int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                      const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                      const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                      int N, const double *eps, long long eps_stride_g, long long eps_stride_r,
                                                      const double *unif, long long unif_stride_g, long long unif_stride_r,
                                                      const double *xi0, long long xi0_stride_g, long long xi0_stride_r,
                                                      double ess_threshold, double *m_pred, double *S_pred, double *m_filt,
                                                      double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                      double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                      double *log_evidence, double *particles, int *ancestors, double *weights,
                                                      int *resampled, double *U_means);

/* The two calls above with seeded draws generated on the device: `N, seed, noise` (noise 0 shared, 1 per record, 2 independent) in
 * place of N and the nine draw arguments eps .. xi0_stride_r, as ffvd_particle_seeded_records_grouped, whose fill launches these are.
 * CONTRACT: every output is, bit for bit, that of the call above on the arrays of ffvd_particle_draws(seed, noise, ..) and the strides
 * of the mode.  A bad noise is FFVD_EINVAL.  (ffvd_particle_seeded_records_grouped itself keeps its two rules.) */
int  ffvd_particle_adaptive_seeded_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs,
                                                   int M, int P, int D, const double *logvariances, const double *loglengthscales,
                                                   const double *fs, const double *const *q_sqrts, int q_mode, int R,
                                                   const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps,
                                                   const double *log_Qs, const double *CC, const double *DD, const double *noise_std,
                                                   int J, const double *Y_obs, int records_per_pass, int N, unsigned long long seed,
                                                   int noise, double ess_threshold, double *m_pred, double *S_pred, double *m_filt,
                                                   double *S_filt, double *lpd, double *lpd_joint, double *y_mean, double *y_var_total,
                                                   double *lpd_mix, double *lpd_gauss, double *ess, double *log_evidence,
                                                   double *particles, int *ancestors, double *weights, int *resampled);

int  ffvd_posterior_particle_adaptive_seeded_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                             const double *logvariances, const double *loglengthscales,
                                                             const double *Xs, const double *ctrl_fit, int C, int T,
                                                             const double *log_Qs, double jitter, int groups_per_pass, int q_mode,
                                                             int R, const double *x0s, const double *S0s, const double *ctrl_roll,
                                                             int steps, const double *CC, const double *DD, const double *noise_std,
                                                             int J, const double *Y_obs, int records_per_pass, int N,
                                                             unsigned long long seed, int noise, double ess_threshold, double *m_pred,
                                                             double *S_pred, double *m_filt, double *S_filt, double *lpd,
                                                             double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,
                                                             double *lpd_gauss, double *ess, double *log_evidence, double *particles,
                                                             int *ancestors, double *weights, int *resampled, double *U_means);

/* Rolling-origin multi-step forecasts in one call: ffvd_op_filter_grouped (same arguments, same outputs, each of which may be NULL),
 * then from every origin o = origins[b] (n_origins rows of the record, strictly ascending, 0 <= o <= steps - 1 - horizon) `horizon`
 * steps of ffvd_op_moment_grouped started at the FILTERED state of row o, N(m_filt[g][o], S_filt[g][o]), with the control rows
 * o + 1 .. o + horizon of `ctrl`: entry k - 1 of a track predicts row o + k of the record given rows 0 .. o.  All (group, origin)
 * tracks of a pass advance in one launch per forecast step; the filtered states are read where the filter left them.  A track is
 * bit-identical to ffvd_op_moment_grouped called with x_lasts = m_filt[:, o], S0s = S_filt[:, o] and those control rows, and does
 * not depend on the other tracks, on the other groups or on tracks_per_pass (0: automatic; otherwise at most that many origins per
 * pass of horizon + 1 launches).
 * Outputs, each may be NULL (at least one output of the call is needed): m_fc G x n_origins x horizon x D, S_fc G x n_origins x
 * horizon x D x D (exactly symmetric), and the pooled summary of ffvd_op_moment_grouped over the groups (equal weights), each
 * (n_origins * horizon) x J, row b * horizon + k - 1 against Y_obs[origins[b] + k]: fc_y_mean, fc_y_var_total, fc_lpd_mix,
 * fc_lpd_gauss (NaN densities where the target is unobserved; means and variances are finite there).
 * Limits: those of ffvd_op_filter_grouped, horizon >= 1, n_origins >= 1, tracks_per_pass >= 0, G * n_origins * horizon * D * D < 2^31;
 * FFVD_EINVAL beyond them, before any device call.  G = 0 or steps = 0: FFVD_OK, nothing is touched. */
int  ffvd_op_forecast_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                              const double *logvariances, const double *loglengthscales, const double *fs,
                              const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                              int C, int steps, const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                              const double *Y_obs, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                              double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total,
                              double *lpd_mix, double *lpd_gauss, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                              double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                              double *fc_lpd_gauss);

/* The same on the arguments of ffvd_op_posterior_filter_grouped: the collapsed posteriors never leave the device.
 * Limits: those of ffvd_op_posterior_filter_grouped and of ffvd_op_forecast_grouped. */
int  ffvd_op_posterior_forecast_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                        const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                        const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s,
                                        const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        double *U_means, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                                        double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                                        double *fc_lpd_gauss);

/* ffvd_op_forecast_grouped with the linearised (extended Kalman) rule of ffvd_op_filter_linear_grouped for the filter AND for the
 * tracks: the arguments, checks, outputs and FFVD_EINVAL cases of ffvd_op_forecast_grouped.  A track advances from the filtered state
 * (mu, S) of its origin without a measurement update: with m, J, v at [mu, c_row] as in ffvd_op_filter_linear_grouped and A = I + J,
 *   mu' = mu + m,   S' = A S A^T + diag(v + Q)   (one expression for (lo, hi), mirrored: exactly symmetric),
 * control row origin + 1 + t at step t.  The filter's outputs are those of ffvd_op_filter_linear_grouped bit for bit.  The quadratic
 * forms k^T Gamma k of all tracks that share a Gamma are one dense product K Gamma on the fp64 matrix cores (Gamma is read once per
 * 128 tracks); they are summed in 128-column tiles, so horizon 1 agrees with the filter's m_pred / S_pred of the next row to rounding,
 * not bit for bit.  A track does not depend on the other tracks, on the other groups or on tracks_per_pass.  SE kernel only
 * (FFVD_EINVAL with a message that says so). */
int  ffvd_op_forecast_linear_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                              const double *logvariances, const double *loglengthscales, const double *fs,
                              const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                              int C, int steps, const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                              const double *Y_obs, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                              double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total,
                              double *lpd_mix, double *lpd_gauss, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                              double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                              double *fc_lpd_gauss);

/* The same on the arguments of ffvd_op_posterior_forecast_grouped: the collapsed posteriors never leave the device. */
int  ffvd_op_posterior_forecast_linear_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                        const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                        const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s,
                                        const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        double *U_means, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                                        double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                                        double *fc_lpd_gauss);

/* ffvd_op_forecast_grouped with the third-degree spherical cubature rule of ffvd_op_filter_cubature_records_grouped for the filter AND
 * for the tracks: the arguments, checks, outputs and FFVD_EINVAL cases of ffvd_op_forecast_grouped.  The filter is that call with one
 * record (R = 1): its outputs are that call's bit for bit, record axis dropped.  A track advances from the filtered state (mu, S) of
 * its origin without a measurement update: with S = L L^T (no pivoting, a pivot <= 0 gives a zero column), the 2D points
 * x_i = [mu +- sqrt(D) L[:, i], c_row] and m, v the mean and variance of the GP conditional at a point, w = 1 / (2D),
 *   mbar = w sum_i m(x_i),   mu' = mu + mbar,
 *   S' = S + w sum_i (m(x_i) - mbar)(m(x_i) - mbar)^T + diag(w sum_i v(x_i)) + V + V^T + diag(Q),   V = w sum_{i<D} dx_i (m(x_i) - m(x_{i+D}))^T
 * (one expression for (lo, hi), mirrored: exactly symmetric), control row origin + 1 + t at step t.  The quadratic forms k^T Gamma k
 * of all points of all tracks that share a Gamma are one dense product K Gamma on the fp64 matrix cores (2D rows of K per track and
 * dim; the product of ffvd_op_forecast_linear_grouped).  Horizon 1 agrees with the filter's m_pred / S_pred of the next row to
 * rounding.  A track does not depend on the other tracks, on the other groups or on tracks_per_pass.  SE kernel only (FFVD_EINVAL
 * with a message that says so). */
int  ffvd_op_forecast_cubature_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                              const double *logvariances, const double *loglengthscales, const double *fs,
                              const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                              int C, int steps, const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                              const double *Y_obs, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                              double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total,
                              double *lpd_mix, double *lpd_gauss, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                              double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                              double *fc_lpd_gauss);

/* The same on the arguments of ffvd_op_posterior_forecast_grouped: the collapsed posteriors never leave the device. */
int  ffvd_op_posterior_forecast_cubature_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                        const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                        const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s,
                                        const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        double *U_means, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                                        double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                                        double *fc_lpd_gauss);

/* ffvd_op_forecast_grouped by particles: the bootstrap particle filter of ffvd_op_filter_particle_records_grouped over the one record
 * (R = 1: its outputs are that call's bit for bit, record axis dropped; cross, m_smooth and S_smooth must be NULL), then from every
 * origin o a track of N equally weighted particles started from the set the filter carries AFTER row o -- the X^- of row o gathered
 * through that row's ancestors, the identity for a row with nothing observed -- and advanced `horizon` steps without weighting or
 * resampling: with (m_i, v_i) the GP conditional of the group at [X_i, c_row], control row origin + 1 + t at step t,
 *   X_i <- X_i + m_i + eps_fc[t, i] sqrt(v_i + Q),
 *   m_fc = mean_i X_i,   S_fc = mean_i (X_i - m_fc)(X_i - m_fc)^T   (upper triangle, mirrored: exactly symmetric),
 *   fc_lpd[g, b, t, j] = log mean_i N(Y_obs[origin + 1 + t, j]; CC[:, j] . X_i + DD_j, noise_std_j^2)   (NaN where that entry is NaN).
 * A track is bit for bit what ffvd_op_filter_particle_records_grouped computes (m_pred, S_pred, particles) over the record cut after
 * its origin and continued by `horizon` all-NaN rows with the draws concatenated; it does not depend on the other tracks, on the
 * other groups or on tracks_per_pass.  The draws are the caller's: N particles, 2 <= N <= 2048; eps [G or 1][steps][N][D],
 * unif [G or 1][steps] in [0, 1), xi0 [G or 1][N][D] (given exactly when S0s is) with a group stride each, eps_fc
 * [G or 1][B or 1][horizon][N][D] with a group and an origin stride; strides in doubles, 0 (shared: common random numbers) or
 * that of the contiguous array; every draw finite.
 * Outputs beside those of ffvd_op_forecast_grouped, each of which may be NULL: ess G x steps and log_evidence G (the filter's),
 * fc_lpd G x B x horizon x J, fc_particles G x B x horizon x N x D.  fc_y_mean, fc_y_var_total and fc_lpd_gauss pool (m_fc, S_fc)
 * over the groups as the Gaussian rules do; fc_lpd_mix = log mean_g exp(fc_lpd[g]), the density of the mixture of all G N particles.
 * Limits: those of ffvd_op_filter_particle_records_grouped with R = 1 and of ffvd_op_forecast_grouped; G * B * horizon * N * D < 2^31;
 * the N kernel rows of one track per group must fit the scratch of a pass (FFVD_EINVAL names the largest N that does).  SE kernel only
 * (FFVD_EINVAL with a message that says so). */
int  ffvd_op_forecast_particle_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                              const double *logvariances, const double *loglengthscales, const double *fs,
                              const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                              int C, int steps, const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                              const double *Y_obs, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                              double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total,
                              double *lpd_mix, double *lpd_gauss, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                              int N, const double *eps, long long eps_stride_g, const double *unif, long long unif_stride_g,
                              const double *xi0, long long xi0_stride_g, const double *eps_fc, long long eps_fc_stride_g,
                              long long eps_fc_stride_b, double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total,
                              double *fc_lpd_mix, double *fc_lpd_gauss, double *ess, double *log_evidence, double *fc_lpd,
                              double *fc_particles);

/* The same on the arguments of ffvd_op_posterior_forecast_grouped: the collapsed posteriors never leave the device. */
int  ffvd_op_posterior_forecast_particle_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                        const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                        const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s,
                                        const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        double *U_means, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                                        int N, const double *eps, long long eps_stride_g, const double *unif, long long unif_stride_g,
                                        const double *xi0, long long xi0_stride_g, const double *eps_fc, long long eps_fc_stride_g,
                                        long long eps_fc_stride_b, double *m_fc, double *S_fc, double *fc_y_mean,
                                        double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss, double *ess,
                                        double *log_evidence, double *fc_lpd, double *fc_particles);

/* ffvd_op_forecast_particle_grouped on the sets of the fully adapted particle filter: the filter of
 * ffvd_particle_adapted_records_grouped over the one record (R = 1: its outputs are that call's bit for bit, record axis dropped),
 * then from every origin o a track of N particles started from a straight copy of the equally weighted FILTERED set that filter
 * stores after row o (no ancestor is read).  With (mean_i, v_i) the GP conditional of the group at [X_i, c_row], control row
 * origin + 1 + t at step t, mu_i = X_i + mean_i and s_i = v_i + Q:
 *   m_fc = mean_i mu_i,   S_fc = mean_i (mu_i - m_fc)(mu_i - m_fc)^T + diag(mean_i s_i)   (exactly symmetric; no draw enters),
 *   fc_lpd[g, b, t, j] = log mean_i N(Y_obs[origin + 1 + t, j]; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + noise_std_j^2)
 *                        (NaN where that entry is NaN),
 *   X_i <- mu_i + eps_fc[t, i] sqrt(s_i);   fc_particles[g, b, t] is this advanced set.
 * These are the adapted filter's m_pred / S_pred / lpd expressions, so the row t = 0 of a track equals that filter's prediction of
 * row origin + 1 bit for bit, and a track is bit for bit what ffvd_particle_adapted_records_grouped computes (m_pred, S_pred,
 * particles) over the record cut after its origin and continued by `horizon` all-NaN rows with the draws concatenated; it does not
 * depend on the other tracks, on the other groups or on tracks_per_pass.  The arguments, the draws, the outputs, the pooled arrays
 * and the limits are ffvd_op_forecast_particle_grouped's.  SE kernel only (FFVD_EINVAL with a message that says so). */
int  ffvd_particle_adapted_forecast_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                              const double *logvariances, const double *loglengthscales, const double *fs,
                              const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl,
                              int C, int steps, const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                              const double *Y_obs, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                              double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total,
                              double *lpd_mix, double *lpd_gauss, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                              int N, const double *eps, long long eps_stride_g, const double *unif, long long unif_stride_g,
                              const double *xi0, long long xi0_stride_g, const double *eps_fc, long long eps_fc_stride_g,
                              long long eps_fc_stride_b, double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total,
                              double *fc_lpd_mix, double *fc_lpd_gauss, double *ess, double *log_evidence, double *fc_lpd,
                              double *fc_particles);

/* The same on the arguments of ffvd_op_posterior_forecast_particle_grouped: the collapsed posteriors never leave the device. */
int  ffvd_posterior_particle_adapted_forecast_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                        const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                        const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s,
                                        const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        double *U_means, int horizon, const int *origins, int n_origins, int tracks_per_pass,
                                        int N, const double *eps, long long eps_stride_g, const double *unif, long long unif_stride_g,
                                        const double *xi0, long long xi0_stride_g, const double *eps_fc, long long eps_fc_stride_g,
                                        long long eps_fc_stride_b, double *m_fc, double *S_fc, double *fc_y_mean,
                                        double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss, double *ess,
                                        double *log_evidence, double *fc_lpd, double *fc_particles);

/* The summary of ffvd_op_moment_grouped for stacks the caller holds (m_x G x steps x D, S_x G x steps x D x D): the same launch.
 * Limits: D <= 8, J <= 8, 0 <= n_test <= steps, G * steps * D * D < 2^31, as ffvd_op_rollout_summary otherwise. */
int  ffvd_op_moment_summary(const double *m_x, const double *S_x, int G, int steps, int D, const double *CC, const double *DD,
                            const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean, double *y_var,
                            double *y_var_total, double *lpd, double *lpd_gauss);

/* One particle-Gibbs sweep over the latent trajectory: the INTENT of BaseModel.PG_for_X_speedup (base_model.py:78-138;
 * as written that op never updates X -- discarded TensorArray.write results (:115), an assign that is never run (:137) --
 * so there is no reference behaviour to match, see oracle/ffvd_pg_oracle.py).  n_free = PG_particles - 1 free particles
 * start at x0 (n_free x D, the N(0, I) draw of :79, injected) and advance side by side; per step tt < X_N - 1:
 * conditional_after_kernel_precalculation at [x_t, ctrl[tt]] with the explicit, whitened U (:93-97), x_{t+1} = x_t + f_mu +
 * eps[tt] * sqrt(f_var + Q) (:99-101), weights logdensity_norm(Y[tt], predict_mean(.), Rchols) of the new particles and of
 * the reference state X_ref[tt+1] (:105-109), n_free categorical draws (:113; inverse CDF of softmax(w) at the injected
 * uniforms unif[tt], first index whose cumulative probability exceeds u) and the gather (:111-115).
 * X_ref: X_N x D; Y: (X_N-1) x Ydim; ctrl: (X_N-1) x C or NULL; Rchols: Ydim x Ydim lower-triangular (= exp(log_Rchols),
 * likelihood.Rchols), Ydim <= 8; eps: (X_N-1) x n_free x D; unif: (X_N-1) x n_free in [0, 1).
 * Outputs: particles X_N x n_free x D (resampled_X of :133) and idx (X_N-1) x n_free (int32, value n_free = reference).
 * The final choice (:135-137) is the caller's: X <- particles[:, final_index] unless final_index == n_free.
 * M <= 2048, P = D + C <= 32, n_free + 1 <= 1024; Lm_inverse_seq upper triangular as for ffvd_op_rollout. */
int  ffvd_op_pg_sweep(int kind, const double *Lm_inverse_seq, const double *Z, int M, int P, int D,
                      const double *logvariance, const double *loglengthscales, const double *U, const double *X_ref,
                      int X_N, const double *Y, int Ydim, const double *ctrl, int C, const double *CC, const double *DD,
                      const double *Rchols, const double *log_Q, int n_free, const double *x0, const double *eps,
                      const double *unif, double *particles, int32_t *idx);

/* CRPS, PIT and predictive quantiles of equal-weight Gaussian mixtures, for stacks the caller holds.  A target is (row t, output j);
 * its predictive distribution is the mixture of K Gaussians N(mu_k, v_k), the components whose log density the summaries return as
 * lpd.  With A(d, v) = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v)) and Phi the standard normal distribution function:
 *   crps[t][j]         = (1/K) sum_k A(y - mu_k, v_k) - (1/(2 K^2)) sum_k sum_l A(mu_k - mu_l, v_k + v_l)
 *   pit[t][j]          = F(y),  F(x) = (1/K) sum_k Phi((x - mu_k) / sqrt v_k)
 *   quantiles[t][j][q] = the x with F(x) = levels[q]        (bisection to neighbouring doubles)
 * crps, pit: n_test x J, NaN where Y_test is NaN; quantiles: steps x J x Q, for every row.  Each output may be NULL, at least one
 * must not be; levels may be NULL with Q = 0 when quantiles is NULL.  The stacks are NOT scanned on the host: a component that is
 * not finite makes the outputs of its targets NaN and nothing else.  K = 0 or steps = 0 returns FFVD_OK and touches nothing.
 * Limits (FFVD_EINVAL, the message names the limit): 1 <= K <= 65536, 1 <= J <= 8, 0 <= Q <= 16, 1e-9 <= level <= 1 - 1e-9,
 * 0 <= n_test <= steps, noise_std finite and positive, every index product below 2^31.  targets_per_pass: 0 (automatic) or the
 * number of targets whose pair sums share one pass of the scratch; no result depends on it.
 *
 * ffvd_score_points: the components are points (rollouts, particle sets), mu_k = sum_d x[k][t][d] CC[d][j] + DD_j, v_k =
 * noise_std[j]^2.  Component k = k1 * K2 + k2 (K = K1 * K2), row t, lies at x + k1 * stride_k1 + k2 * stride_k2 + t * stride_t
 * (strides in doubles, D contiguous): [K][steps][D] is K1 = K, K2 = 1, stride_k1 = steps * D, stride_t = D; [G][T][N][D] is
 * K1 = G, K2 = N, stride_k1 = T * N * D, stride_k2 = D, stride_t = N * D.  D <= 32. */
int  ffvd_score_points(const double *x, int K1, int K2, int steps, int D, long long stride_k1, long long stride_k2, long long stride_t,
                       const double *CC, const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                       const double *levels, int Q, int targets_per_pass, double *crps, double *pit, double *quantiles);

/* The same for Gaussian states (m_x G x steps x D, S_x G x steps x D x D): mu_g = CC_j^T m[g][t] + DD_j, v_g = CC_j^T S[g][t] CC_j +
 * noise_std[j]^2, as ffvd_op_moment_summary; K = G.  D <= 8. */
int  ffvd_score_moments(const double *m_x, const double *S_x, int G, int steps, int D, const double *CC, const double *DD,
                        const double *noise_std, int J, const double *Y_test, int n_test, const double *levels, int Q,
                        int targets_per_pass, double *crps, double *pit, double *quantiles);

#ifdef __cplusplus
}
#endif
#endif /* FFVD_ABI_H */
