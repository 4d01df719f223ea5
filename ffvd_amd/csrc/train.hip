// Optimiser and shard entry points of the C ABI: Adam / SG-HMC state and updates on the resident parameters, the plain steps, the
// sharded step in its three-step and its native-RCCL form, the T-shard calls.  The launch sequences themselves are abi.hip's
// (forward, T-shard local / finish) and backward.hip's; this file checks arguments, orders the calls and reports.
#include "handle.h"
#include "optim.h"

#include <cmath>
#include <string>
#include <vector>

using namespace ffvd;

// ---- argument checks and result fetches every entry point below shares ---------------------------------------------------------
static int check_adam_hypers(ffvd_handle *h, const char *who, double lr, double beta1, double beta2, double eps) {
    if (!(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return set_error(h, FFVD_EINVAL, std::string(who) + ": bad hyper-parameter");
    return FFVD_OK;
}

static int check_sghmc_args(ffvd_handle *h, const char *who, const ffvd_params *noise, double epsilon, double mdecay, uint32_t sample_mask) {
    if (!noise || !(epsilon > 0.0) || !(mdecay >= 0.0)) return set_error(h, FFVD_EINVAL, std::string(who) + ": bad argument");
    if (sample_mask & FFVD_TRAIN_X)
        return set_error(h, FFVD_EINVAL, std::string(who) + ": X is never an SG-HMC variable (dgp_model.py:213-244)");
    return FFVD_OK;
}

static int check_grad(ffvd_handle *h, const char *who) {
    return h->cfg.grad ? FFVD_OK : set_error(h, FFVD_EINVAL, std::string(who) + ": the handle was created without grad = 1");
}
static int check_grad_handle(ffvd_handle *h, const char *who) {
    return h ? check_grad(h, who) : set_error(nullptr, FFVD_EINVAL, std::string(who) + ": null handle");
}

// The 8 sums at the head of gw.pack to h_sums behind whatever copy the caller has enqueued, ONE synchronisation, FFVD_ENOTPD
// "<who>: non-finite <tail>" unless they are finite.  own_result: this rank's result block (chain nll, info flags) comes along and its
// factorisation flags are looked at first -- the end of a pending backward pass (train_S_total).
static const char *const TSHARD_APPLY_TAIL = "sums in the exchanged block (a factorisation failed on a shard); parameters untouched";
static int fetch_pack_sums(ffvd_handle *h, const char *who, const char *tail, bool own_result = false) {
    hipStream_t s = h->stream;
    if (own_result) HIP_TRY(hipMemcpyAsync(h->h_res, h->resblk, h->res_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h->h_sums, h->gw.pack, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (own_result) {
        h->train_S_total = 0;
        int rc;
        if ((rc = check_info(h))) return rc;
    }
    return check_finite(h, h->h_sums, 8, who, tail);
}

// one of the handle's exchange buffers to or from a host array of the caller's, complete on return
static int exchange_copy(ffvd_handle *h, void *dst, const void *src, size_t count, hipMemcpyKind kind) {
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(double), kind, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FFVD_OK;
}

// ---- optimiser state and updates on the resident parameters -------------------------------------------------------------
// parameter, gradient and element count per array (handle.h PARAM_MEMBER order); U only where it has a gradient
struct ParamTable { double *theta[NPARAM]; const double *grad[NPARAM]; size_t n[NPARAM]; };
static ParamTable param_table(const ffvd_handle *h) {
    const ffvd_handle::GradWs &g = h->gw;
    ParamTable t{{}, {g.dX, g.dZ, g.dlogvar, g.dloglen, g.dlogQ, g.dCC, g.dDD, g.dlogR, g.dU}, {}};
    for (int i = 0; i < NPARAM; ++i) {
        t.theta[i] = const_cast<double *>(h->cur.*PARAM_MEMBER[i]);
        t.n[i] = (i == PARAM_U && !g.dU) ? 0 : param_count(h, i);
    }
    return t;
}

extern "C" int ffvd_optimizer_reset(ffvd_handle *h) {
    int rc;
    if ((rc = check_grad_handle(h, "ffvd_optimizer_reset"))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    const ParamTable p = param_table(h);
    for (int i = 0; i < NPARAM; ++i) {
        const size_t n = p.n[i];
        if (!n) continue;
        if (!h->adam_m[i]) { HIP_TRY(dev_alloc(h, &h->adam_m[i], n)); HIP_TRY(dev_alloc(h, &h->adam_v[i], n)); }
        HIP_TRY(hipMemsetAsync(h->adam_m[i], 0, n * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(h->adam_v[i], 0, n * sizeof(double), h->stream));
    }
    h->adam_t = 0;
    h->adam_ready = true;
    return FFVD_OK;
}

static int adam_update(ffvd_handle *h, double lr, double beta1, double beta2, double eps, uint32_t train_mask) {
    const ParamTable p = param_table(h);
    OptTable tab{};
    for (int i = 0; i < NPARAM; ++i) {
        if (!(train_mask & (1u << i)) || p.n[i] == 0) continue;
        OptTensor &t = tab.t[tab.count++];
        t.theta = p.theta[i]; t.grad = p.grad[i]; t.s0 = h->adam_m[i]; t.s1 = h->adam_v[i]; t.n = (int64_t)p.n[i];
    }
    h->adam_t += 1;
    const double lr_t = lr * sqrt(1.0 - pow(beta2, (double)h->adam_t)) / (1.0 - pow(beta1, (double)h->adam_t));
    launch_adam(h->stream, tab, lr_t, beta1, beta2, eps);
    HIP_TRY(hipGetLastError());
    return FFVD_OK;
}

static int sghmc_prepare(ffvd_handle *h, uint32_t sample_mask, const ffvd_params *noise, const char *who) {
    const ParamTable p = param_table(h);
    for (int i = 1; i < NPARAM; ++i) {
        const size_t n = p.n[i];
        if (!(sample_mask & (1u << i)) || n == 0) continue;
        const double *nz = noise->*PARAM_MEMBER[i];
        if (!nz) return set_error(h, FFVD_EINVAL, std::string(who) + ": a sampled array has no noise array");
        if (!h->hmc[i][0]) {            // xi, g, g2 <- 1, p <- 0 (base_model.py:151-154)
            std::vector<double> ones(n, 1.0);
            for (int k = 0; k < 5; ++k) HIP_TRY(dev_alloc(h, &h->hmc[i][k], n));
            // on the handle's stream, behind whatever dev_alloc enqueued there for these blocks (FFVD_WS_POISON).  `ones` is the source of
            // asynchronous copies: the stream is waited for on every path before it goes out of scope
            hipError_t e = hipSuccess;
            for (int k = 0; k < 3 && e == hipSuccess; ++k)
                e = hipMemcpyAsync(h->hmc[i][k], ones.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess) e = hipMemsetAsync(h->hmc[i][3], 0, n * sizeof(double), h->stream);      // the stream the update reads it on
            const hipError_t es = hipStreamSynchronize(h->stream);
            HIP_TRY(e);
            HIP_TRY(es);
        }
        HIP_TRY(hipMemcpyAsync(h->hmc[i][4], nz, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    return FFVD_OK;
}

static int sghmc_update(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in) {
    const ParamTable p = param_table(h);
    OptTable tab{};
    for (int i = 1; i < NPARAM; ++i) {
        if (!(sample_mask & (1u << i)) || p.n[i] == 0) continue;
        OptTensor &t = tab.t[tab.count++];
        t.theta = p.theta[i]; t.grad = p.grad[i]; t.s0 = h->hmc[i][0]; t.s1 = h->hmc[i][1]; t.s2 = h->hmc[i][2];
        t.s3 = h->hmc[i][3]; t.noise = h->hmc[i][4]; t.n = (int64_t)p.n[i];
    }
    // X_N = rows of X (dgp_model.py:203) -- of the JOB's trajectory: a T-shard handle holds T_r + 1 of its T_total + 1 rows
    const double x_n = (double)((h->cfg.T_total > 0 ? h->cfg.T_total : h->cfg.T) + 1);
    launch_sghmc(h->stream, tab, epsilon, mdecay, x_n, burn_in);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));           // the noise arrays are the caller's: done with them on return
    return FFVD_OK;
}

// ---- plain steps: one handle holds the whole job ----------------------------------------------------------------------------------------
static int check_whole_job(ffvd_handle *h, const char *who) {
    int rc;
    if ((rc = check_grad_handle(h, who))) return rc;
    if (h->Dl != h->cfg.D)
        return set_error(h, FFVD_EINVAL, std::string(who) + ": a latent-dim shard holds partial gradients; use " + who + "_allreduce");
    if (h->comm_world > 1)
        return set_error(h, FFVD_EINVAL, std::string(who) + ": this handle is one rank of a multi-rank communicator, its gradient is a share of "
                                         "the job's; use " + who + "_allreduce");
    return FFVD_OK;
}

extern "C" int ffvd_adam_step(ffvd_handle *h, double lr, double beta1, double beta2, double eps, uint32_t train_mask,
                              double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = check_whole_job(h, "ffvd_adam_step"))) return rc;
    if ((rc = check_adam_hypers(h, "ffvd_adam_step", lr, beta1, beta2, eps))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = ready(h, "ffvd_adam_step"))) return rc;
    if (!h->adam_ready && (rc = ffvd_optimizer_reset(h))) return rc;
    // (a failed factorisation leaves the parameters untouched)
    if ((rc = run_forward_backward(h, h->cfg.S_local))) return rc;
    if ((rc = adam_update(h, lr, beta1, beta2, eps, train_mask))) return rc;
    report_local(h, out_terms, out_nll);
    return FFVD_OK;
}

extern "C" int ffvd_sghmc_step(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in,
                               const ffvd_params *noise, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = check_whole_job(h, "ffvd_sghmc_step"))) return rc;
    if ((rc = check_sghmc_args(h, "ffvd_sghmc_step", noise, epsilon, mdecay, sample_mask))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = ready(h, "ffvd_sghmc_step"))) return rc;
    if ((rc = sghmc_prepare(h, sample_mask, noise, "ffvd_sghmc_step"))) return rc;
    if ((rc = run_forward_backward(h, h->cfg.S_local))) return rc;
    if ((rc = sghmc_update(h, epsilon, mdecay, sample_mask, burn_in))) return rc;
    report_local(h, out_terms, out_nll);
    return FFVD_OK;
}

// ---- sharded, device-resident training step (multi-GPU counterpart of adam.minimize(nll), dgp_model.py:303-305 /
// train_hypers, base_model.py:944-950, and of one burn_in_op / sample_op, base_model.py:143-179) ---------------------------
// Every rank: forward + backward with the whole job's chain count as the divisor, so that its gradient block is its ADDITIVE
// share; ONE all-reduce(sum) of [8 term sums | shared-parameter gradients (| dX for latent-dim shards)] in place in HBM;
// then the fused update from the reduced block.  No gradient crosses PCIe; the only host traffic is the result block.
static int train_local(ffvd_handle *h, int S_total, const char *who) {
    int rc;
    if ((rc = check_grad(h, who))) return rc;
    if (S_total < h->cfg.S_local) return set_error(h, FFVD_EINVAL, std::string(who) + ": S_total < S_local");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = ready(h, who))) return rc;
    h->train_S_total = 0;
    if ((rc = enqueue_forward_backward(h, S_total))) return rc;
    HIP_TRY(hipMemcpyAsync(h->gw.pack, h->out_terms, 8 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    h->train_S_total = S_total;
    return FFVD_OK;
}

// doubles of the block that take part in the exchange: chain shards keep dX (their own chains' rows) out of it
static size_t train_exchange_count(const ffvd_handle *h) {
    return (h->Dl != h->cfg.D) ? h->gw.pack_total : h->gw.pack_shared;
}

// The end of a sharded step: result block + the (reduced) sums to the host, the optimiser's update, the job's sums to the caller.  A
// failed factorisation anywhere leaves the parameters as they are.
template <class Update>
static int train_finish(ffvd_handle *h, const char *who, Update update, double out_terms[8], double *out_nll) {
    if (h->train_S_total <= 0) return set_error(h, FFVD_EINVAL, std::string(who) + ": no pending backward pass (ffvd_train_local first)");
    int rc;
    if ((rc = fetch_pack_sums(h, who, "sums after the exchange (a factorisation failed or was abandoned on another rank); parameters untouched", true)))
        return rc;
    if ((rc = update())) return rc;
    report_sums(h->h_sums, out_terms, out_nll);
    return FFVD_OK;
}

// ... and the whole step through native RCCL: `prepare` is what the optimiser needs before the backward pass (state, noise upload)
template <class Prepare, class Update>
static int step_allreduce(ffvd_handle *h, const char *who, void *rccl_comm, int S_total, Prepare prepare, Update update,
                          double out_terms[8], double *out_nll) {
    int rc;
    if (!rccl_comm && !h->comm) return set_error(h, FFVD_EINVAL, std::string(who) + ": no communicator (pass one or call ffvd_comm_init)");
    if ((rc = prepare())) return rc;
    if ((rc = train_local(h, S_total, who))) return rc;
    if ((rc = ffvd_allreduce_sum_async(h, rccl_comm, h->gw.pack, (int64_t)train_exchange_count(h)))) { h->train_S_total = 0; return rc; }
    return train_finish(h, who, update, out_terms, out_nll);
}

extern "C" int ffvd_train_local(ffvd_handle *h, int S_total) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_train_local: null handle");
    return train_local(h, S_total, "ffvd_train_local");
}

extern "C" int64_t ffvd_train_exchange_count(const ffvd_handle *h) { return (h && h->cfg.grad) ? (int64_t)train_exchange_count(h) : 0; }

extern "C" void *ffvd_train_exchange_ptr(ffvd_handle *h) { return (h && h->cfg.grad) ? (void *)h->gw.pack : nullptr; }

extern "C" int ffvd_train_exchange_get(ffvd_handle *h, double *host_out) {
    if (!h || !host_out || !h->cfg.grad) return set_error(h, FFVD_EINVAL, "ffvd_train_exchange_get: bad argument");
    return exchange_copy(h, host_out, h->gw.pack, train_exchange_count(h), hipMemcpyDeviceToHost);
}

extern "C" int ffvd_train_exchange_set(ffvd_handle *h, const double *host_in) {
    if (!h || !host_in || !h->cfg.grad) return set_error(h, FFVD_EINVAL, "ffvd_train_exchange_set: bad argument");
    return exchange_copy(h, h->gw.pack, host_in, train_exchange_count(h), hipMemcpyHostToDevice);
}

extern "C" int ffvd_adam_apply(ffvd_handle *h, double lr, double beta1, double beta2, double eps, uint32_t train_mask,
                               double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = check_grad_handle(h, "ffvd_adam_apply"))) return rc;
    if ((rc = check_adam_hypers(h, "ffvd_adam_apply", lr, beta1, beta2, eps))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (!h->adam_ready && (rc = ffvd_optimizer_reset(h))) return rc;
    return train_finish(h, "ffvd_adam_apply", [&] { return adam_update(h, lr, beta1, beta2, eps, train_mask); }, out_terms, out_nll);
}

extern "C" int ffvd_sghmc_apply(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in,
                                const ffvd_params *noise, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = check_grad_handle(h, "ffvd_sghmc_apply"))) return rc;
    if ((rc = check_sghmc_args(h, "ffvd_sghmc_apply", noise, epsilon, mdecay, sample_mask))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = sghmc_prepare(h, sample_mask, noise, "ffvd_sghmc_apply"))) return rc;
    return train_finish(h, "ffvd_sghmc_apply", [&] { return sghmc_update(h, epsilon, mdecay, sample_mask, burn_in); }, out_terms, out_nll);
}

extern "C" int ffvd_adam_step_allreduce(ffvd_handle *h, void *rccl_comm, int S_total, double lr, double beta1, double beta2,
                                        double eps, uint32_t train_mask, double out_terms[8], double *out_nll) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_adam_step_allreduce: null handle");
    int rc;
    if ((rc = check_adam_hypers(h, "ffvd_adam_step_allreduce", lr, beta1, beta2, eps))) return rc;
    return step_allreduce(h, "ffvd_adam_step_allreduce", rccl_comm, S_total,
                          [&] { return (h->cfg.grad && !h->adam_ready) ? ffvd_optimizer_reset(h) : FFVD_OK; },      // (no grad: train_local says so)
                          [&] { return adam_update(h, lr, beta1, beta2, eps, train_mask); }, out_terms, out_nll);
}

extern "C" int ffvd_sghmc_step_allreduce(ffvd_handle *h, void *rccl_comm, int S_total, double epsilon, double mdecay,
                                         uint32_t sample_mask, int burn_in, const ffvd_params *noise, double out_terms[8],
                                         double *out_nll) {
    int rc;
    if ((rc = check_grad_handle(h, "ffvd_sghmc_step_allreduce"))) return rc;
    if ((rc = check_sghmc_args(h, "ffvd_sghmc_step_allreduce", noise, epsilon, mdecay, sample_mask))) return rc;
    auto prepare = [&]() -> int {
        HIP_TRY(hipSetDevice(h->cfg.device_id));
        int r = ready(h, "ffvd_sghmc_step_allreduce");
        return r ? r : sghmc_prepare(h, sample_mask, noise, "ffvd_sghmc_step_allreduce");
    };
    return step_allreduce(h, "ffvd_sghmc_step_allreduce", rccl_comm, S_total, prepare,
                          [&] { return sghmc_update(h, epsilon, mdecay, sample_mask, burn_in); }, out_terms, out_nll);
}

// ---- T-shard fallback (include/ffvd_abi.h "T-shard"); the launch sequences are abi.hip's ------------------------------------
static int tshard_ready(ffvd_handle *h, const char *who) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, std::string(who) + ": null handle");
    if (h->cfg.T_total <= 0) return set_error(h, FFVD_EINVAL, std::string(who) + ": the handle is not a T-shard (cfg.T_total = 0)");
    return ready(h, who);
}

extern "C" int64_t ffvd_tshard_count(const ffvd_handle *h) { return h ? h->ts_count : 0; }

extern "C" int ffvd_tshard_local(ffvd_handle *h) {
    int rc;
    if ((rc = tshard_ready(h, "ffvd_tshard_local"))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    return enqueue_tshard_local(h);
}

extern "C" int ffvd_tshard_get(ffvd_handle *h, double *host_out) {
    int rc;
    if ((rc = tshard_ready(h, "ffvd_tshard_get"))) return rc;
    if (!host_out) return set_error(h, FFVD_EINVAL, "ffvd_tshard_get: null output");
    return exchange_copy(h, host_out, h->tsbuf, (size_t)h->ts_count, hipMemcpyDeviceToHost);
}

extern "C" int ffvd_tshard_set(ffvd_handle *h, const double *host_in) {
    int rc;
    if ((rc = tshard_ready(h, "ffvd_tshard_set"))) return rc;
    if (!host_in) return set_error(h, FFVD_EINVAL, "ffvd_tshard_set: null input");
    return exchange_copy(h, h->tsbuf, host_in, (size_t)h->ts_count, hipMemcpyHostToDevice);
}

// The finish (S_total > 0: and the backward pass behind it) with the recovery of an abandoned dataflow Cholesky(A).
static int tshard_finish_run(ffvd_handle *h, int S_total, const char *who, double out_terms[8], double *out_nll) {
    int rc;
    // The finish is a pure function of the exchanged buffer (read-only here) and of this rank's K_uu chain, and no collective
    // follows inside the call: a dataflow Cholesky(A) that gave up on a bounded wait is re-run ONCE with the launch-per-column
    // variant, like the single-rank entry points (fetch_with_stall_recovery).  A failure of the K_uu chain itself (local phase,
    // BEFORE the exchange) has already turned the exchanged chain sums into NaN on every rank.
    for (int attempt = 0;; ++attempt) {
        {
            CholOverrideGuard guard;
            if (attempt == 1) {
                guard.force_left();
                HIP_TRY(hipMemsetAsync(h->info + h->Dl, 0, (size_t)h->nbatch * sizeof(int32_t), h->stream));
            }
            if ((rc = enqueue_tshard_finish(h))) return rc;
            if (S_total > 0) {
                // backward pass on the job's factorisation: this shard's ADDITIVE share of every gradient (grad_finalize: the
                // M x M-side terms and the priors count on the first shard only), dX for the shard's own rows.  The term sums
                // head the block like in a sharded training step -- the job's on the first shard, zero elsewhere -- so that
                // ONE all-reduce(sum) of ffvd_train_exchange_count doubles completes both.
                if ((rc = enqueue_grad_b(h, S_total))) return rc;
                if (h->cfg.t_begin == 0)
                    HIP_TRY(hipMemcpyAsync(h->gw.pack, h->out_terms, 8 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
                else HIP_TRY(hipMemsetAsync(h->gw.pack, 0, 8 * sizeof(double), h->stream));
            }
        }
        HIP_TRY(hipMemcpyAsync(h->h_res, h->resblk, h->res_bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        rc = check_info(h);
        bool kuu_ok = true;
        for (int i = 0; i < h->Dl; ++i) kuu_ok = kuu_ok && h->h_info[i] == 0;
        if (rc == FFVD_EDEVICE && h->stalled && kuu_ok && attempt == 0) continue;
        if (rc == FFVD_OK && attempt == 1) {
            if (h->stall_recoveries++ == 0)
                h->warning = "warning: the one-launch (dataflow) Cholesky gave up on a bounded wait; the T-shard finish was re-run with "
                             "the launch-per-column Cholesky and completed";
            h->err = h->warning;
        }
        break;
    }
    if (rc) return rc;
    if ((rc = check_finite(h, h->h_out, 7, who, "sums after the exchange (a factorisation failed or was abandoned on another rank)"))) return rc;
    report_local(h, out_terms, out_nll);
    return FFVD_OK;
}

extern "C" int ffvd_tshard_finish(ffvd_handle *h, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = tshard_ready(h, "ffvd_tshard_finish"))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    return tshard_finish_run(h, 0, "ffvd_tshard_finish", out_terms, out_nll);
}

// ---- gradient of a T-sharded job -------------------------------------------------------------------------
// After the exchange of the raw tiles every shard holds the job's A, its factor, u and Gamma; the K_fu side of the backward pass
// (E = (2 K_fu Gamma + alpha delta u^T) o K_fu and its reductions) runs over the shard's own rows and is additive over shards,
// like the likelihood / transition sums; the M x M side (K_uu chain rule, tr(A^-1 G), u^T G u, priors) is the same on every shard
// and counted on the first.  dX covers the shard's own T + 1 rows: the row two neighbouring shards share (the last of one, the
// first of the next) gets a part from each -- the caller adds them.
static int tshard_grad_ready(ffvd_handle *h, const char *who, int S_total) {
    int rc;
    if ((rc = tshard_ready(h, who)) || (rc = check_grad(h, who))) return rc;
    if (S_total < h->cfg.S_local) return set_error(h, FFVD_EINVAL, std::string(who) + ": S_total < S_local");
    return FFVD_OK;
}

extern "C" int ffvd_tshard_finish_grad(ffvd_handle *h, int S_total, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = tshard_grad_ready(h, "ffvd_tshard_finish_grad", S_total))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    return tshard_finish_run(h, S_total, "ffvd_tshard_finish_grad", out_terms, out_nll);
}

extern "C" int ffvd_tshard_grad_fetch(ffvd_handle *h, double out_terms[8], const ffvd_grads *gout) {
    int rc;
    if ((rc = tshard_grad_ready(h, "ffvd_tshard_grad_fetch", h ? h->cfg.S_local : 0))) return rc;
    if (!gout) return set_error(h, FFVD_EINVAL, "ffvd_tshard_grad_fetch: null gradient struct");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = copy_grads_out(h, gout))) return rc;
    if ((rc = fetch_pack_sums(h, "ffvd_tshard_grad_fetch", "sums in the exchanged block (a factorisation failed on another rank)"))) return rc;
    report_sums(h->h_sums, out_terms, nullptr);
    return FFVD_OK;
}

// Optimiser step of a T-sharded job (dgp_model.py:303-305 trains every variable).  After ffvd_tshard_grad_fetch /
// ffvd_elbo_tshard_grad the exchanged block in gw.pack holds the WHOLE job's shared-parameter gradients, identical on every shard;
// dX holds this shard's own T + 1 rows, whose first and last row each lack the part of the neighbouring shard.  The caller adds
// those parts (one small exchange of boundary rows, ffvd_amd/distributed.py) and hands the rows back here: they replace gw.dX and the
// fused Adam update runs over every parameter array.  Shared parameters receive the same gradient and carry the same optimiser
// state on every shard, the two copies of a boundary row likewise: the shards' parameters stay identical without a broadcast.
extern "C" int ffvd_tshard_adam_apply(ffvd_handle *h, const double *dX_rows, double lr, double beta1, double beta2, double eps,
                                      uint32_t train_mask, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = tshard_grad_ready(h, "ffvd_tshard_adam_apply", h ? h->cfg.S_local : 0))) return rc;
    if (!dX_rows) return set_error(h, FFVD_EINVAL, "ffvd_tshard_adam_apply: null dX rows");
    if ((rc = check_adam_hypers(h, "ffvd_tshard_adam_apply", lr, beta1, beta2, eps))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (!h->adam_ready && (rc = ffvd_optimizer_reset(h))) return rc;
    // the host rows are the caller's: the upload is complete behind the synchronisation of the fetch
    HIP_TRY(hipMemcpyAsync(h->gw.dX, dX_rows, param_count(h, 0) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = fetch_pack_sums(h, "ffvd_tshard_adam_apply", TSHARD_APPLY_TAIL))) return rc;
    if ((rc = adam_update(h, lr, beta1, beta2, eps, train_mask))) return rc;
    report_sums(h->h_sums, out_terms, out_nll);
    return FFVD_OK;
}

// ... and the SG-HMC update (burn_in_op / sample_op, base_model.py:143-179) of a T-sharded job: X is never an SG-HMC variable
// (dgp_model.py:213-244), so the exchanged block is all it needs -- every shard applies the same update with the same noise.
extern "C" int ffvd_tshard_sghmc_apply(ffvd_handle *h, double epsilon, double mdecay, uint32_t sample_mask, int burn_in,
                                       const ffvd_params *noise, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = tshard_grad_ready(h, "ffvd_tshard_sghmc_apply", h ? h->cfg.S_local : 0))) return rc;
    if ((rc = check_sghmc_args(h, "ffvd_tshard_sghmc_apply", noise, epsilon, mdecay, sample_mask))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = sghmc_prepare(h, sample_mask, noise, "ffvd_tshard_sghmc_apply"))) return rc;
    if ((rc = fetch_pack_sums(h, "ffvd_tshard_sghmc_apply", TSHARD_APPLY_TAIL))) return rc;
    if ((rc = sghmc_update(h, epsilon, mdecay, sample_mask, burn_in))) return rc;
    report_sums(h->h_sums, out_terms, out_nll);
    return FFVD_OK;
}

extern "C" int ffvd_elbo_tshard(ffvd_handle *h, void *rccl_comm, double out_terms[8], double *out_nll) {
    int rc;
    if ((rc = tshard_ready(h, "ffvd_elbo_tshard"))) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = enqueue_tshard_local(h))) return rc;
    if ((rc = ffvd_allreduce_sum_async(h, rccl_comm, h->tsbuf, h->ts_count))) return rc;      // the ONE exchange step
    return ffvd_tshard_finish(h, out_terms, out_nll);
}
// nll + gradient of a T-sharded job: two exchange steps (raw tiles + chain sums; then the gradient block), both native RCCL
extern "C" int ffvd_elbo_tshard_grad(ffvd_handle *h, void *rccl_comm, int S_total, double out_terms[8], double *out_nll,
                                     const ffvd_grads *gout) {
    int rc;
    if ((rc = tshard_grad_ready(h, "ffvd_elbo_tshard_grad", S_total))) return rc;
    if (!gout) return set_error(h, FFVD_EINVAL, "ffvd_elbo_tshard_grad: null gradient struct");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if ((rc = enqueue_tshard_local(h))) return rc;
    if ((rc = ffvd_allreduce_sum_async(h, rccl_comm, h->tsbuf, h->ts_count))) return rc;
    // a failed finish still takes part in the second exchange (NaN sums at the head of its block): the ranks stay in step
    const int rc_fin = tshard_finish_run(h, S_total, "ffvd_elbo_tshard_grad", nullptr, nullptr);
    if (rc_fin) {
        std::vector<double> nan8(8, std::nan(""));
        HIP_TRY(hipMemcpy(h->gw.pack, nan8.data(), 8 * sizeof(double), hipMemcpyHostToDevice));
    }
    const std::string first_err = rc_fin ? h->err : std::string();
    if ((rc = ffvd_allreduce_sum_async(h, rccl_comm, h->gw.pack, (int64_t)h->gw.pack_shared))) return rc;
    if (rc_fin) { HIP_TRY(hipStreamSynchronize(h->stream)); return set_error(h, rc_fin, first_err); }
    if ((rc = ffvd_tshard_grad_fetch(h, nullptr, gout))) return rc;
    report_sums(h->h_sums, out_terms, out_nll);
    return FFVD_OK;
}
