// C ABI of libffvd_hip.so (see include/ffvd_abi.h): handle lifetime, resident buffers, the per-iteration
// launch sequence of the ELBO and of a T-shard, parameters in and out.  The multi-kernel backward pass is in backward.hip, optimiser
// steps and the shard entry points in train.hip, the RCCL binding in comm.hip (the handle all four see: handle.h); the stateless
// ffvd_op_* operators are in ops.hip, ops_loops.hip and ops_grouped.hip.
#include "handle.h"
#include "kernels.h"
#include "kernels_f32.h"
#include "grad.h"
#include "optim.h"
#include "tiny.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace ffvd;

static thread_local std::string g_last_error;
std::string &ffvd::last_error() { return g_last_error; }

// fixed sizes of the schedule (plan_schedule, create_impl)
constexpr int F32C_FLUSH_TILES = 128;       // fp32 summation chains of the Gram product are cut every 4096 rows (128 t-tiles of 32 rows)
constexpr int SMALL_SIDE_WGS = 512;         // tile-pass workgroups (one round of the chip) up to which an iteration counts as tiny (small_side)
constexpr int SMALL_SIDE_ROWS = 32;         // block rows of the K_uu chain (Dl * 2 * Mp / 64) up to which that iteration's side chain is ONE dataflow launch

int ffvd::set_error(ffvd_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    g_last_error = msg;
    return code;
}

extern "C" const char *ffvd_last_error(const ffvd_handle *h) {
    return h ? h->err.c_str() : g_last_error.c_str();
}

extern "C" int64_t ffvd_workspace_bytes(const ffvd_handle *h) { return h ? h->ws_bytes : 0; }

extern "C" int ffvd_destroy(ffvd_handle *h) {
    if (!h) return FFVD_OK;
    hipSetDevice(h->cfg.device_id);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->comm) ffvd_comm_destroy(h);
    for (void *p : h->allocs) hipFree(p);
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    if (h->h_res) hipHostFree(h->h_res);
    if (h->tiny_ring_made) { tiny_ring_destroy(h->tiny_ring[0]); tiny_ring_destroy(h->tiny_ring[1]); }
    if (h->aux) { hipStreamSynchronize(h->aux); hipStreamDestroy(h->aux); }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->ev_join2) hipEventDestroy(h->ev_join2);
    if (h->ev_kuu) hipEventDestroy(h->ev_kuu);
    if (h->ev_tiles) hipEventDestroy(h->ev_tiles);
    if (h->ev_go) hipEventDestroy(h->ev_go);
    if (h->ev_hwords) hipEventDestroy(h->ev_hwords);
    if (h->ev_prior) hipEventDestroy(h->ev_prior);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return FFVD_OK;
}

static int create_impl(const ffvd_config *cfg, ffvd_handle *h) {
    const ffvd_config &c = h->cfg;
    {
        auto on = [](const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; };
        ffvd_handle::Switches &w = h->sw;
        w.grad_explicit = on("FFVD_GRAD_EXPLICIT");   w.no_defer_trace = on("FFVD_NO_DEFER_TRACE");
        w.no_kfu_first = on("FFVD_NO_KFU_FIRST");     w.grad_serial = on("FFVD_GRAD_SERIAL");
        w.whiten_products = on("FFVD_GRAD_WHITEN_PRODUCTS");   w.lt_armed = on("FFVD_GRAD_LT_ARMED");
        w.no_linear_lowrank = on("FFVD_NO_LINEAR_LOWRANK");
        w.debug_sync = on("FFVD_DEBUG_SYNC");
        w.no_tiny = on("FFVD_NO_TINY");               w.no_tiny_a = on("FFVD_NO_TINY_A");
        w.ws_poison = on("FFVD_WS_POISON");
        if (const char *e = getenv("FFVD_DEBUG_SIDE_DELAY_US")) w.side_delay_us = atoi(e);
        if (const char *e = getenv("FFVD_DEBUG_MAIN_DELAY_US")) w.main_delay_us = atoi(e);
    }
    h->P = c.D + c.C;
    h->Dl = c.d_count > 0 ? c.d_count : c.D;
    h->Mp = round_up(c.M, NB);
    h->Tp = round_up(c.T, STRIP);
    h->ng = (h->Mp + 511) / 512;
    h->nbatch = c.S_local * h->Dl;
    const size_t Mp = h->Mp, Tp = h->Tp, Dl = h->Dl, P = h->P;
    // chains per pass: every launch should cover as many (chain, dim) units as possible (the batched Cholesky and
    // the Gram grid need >= 1 workgroup per CU); F costs Dl*Tp*Mp*8 bytes per chain, budget 48 GiB of the 288 GB.
    if (c.chains_per_pass > 0) h->cpp = c.chains_per_pass;
    else {
        const size_t per_chain = Dl * Tp * Mp * (c.dtype == FFVD_F32C ? sizeof(float) : sizeof(double));
        size_t n = ((size_t)48 << 30) / (per_chain ? per_chain : 1);
        if (n < 1) n = 1;
        if (n > (size_t)c.S_local) n = c.S_local;
        h->cpp = (int)n;
    }
    if (h->cpp > c.S_local || c.grad || c.T_total > 0) h->cpp = c.S_local;      // backward pass, T-shards: one pass over all chains
    HIP_TRY(hipSetDevice(c.device_id));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    {   // the side stream carries a short latency-bound chain: give it the highest priority
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, hi));
    }
    HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_join2, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_kuu, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_tiles, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_go, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_hwords, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_prior, hipEventDisableTiming));
    HIP_TRY(dev_alloc(h, &h->prior_sums, 16));
    HIP_TRY(dev_alloc(h, &h->X, (size_t)c.S_local * (c.T + 1) * c.D));
    HIP_TRY(dev_alloc(h, &h->Z, (size_t)c.M * P));
    HIP_TRY(dev_alloc(h, &h->U, (size_t)c.M * c.D));
    HIP_TRY(dev_alloc(h, &h->logvar, (size_t)c.D));
    HIP_TRY(dev_alloc(h, &h->loglen, (size_t)c.D * P));
    HIP_TRY(dev_alloc(h, &h->logQ, (size_t)c.D));
    HIP_TRY(dev_alloc(h, &h->CC, (size_t)c.D * c.Ydim));
    HIP_TRY(dev_alloc(h, &h->DD, (size_t)c.Ydim));
    HIP_TRY(dev_alloc(h, &h->logR, (size_t)c.Ydim * c.Ydim));
    HIP_TRY(dev_alloc(h, &h->Y, (size_t)c.T * c.Ydim));
    HIP_TRY(dev_alloc(h, &h->ctrl, (size_t)c.T * c.C));
    HIP_TRY(dev_alloc(h, &h->variance, Dl));
    HIP_TRY(dev_alloc(h, &h->len, Dl * P));
    HIP_TRY(dev_alloc(h, &h->Zs, Dl * Mp * P));
    HIP_TRY(dev_alloc(h, &h->zz, Dl * Mp));
    HIP_TRY(dev_alloc(h, &h->Kuu, Dl * 2 * Mp * Mp));
    // reference route of the collapsed branch: K_fu is built once (kfu_build) and projected by a triangular GEMM
    // (explicit-U branch: only from 64 units of the headline size on -- below that the single fused kernel is quicker:
    //  1.10 vs 1.21 ms on config 5's 16 units -- or when the backward pass needs K_fu anyway)
    const bool big_a = (size_t)h->nbatch * Tp * Mp >= (size_t)64 * 4096 * 512 || c.grad;
    const bool grad_ref = c.grad && c.branch == FFVD_BRANCH_B && c.route == FFVD_ROUTE_REFERENCE;    // backward pass in the reference's op order
    const bool proj_gemm = (c.branch == FFVD_BRANCH_A && big_a) || (c.branch == FFVD_BRANCH_B && c.route == FFVD_ROUTE_REFERENCE);
    h->ngr = (proj_gemm && c.dtype != FFVD_F32C) ? (int)((Mp + 127) / 128) : 0;
    HIP_TRY(dev_alloc(h, &h->rowsq, (size_t)h->nbatch * (h->ngr > h->ng ? h->ngr : h->ng) * Tp));
    HIP_TRY(dev_alloc(h, &h->fmean, (size_t)h->nbatch * (h->ngr > h->ng ? h->ngr : h->ng) * Tp));
    if (c.branch == FFVD_BRANCH_B) {
        const size_t pass_b = (size_t)h->cpp * Dl;
        if (c.dtype == FFVD_F32C) {
            HIP_TRY(dev_alloc(h, &h->Kf32, pass_b * Tp * Mp));
            HIP_TRY(dev_alloc(h, &h->F32, pass_b * Tp * Mp));
            HIP_TRY(dev_alloc(h, &h->Linv32, Dl * Mp * Mp));
            h->nsq = proj_f32_ntiles((int)Tp, (int)Mp);
            HIP_TRY(dev_alloc(h, &h->sqpart, (size_t)h->nbatch * h->nsq));
            HIP_TRY(dev_alloc(h, &h->sqsum, (size_t)h->nbatch));
        } else {
            HIP_TRY(dev_alloc(h, &h->F, pass_b * Tp * Mp));
            if (h->ngr) HIP_TRY(dev_alloc(h, &h->Kf2, pass_b * Tp * Mp));
        }
        const size_t hrows = c.grad ? 2 * Mp + NB : Mp + NB;     // grad: Mp identity rows (-> L_A^-T) before the b row
        HIP_TRY(dev_alloc(h, &h->H, pass_b * hrows * Mp));
        HIP_TRY(hipMemsetAsync(h->H, 0, pass_b * hrows * Mp * sizeof(double), h->stream));
    }
    h->ntiles = gram_ntiles(h->Mp);
    const bool grad_a = c.grad && c.branch == FFVD_BRANCH_A;
    if (c.branch == FFVD_BRANCH_A && (grad_a || h->ngr)) {                       // K_fu (projection GEMM input, backward pass)
        HIP_TRY(dev_alloc(h, &h->F, (size_t)(grad_a ? h->nbatch : h->cpp * Dl) * Tp * Mp));
        HIP_TRY(dev_alloc(h, &h->ucolA, Dl * Mp));
    }
    if ((c.branch == FFVD_BRANCH_B && c.route == FFVD_ROUTE_GRAM) || grad_a || grad_ref) {
        HIP_TRY(dev_alloc(h, &h->Kcopy, Dl * Mp * Mp));
        HIP_TRY(dev_alloc(h, &h->Linv, Dl * Mp * Mp));
        HIP_TRY(hipMemsetAsync(h->Linv, 0, Dl * Mp * Mp * sizeof(double), h->stream));     // blocks above the diagonal stay zero
        HIP_TRY(dev_alloc(h, &h->Kinv, Dl * Mp * Mp));
        HIP_TRY(dev_alloc(h, &h->trpart, (size_t)h->nbatch * h->ntiles));
        HIP_TRY(dev_alloc(h, &h->kterms, Dl * 2));
    }
    if (c.grad) { int rcg = alloc_grad_workspace(h); if (rcg) return rcg; }
    HIP_TRY(dev_alloc(h, &h->hterms, (size_t)h->nbatch * 2));
    if (c.T_total > 0) {        // the chain sums live at the tail of the exchange buffer: one all-reduce covers both
        const size_t raw = (size_t)h->nbatch * (Mp + 1) * Mp;
        h->ts_count = (int64_t)(raw + (size_t)c.S_local * 8);
        HIP_TRY(dev_alloc(h, &h->tsbuf, (size_t)h->ts_count));
        HIP_TRY(hipMemsetAsync(h->tsbuf, 0, (size_t)h->ts_count * sizeof(double), h->stream));   // tiles above the diagonal stay 0
        h->chain_terms = h->tsbuf + raw;
    } else
        HIP_TRY(dev_alloc(h, &h->chain_terms, (size_t)c.S_local * 8));
    HIP_TRY(dev_alloc(h, &h->chain_partial, (size_t)c.S_local * 128));        // [S][<= 32 row ranges][4] (launch_chain_reduce)
    {
        const size_t nS = (size_t)(c.S_local ? c.S_local : 1), ninfo = (size_t)(Dl + h->nbatch);
        const size_t ndbl = 8 + nS + (ninfo + 1) / 2;
        HIP_TRY(dev_alloc(h, &h->resblk, ndbl));
        h->res_bytes = ndbl * sizeof(double);
        h->out_terms = h->resblk;
        h->chain_nll = h->resblk + 8;
        h->info = reinterpret_cast<int32_t *>(h->resblk + 8 + nS);
        HIP_TRY(hipHostMalloc((void **)&h->h_res, h->res_bytes + 8 * sizeof(double)));
        h->h_sums = h->h_res + ndbl;                 // whole-job sums of a sharded training step (behind the result block)
        h->h_out = h->h_res;
        h->h_chain = h->h_res + 8;
        h->h_info = reinterpret_cast<int32_t *>(h->h_res + 8 + nS);
    }
    if (c.branch == FFVD_BRANCH_B && c.dtype != FFVD_F32C) {
        const int upass = h->cpp * (int)Dl;
        // the K_fu build forms delta^T K_fu (Gram route) / the projection GEMM forms delta^T F (reference route): the Gram kernel has no row
        const bool ext_row = (c.route == FFVD_ROUTE_GRAM && c.T_total == 0) || (c.route == FFVD_ROUTE_REFERENCE && h->ngr > 0);
        // Few chains (one pass, no backward pass): the K_uu side chain goes BEHIND the tile pass as one dataflow launch (beside Cholesky(A)),
        // and the tile pass takes the row ranges that fill the chip's 512 slots exactly -- beside the pass, the chain's two dozen launches
        // only ran where the pass left slots free, which is what held the pass at three ranges (plan_schedule, side_late)
        const bool late_ok = c.route == FFVD_ROUTE_GRAM && !c.grad && c.T_total == 0 && c.S_local <= h->cpp && !h->sw.no_defer_trace &&
                             (size_t)Dl * 2 * (Mp / NB) <= 64 && (size_t)Dl * 2 * (Mp / NB) > (size_t)SMALL_SIDE_ROWS &&
                             potrf_flow_forms_inverse((int)Mp, (int)Dl, CHOL_FLOW);
        h->side_late = late_ok && upass <= 96;
        if (h->side_late) {
            h->gsplit = gram_ksplit((int)Mp, upass, (int)Tp, ext_row ? 0 : 1, true);
            if (h->gsplit <= 1) h->side_late = false;
        }
        if (!h->side_late) h->gsplit = gram_ksplit((int)Mp, upass, (int)Tp, ext_row ? 0 : 1);
        if (ext_row) HIP_TRY(dev_alloc(h, &h->growpart, (size_t)upass * (Tp / 64) * Mp));
        h->gtail_wg = gram_tail_wg((int)Mp, upass, h->gsplit, ext_row ? 0 : 1);
        if (h->gtail_wg > 0) {
            HIP_TRY(dev_alloc(h, &h->gtail, gram_tail_doubles(h->gtail_wg)));
            HIP_TRY(hipMemsetAsync(h->gtail, 0, gram_tail_doubles(h->gtail_wg) * sizeof(double), h->stream));   // counters start at 0
        }
        if (h->gsplit > 1) HIP_TRY(dev_alloc(h, &h->gpart, gram_part_doubles((int)Mp, upass, h->gsplit)));
        else if (c.route == FFVD_ROUTE_GRAM && (size_t)upass * Tp * Mp >= (size_t)128 * 4096 * 512)
            // a K_fu build of 0.4 ms or more: the K_uu chain as ONE dataflow launch finishes beside it, the main stream
            // joins before the Gram kernel, which then forms the trace partials in its own epilogue
            h->kuu_flow_sched = true;
        else if (c.route == FFVD_ROUTE_GRAM && (size_t)upass * Tp * Mp >= (size_t)64 * 4096 * 512 && !h->sw.no_defer_trace) {
            HIP_TRY(dev_alloc(h, &h->graw, (size_t)upass * (Mp + 1) * Mp));   // raw tiles + trace pass beside Cholesky(A)
            // (unsplit pass of up to 16 chains: the chain's launches were starved by the pass and ended 0.1 ms behind Cholesky(A) -- behind
            //  the pass as one dataflow launch as well)
            h->side_late = late_ok && upass <= 64;
        }
    }
    if (c.branch == FFVD_BRANCH_A && !c.grad && !h->sw.no_linear_lowrank && linear_lowrank_supported(c.kernel_kind, P))
        HIP_TRY(dev_alloc(h, &h->lrpart, linear_lowrank_doubles((int)Mp, (int)Dl, P)));
    if (c.dtype == FFVD_F64 && c.T_total == 0 && !h->sw.no_tiny && !(c.branch == FFVD_BRANCH_A && h->sw.no_tiny_a)) {      // (both branches since round 5)
        // The whole iteration as ONE launch when every role's workgroup fits on the chip at once (tiny.hip).  The multi-kernel
        // workspaces above stay: a launch abandoned on a bounded wait is re-run on them (fetch_with_stall_recovery).
        int cus = 0;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c.device_id) == hipSuccess) cus = prop.multiProcessorCount;
        h->tiny = tiny_plan(c.kernel_kind, c.T, c.D, c.C, c.M, c.S_local, (int)Dl, c.grad, cus);
        h->tiny_cus = cus;
        if (h->tiny.ok) {
            // The plan needs every workgroup resident at once, and a wave is resident only with its scratch: the figure the loaded
            // code object reports must be the one this file was validated with, and the launch's total must stay within a budget
            // the runtime grants without throttling wave slots (checked where the handle is made, not assumed).
            size_t pb = 0;
            const int wpu_max = 1 + h->tiny.nstrips + (h->tiny.side ? h->tiny.NT : 0);
            if (tiny_kernel_private_bytes(h->tiny.nw, c.branch == FFVD_BRANCH_B ? 1 : 0, &pb) != hipSuccess || pb > TINY_PRIVATE_BYTES_MAX ||
                pb * 64 * h->tiny.nw * (size_t)h->tiny.nunits * wpu_max > TINY_PRIVATE_LAUNCH_BUDGET) {
                char wmsg[256];
                snprintf(wmsg, sizeof wmsg, "warning: one-launch iteration not used: its kernel reports %zu bytes of private memory per lane "
                         "(validated up to %zu; launch budget %zu MB)", pb, TINY_PRIVATE_BYTES_MAX, TINY_PRIVATE_LAUNCH_BUDGET >> 20);
                h->warning = wmsg;
                h->err = h->warning;
                h->tiny.ok = false;
            }
            h->tiny_private_bytes = pb;
        }
        if (h->tiny.ok) {
            HIP_TRY(dev_alloc(h, &h->tiny_scratch, tiny_scratch_doubles(h->tiny, c.T, (int)P, c.M, c.S_local, (int)Dl, c.D, c.Ydim, c.grad)));
            HIP_TRY(dev_alloc(h, &h->tiny_flags, tiny_flag_ints(h->tiny, c.S_local)));
            HIP_TRY(hipMemsetAsync(h->tiny_flags, 0, tiny_flag_ints(h->tiny, c.S_local) * sizeof(int), h->stream));
            HIP_TRY(dev_alloc(h, &h->tiny_dargs, 2));
            HIP_TRY(tiny_ring_create(h->tiny_ring[0]));
            HIP_TRY(tiny_ring_create(h->tiny_ring[1]));
            h->tiny_ring_made = true;
        }
    }
    HIP_TRY(dev_alloc(h, &h->dinvK, potrf_scratch_doubles((int)Mp, (int)Dl)));
    HIP_TRY(dev_alloc(h, &h->dinvH, potrf_scratch_doubles((int)Mp, h->nbatch ? h->nbatch : 1)));
    HIP_TRY(hipMemsetAsync(h->U, 0, (size_t)(c.M * c.D ? c.M * c.D : 1) * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(h->loglen, 0, (size_t)c.D * P * sizeof(double), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)cfg;
    return FFVD_OK;
}

extern "C" int ffvd_create(const ffvd_config *cfg, ffvd_handle **out) {
    if (!cfg || !out) return set_error(nullptr, FFVD_EINVAL, "ffvd_create: null argument");
    *out = nullptr;
    char msg[256];
    if (cfg->T < 1 || cfg->D < 1 || cfg->C < 0 || cfg->M < 1 || cfg->S_local < 1 || cfg->Ydim < 1) {
        snprintf(msg, sizeof msg, "ffvd_create: bad shape T=%d D=%d C=%d M=%d S_local=%d Ydim=%d", cfg->T, cfg->D,
                 cfg->C, cfg->M, cfg->S_local, cfg->Ydim);
        return set_error(nullptr, FFVD_EINVAL, msg);
    }
    if (cfg->D + cfg->C > MAXP) {
        snprintf(msg, sizeof msg, "ffvd_create: GP input dim P = D + C = %d exceeds %d", cfg->D + cfg->C, MAXP);
        return set_error(nullptr, FFVD_EINVAL, msg);
    }
    if (cfg->dtype != FFVD_F64 && cfg->dtype != FFVD_F32C) return set_error(nullptr, FFVD_EINVAL, "ffvd_create: unknown dtype");
    if (cfg->dtype == FFVD_F32C && (cfg->branch != FFVD_BRANCH_B || cfg->route != FFVD_ROUTE_REFERENCE))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: FFVD_F32C is the collapsed-U branch on FFVD_ROUTE_REFERENCE");
    if (cfg->kernel_kind != FFVD_KERNEL_SE && cfg->kernel_kind != FFVD_KERNEL_LINEAR)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: unknown kernel_kind");
    if (cfg->branch != FFVD_BRANCH_A && cfg->branch != FFVD_BRANCH_B)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: unknown branch");
    if (cfg->prior_type != FFVD_PRIOR_UNIFORM && cfg->prior_type != FFVD_PRIOR_NORMAL)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: unsupported prior_type (uniform / normal only)");
    const int dcount = cfg->d_count > 0 ? cfg->d_count : cfg->D;
    if (cfg->d_begin < 0 || cfg->d_begin + dcount > cfg->D)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: latent-dim shard [d_begin, d_begin + d_count) out of range");
    if (!(cfg->jitter >= 0.0)) return set_error(nullptr, FFVD_EINVAL, "ffvd_create: jitter must be >= 0");
    if (cfg->route != FFVD_ROUTE_REFERENCE && cfg->route != FFVD_ROUTE_GRAM)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: unknown route");
    if (cfg->grad && cfg->branch == FFVD_BRANCH_B && cfg->kernel_kind != FFVD_KERNEL_SE && cfg->dtype == FFVD_F32C)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: grad = 1 with fp32 contractions needs the SE kernel (the LinearK backward pass is fp64)");
    if (cfg->route == FFVD_ROUTE_GRAM && cfg->branch != FFVD_BRANCH_B)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: FFVD_ROUTE_GRAM only applies to the collapsed-U branch");
    if (cfg->T_total < 0 || cfg->t_begin < 0 || (cfg->T_total > 0 && cfg->t_begin + cfg->T > cfg->T_total))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: T-shard [t_begin, t_begin + T) outside [0, T_total)");
    if (cfg->T_total > 0 && (cfg->branch != FFVD_BRANCH_B || cfg->route != FFVD_ROUTE_GRAM || cfg->dtype != FFVD_F64))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: a T-shard (T_total > 0) is the collapsed-U branch on FFVD_ROUTE_GRAM in fp64");
    if (cfg->T_total > 0 && cfg->grad && (cfg->d_begin != 0 || (cfg->d_count > 0 && cfg->d_count != cfg->D)))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_create: grad = 1 on a T-shard needs every latent dim on the handle (T-shards and dim shards do not combine in the backward pass)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device_id < 0 || cfg->device_id >= ndev) {
        snprintf(msg, sizeof msg, "ffvd_create: device %d not available (%d HIP devices visible)", cfg->device_id, ndev);
        return set_error(nullptr, FFVD_EDEVICE, msg);
    }
    ffvd_handle *h = new (std::nothrow) ffvd_handle();
    if (!h) return set_error(nullptr, FFVD_ENOMEM, "ffvd_create: host allocation failed");
    h->cfg = *cfg;
    int rc = create_impl(cfg, h);
    if (rc != FFVD_OK) {
        std::string m = h->err;
        ffvd_destroy(h);
        return set_error(nullptr, rc, m);
    }
    *out = h;
    return FFVD_OK;
}

extern "C" int ffvd_sync(ffvd_handle *h) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_sync: null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->info_pending) {      // report what the _async forms could not: a failed factorisation (include/ffvd_abi.h)
        h->info_pending = false;
        HIP_TRY(hipMemcpyAsync(h->h_info, h->info, (size_t)(h->Dl + h->nbatch) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return check_info(h);
    }
    return FFVD_OK;
}

static int copy_in(ffvd_handle *h, double *dst, const double *src, size_t count, int on_device) {
    if (count == 0) return FFVD_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           h->stream));
    return FFVD_OK;
}

extern "C" int ffvd_set_data(ffvd_handle *h, const double *Y, const double *control_inputs, int on_device) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_set_data: null handle");
    const ffvd_config &c = h->cfg;
    if (!Y) return set_error(h, FFVD_EINVAL, "ffvd_set_data: Y is null");
    if (c.C > 0 && !control_inputs) return set_error(h, FFVD_EINVAL, "ffvd_set_data: control_inputs is null but C > 0");
    HIP_TRY(hipSetDevice(c.device_id));
    int rc;
    if ((rc = copy_in(h, h->Y, Y, (size_t)c.T * c.Ydim, on_device))) return rc;
    if ((rc = copy_in(h, h->ctrl, control_inputs, (size_t)c.T * c.C, on_device))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->have_data = true;
    return FFVD_OK;
}

static int check_params(ffvd_handle *h, const ffvd_params *p, const char *who) {
    const ffvd_config &c = h->cfg;
    std::string w(who);
    if (!p) return set_error(h, FFVD_EINVAL, w + ": params is null");
    if (!p->X || !p->Z || !p->logvariance || !p->log_Q || !p->CC || !p->DD || !p->log_Rchols)
        return set_error(h, FFVD_EINVAL, w + ": a required parameter pointer is null (X, Z, logvariance, log_Q, CC, DD, log_Rchols)");
    if (c.kernel_kind == FFVD_KERNEL_SE && !p->loglengthscales)
        return set_error(h, FFVD_EINVAL, w + ": loglengthscales is null for the SquaredExponential kernel");
    if (c.branch == FFVD_BRANCH_A && !p->U)
        return set_error(h, FFVD_EINVAL, w + ": U is null in the explicit-U branch");
    return FFVD_OK;
}

extern "C" int ffvd_set_params(ffvd_handle *h, const ffvd_params *p, int on_device) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_set_params: null handle");
    int rc = check_params(h, p, "ffvd_set_params");
    if (rc) return rc;
    const ffvd_config &c = h->cfg;
    const size_t P = h->P;
    HIP_TRY(hipSetDevice(c.device_id));
    if ((rc = copy_in(h, h->X, p->X, (size_t)c.S_local * (c.T + 1) * c.D, on_device))) return rc;
    if ((rc = copy_in(h, h->Z, p->Z, (size_t)c.M * P, on_device))) return rc;
    if (p->U && (rc = copy_in(h, h->U, p->U, (size_t)c.M * c.D, on_device))) return rc;
    if ((rc = copy_in(h, h->logvar, p->logvariance, (size_t)c.D, on_device))) return rc;
    if (p->loglengthscales && (rc = copy_in(h, h->loglen, p->loglengthscales, (size_t)c.D * P, on_device))) return rc;
    if ((rc = copy_in(h, h->logQ, p->log_Q, (size_t)c.D, on_device))) return rc;
    if ((rc = copy_in(h, h->CC, p->CC, (size_t)c.D * c.Ydim, on_device))) return rc;
    if ((rc = copy_in(h, h->DD, p->DD, (size_t)c.Ydim, on_device))) return rc;
    if ((rc = copy_in(h, h->logR, p->log_Rchols, (size_t)c.Ydim * c.Ydim, on_device))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cur.X = h->X; h->cur.Z = h->Z; h->cur.U = h->U; h->cur.logvariance = h->logvar;
    h->cur.loglengthscales = h->loglen; h->cur.log_Q = h->logQ; h->cur.CC = h->CC; h->cur.DD = h->DD;
    h->cur.log_Rchols = h->logR;
    h->have_params = true;
    return FFVD_OK;
}

// ---- the per-iteration launch sequence -------------------------------------------------------
// Stage timing: an event is recorded after each stage's launches; the interval ending at an event is
// attributed to that stage (stage -1 = origin of an iteration).  Events come from a pool owned by the handle.
struct StageTimer {
    ffvd_handle *h;
    void mark(int stage_id) {
        if (h->ev_used == h->ev_pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            h->ev_pool.push_back(e);
            h->ev_stage.push_back(0);
        }
        hipEventRecord(h->ev_pool[h->ev_used], h->stream);
        h->ev_stage[h->ev_used] = stage_id;
        ++h->ev_used;
    }
};

// ---- which schedule an iteration runs: EVERY flag in one place -------------------------------------------------------
// enqueue_elbo consumes these and computes none of its own; what it still tracks by itself is launch PROGRESS (which buffers a
// launch already produced: linv_done, kinv_done, hwords_zeroed, reduce_done ...).  The only run-time input besides the handle's
// constants is the Cholesky variant forced for the calling thread (stall recovery / FFVD_CHOL), through potrf_flow_selected.
struct ElboSchedule {
    bool gram_route, grad_a, grad_ref;
    bool lt_rows, lt_virtual;       // Gram-route training: L^T in the extension rows of A (read in place by the dataflow kernel)
    int first_units, ns_first;
    bool late_join;                 // split-K first pass: the K_uu chain only has to be back for the combine pass
    bool defer_trace;               //   ... one pass: the combine pass waits for the K_uu COPY only, trace partials follow on the side stream, and the
                                    //   main stream's K_fu build + tile pass are enqueued before the chain's launches
    bool defer_full;                // unsplit first pass beside the chain: raw tiles kept, trace pass on the side stream
    bool side_chain;                // Gram route: the K_uu chain runs on the side stream
    bool kuu_flow;                  //   ... as ONE dataflow launch resident before the K_fu build, joined before the Gram kernel
    bool kfu_first, ident_on_side;
    bool zt_rows, ref_side;         // explicit-U / reference route: the chain's dataflow launch beside the K_fu build
    bool side_late;                 // few chains: the side chain as one dataflow launch BEHIND the tile pass, trace partials and reductions behind it on the side stream
    bool small_side;                // tiny iteration on the multi-kernel path: the side chain as one dataflow launch, reductions on the main stream
    bool chain_flow_here;           // the chain is the dataflow launch on the stream that builds K_uu (the build zeroes its words)
    bool reduce_early;
    const char *name;
};
static ElboSchedule plan_schedule(const ffvd_handle *h) {
    const ffvd_config &c = h->cfg;
    const int Mp = h->Mp, Tp = h->Tp, Dl = h->Dl;
    ElboSchedule sc{};
    sc.gram_route = (c.branch == FFVD_BRANCH_B && c.route == FFVD_ROUTE_GRAM);
    sc.grad_a = c.grad && c.branch == FFVD_BRANCH_A;
    sc.grad_ref = c.grad && c.branch == FFVD_BRANCH_B && !sc.gram_route;
    sc.first_units = ((c.S_local < h->cpp) ? c.S_local : h->cpp) * Dl;
    sc.ns_first = (h->cpp <= c.S_local) ? h->cpp : c.S_local;
    sc.late_join = sc.gram_route && h->gpart && sc.first_units == h->cpp * Dl;
    sc.lt_rows = c.grad && sc.gram_route && h->gw.whitened && !h->sw.whiten_products;
    sc.lt_virtual = sc.lt_rows && !h->sw.lt_armed && potrf_flow_selected(Mp, h->nbatch, CHOL_FLOW);
    sc.defer_trace = sc.late_join && c.S_local <= h->cpp && !h->sw.no_defer_trace;
    sc.defer_full = sc.gram_route && !sc.late_join && h->graw;
    sc.zt_rows = h->lrpart != nullptr;
    sc.ref_side = !sc.gram_route && h->ngr > 0 && c.dtype != FFVD_F32C && h->aux &&
                  potrf_flow_selected(Mp, Dl, CHOL_FLOW);
    sc.side_chain = sc.gram_route && (sc.late_join || (size_t)sc.first_units * Tp * Mp >= (size_t)64 * 4096 * 512);
    sc.kuu_flow = sc.side_chain && h->kuu_flow_sched && !sc.late_join;
    sc.kfu_first = sc.side_chain && (sc.defer_trace || (sc.defer_full && !h->sw.no_kfu_first));
    sc.ident_on_side = sc.side_chain && c.grad && (sc.defer_full || sc.defer_trace) && !sc.lt_rows;
    const bool on_side = sc.ref_side || sc.side_chain;          // sk != s
    const bool kuu_on_main = sc.ref_side || sc.kuu_flow;        // K_uu is built (and its chain launched) before the common chain code
    sc.reduce_early = sc.gram_route && on_side;
    sc.small_side = sc.defer_trace && !c.grad && !kuu_on_main && on_side &&
                    (size_t)sc.first_units * h->ntiles * (h->gsplit > 1 ? h->gsplit : 1) <= (size_t)SMALL_SIDE_WGS &&
                    (size_t)Dl * 2 * (Mp / NB) <= (size_t)SMALL_SIDE_ROWS;
    // (Round 4, measured and not kept: at 8-16 chains the side chain -- a dozen dependent right-looking launches -- is starved of slots by
    //  the tile pass and its tail ends 0.14 ms behind Cholesky(A).  As ONE dataflow launch beside the K_fu build it holds its slots
    //  against the tile pass instead: that pass 1.43 instead of 1.18 ms at 16 chains, the iteration 1.91 either way; a main stream whose
    //  CU mask leaves 8-32 compute units to the side stream runs 1.2 x slower; `small_side` widened to these sizes: 1.19 vs 1.14 ms at 8.)
    sc.side_late = h->side_late && (sc.defer_trace || (sc.defer_full && sc.kfu_first)) && !kuu_on_main && on_side && !sc.small_side &&
                   potrf_flow_forms_inverse(Mp, Dl, CHOL_FLOW);            // (a forced launch-per-column Cholesky: the first-half schedule)
    sc.chain_flow_here = !kuu_on_main && (!on_side || sc.small_side || sc.side_late) && potrf_flow_selected(Mp, Dl, CHOL_FLOW);
    // invariants the launch code relies on (a violated one would be a silent wrong answer, not a crash)
    if ((sc.defer_full && sc.late_join) || (sc.defer_trace && !sc.late_join) || (sc.kuu_flow && sc.defer_full) || (sc.small_side && sc.kuu_flow) ||
        (sc.side_late && (sc.small_side || !(sc.defer_trace || sc.defer_full) || !sc.chain_flow_here)) ||
        (sc.ref_side && sc.side_chain) || (sc.kuu_flow && h->graw))
        sc.name = nullptr;
    else if (!sc.gram_route) sc.name = sc.ref_side ? "projection route, K_uu chain as one dataflow launch on the side stream beside the K_fu build"
                                                   : "projection route, serial (K_uu chain on the main stream)";
    else if (sc.kuu_flow) sc.name = "full unsplit: K_uu chain as one dataflow launch beside the K_fu build, joined before the Gram kernel";
    else if (sc.side_late && sc.defer_full) sc.name = "side late: unsplit pass with raw tiles, the K_uu chain as one dataflow launch behind it beside Cholesky(A), trace pass behind the chain";
    else if (sc.defer_full && sc.side_chain) sc.name = "unsplit with raw tiles: K_uu chain beside K_fu build and Gram kernel, trace pass on the side stream, joined at finalize";
    else if (sc.side_late) sc.name = "side late: split-K one pass filling the chip, the K_uu chain as one dataflow launch behind it beside Cholesky(A), trace partials behind the chain";
    else if (sc.small_side) sc.name = "small side: split-K one pass, side chain as one dataflow launch, reductions and trace partials on the main stream";
    else if (sc.defer_trace) sc.name = "split-K one pass, late join: combine waits for the K_uu copy, trace partials on the side stream";
    else if (sc.late_join) sc.name = "split-K several passes: the first combine pass waits for the whole chain";
    else sc.name = "serial: K_uu chain on the main stream in front of the K_fu build";
    return sc;
}
extern "C" const char *ffvd_schedule_name(const ffvd_handle *h) {
    if (!h) return "";
    if (h->stall_hold > 0) return "stall back-off: multi-kernel schedule with the launch-per-column Cholesky (no inter-workgroup waits) until the next probe";
    if (h->tiny.ok && potrf_override_current() == CHOL_FORCE_NONE) return "one launch (tiny.hip)";
    const ElboSchedule sc = plan_schedule(h);
    return sc.name ? sc.name : "INVALID";
}

// Fork the side stream off the main stream.  Diagnostic switches (schedule tests): a spin kernel at the head of the side stream
// (FFVD_DEBUG_SIDE_DELAY_US) and / or of the main stream behind the fork (FFVD_DEBUG_MAIN_DELAY_US) -- results must not change.
int ffvd::fork_side(ffvd_handle *h, hipEvent_t ev, hipStream_t from, hipStream_t to) {
    HIP_TRY(hipEventRecord(ev, from));
    HIP_TRY(hipStreamWaitEvent(to, ev, 0));
    if (h->sw.side_delay_us > 0) launch_spin(to, h->sw.side_delay_us);
    if (h->sw.main_delay_us > 0) launch_spin(from, h->sw.main_delay_us);
    return FFVD_OK;
}

// The iteration (with_grad: and its backward pass, gradients scaled by 1 / S_total into the arrays of gw) as ONE launch: tiny.hip.
static bool tiny_selected(const ffvd_handle *h) { return h->tiny.ok && potrf_override_current() == CHOL_FORCE_NONE; }
static int enqueue_tiny(ffvd_handle *h, double *out_dev, StageTimer *st, bool with_grad, int S_total) {
    StageTimer live{h};
    if (!st && h->timing_on) st = &live;
    const ffvd_config &c = h->cfg;
    const ffvd_params &p = h->cur;
    hipStream_t s = h->stream;
    if (st) st->mark(-1);
    if (h->tiny_dirty) {
        HIP_TRY(hipMemsetAsync(h->tiny_flags, 0, tiny_flag_ints(h->tiny, c.S_local) * sizeof(int), s));
        h->tiny_dirty = false;
    }
    TinyArgs a;
    memset(&a, 0, sizeof a);        // padding included: the block is compared bytewise with what the device copy holds (launch_tiny)
    a.kind = c.kernel_kind; a.T = c.T; a.D = c.D; a.C = c.C; a.P = h->P; a.M = c.M; a.Dl = h->Dl; a.d_begin = c.d_begin;
    a.S = c.S_local; a.Ydim = c.Ydim; a.prior_type = c.prior_type; a.shared_terms = c.shared_terms;
    a.grad = with_grad ? 1 : 0; a.S_total = S_total; a.jitter = c.jitter;
    a.branch = (c.branch == FFVD_BRANCH_B) ? 1 : 0; a.U = p.U;
    a.X = p.X; a.Z = p.Z; a.logvar = p.logvariance; a.loglen = p.loglengthscales; a.log_Q = p.log_Q; a.CC = p.CC; a.DD = p.DD;
    a.logR = p.log_Rchols; a.Y = h->Y; a.ctrl = h->ctrl;
    tiny_bind_scratch(a, h->tiny, h->tiny_scratch, h->tiny_flags);
    {   // all workgroups of a unit on one XCD when the padded grid (8 x ceil(units / 8) unit slots) still fits the chip
        const int wpu = 1 + h->tiny.nstrips + (a.side ? h->tiny.NT : 0);
        a.xcd_map = (8 * wpu * ((h->tiny.nunits + 7) / 8) <= h->tiny_cus) ? 1 : 0;
    }
    a.info = h->info; a.chain_nll = h->chain_nll; a.out_terms = out_dev ? out_dev : h->out_terms;
    if (with_grad) {
        const ffvd_handle::GradWs &g = h->gw;
        a.dX = g.dX; a.dZ = g.dZ; a.dlogvar = g.dlogvar; a.dloglen = g.dloglen; a.dlogQ = g.dlogQ; a.dCC = g.dCC; a.dDD = g.dDD;
        a.dlogR = g.dlogR; a.dU = g.dU;
    }
    HIP_TRY(launch_tiny(s, a, h->tiny, h->tiny_dargs + (with_grad ? 1 : 0), h->tiny_ring[with_grad ? 1 : 0]));
    if (st) { st->mark(2); st->mark(4); }
    DBG_SYNC(h, with_grad ? "one-launch iteration + backward pass" : "one-launch iteration");
    return FFVD_OK;
}


// ---- argument blocks of the forward iteration's launches: one builder each, shared by every schedule --------------------------------
static ProjectArgs elbo_project_args(const ffvd_handle *h, const HyperView &hv, int s0, int ns, bool gram_route) {
    const ffvd_config &c = h->cfg;
    const ffvd_params &p = h->cur;
    const size_t msq = (size_t)h->Mp * h->Mp, kstride = 2 * msq;
    ProjectArgs pa{};
    pa.kind = c.kernel_kind;
    pa.x = p.X; pa.x_chain_stride = (size_t)(c.T + 1) * c.D; pa.x_ld = c.D; pa.x_cols = c.D;
    pa.ctrl = h->ctrl; pa.T = c.T; pa.Tp = h->Tp; pa.C = c.C; pa.P = h->P; pa.M = c.M; pa.Mp = h->Mp; pa.Dl = h->Dl;
    pa.d_begin = c.d_begin; pa.hv = hv; pa.W = h->Kuu + msq; pa.w_stride = kstride;
    pa.U = p.U; pa.u_ld = c.D; pa.b0 = s0 * h->Dl; pa.nb = ns * h->Dl;
    pa.F = (c.branch == FFVD_BRANCH_B) ? h->F : nullptr;
    pa.rowsq = h->rowsq;
    pa.fmean = (c.branch == FFVD_BRANCH_A) ? h->fmean : nullptr;
    pa.ng = h->ng;
    pa.gpart = gram_route ? h->growpart : nullptr;      // Gram route: delta^T K_fu is summed where K_fu is made
    return pa;
}
static size_t elbo_h_stride(const ffvd_handle *h) { return (size_t)(h->cfg.grad ? 2 * h->Mp + NB : h->Mp + NB) * h->Mp; }
static GramArgs elbo_gram_args(const ffvd_handle *h, int s0, int ns, bool gram_route) {
    const ffvd_config &c = h->cfg;
    const ffvd_params &p = h->cur;
    const int Mp = h->Mp;
    const size_t msq = (size_t)Mp * Mp;
    GramArgs ga{};
    ga.mode = gram_route ? GRAM_KFU : GRAM_F;
    ga.A = h->F; ga.a_stride = (size_t)h->Tp * Mp; ga.rows = h->Tp; ga.with_row = h->growpart ? 0 : 1;
    ga.X = p.X; ga.log_Q = p.log_Q; ga.T = c.T; ga.D = c.D; ga.Mp = Mp; ga.Dl = h->Dl;
    ga.d_begin = c.d_begin; ga.b0 = s0 * h->Dl; ga.nb = ns * h->Dl; ga.yn_over_batch = 1.0;
    ga.H = h->H; ga.h_stride = elbo_h_stride(h);
    if (c.grad) ga.brow = 2 * Mp;   // rows [Mp, 2Mp) hold I (they become L_A^-T), the b row moves to 2 Mp
    ga.Kadd = h->Kcopy; ga.kadd_stride = msq; ga.Kinv = h->Kinv; ga.kinv_stride = msq; ga.trpart = h->trpart;
    if (h->gpart) { ga.ksplit = h->gsplit; ga.part = h->gpart; }     // same row ranges in every pass of this handle
    // tail split of the last partial round (full passes only: launch_gram drops it when the unit count differs)
    if (h->gtail) { ga.tail_wg = h->gtail_wg; ga.tail_part = h->gtail; }
    return ga;
}
static ReduceArgs elbo_reduce_args(const ffvd_handle *h, bool gram_route) {
    const ffvd_config &c = h->cfg;
    const ffvd_params &p = h->cur;
    ReduceArgs ra{};
    ra.kind = c.kernel_kind; ra.branch = c.branch; ra.X = p.X; ra.ctrl = h->ctrl; ra.Y = h->Y;
    ra.log_Q = p.log_Q; ra.CC = p.CC; ra.DD = p.DD; ra.log_Rchols = p.log_Rchols; ra.variance = h->variance;
    ra.T = c.T; ra.Tp = h->Tp; ra.D = c.D; ra.C = c.C; ra.Ydim = c.Ydim; ra.Dl = h->Dl; ra.d_begin = c.d_begin;
    ra.S = c.S_local; ra.ng = h->ng; ra.shared_terms = c.shared_terms;
    ra.xk = p.X; ra.xk_chain_stride = (size_t)(c.T + 1) * c.D; ra.xk_ld = c.D; ra.xk_cols = c.D;
    ra.rowsq = (gram_route || c.dtype == FFVD_F32C) ? nullptr : h->rowsq; ra.fmean = h->fmean; ra.chain_terms = h->chain_terms;
    if (h->ngr) ra.ng = h->ngr;
    if (h->lrpart) ra.ng = 1;            // LinearK through its rank: one value per (unit, row)
    return ra;
}
// (trpart / ntiles / fsq_from_trpart of the fp32-contraction path and `whitened` of the training forward are set by the caller)
static FinalizeArgs elbo_finalize_args(const ffvd_handle *h, double *out_dev, bool gram_route) {
    const ffvd_config &c = h->cfg;
    const ffvd_params &p = h->cur;
    FinalizeArgs fa{};
    fa.kind = c.kernel_kind; fa.branch = c.branch; fa.prior_type = c.prior_type; fa.shared_terms = c.shared_terms;
    fa.T = c.T; fa.D = c.D; fa.P = h->P; fa.M = c.M; fa.Ydim = c.Ydim; fa.Dl = h->Dl; fa.d_begin = c.d_begin;
    fa.S = c.S_local; fa.Z = p.Z; fa.U = p.U; fa.logvar = p.logvariance; fa.loglen = p.loglengthscales;
    fa.log_Q = p.log_Q; fa.CC = p.CC; fa.DD = p.DD; fa.log_Rchols = p.log_Rchols;
    fa.chain_terms = h->chain_terms; fa.hterms = h->hterms; fa.chain_nll = h->chain_nll;
    fa.route = gram_route ? 1 : 0; fa.kterms = h->kterms; fa.trpart = h->trpart; fa.ntiles = h->ntiles;
    fa.out_terms = out_dev ? out_dev : h->out_terms;
    fa.info = h->info; fa.ninfo = h->Dl + h->nbatch;       // any failed / abandoned factorisation of this rank -> NaN sums on every rank
    return fa;
}


// ---- the multi-kernel forward iteration, phase by phase -------------------------------------------------------
// enqueue_elbo used to be one 425-line function; it is now the sequence below, each phase a function of its own over one context.
// The SCHEDULE is sc (plan_schedule: every flag decided in one place, named, checked); the context only adds launch PROGRESS -- which
// buffers a launch has produced so far -- and the two streams.  Launch order is exactly what it was: results are bit-identical.
//
// Event graphs of the named schedules (M = main stream, S = side stream; "->e" records, "e->" waits):
//   full unsplit (kuu_flow)   M: prep, K_uu build ->fork | reductions | go-> build(K_fu), brow | join-> Gram | hwords-> Chol(A), finish | finalize
//                             S: fork-> clear ->go | chain (one dataflow launch: L, L^-1, K^-1) | clear H words ->hwords | log|K| ->join
//   unsplit + raw tiles       M: prep ->fork | build, brow | kuu-> Gram(raw) ->tiles | Chol(A) | join2-> finalize
//   (defer_full)              S: fork-> K_uu build ->kuu | chain (launches) | K^-1, log|K| ->join | reductions | tiles-> trace pass ->join2
//   split-K one pass          M: prep ->fork | build, brow, tile pass ->tiles | kuu-> combine (no trace) | Chol(A) | join2-> finalize
//   (defer_trace)             S: fork-> K_uu build ->kuu | chain | K^-1, log|K| ->join | reductions | tiles-> trace partials ->join2
//   side late                 as the two above, but the chain is ONE dataflow launch enqueued behind the tile pass (tiles-> chain), the
//                             reductions in front of it, the trace pass behind it
//   small side                split-K one pass with the chain as one dataflow launch; reductions and trace partials on M (join-> trace)
//   split-K several passes    M: ... tile pass | join-> combine with trace | Chol(A) ... per pass
//   projection route, side    M: prep, K_uu build ->fork | go-> build | join-> projection GEMM, brow | Gram | Chol(H) | reductions, finalize
//   (ref_side)                S: fork-> clear ->go | chain (dataflow) | [K^-1, log|K| for a backward pass] ->join
//   serial                    everything on M in dependence order.
struct FwdCtx {
    ffvd_handle *h;
    double *out_dev;
    StageTimer *st;
    ElboSchedule sc;
    HyperView hv;
    hipStream_t s, sk;              // main stream; the stream that carries the K_uu chain (= s while nothing runs beside the main stream)
    size_t msq, kstride;
    ReduceArgs ra;
    // launch progress, not schedule
    bool kuu_on_main = false;       // K_uu is built (and its chain launched) before the common chain code
    bool linv_done = false;         // L^-1 comes / came out of the factorisation itself
    bool kinv_done = false;         // K^-1 came out of the chain's dataflow launch (no product launch)
    bool hwords_zeroed = false;     // Cholesky(A)'s progress words were cleared on the side stream (ev_hwords)
    bool ident_early = false;       // training: the identity rows of the first pass were re-armed early on the main stream
    bool reduce_done = false, reduce_launched = false, trace_on_main = false;
    bool chain_deferred = false;    // the chain is enqueued behind the first pass's Gram launch
    int prior_early = 0;            // the parameter-only sums of the assembly were formed early: 1 on the main stream, 2 on the side stream (ev_prior)

    ProjectArgs project_args(int s0, int ns) const { return elbo_project_args(h, hv, s0, ns, sc.gram_route); }
    GramArgs gram_args(int s0, int ns) const { return elbo_gram_args(h, s0, ns, sc.gram_route); }
    // Gram route: the row b = delta^T K_fu / Q of a pass, from the partial sums its K_fu build left behind (kernels.h ProjectArgs::gpart)
    void brow_finish(int s0, int ns) const {
        if (!h->growpart) return;
        const ffvd_config &c = h->cfg;
        launch_brow_finish(s, h->growpart, h->Tp / 64, h->Mp, h->Dl, c.d_begin, s0 * h->Dl, ns * h->Dl, h->cur.log_Q, 1.0, h->H,
                           elbo_h_stride(h), c.grad ? 2 * h->Mp : h->Mp);
    }
};

// The ten parameter-only sums of the nll assembly (priors, log R, log sqrt Q: finalize_priors) are a function of the parameters alone:
// formed EARLY they leave the finalize launch at the iteration's tail -- one workgroup, a chain of dependent loads -- with the
// per-chain assembly only (19 -> 9 us of every forward iteration's tail; the same code, the same bits).  Where: on the main stream
// inside its wait for the chain's kernel (full-batch and projection-route schedules), or as the side stream's first launch where
// that stream idles at the start (few-chain schedules); schedules without a slack window keep them in the finalize launch.
static int fwd_prior_sums(FwdCtx &x, hipStream_t stream) {
    ffvd_handle *h = x.h;
    if (x.prior_early) return FFVD_OK;
    launch_prior_sums(stream, elbo_finalize_args(h, x.out_dev, x.sc.gram_route), h->prior_sums);
    if (stream != x.s) {
        HIP_TRY(hipEventRecord(h->ev_prior, stream));
        x.prior_early = 2;
    } else x.prior_early = 1;
    return FFVD_OK;
}

// Projection route / explicit-U branch on the projection GEMM (fp64): only the GEMM needs the chain's W = L^-T, the K_fu build does
// not -- the chain's dataflow launch goes to the side stream (resident before the build floods the chip) and the main stream waits
// for it in front of the first projection GEMM: config 2 in the reference's op order 6.31 -> 6.05 ms.  LinearK through its rank
// (zt_rows): the chain carries Z^T instead of the identity rows.
static int fwd_chain_ref_side(FwdCtx &x) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const int Mp = h->Mp, Dl = h->Dl;
    const bool zt_rows = x.sc.zt_rows, wants_linv = x.sc.grad_a || x.sc.grad_ref;
    x.sk = h->aux;
    launch_kuu_build(x.s, c.kernel_kind, x.hv, c.M, Mp, h->P, Dl, c.jitter, h->Kuu, wants_linv ? h->Kcopy : nullptr, zt_rows);
    { int rcf = fork_side(h, h->ev_fork, x.s, x.sk); if (rcf) return rcf; }
    potrf_flow_clear(x.sk, h->dinvK, Dl);
    HIP_TRY(hipEventRecord(h->ev_go, x.sk));
    x.linv_done = wants_linv;
    launch_potrf_ext(x.sk, h->Kuu, Mp, zt_rows ? NB : Mp, zt_rows ? 0 : Mp, Dl, x.kstride, h->info, h->dinvK, CHOL_FLOW,
                     x.linv_done ? h->Linv : nullptr, x.msq, true);
    { int rcp = fwd_prior_sums(x, x.s); if (rcp) return rcp; }      // (fills the main stream's wait below)
    HIP_TRY(hipStreamWaitEvent(x.s, h->ev_go, 0));
    x.kuu_on_main = true;          // (built and factorised: fwd_chain_rest adds K^-1 / log|K| where a backward pass wants them)
    return FFVD_OK;
}

// Gram route: nothing of the K_fu build depends on K_uu, so the latency-bound K_uu chain runs on the side stream.  This is the fork
// and whatever the schedule wants on either stream BEFORE the chain's own launches (fwd_chain_rest): the full-batch schedule's
// dataflow chain and the work that fills the main stream's wait for it; the first pass's K_fu build / tile pass when the main
// stream is the critical one (kfu_first, defer_trace); the identity rows of a training pass on the side stream.
static int fwd_chain_fork(FwdCtx &x) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const ElboSchedule &sc = x.sc;
    const int Mp = h->Mp, Dl = h->Dl;
    hipStream_t s = x.s;
    x.sk = h->aux;
    hipStream_t sk = x.sk;
    x.kuu_on_main = sc.kuu_flow;
    if (x.kuu_on_main)
        launch_kuu_build(s, c.kernel_kind, x.hv, c.M, Mp, h->P, Dl, c.jitter, h->Kuu, h->Kcopy);
    { int rcf = fork_side(h, h->ev_fork, s, sk); if (rcf) return rcf; }
    if (!x.kuu_on_main && !sc.small_side) { int rcp = fwd_prior_sums(x, sk); if (rcp) return rcp; }      // (the side stream idles here; small side: its chain is the critical path)
    if (x.kuu_on_main) {
        HIP_TRY(hipEventRecord(h->ev_kuu, s));
        x.linv_done = potrf_flow_selected(Mp, Dl, CHOL_FLOW);      // L^-1 comes out of the factorisation itself
        if (x.linv_done) {
            // The chain's 64-odd row workgroups (76.8 KB of LDS, 256 VGPRs) must be on the chip BEFORE the K_fu build
            // floods it with small ones, or they wait for that kernel to drain: the main stream resumes one
            // cross-queue hop after the clear that sits directly in front of the chain's kernel
            potrf_flow_clear(sk, h->dinvK, Dl);
            HIP_TRY(hipEventRecord(h->ev_go, sk));
        }
        x.kinv_done = x.linv_done && potrf_flow_forms_inverse(Mp, Dl, CHOL_FLOW);
        launch_potrf_ext(sk, h->Kuu, Mp, Mp, Mp, Dl, x.kstride, h->info, h->dinvK, CHOL_FLOW, h->Linv, x.msq, x.linv_done, false,
                         x.kinv_done ? h->Kinv : nullptr, x.msq);
        if (x.linv_done) {
            launch_chain_reduce(s, x.ra, h->chain_partial);      // inputs only; fills the wait below
            x.reduce_done = true;
            { int rcp = fwd_prior_sums(x, s); if (rcp) return rcp; }      // (likewise)
            if (c.grad && c.branch == FFVD_BRANCH_B && !sc.lt_rows) {
                // training: the identity rows that become L_A^-T are re-armed here too (rows the K_fu build and the Gram
                // kernel do not touch) instead of between the K_fu build and the Gram kernel
                const GramArgs gi = x.gram_args(0, sc.ns_first);
                launch_set_identity(s, h->H, gi.h_stride, Mp, Mp, sc.ns_first * Dl);
                x.ident_early = true;
            }
            HIP_TRY(hipStreamWaitEvent(s, h->ev_go, 0));
            if (c.S_local <= h->cpp) {          // single pass: the words of Cholesky(A) are cleared here, off the main stream
                potrf_flow_clear(sk, h->dinvH, h->nbatch);
                HIP_TRY(hipEventRecord(h->ev_hwords, sk));      // the factorisation that trusts this clear waits for THIS event
                x.hwords_zeroed = true;
            }
        }
    }
    if (sc.kfu_first) {         // the first pass's K_fu build goes to the main stream before the chain is enqueued
        if (x.st) x.st->mark(0);
        launch_kfu_build(s, x.project_args(0, sc.ns_first));
        x.brow_finish(0, sc.ns_first);
        if (x.st) x.st->mark(1);
    }
    if (sc.defer_trace) {       // ... and so does the split-K tile pass (it needs neither K_uu nor K^-1)
        const GramArgs ga = x.gram_args(0, c.S_local);
        launch_gram(s, ga, 1);
        HIP_TRY(hipEventRecord(h->ev_tiles, s));
    }
    // training: the identity rows that become L_A^-T are re-armed on the side stream, ahead of the K_uu build whose
    // event the main stream waits for anyway (0.05 ms off the critical path at the full batch)
    if (sc.ident_on_side) {
        const GramArgs ga = x.gram_args(0, sc.ns_first);
        launch_set_identity(sk, h->H, ga.h_stride, Mp, Mp, sc.ns_first * Dl);
    }
    return FFVD_OK;
}

// The K_uu chain's own launches on x.sk (unless the prelude already enqueued its factorisation): Cholesky with the L^-T rows, then --
// Gram route and backward passes -- K^-1 = L^-T L^-1 and log|K|, the join event, and the per-chain reductions where they ride behind
// the chain.
static int fwd_chain_rest(FwdCtx &x) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const ElboSchedule &sc = x.sc;
    const int Mp = h->Mp, Dl = h->Dl;
    hipStream_t s = x.s, sk = x.sk;
    const size_t msq = x.msq, kstride = x.kstride;
    const bool zt_rows = sc.zt_rows, needs_inverse = sc.gram_route || sc.grad_a || sc.grad_ref;
    if (!x.kuu_on_main) {
        // chain on the main stream = on the critical path with nothing beside it: the dataflow launch; on the side stream
        // (beside the K_fu build / tile pass of a small batch) the right-looking launches, whose workgroups come and go
        const bool chain_flow = sc.chain_flow_here;
        if (chain_flow && needs_inverse) x.linv_done = true;
        if (chain_flow && (sc.small_side || sc.side_late) && sc.gram_route && potrf_flow_forms_inverse(Mp, Dl, CHOL_FLOW)) x.kinv_done = true;
        if (sc.side_late) {
            // the reductions of the inputs first (they need nothing), then the chain once the tile pass has left the chip
            if (sc.reduce_early && !x.reduce_done) { launch_chain_reduce(sk, x.ra, h->chain_partial); x.reduce_launched = true; }
            HIP_TRY(hipStreamWaitEvent(sk, h->ev_tiles, 0));
        }
        launch_potrf_ext(sk, h->Kuu, Mp, zt_rows ? NB : Mp, zt_rows ? 0 : Mp, Dl, kstride, h->info, h->dinvK,
                         chain_flow ? CHOL_FLOW : CHOL_AUTO, x.linv_done ? h->Linv : nullptr, msq, chain_flow /* words zeroed by the build */,
                         false, x.kinv_done ? h->Kinv : nullptr, msq, nullptr, 0, 1, sc.small_side || sc.side_late);
    }
    if (needs_inverse) {
        // K^-1 = L^-T L^-1 (shared by all chains) and log|K|
        if (!x.linv_done) launch_transpose(sk, h->Kuu + msq, kstride, h->Linv, msq, Mp, Dl);
        GramArgs gk{};
        gk.mode = GRAM_PLAIN; gk.A = h->Linv; gk.a_stride = msq; gk.rows = Mp; gk.with_row = 0; gk.Mp = Mp; gk.Dl = Dl;
        gk.d_begin = c.d_begin; gk.b0 = 0; gk.nb = Dl; gk.yn_over_batch = 1.0; gk.H = h->Kinv; gk.h_stride = msq;
        if (x.kinv_done) {
            // (the identity-row workgroups of the chain's launch have formed it: potrf_flow.hip, df_inverse_tiles)
        } else if (c.grad || x.kuu_on_main) {
            // the backward pass reads K^-1 everywhere, the Gram kernel only writes lower tiles; and beside the K_fu build
            // (kuu_on_main: the main stream waits for this product) 256-thread workgroups find a slot where the Gram
            // kernel's 1024-thread ones wait for the build to drain (0.19 against 0.05 ms)
            AtbArgs ak{};
            ak.mode = ATB_PLAIN; ak.A = h->Linv; ak.a_stride = msq; ak.lda = Mp; ak.nA = Mp; ak.B = h->Linv; ak.b_stride = msq;
            ak.ldb = Mp; ak.nB = Mp; ak.rows = Mp; ak.C = h->Kinv; ak.c_stride = msq; ak.ldc = Mp; ak.nb = Dl; ak.Dl = Dl;
            ak.k_lower = 1;                                  // L^-1 is lower triangular
            ak.small_tiles = x.kuu_on_main ? 1 : 0;
            launch_atb(sk, ak);
        } else launch_gram(sk, gk);     // (split-K here was measured slower: 0.42 vs 0.37 ms for the K_uu stage)
        launch_h_finish(sk, h->Kuu, Mp, kstride, Dl, h->kterms);
        if (sk != s) HIP_TRY(hipEventRecord(h->ev_join, sk));
    } else if (sc.ref_side) HIP_TRY(hipEventRecord(h->ev_join, sk));
    // the per-chain likelihood / transition reductions depend on the inputs only (Gram route: no row sums of F), so
    // they ride on the side stream behind the K_uu chain and are back long before finalize needs them (kuu_on_main: they
    // already ran on the main stream while it waited for the chain's kernel to be dispatched)
    if (sc.reduce_early && !x.reduce_done && !sc.small_side /* reductions on the main stream */ && !x.reduce_launched) {
        launch_chain_reduce(sk, x.ra, h->chain_partial);
        HIP_TRY(hipEventRecord(h->ev_join2, sk));
    }
    return FFVD_OK;
}

// K(X_combine, Z) of one pass and what turns it into the pass's F / fmean / row sums: five forms, by route, branch and arithmetic.
static int fwd_pass_project(FwdCtx &x, int s0, int ns) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const ElboSchedule &sc = x.sc;
    const ffvd_params &p = h->cur;
    const int Mp = h->Mp, Tp = h->Tp, Dl = h->Dl;
    hipStream_t s = x.s, sk = x.sk;
    const size_t msq = x.msq, kstride = x.kstride;
    ProjectArgs pa = x.project_args(s0, ns);
    if (sc.gram_route) {
        if (!(sc.kfu_first && s0 == 0)) { launch_kfu_build(s, pa); x.brow_finish(s0, ns); }
        if (s0 == 0 && sk != s && !sc.late_join) HIP_TRY(hipStreamWaitEvent(s, sc.defer_full ? h->ev_kuu : h->ev_join, 0));
    } else if (c.dtype == FFVD_F32C) {
        if (s0 == 0) launch_linv_f32(s, h->Kuu + msq, kstride, h->Linv32, Mp, Dl);     // L^-1 as the fp32 B operand
        launch_kfu_build_f32(s, pa, h->Kf32);                     // K(X_combine, Z)           (:240)
        ProjF32Args pg{};
        pg.Kf = h->Kf32; pg.kf_stride = (size_t)Tp * Mp; pg.LinvT = h->Linv32; pg.F = h->F32; pg.f_stride = (size_t)Tp * Mp;
        pg.sqpart = h->sqpart; pg.Tp = Tp; pg.Mp = Mp; pg.Dl = Dl; pg.b0 = s0 * Dl; pg.nb = ns * Dl;
        launch_proj_gemm_f32(s, pg);                              // tilde_F = Knm Lm^-T, sum F^2  (:242,:255)
    } else if (h->ngr && c.branch == FFVD_BRANCH_B) {
        pa.F = h->Kf2;
        launch_kfu_build(s, pa);                                  // K(X_combine, Z)           (:240)
        ProjGemmArgs pg{};
        pg.Kf = h->Kf2; pg.kf_stride = (size_t)Tp * Mp; pg.W = h->Kuu + msq; pg.w_stride = kstride;
        pg.F = h->F; pg.f_stride = (size_t)Tp * Mp; pg.rowsq = h->rowsq; pg.Tp = Tp; pg.Mp = Mp; pg.Dl = Dl;
        pg.b0 = s0 * Dl; pg.nb = ns * Dl;
        pg.gpart = h->growpart; pg.X = p.X; pg.T = c.T; pg.D = c.D; pg.d_begin = c.d_begin;      // delta^T F by 128-row tiles (:247-248)
        if (sc.ref_side && s0 == 0) HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));               // W = L^-T from the side stream's chain
        launch_proj_gemm(s, pg);                                  // tilde_F = Knm Lm^-T, sum F^2  (:242,:255)
        if (h->growpart)
            launch_brow_finish(s, h->growpart, (int)((Tp + 127) / 128), Mp, Dl, c.d_begin, s0 * Dl, ns * Dl, p.log_Q, 1.0, h->H,
                               elbo_h_stride(h), c.grad ? 2 * Mp : Mp);
    } else if (h->lrpart) {
        // explicit-U branch, LinearK, forward only: fmean and sum_j F^2 through the kernel's rank P (no K_fu, no F)
        if (sk != s && s0 == 0) HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
        launch_linear_lowrank(s, pa, h->lrpart);
    } else if (c.branch == FFVD_BRANCH_A && h->ngr) {
        // explicit-U branch: K_fu once, then the triangular GEMM with fvar / fmean folded into its epilogue (F unstored)
        pa.F = h->F + (sc.grad_a ? (size_t)s0 * Dl * Tp * Mp : 0);
        launch_kfu_build(s, pa);
        if (sc.ref_side && s0 == 0) HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));               // W = L^-T from the side stream's chain
        if (s0 == 0) launch_ucols(s, p.U, c.M, Mp, c.D, c.d_begin, Dl, h->ucolA);
        ProjGemmArgs pg{};
        pg.Kf = pa.F; pg.kf_stride = (size_t)Tp * Mp; pg.W = h->Kuu + msq; pg.w_stride = kstride;
        pg.F = nullptr; pg.f_stride = 0; pg.rowsq = h->rowsq; pg.fmean = h->fmean; pg.u = h->ucolA; pg.u_stride = Mp;
        pg.Tp = Tp; pg.Mp = Mp; pg.Dl = Dl; pg.b0 = s0 * Dl; pg.nb = ns * Dl;
        launch_proj_gemm(s, pg);
    } else {
        if (sc.grad_a) {                    // (FFVD_FUSED_PROJECT) the backward pass still needs K_fu itself
            pa.F = h->F;
            launch_kfu_build(s, pa);
            pa.F = nullptr;
        }
        launch_project(s, pa);
    }
    if (x.st && !(sc.kfu_first && s0 == 0)) x.st->mark(1);
    DBG_SYNC(h, "forward: K_fu / projection");
    return FFVD_OK;
}

// H = F^T F / Q + I (projection route) or A = K_uu + K_uf K_fu / Q (Gram route) of one pass: the tile pass + combine of a split-K
// launch, the unsplit launch with raw tiles beside the chain, the fp32 product, or the plain unsplit launch.
static int fwd_pass_gram(FwdCtx &x, int s0, int ns, GramArgs &ga, bool &trace_pending, bool &acopy_done) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const ElboSchedule &sc = x.sc;
    const ffvd_params &p = h->cur;
    const int Mp = h->Mp, Tp = h->Tp, Dl = h->Dl;
    hipStream_t s = x.s, sk = x.sk;
    if (sc.lt_rows) {
        // (armed right in front of the factorisation, when at all: L comes from the K_uu chain)
    } else if (c.grad && !((sc.ident_on_side || x.ident_early) && s0 == 0)) launch_set_identity(s, h->H, ga.h_stride, Mp, Mp, ns * Dl);
    if (s0 == 0 && sc.late_join) {
        if (!sc.defer_trace) launch_gram(s, ga, 1);
        if (sc.defer_trace) {
            if (!sc.defer_trace) HIP_TRY(hipEventRecord(h->ev_tiles, s));
            HIP_TRY(hipStreamWaitEvent(s, h->ev_kuu, 0));
            ga.trace_mode = 1;
            // side late: the trace pass runs long after this one (behind the K_uu chain) -- it reads the summed raw tiles this
            // pass leaves in partial 0 instead of all the row ranges again (134 MB at 4 chains: 20-27 us of the iteration's tail)
            ga.raw_summed = (sc.side_late || sc.small_side) ? 1 : 0;      // (small side: the trace pass follows on this stream)
            launch_gram(s, ga, 2);
            if (sc.side_late) HIP_TRY(hipEventRecord(h->ev_tiles, s));      // (the trace pass waits for THIS record)
            trace_pending = true;      // enqueued behind the factorisation: the main stream is the critical one
        } else {
            HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
            launch_gram(s, ga, 2);
        }
    } else if (s0 == 0 && sc.defer_full && sk != s) {
        ga.mode = GRAM_KFU_RAW; ga.part = h->graw; ga.ksplit = 1;
        if (c.grad) { ga.Hcopy = h->gw.Acopy; ga.hcopy_stride = x.msq; acopy_done = true; }
        launch_gram(s, ga);
        HIP_TRY(hipEventRecord(h->ev_tiles, s));
        trace_pending = true;
    } else if (c.dtype == FFVD_F32C) {
        GramF32Args gf{};
        gf.F = h->F32; gf.f_stride = (size_t)Tp * Mp; gf.rows = Tp; gf.with_row = 1; gf.brow = c.grad ? 2 * Mp : Mp;
        gf.X = p.X; gf.log_Q = p.log_Q; gf.T = c.T; gf.D = c.D; gf.Mp = Mp; gf.Dl = Dl; gf.d_begin = c.d_begin;
        gf.b0 = s0 * Dl; gf.nb = ns * Dl; gf.yn_over_batch = 1.0; gf.H = h->H; gf.h_stride = ga.h_stride;
        gf.flush = F32C_FLUSH_TILES;
        launch_gram_f32(s, gf);                               // H = F^T F / Q + I, b = delta^T F / Q  (:246-248)
    } else {
        // training: the unsplit Gram kernel stores the symmetric copy of A itself (no copy + symmetrize launches: 0.25 ms)
        if (c.grad && sc.gram_route && !ga.part) { ga.Hcopy = h->gw.Acopy; ga.hcopy_stride = x.msq; acopy_done = true; }
        launch_gram(s, ga);
    }
    if (x.st) x.st->mark(2);
    DBG_SYNC(h, "forward: Gram");
    return FFVD_OK;
}

// Gram-route training without L^T rows (FFVD_GRAD_WHITEN_PRODUCTS): H = W^T A W (W = L^-T of K_uu) replaces A in the slab, b = W^T c
// replaces c: the factorisation, the explicit inverse and everything the backward pass derives from them then live in the whitened
// variables, where cond(H) is about 1e4 instead of the 1e7 of A
static int fwd_whiten_products(FwdCtx &x, int ns, const GramArgs &ga) {
    ffvd_handle *h = x.h;
    ffvd_handle::GradWs &g = h->gw;
    const int Mp = h->Mp, Dl = h->Dl, nbp = ns * Dl;
    const size_t msq = x.msq, kstride = x.kstride;
    hipStream_t s = x.s;
    if (x.sk != s) HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));       // W and L^-1 come from the K_uu chain
    launch_symmetrize(s, g.Acopy, Mp, nbp);                            // (the saved copy holds the lower triangle)
    AtbArgs t1{};
    t1.mode = ATB_PLAIN; t1.A = g.Acopy; t1.a_stride = msq; t1.lda = Mp; t1.nA = Mp;
    t1.B = h->Kuu + msq; t1.b_stride = kstride; t1.ldb = Mp; t1.nB = Mp; t1.b_per_dim = 1; t1.rows = Mp;
    t1.C = g.T1; t1.c_stride = msq; t1.ldc = Mp; t1.nb = nbp; t1.Dl = Dl; t1.krange = 8; t1.small_tiles = 1;      // W upper triangular
    launch_atb(s, t1);                                                  // T1 = A W
    AtbArgs t2{};
    t2.mode = ATB_PLAIN; t2.A = h->Kuu + msq; t2.a_stride = kstride; t2.lda = Mp; t2.nA = Mp; t2.a_per_dim = 1;
    t2.B = g.T1; t2.b_stride = msq; t2.ldb = Mp; t2.nB = Mp; t2.rows = Mp;
    t2.C = h->H; t2.c_stride = ga.h_stride; t2.ldc = Mp; t2.nb = nbp; t2.Dl = Dl; t2.krange = 4; t2.sym = 1; t2.small_tiles = 1;
    launch_atb(s, t2);                                                  // H = W^T T1 into rows [0, Mp)
    launch_matvec(s, h->Linv, msq, h->H + 2 * msq, ga.h_stride, Mp, g.bw, 1, Mp, Mp, nbp, Dl);   // b = W^T c
    HIP_TRY(hipMemcpy2DAsync(h->H + 2 * msq, ga.h_stride * sizeof(double), g.bw, (size_t)Mp * sizeof(double),
                             (size_t)Mp * sizeof(double), (size_t)nbp, hipMemcpyDeviceToDevice, s));
    return FFVD_OK;
}

// Cholesky of the pass's H / A slabs (one dataflow launch, the row b as a vector; training: with the L^T / identity rows), log|.| and
// the quadratic term; in front of it the trace pass on the side stream where the schedule defers it, behind it the trace pass /
// reductions of the small-side schedule.
static int fwd_pass_factor(FwdCtx &x, int s0, int ns, GramArgs &ga, bool &trace_pending, const bool acopy_done) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const ElboSchedule &sc = x.sc;
    const int Mp = h->Mp, Dl = h->Dl;
    hipStream_t s = x.s, sk = x.sk;
    const size_t msq = x.msq, kstride = x.kstride;
    int rc;
    if (trace_pending && sc.small_side) {
        // tiny iteration: the trace partials wait for the chain on the MAIN stream, behind Cholesky(A) -- one cross-stream
        // hop (chain -> here) instead of two (tile pass -> side stream, side stream -> finalize)
        x.trace_on_main = true;
    } else if (trace_pending) {
        if (x.chain_deferred && s0 == 0 && (rc = fwd_chain_rest(x)) != FFVD_OK) return rc;      // (waits for ev_tiles itself)
        // trace partials from the raw tiles, on the side stream (K^-1 precedes in its order).  Enqueued AHEAD of the
        // factorisation: that is one launch whose row workgroups hold every slot of the chip for most of its length,
        // and a kernel that arrives behind it only starts when they leave (finalize then waited 0.26 ms for this pass)
        HIP_TRY(hipStreamWaitEvent(sk, h->ev_tiles, 0));
        launch_gram(sk, ga, 3);
        HIP_TRY(hipEventRecord(h->ev_join2, sk));                 // supersedes the record after the reductions
        trace_pending = false;
    }
    const bool words = x.hwords_zeroed && s0 == 0;
    if (c.grad) {       // keep A = K_uu + K_uf K_fu / Q: the factorisation overwrites it in place
        if (!acopy_done)
            HIP_TRY(hipMemcpy2DAsync(h->gw.Acopy, msq * sizeof(double), h->H, ga.h_stride * sizeof(double),
                                     msq * sizeof(double), (size_t)ns * Dl, hipMemcpyDeviceToDevice, s));
        if (sc.lt_rows) {
            if (sk != s && s0 == 0) HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));       // L (and W, L^-1 for the backward pass) come from the K_uu chain
            if (!sc.lt_virtual) launch_set_lt_rows(s, h->Kuu, kstride, Dl, h->H, ga.h_stride, Mp, Mp, ns * Dl);
        } else if (h->gw.whitened && sc.gram_route) {
            if ((rc = fwd_whiten_products(x, ns, ga)) != FFVD_OK) return rc;
        }
        if (words) HIP_TRY(hipStreamWaitEvent(s, h->ev_hwords, 0));      // the side-stream clear of these words
        launch_potrf_ext(s, h->H, Mp, Mp + NB, Mp, ns * Dl, ga.h_stride, h->info + Dl + s0 * Dl, h->dinvH, CHOL_FLOW, nullptr, 0,
                         words, true, nullptr, 0, sc.lt_virtual ? h->Kuu : nullptr, kstride, Dl);
        launch_h_finish(s, h->H, Mp, ga.h_stride, ns * Dl, h->hterms + (size_t)2 * s0 * Dl, 2 * Mp);
    } else {
        if (words) HIP_TRY(hipStreamWaitEvent(s, h->ev_hwords, 0));      // the side-stream clear of these words
        launch_potrf_ext(s, h->H, Mp, NB, 0, ns * Dl, ga.h_stride, h->info + Dl + s0 * Dl, h->dinvH, CHOL_FLOW, nullptr, 0, words, true);
        launch_h_finish(s, h->H, Mp, ga.h_stride, ns * Dl, h->hterms + (size_t)2 * s0 * Dl);
    }
    if (sc.small_side && !x.reduce_launched) { launch_chain_reduce(s, x.ra, h->chain_partial); x.reduce_launched = true; }
    if (trace_pending && x.trace_on_main) {
        HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
        launch_gram(s, ga, 3);
        trace_pending = false;
    }
    if (x.st) x.st->mark(3);
    DBG_SYNC(h, "forward: Cholesky(H) + solves");
    return FFVD_OK;
}

// the per-chain reductions where nothing ran them early, the join with the side stream, the nll assembly
static int fwd_finalize(FwdCtx &x) {
    ffvd_handle *h = x.h;
    const ffvd_config &c = h->cfg;
    const ElboSchedule &sc = x.sc;
    hipStream_t s = x.s;
    if (!sc.reduce_early) launch_chain_reduce(s, x.ra, h->chain_partial);
    else if (!x.reduce_done && !x.trace_on_main) HIP_TRY(hipStreamWaitEvent(s, h->ev_join2, 0));
    FinalizeArgs fa = elbo_finalize_args(h, x.out_dev, sc.gram_route);
    if (x.prior_early) {
        if (x.prior_early == 2) HIP_TRY(hipStreamWaitEvent(s, h->ev_prior, 0));
        fa.prior_sums = h->prior_sums;
    }
    fa.whitened = (c.grad && h->gw.whitened && sc.gram_route && !sc.lt_rows) ? 1 : 0;      // L^T rows: the slab holds the factor of A itself
    if (c.dtype == FFVD_F32C) {           // sum_t |F_t|^2 per unit from the projection's fp64 tile sums
        launch_sum_partials(s, h->sqpart, h->nsq, h->nbatch, h->sqsum);
        fa.trpart = h->sqsum; fa.ntiles = 1; fa.fsq_from_trpart = 1;
    } else if (sc.grad_ref)               // the backward pass wants the same per-unit sum (dl/dalpha): all row sums of F^2 of a unit
        launch_sum_partials(s, h->rowsq, h->ngr * h->Tp, h->nbatch, h->gw.fsq);
    launch_finalize(s, fa);
    if (x.st) x.st->mark(4);
    DBG_SYNC(h, "forward: reductions + finalize");
    HIP_TRY(hipGetLastError());
    return FFVD_OK;
}

static int enqueue_elbo(ffvd_handle *h, double *out_dev, StageTimer *st) {
    if (tiny_selected(h)) return enqueue_tiny(h, out_dev, st, false, h->cfg.S_local);
    StageTimer live{h};
    if (!st && h->timing_on) st = &live;
    const ffvd_config &c = h->cfg;
    const ffvd_params &p = h->cur;
    const int Mp = h->Mp, Dl = h->Dl;
    if (st) st->mark(-1);
    launch_prep_hypers(h->stream, c.kernel_kind, p.Z, c.M, Mp, h->P, Dl, c.d_begin, p.logvariance, p.loglengthscales,
                       h->variance, h->len, h->Zs, h->zz, h->info, Dl + h->nbatch);
    FwdCtx x{};
    x.h = h; x.out_dev = out_dev; x.st = st;
    x.sc = plan_schedule(h);
    if (!x.sc.name) return set_error(h, FFVD_EINVAL, "internal: inconsistent schedule flags (plan_schedule)");
    x.hv = HyperView{h->variance, h->len, h->Zs, h->zz};
    x.s = h->stream; x.sk = h->stream;
    x.msq = (size_t)Mp * Mp; x.kstride = 2 * x.msq;
    x.ra = elbo_reduce_args(h, x.sc.gram_route);
    const ElboSchedule &sc = x.sc;
    int rc;
    // ---- the K_uu chain: where it runs, what is enqueued around it ----
    if (sc.ref_side && (rc = fwd_chain_ref_side(x)) != FFVD_OK) return rc;
    if (sc.side_chain && (rc = fwd_chain_fork(x)) != FFVD_OK) return rc;
    if (!x.kuu_on_main) {
        launch_kuu_build(x.sk, c.kernel_kind, x.hv, c.M, Mp, h->P, Dl, c.jitter, h->Kuu,
                         (sc.gram_route || sc.grad_a || sc.grad_ref) ? h->Kcopy : nullptr, sc.zt_rows, sc.chain_flow_here ? h->dinvK : nullptr);
        if (sc.defer_trace || (sc.defer_full && x.sk != x.s)) HIP_TRY(hipEventRecord(h->ev_kuu, x.sk));
    }
    x.chain_deferred = sc.side_late && sc.defer_full;       // the chain is enqueued behind the first pass's Gram launch (fwd_pass_factor)
    if (!x.chain_deferred && (rc = fwd_chain_rest(x)) != FFVD_OK) return rc;
    DBG_SYNC(h, "forward: K_uu chain");
    if (st && !sc.kfu_first) st->mark(0);
    // ---- the passes over the chains: projection / K_fu, Gram, factorisation ----
    for (int s0 = 0; s0 < c.S_local; s0 += h->cpp) {
        const int ns = (s0 + h->cpp <= c.S_local) ? h->cpp : c.S_local - s0;
        if ((rc = fwd_pass_project(x, s0, ns)) != FFVD_OK) return rc;
        if (c.branch != FFVD_BRANCH_B) continue;
        GramArgs ga = x.gram_args(s0, ns);
        bool trace_pending = false, acopy_done = false;      // acopy_done: the Gram kernel stored the copy of A itself
        if ((rc = fwd_pass_gram(x, s0, ns, ga, trace_pending, acopy_done)) != FFVD_OK) return rc;
        if ((rc = fwd_pass_factor(x, s0, ns, ga, trace_pending, acopy_done)) != FFVD_OK) return rc;
    }
    return fwd_finalize(x);
}

int ffvd::ready(ffvd_handle *h, const char *who) {
    if (!h->have_data) return set_error(h, FFVD_EINVAL, std::string(who) + ": call ffvd_set_data first");
    if (!h->have_params) return set_error(h, FFVD_EINVAL, std::string(who) + ": no parameters bound (ffvd_set_params or pass params)");
    return FFVD_OK;
}

int ffvd::check_info(ffvd_handle *h) {
    const int Dl = h->Dl;
    h->stalled = false;
    for (int i = 0; i < Dl + h->nbatch; ++i) {
        if (h->h_info[i] < 0) {        // the dataflow Cholesky bounds every wait (potrf_flow.hip, potrf_df_kernel); so does tiny.hip
            h->stalled = true;
            h->tiny_dirty = true;
            return set_error(h, FFVD_EDEVICE, "blocked Cholesky abandoned: a block row waited more than 1 s for the row above it");
        }
        if (h->h_info[i] != 0) {
            char msg[256];
            if (i < Dl)
                snprintf(msg, sizeof msg, "Cholesky of K_uu + jitter*I failed: latent dim %d, pivot %d is not positive",
                         h->cfg.d_begin + i, h->h_info[i] - 1);
            else
                snprintf(msg, sizeof msg, "Cholesky of H failed: chain %d, latent dim %d, pivot %d is not positive",
                         (i - Dl) / Dl, h->cfg.d_begin + (i - Dl) % Dl, h->h_info[i] - 1);
            return set_error(h, FFVD_ENOTPD, msg);
        }
    }
    return FFVD_OK;
}

int ffvd::check_finite(ffvd_handle *h, const double *sums, int n, const char *who, const char *what) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(sums[i])) return set_error(h, FFVD_ENOTPD, std::string(who) + ": non-finite " + what);
    return FFVD_OK;
}

// Stall recovery (VERDICT r2 W10 / ADVICE r2): the dataflow Cholesky's forward progress rests on in-order workgroup dispatch; its
// waits are bounded, and when one fires (info = -1) the whole launch is abandoned.  The iteration is a pure function of resident
// inputs, so it is simply enqueued AGAIN, once, in this process, with the left-looking launch-per-column Cholesky, which has no
// inter-workgroup waits (every launch re-zeroes what it needs; the dataflow launches of later iterations clear their own words).
// A second failure is reported as FFVD_EDEVICE.  The first recovery leaves a note for ffvd_last_error.  Collective entry points
// (ffvd_elbo_allreduce, ffvd_*_step_allreduce, T-shards) do NOT retry: the other ranks have already moved on.
// (The override is reset by CholOverrideGuard, abi_internal.h.)

// A stall is remembered.  The one-launch iteration and the dataflow Cholesky need every workgroup resident at once; a
// co-tenant that keeps compute units busy makes EVERY call wait out its bounded spin (1 s) before the recovery runs -- FFVD_OK each
// time, an hour of waiting over the 4000 outer iterations of FFVD_Main.py.  So after a recovery the handle stays on the schedule without
// inter-workgroup waits (launch-per-column Cholesky, multi-kernel iteration) for `stall_hold` calls, then probes the fast path again;
// a probe that stalls doubles the hold (16, 32, ... 1024 calls), one that succeeds resets it.  ffvd_schedule_name reports the state.
static constexpr int STALL_HOLD_FIRST = 16, STALL_HOLD_MAX = 1024;

template <class Enqueue>
static int fetch_with_stall_recovery(ffvd_handle *h, Enqueue enqueue) {
    int rc;
    const bool held = h->stall_hold > 0;        // back-off: this call does not try the paths that stalled
    if (held) --h->stall_hold;
    for (int attempt = held ? 1 : 0;; ++attempt) {
        {
            CholOverrideGuard guard;
            if (attempt == 1) guard.force_left();
            const auto t0 = std::chrono::steady_clock::now();
            rc = enqueue();
            h->enq_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            ++h->enq_calls;
        }
        if (rc) return rc;
        hipError_t e1 = hipMemcpyAsync(h->h_res, h->resblk, h->res_bytes, hipMemcpyDeviceToHost, h->stream);      // terms, chain nll, info flags
        hipError_t e2 = (e1 == hipSuccess) ? hipStreamSynchronize(h->stream) : e1;
        if (e2 != hipSuccess) return set_error(h, FFVD_EDEVICE, std::string("result copy failed: ") + hipGetErrorString(e2));
        rc = check_info(h);
        if (rc == FFVD_OK && attempt == 1 && !held) {
            if (h->stall_recoveries++ == 0)
                h->warning = "warning: the one-launch (dataflow) Cholesky gave up on a bounded wait; the iteration was re-run with "
                             "the launch-per-column Cholesky and completed";
            h->err = h->warning;
            h->stall_hold = h->stall_hold_next;
            h->stall_hold_next = std::min(2 * h->stall_hold_next, STALL_HOLD_MAX);
        } else if (rc == FFVD_OK && attempt == 0 && h->stall_hold_next != STALL_HOLD_FIRST) {
            h->stall_hold_next = STALL_HOLD_FIRST;      // the fast path ran through again: forget the history
        }
        if (!(rc == FFVD_EDEVICE && h->stalled && attempt == 0)) return rc;
    }
}

extern "C" int ffvd_stall_recoveries(const ffvd_handle *h) { return h ? h->stall_recoveries : 0; }
extern "C" int ffvd_stall_hold(const ffvd_handle *h) { return h ? h->stall_hold : 0; }

// Debug (tools/sync_step.py): average host time of one iteration's enqueue in microseconds, -1 before the first call.
extern "C" double ffvd_debug_enqueue_us(const ffvd_handle *h) {
    return (h && h->enq_calls > 0) ? (double)h->enq_ns / (double)h->enq_calls * 1e-3 : -1.0;
}

extern "C" int ffvd_single_launch(const ffvd_handle *h) { return (h && h->tiny.ok) ? h->tiny.nw : 0; }
// Debug / tests: scratch bytes per lane of the one-launch kernel (0 when the shape has no one-launch plan); how often the argument
// block of the forward (which = 0) / forward + backward (1) launch travelled to the device.
extern "C" int64_t ffvd_debug_tiny_private_bytes(const ffvd_handle *h) { return h ? (int64_t)h->tiny_private_bytes : 0; }
extern "C" int ffvd_debug_tiny_uploads(const ffvd_handle *h, int which) {
    return (h && h->tiny_ring_made && (which == 0 || which == 1)) ? h->tiny_ring[which].uploads : 0;
}

// Debug: copy `count` doubles of the one-launch path's scratch block, starting at `offset`, to the host (tools only).
extern "C" int64_t ffvd_debug_tiny_scratch(ffvd_handle *h, int64_t offset, int64_t count, double *out) {
    if (!h || !h->tiny.ok) return -1;
    const ffvd_config &c = h->cfg;
    const int64_t total = (int64_t)tiny_scratch_doubles(h->tiny, c.T, h->P, c.M, c.S_local, h->Dl, c.D, c.Ydim, c.grad);
    if (!out) return total;
    if (offset < 0 || offset + count > total) return -1;
    hipStreamSynchronize(h->stream);
    return hipMemcpy(out, h->tiny_scratch + offset, (size_t)count * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? total : -1;
}

extern "C" int ffvd_elbo(ffvd_handle *h, const ffvd_params *p, uint32_t flags, double out_terms[8], double *out_nll) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_elbo: null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    int rc;
    if (p) {
        if (flags & FFVD_PARAMS_ON_DEVICE) {
            if ((rc = check_params(h, p, "ffvd_elbo"))) return rc;
            h->cur = *p;
            if (!h->cur.U) h->cur.U = h->U;
            if (!h->cur.loglengthscales) h->cur.loglengthscales = h->loglen;
            h->have_params = true;
        } else if ((rc = ffvd_set_params(h, p, 0))) return rc;
    }
    if ((rc = ready(h, "ffvd_elbo"))) return rc;
    if ((rc = fetch_with_stall_recovery(h, [&] { return enqueue_elbo(h, nullptr, nullptr); }))) return rc;
    report_local(h, out_terms, out_nll);
    return FFVD_OK;
}

extern "C" int ffvd_elbo_async(ffvd_handle *h, double *out_terms_dev) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_elbo_async: null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    int rc;
    if ((rc = ready(h, "ffvd_elbo_async"))) return rc;
    h->info_pending = true;
    return enqueue_elbo(h, out_terms_dev, nullptr);
}

extern "C" void *ffvd_get_stream(ffvd_handle *h) { return h ? (void *)h->stream : nullptr; }

extern "C" int ffvd_chain_nll(ffvd_handle *h, double *out) {
    if (!h || !out) return set_error(h, FFVD_EINVAL, "ffvd_chain_nll: null argument");
    memcpy(out, h->h_chain, (size_t)h->cfg.S_local * sizeof(double));
    return FFVD_OK;
}

extern "C" int ffvd_time_elbo(ffvd_handle *h, int iters, float *out_ms) {
    if (!h || !out_ms || iters < 1) return set_error(h, FFVD_EINVAL, "ffvd_time_elbo: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    int rc;
    if ((rc = ready(h, "ffvd_time_elbo"))) return rc;
    struct EventPair {          // destroyed on every exit path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~EventPair() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    HIP_TRY(hipEventRecord(ev.e0, h->stream));
    for (int i = 0; i < iters; ++i)
        if ((rc = enqueue_elbo(h, nullptr, nullptr))) return rc;
    HIP_TRY(hipEventRecord(ev.e1, h->stream));
    HIP_TRY(hipMemcpyAsync(h->h_info, h->info, (size_t)(h->Dl + h->nbatch) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipEventElapsedTime(out_ms, ev.e0, ev.e1));
    return check_info(h);
}

static void drain_stage_times(ffvd_handle *h, double ms[8], int32_t n[8]) {
    for (int i = 0; i < 8; ++i) { ms[i] = 0.0; n[i] = 0; }
    for (size_t i = 1; i < h->ev_used; ++i) {
        const int st = h->ev_stage[i];
        if (st < 0 || st >= 8) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, h->ev_pool[i - 1], h->ev_pool[i]) == hipSuccess) { ms[st] += t; ++n[st]; }
    }
    h->ev_used = 0;
}

extern "C" int ffvd_profile_stages(ffvd_handle *h, float out_ms[8]) {
    if (!h || !out_ms) return set_error(h, FFVD_EINVAL, "ffvd_profile_stages: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    int rc;
    if ((rc = ready(h, "ffvd_profile_stages"))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->ev_used = 0;
    StageTimer st{h};
    if ((rc = enqueue_elbo(h, nullptr, &st))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    double ms[8];
    int32_t n[8];
    drain_stage_times(h, ms, n);
    for (int i = 0; i < 8; ++i) out_ms[i] = (float)ms[i];
    return FFVD_OK;
}

extern "C" int ffvd_stage_timing(ffvd_handle *h, int enable) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_stage_timing: null handle");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->timing_on = enable != 0;
    h->ev_used = 0;
    return FFVD_OK;
}

extern "C" int ffvd_stage_times(ffvd_handle *h, double out_ms[8], int32_t out_launches[8]) {
    if (!h || !out_ms || !out_launches) return set_error(h, FFVD_EINVAL, "ffvd_stage_times: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    HIP_TRY(hipStreamSynchronize(h->stream));
    drain_stage_times(h, out_ms, out_launches);
    return FFVD_OK;
}

// ---- backward pass: backward.hip (enqueue_grad, copy_grads_out); it runs on the handle's streams right behind the forward kernels ----------
// forward + backward pass of one training iteration: ONE launch where the handle has the small-problem plan (tiny.hip)
int ffvd::enqueue_forward_backward(ffvd_handle *h, int S_total) {
    if (h->cfg.grad && tiny_selected(h)) return enqueue_tiny(h, nullptr, nullptr, true, S_total);
    const int r = enqueue_elbo(h, nullptr, nullptr);
    return r ? r : enqueue_grad(h, S_total);
}
int ffvd::run_forward_backward(ffvd_handle *h, int S_total) {
    return fetch_with_stall_recovery(h, [&] { return enqueue_forward_backward(h, S_total); });
}

extern "C" int ffvd_elbo_grad(ffvd_handle *h, const ffvd_params *p, uint32_t flags, int S_total, double out_terms[8],
                              double *out_nll, const ffvd_grads *gout) {
    if (!h) return set_error(nullptr, FFVD_EINVAL, "ffvd_elbo_grad: null handle");
    if (!h->cfg.grad) return set_error(h, FFVD_EINVAL, "ffvd_elbo_grad: the handle was created without grad = 1");
    if (!gout) return set_error(h, FFVD_EINVAL, "ffvd_elbo_grad: null gradient struct");
    if (S_total < h->cfg.S_local) return set_error(h, FFVD_EINVAL, "ffvd_elbo_grad: S_total < S_local");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    int rc;
    if (p) {
        if (flags & FFVD_PARAMS_ON_DEVICE) {
            if ((rc = check_params(h, p, "ffvd_elbo_grad"))) return rc;
            h->cur = *p;
            if (!h->cur.U) h->cur.U = h->U;
            if (!h->cur.loglengthscales) h->cur.loglengthscales = h->loglen;
            h->have_params = true;
        } else if ((rc = ffvd_set_params(h, p, 0))) return rc;
    }
    if ((rc = ready(h, "ffvd_elbo_grad"))) return rc;
    if ((rc = run_forward_backward(h, S_total))) return rc;
    if ((rc = copy_grads_out(h, gout))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    report_local(h, out_terms, out_nll);
    return FFVD_OK;
}

// ffvd_get_params / ffvd_update_params: the bound arrays to / from the host arrays of `host` (NULL = skip), complete on return
static int copy_params(ffvd_handle *h, const ffvd_params *host, hipMemcpyKind kind) {
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    for (int i = 0; i < NPARAM; ++i) {
        double *dev = const_cast<double *>(h->cur.*PARAM_MEMBER[i]), *hp = const_cast<double *>(host->*PARAM_MEMBER[i]);
        const bool out = kind == hipMemcpyDeviceToHost;
        if (dev && hp && param_count(h, i))
            HIP_TRY(hipMemcpyAsync(out ? hp : dev, out ? dev : hp, param_count(h, i) * sizeof(double), kind, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FFVD_OK;
}

extern "C" int ffvd_get_params(ffvd_handle *h, const ffvd_params *out) {
    if (!h || !out) return set_error(h, FFVD_EINVAL, "ffvd_get_params: null argument");
    if (!h->have_params) return set_error(h, FFVD_EINVAL, "ffvd_get_params: no parameters bound");
    return copy_params(h, out, hipMemcpyDeviceToHost);
}

// ffvd_update_params: overwrite some of the bound parameter arrays from host memory (NULL = keep).
extern "C" int ffvd_update_params(ffvd_handle *h, const ffvd_params *p) {
    if (!h || !p) return set_error(h, FFVD_EINVAL, "ffvd_update_params: null argument");
    if (!h->have_params) return set_error(h, FFVD_EINVAL, "ffvd_update_params: no parameters bound yet (ffvd_set_params)");
    return copy_params(h, p, hipMemcpyHostToDevice);
}

// ---- T-shard fallback (include/ffvd_abi.h "T-shard"): the two launch sequences; entry points in train.hip ------------------
// this shard's rows: raw Gram tiles K_uf K_fu + delta^T K_fu rows into the exchange buffer, likelihood / transition /
// trace sums into its tail.  The K_uu chain (identical on every rank) runs first on the same stream.
int ffvd::enqueue_tshard_local(ffvd_handle *h) {
    const ffvd_config &c = h->cfg;
    const int Mp = h->Mp, Tp = h->Tp, Dl = h->Dl, P = h->P;
    hipStream_t s = h->stream;
    const ffvd_params &p = h->cur;
    const size_t msq = (size_t)Mp * Mp, kstride = 2 * msq;
    launch_prep_hypers(s, c.kernel_kind, p.Z, c.M, Mp, P, Dl, c.d_begin, p.logvariance, p.loglengthscales, h->variance, h->len,
                       h->Zs, h->zz, h->info, Dl + h->nbatch);
    HyperView hv{h->variance, h->len, h->Zs, h->zz};
    launch_kuu_build(s, c.kernel_kind, hv, c.M, Mp, P, Dl, c.jitter, h->Kuu, h->Kcopy);
    launch_potrf_ext(s, h->Kuu, Mp, Mp, Mp, Dl, kstride, h->info, h->dinvK);
    launch_transpose(s, h->Kuu + msq, kstride, h->Linv, msq, Mp, Dl);
    GramArgs gk{};
    gk.mode = GRAM_PLAIN; gk.A = h->Linv; gk.a_stride = msq; gk.rows = Mp; gk.with_row = 0; gk.Mp = Mp; gk.Dl = Dl;
    gk.d_begin = c.d_begin; gk.b0 = 0; gk.nb = Dl; gk.yn_over_batch = 1.0; gk.H = h->Kinv; gk.h_stride = msq;
    launch_gram(s, gk);                                                     // K^-1 = L^-T L^-1
    launch_h_finish(s, h->Kuu, Mp, kstride, Dl, h->kterms);                 // log|K|
    launch_kfu_build(s, elbo_project_args(h, hv, 0, c.S_local, true));     // (a T-shard has no growpart: the row comes from the Gram launch)
    GramArgs gr{};
    gr.mode = GRAM_PLAIN; gr.A = h->F; gr.a_stride = (size_t)Tp * Mp; gr.rows = Tp; gr.with_row = 1; gr.brow = Mp;
    gr.X = p.X; gr.log_Q = p.log_Q; gr.T = c.T; gr.D = c.D; gr.Mp = Mp; gr.Dl = Dl; gr.d_begin = c.d_begin; gr.b0 = 0;
    gr.nb = h->nbatch; gr.yn_over_batch = 1.0; gr.H = h->tsbuf; gr.h_stride = (size_t)(Mp + 1) * Mp;
    if (h->gpart) { gr.ksplit = h->gsplit; gr.part = h->gpart; }
    launch_gram(s, gr);                                                     // raw sum over this shard's rows
    ReduceArgs ra = elbo_reduce_args(h, true);
    ra.skip_x0 = c.t_begin > 0;
    ra.info = h->info; ra.ninfo = Dl;       // a failed / abandoned K_uu chain of THIS shard turns its chain sums into NaN: they are part of the exchange
    launch_chain_reduce(s, ra, h->chain_partial);
    HIP_TRY(hipGetLastError());
    return FFVD_OK;
}

// on the all-reduced sums: A = K_uu + K_uf K_fu / Q, the trace partials, Cholesky(A), the solve, the assembly
int ffvd::enqueue_tshard_finish(ffvd_handle *h) {
    const ffvd_config &c = h->cfg;
    const int Mp = h->Mp, Dl = h->Dl;
    hipStream_t s = h->stream;
    const ffvd_params &p = h->cur;
    const size_t msq = (size_t)Mp * Mp;
    GramArgs ga{};
    ga.mode = GRAM_KFU; ga.rows = h->Tp; ga.with_row = 1; ga.brow = Mp;
    ga.X = p.X; ga.log_Q = p.log_Q; ga.T = c.T; ga.D = c.D; ga.Mp = Mp; ga.Dl = Dl; ga.d_begin = c.d_begin; ga.b0 = 0;
    ga.nb = h->nbatch; ga.yn_over_batch = 1.0; ga.H = h->H; ga.h_stride = (size_t)(Mp + NB) * Mp;
    ga.Kadd = h->Kcopy; ga.kadd_stride = msq; ga.Kinv = h->Kinv; ga.kinv_stride = msq; ga.trpart = h->trpart;
    ga.part = h->tsbuf; ga.ksplit = 1;
    if (c.grad) {
        // training forward (round 4: T-shards have a backward pass): the slab keeps Mp extension rows in front of the b row -- L^T there,
        // so that the factorisation of A leaves L_H^-T and y = L_A^-1 c, exactly what enqueue_grad_b reads -- and
        // A itself is saved before it is overwritten
        ga.brow = 2 * Mp; ga.h_stride = (size_t)(2 * Mp + NB) * Mp;
        launch_gram(s, ga, 4);
        HIP_TRY(hipMemcpy2DAsync(h->gw.Acopy, msq * sizeof(double), h->H, ga.h_stride * sizeof(double), msq * sizeof(double),
                                 (size_t)h->nbatch, hipMemcpyDeviceToDevice, s));
        // (FFVD_GRAD_EXPLICIT: identity rows instead, the factorisation then leaves L_A^-T -- the unwhitened form of the backward pass)
        const bool lt_virtual = h->gw.whitened && !h->sw.lt_armed && potrf_flow_selected(Mp, h->nbatch, CHOL_FLOW);
        if (!h->gw.whitened) launch_set_identity(s, h->H, ga.h_stride, Mp, Mp, h->nbatch);
        else if (!lt_virtual) launch_set_lt_rows(s, h->Kuu, (size_t)2 * msq, Dl, h->H, ga.h_stride, Mp, Mp, h->nbatch);
        launch_potrf_ext(s, h->H, Mp, Mp + NB, Mp, h->nbatch, ga.h_stride, h->info + Dl, h->dinvH, CHOL_FLOW, nullptr, 0, false, true,
                         nullptr, 0, lt_virtual ? h->Kuu : nullptr, (size_t)2 * msq, Dl);
        launch_h_finish(s, h->H, Mp, ga.h_stride, h->nbatch, h->hterms, 2 * Mp);
    } else {
        launch_gram(s, ga, 4);
        launch_potrf_ext(s, h->H, Mp, NB, 0, h->nbatch, ga.h_stride, h->info + Dl, h->dinvH, CHOL_FLOW, nullptr, 0, false, true);
        launch_h_finish(s, h->H, Mp, ga.h_stride, h->nbatch, h->hterms);
    }
    FinalizeArgs fa = elbo_finalize_args(h, nullptr, true);
    fa.T = c.T_total;                                   // every /T of dgp_model.py:261-297 is the whole job's
    launch_finalize(s, fa);
    HIP_TRY(hipGetLastError());
    return FFVD_OK;
}
