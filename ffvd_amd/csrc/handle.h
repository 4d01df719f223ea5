// The handle behind the C ABI and what the sources that see inside it share: abi.hip (lifetime, the forward iteration), backward.hip
// (the multi-kernel backward pass), train.hip (optimiser steps, shards) and comm.hip (RCCL).  The operator sources (ops*.hip) and every other source keep the
// opaque type.
#pragma once
#include "abi_internal.h"
#include "tiny.h"

#include <cstring>
#include <string>
#include <vector>

struct ffvd_handle {
    ffvd_config cfg;
    int P = 0, Mp = 0, Tp = 0, Dl = 0, nbatch = 0, ng = 0, cpp = 0;
    hipStream_t stream = nullptr;
    double *dinvK = nullptr, *dinvH = nullptr;   // Cholesky scratch (kernels.h DINV_STRIDE per matrix)
    double *gpart = nullptr;                     // split-K partial tiles of the Gram kernel (few units per pass)
    int gsplit = 1;
    bool side_late = false;     // few chains, forward: the K_uu side chain as ONE dataflow launch BEHIND the tile pass (plan_schedule); decided with gsplit at create
    double *graw = nullptr;                      // unsplit first pass: raw Gram tiles for the deferred trace pass
    double *gtail = nullptr;                     // unsplit passes: blocks + counters of the tail split (kernels.h GramArgs)
    int gtail_wg = 0;
    double *lrpart = nullptr;                    // LinearK explicit-U forward: partial sums of G = C C^T and v = C u per column block (kernels.h)
    double *growpart = nullptr;                  // Gram route: per-64-row-block partial sums of delta^T K_fu from the K_fu build
    hipStream_t aux = nullptr;          // side stream: the K_uu chain runs beside the K_fu build (Gram route)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr, ev_kuu = nullptr, ev_tiles = nullptr, ev_go = nullptr;
    hipEvent_t ev_hwords = nullptr;     // recorded right behind a side-stream clear of Cholesky(A)'s progress words: the launch that trusts the clear waits for IT
    hipEvent_t ev_prior = nullptr;      // recorded behind an early prior-sums launch on the side stream (fwd_prior_sums)
    double *prior_sums = nullptr;       // [16] the ten parameter-only sums of the nll assembly, formed early in the iteration
    std::string err;
    std::vector<void *> allocs;
    int64_t ws_bytes = 0;
    // diagnostic switches, read from the environment ONCE when the handle is created
    struct Switches {
        bool grad_explicit = false;       // FFVD_GRAD_EXPLICIT=1: the explicit-inverse backward pass
        bool no_defer_trace = false;      // FFVD_NO_DEFER_TRACE=1: trace partials in the Gram / combine epilogue (the main stream then waits for K^-1)
        bool no_kfu_first = false;        // FFVD_NO_KFU_FIRST=1: the side chain enqueued before the main stream's K_fu build (unsplit pass with raw tiles)
        bool grad_serial = false;         // FFVD_GRAD_SERIAL=1: the K_uu side of the backward pass on the main stream
        bool no_linear_lowrank = false;   // FFVD_NO_LINEAR_LOWRANK=1: LinearK explicit-U forward through the M-wide projection (rounds 1-2)
        bool lt_armed = false;            // FFVD_GRAD_LT_ARMED=1: write the L^T rows to memory (launch_set_lt_rows) even where the dataflow kernel could read L itself
        bool whiten_products = false;     // FFVD_GRAD_WHITEN_PRODUCTS=1: training forward forms H = W^T A W with two products (round 1/2) instead of arming L^T rows
        bool debug_sync = false;    // FFVD_DEBUG_SYNC: name every launch group on stderr and wait for it (locates a faulting kernel)
        int side_delay_us = 0;      // FFVD_DEBUG_SIDE_DELAY_US=n: a spin kernel of n us at the head of every side-stream fork (schedule tests: results
        int main_delay_us = 0;      //   must not depend on which stream is late); FFVD_DEBUG_MAIN_DELAY_US=n: the same on the main stream behind a fork
        bool no_tiny = false;       // FFVD_NO_TINY=1: the multi-kernel schedule also at the reference's own experiment size (rounds 1-3)
        bool no_tiny_a = false;     // FFVD_NO_TINY_A=1: ... for the explicit-U branch only (rounds 1-4)
        bool ws_poison = false;     // FFVD_WS_POISON=1: every handle allocation starts as 0xFF bytes (NaN) instead of whatever hipMalloc returns
                                    //   (history tests: no result may depend on what a workspace held before the call)
    } sw;
    // resident parameters / data (handle-owned copies)
    double *X = nullptr, *Z = nullptr, *U = nullptr, *logvar = nullptr, *loglen = nullptr, *logQ = nullptr;
    double *CC = nullptr, *DD = nullptr, *logR = nullptr, *Y = nullptr, *ctrl = nullptr;
    ffvd_params cur{};          // pointers the kernels read (resident copies or caller's device pointers)
    bool have_params = false, have_data = false;
    void *comm = nullptr;       // RCCL communicator created by ffvd_comm_init (owned by the handle), else null
    int comm_world = 1, comm_rank = 0;
    int tiny_cus = 0;           // compute units of the device (one-launch plan)
    double *tsbuf = nullptr;    // T-shard exchange buffer: [nbatch][(Mp+1) x Mp] raw Gram tiles + delta^T K_fu rows, then [S][8] chain sums
    int64_t ts_count = 0;
    double *stage = nullptr;    // staging buffer of ffvd_allreduce_sum
    int64_t stage_count = 0;
    bool kuu_flow_sched = false;   // schedule of the big unsplit Gram pass, decided in ffvd_create (see there)
    // one-launch iteration of the reference's own experiment size (tiny.hip): decided once in ffvd_create
    ffvd::TinyPlan tiny{};
    double *tiny_scratch = nullptr;
    int *tiny_flags = nullptr;
    ffvd::TinyArgs *tiny_dargs = nullptr;     // [2] device copies of the argument block (forward / forward + backward)
    ffvd::TinyArgRing tiny_ring[2];           // per copy: pinned upload slots guarded by events + what the device copy holds (tiny.h)
    bool tiny_ring_made = false;
    size_t tiny_private_bytes = 0;      // scratch per lane of the one-launch kernel as the loaded code object reports it
    bool tiny_dirty = false;       // a launch was abandoned on a bounded wait: its hand-off words are re-zeroed before the next one
    bool info_pending = false;  // an ffvd_elbo_async was enqueued whose Cholesky info flags nobody has looked at yet
    // workspace
    double *variance = nullptr, *len = nullptr, *Zs = nullptr, *zz = nullptr;
    double *Kuu = nullptr, *F = nullptr, *H = nullptr, *rowsq = nullptr, *fmean = nullptr;
    double *ucolA = nullptr;        // explicit-U branch: U columns of the local dims, zero padded to Mp
    double *Kf2 = nullptr;          // reference route, branch B: K_fu (input of the projection GEMM); F keeps K_fu L^-T
    int ngr = 0;                    // row-sum partials per unit in that path (128-column tiles)
    // fp32-contraction path (cfg.dtype == FFVD_F32C): K_fu, F = K_fu L^-T, L^-1 as fp32 GEMM operands; per-tile and
    // per-unit sums of F^2 (fp64)
    float *Kf32 = nullptr, *F32 = nullptr, *Linv32 = nullptr;
    double *sqpart = nullptr, *sqsum = nullptr;
    int nsq = 0;
    double *Kcopy = nullptr, *Linv = nullptr, *Kinv = nullptr, *trpart = nullptr, *kterms = nullptr;   // GRAM route
    int ntiles = 0;
    double *chain_partial = nullptr;
    // backward-pass workspace (cfg.grad)
    struct GradWs {
        double *Acopy = nullptr, *u = nullptr, *LAinv = nullptr, *Gamma = nullptr, *gam_part = nullptr, *uku = nullptr;
        // whitened backward (collapsed branch): T1 = A W, later B = L_H^-1 L^-1; w = H^-1 b; b = W^T c staging; identity
        // matrix (w^T w through the u^T K u kernel); two more per-dim products of the K_uu side
        double *T1 = nullptr, *wv = nullptr, *bw = nullptr, *Ident = nullptr, *P2 = nullptr, *P3 = nullptr;
        bool whitened = false;
        double *E = nullptr, *rp = nullptr, *rsum = nullptr, *ez = nullptr, *kfu = nullptr;
        float *Gam32 = nullptr;         // fp32-contraction backward: Gamma rounded to fp32, the right operand of R = K_fu Gamma
        double *fsq = nullptr;          // reference route, fp64: sum_t |F_t|^2 per unit (the fp32 path has sqsum)
        double *cs_part = nullptr, *etx_part = nullptr, *rx2_part = nullptr, *dz_unit = nullptr, *dll_unit = nullptr, *dls_unit = nullptr;
        double *Asum = nullptr, *GamSum = nullptr, *Gs = nullptr, *gsum = nullptr, *P1 = nullptr, *KGK = nullptr, *Epsi = nullptr;
        double *rsum2 = nullptr, *ez2 = nullptr, *cs2 = nullptr, *etx2 = nullptr, *rx22 = nullptr, *dz_kuu = nullptr, *dll_kuu = nullptr, *dls_kuu = nullptr;
        double *shared_part = nullptr, *dX = nullptr, *dZ = nullptr, *dlogvar = nullptr, *dloglen = nullptr, *dlogQ = nullptr;
        size_t small_count = 0;         // doubles in the block dlogvar | dloglen | dlogQ | dCC | dDD | dlogR (one allocation)
        double *dCC = nullptr, *dDD = nullptr, *dlogR = nullptr;
        // explicit-U branch
        double *Gu = nullptr, *Gsum = nullptr, *r = nullptr, *dalpha = nullptr, *ucol = nullptr, *beta = nullptr, *du = nullptr;
        double *GammaA = nullptr, *Lclean = nullptr, *dU = nullptr, *xsq = nullptr;
        int ngam = 0, sp_stride = 0;
        // Exchange block of a sharded training step (ffvd_adam_step_allreduce): [8 term sums | dZ | dlogvar..dlogR | dU | dX],
        // every segment starting on a 256-byte boundary.  The gradient arrays above ARE these segments, so the block is
        // all-reduced in place with no packing pass; dX comes last because chain shards keep it out of the exchange.
        double *pack = nullptr;
        size_t pack_shared = 0, pack_total = 0;     // doubles up to (excluding) dX / including dX
    } gw;
    double *hterms = nullptr, *chain_terms = nullptr, *chain_nll = nullptr, *out_terms = nullptr;
    int32_t *info = nullptr;
    // Adam state for ffvd_adam_step: first/second moments per parameter array (order of FFVD_TRAIN_* bits), step count
    double *adam_m[9] = {nullptr}, *adam_v[9] = {nullptr};
    double *hmc[9][5] = {{nullptr}};     // SG-HMC state per array: xi, g, g2, p and the uploaded noise
    int64_t adam_t = 0;
    bool adam_ready = false;
    // result block and its pinned host staging: [8 term sums][S_local chain nll][Dl + nbatch info flags], contiguous on the device (resblk) and in
    // pinned host memory (h_res) so that one copy brings everything back; out_terms / chain_nll / info and h_out /
    // h_chain / h_info point into the two blocks
    double *resblk = nullptr, *h_res = nullptr;
    size_t res_bytes = 0;
    double *h_out = nullptr, *h_chain = nullptr, *h_sums = nullptr;
    int32_t *h_info = nullptr;
    int train_S_total = 0;      // > 0: ffvd_train_local has left a backward pass (scaled 1 / S_total) in gw.pack
    bool stalled = false;       // check_info saw info = -1: the dataflow Cholesky gave up on a bounded wait
    int stall_recoveries = 0;   // iterations re-run with the launch-per-column Cholesky after such a stall
    int stall_hold = 0;         // > 0: this many further calls stay on the schedule without inter-workgroup waits (fetch_with_stall_recovery)
    int stall_hold_next = 16;   // length of the next hold: doubles with every stalled probe (cap 1024), back to 16 after a clean one
    long long enq_ns = 0, enq_calls = 0;      // host time spent enqueueing iterations (ffvd_debug_enqueue_us: tools)
    std::string warning;        // one-time note about the first recovery (ffvd_last_error returns it while no error is pending)
    // optional live stage timing (HIP events on the handle's stream)
    bool timing_on = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_stage;
    size_t ev_used = 0;
};

// a device allocation owned by the handle: freed by ffvd_destroy, counted in ffvd_workspace_bytes.  With FFVD_WS_POISON the block is
// filled with NaN bytes on the handle's stream (which exists before the first allocation): the clears that create_impl and the
// workspace builders enqueue behind an allocation follow on the same stream and still win.
template <class T>
static hipError_t dev_alloc(ffvd_handle *h, T **p, size_t count) {
    size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc((void **)p, bytes);
    if (e == hipSuccess) {
        h->allocs.push_back((void *)*p);
        h->ws_bytes += (int64_t)bytes;
        if (h->sw.ws_poison) e = hipMemsetAsync((void *)*p, 0xFF, bytes, h->stream);
    }
    return e;
}

// FFVD_DEBUG_SYNC=1: print the name of the launch group just enqueued and wait for both streams, so that a faulting kernel is the
// one named last (diagnostic only; read once per handle)
#define DBG_SYNC(h, name)                                                                              \
    do {                                                                                               \
        if ((h)->sw.debug_sync) {                                                                      \
            fprintf(stderr, "[ffvd debug] %s ...", name); fflush(stderr);                             \
            hipError_t e1_ = hipStreamSynchronize((h)->stream), e2_ = hipStreamSynchronize((h)->aux);  \
            fprintf(stderr, " %s\n", (e1_ == hipSuccess && e2_ == hipSuccess) ? "ok" : hipGetErrorString(e1_ != hipSuccess ? e1_ : e2_)); \
        }                                                                                              \
    } while (0)

namespace ffvd {

// The nine parameter arrays in the order of the FFVD_TRAIN_* bits (bit i = array i): the member of an ffvd_params and the element
// count.  U counts M x D here (ffvd_get_params, ffvd_update_params); the optimiser table of train.hip gives it 0 where U has no gradient.
constexpr int NPARAM = 9, PARAM_U = 8;
constexpr const double *ffvd_params::*PARAM_MEMBER[NPARAM] = {
    &ffvd_params::X,  &ffvd_params::Z,  &ffvd_params::logvariance, &ffvd_params::loglengthscales, &ffvd_params::log_Q,
    &ffvd_params::CC, &ffvd_params::DD, &ffvd_params::log_Rchols,  &ffvd_params::U};
inline size_t param_count(const ffvd_handle *h, int i) {
    const ffvd_config &c = h->cfg;
    const size_t P = h->P, J = c.Ydim;
    const size_t n[NPARAM] = {(size_t)c.S_local * (c.T + 1) * c.D, (size_t)c.M * P, (size_t)c.D, (size_t)c.D * P, (size_t)c.D,
                              (size_t)c.D * J, J, J * J, (size_t)c.M * c.D};
    return n[i];
}

// results to the caller (either pointer may be null): the 8 sums and nll = NLL / chains -- the COUNT among a job's reduced sums
// (report_sums), S_local for this rank's own result block (report_local)
inline void report_sums(const double sums[8], double out_terms[8], double *out_nll, double chains = 0.0) {
    if (out_terms) memcpy(out_terms, sums, 8 * sizeof(double));
    if (out_nll) *out_nll = sums[FFVD_TERM_NLL] / (chains > 0.0 ? chains : sums[FFVD_TERM_COUNT]);
}
inline void report_local(const ffvd_handle *h, double out_terms[8], double *out_nll) {
    report_sums(h->h_out, out_terms, out_nll, (double)h->cfg.S_local);
}

// abi.hip: fork the side stream off the main stream; data and parameters bound; the factorisation flags of the fetched result block;
// FFVD_ENOTPD "<who>: non-finite <what>" unless the n sums are finite; the two launch sequences of a T-shard; forward + backward pass
// of one training iteration, enqueued / run to its result block with the recovery of a stalled dataflow Cholesky
int fork_side(ffvd_handle *h, hipEvent_t ev, hipStream_t from, hipStream_t to);
int ready(ffvd_handle *h, const char *who);
int check_info(ffvd_handle *h);
int check_finite(ffvd_handle *h, const double *sums, int n, const char *who, const char *what);
int enqueue_tshard_local(ffvd_handle *h);
int enqueue_tshard_finish(ffvd_handle *h);
int enqueue_forward_backward(ffvd_handle *h, int S_total);
int run_forward_backward(ffvd_handle *h, int S_total);

// backward.hip: the backward-pass workspace h->gw (create_impl, cfg.grad), the multi-kernel backward pass behind a forward
// iteration (enqueue_grad_b: its collapsed branch, which a T-shard finish calls directly), gradients to the caller's host arrays
int alloc_grad_workspace(ffvd_handle *h);
int enqueue_grad(ffvd_handle *h, int S_total);
int enqueue_grad_b(ffvd_handle *h, int S_total);
int copy_grads_out(ffvd_handle *h, const ffvd_grads *gout);

}  // namespace ffvd
