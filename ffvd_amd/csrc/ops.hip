// The stateless operator entry points of the C ABI (ffvd_op_*, include/ffvd_abi.h): what the Python mirror of the reference API
// calls.  Temporaries per call, not the hot path.  Shares only abi_internal.h with abi.hip.
#include "abi_internal.h"
#include "kernels.h"
#include "grad.h"
#include "optim.h"
#include "step_bodies.h"
#include "rollout_group.h"
#include "posterior_group.h"
#include "conditional_group.h"
#include "predict_summary.h"
#include "moment_group.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

using namespace ffvd;

static std::atomic<int> g_rollout_fallbacks{0};     // ffvd_op_rollout calls of this process that fell back from the resident loop to the per-step launches

// ---- operator-level entry points (temporaries per call; not the hot path) -------------------------------------------------------------
// Round 5: the temporaries come from a per-thread cache instead of hipMalloc / hipFree / hipStreamCreate per call.  A rollout call made
// ~27 allocations and as many frees around 200 steps of 15 us: 2.7 ms of host work per call (profiles/r04_next_rows.json: 27.6 us per
// step of a 200-step call against 15.3 marginal).  A block is handed out again when its size fits (smallest block that is large enough
// and at most 4 x the request); the cache is bounded (256 blocks / 8 GiB: beyond that everything idle is freed) and can be released
// with ffvd_op_release_cache().  Nothing relies on fresh memory being zero (hipMalloc never promised that).
namespace {
struct OpCache {
    struct Block { void *p; size_t bytes; bool busy; };
    std::vector<Block> blocks;
    size_t total = 0;
    hipStream_t stream = nullptr;
    int device = -1;
    void *pinned = nullptr;             // page-locked staging block for large results (a device-to-host copy into fresh pageable memory
    size_t pinned_bytes = 0;            //  pins its pages on the fly: 13 MB took up to 30 ms; through this block + memcpy: ~3)
    void release_idle() {
        std::vector<Block> keep;
        for (Block &b : blocks) {
            if (b.busy) keep.push_back(b);
            else { hipFree(b.p); total -= b.bytes; }
        }
        blocks.swap(keep);
    }
    void release_all() {
        release_idle();
        if (stream && blocks.empty()) { hipStreamDestroy(stream); stream = nullptr; }
        if (pinned) { hipHostFree(pinned); pinned = nullptr; pinned_bytes = 0; }
    }
    ~OpCache() { /* process exit: the runtime may already be gone; leave the memory to it */ }
};
thread_local OpCache g_op_cache;

struct Scratch {
    std::vector<size_t> mine;           // indices into the cache of the blocks this call holds
    hipStream_t stream = nullptr;
    // host staging buffers of this call (host()).  A member, so it outlives the destructor body: an asynchronous upload may read its
    // source until the stream has been synchronised, on the early error returns as well.
    std::deque<std::vector<double>> staged;
    bool begin() {
        OpCache &c = g_op_cache;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        if (c.device != dev) {           // (another device was made current on this thread: start over)
            c.release_all();
            c.device = dev;
        }
        if (!c.stream && hipStreamCreate(&c.stream) != hipSuccess) return false;
        stream = c.stream;
        return true;
    }
    ~Scratch() {
        if (stream) hipStreamSynchronize(stream);
        OpCache &c = g_op_cache;
        for (size_t i : mine) c.blocks[i].busy = false;
        if (c.blocks.size() > 256 || c.total > ((size_t)8 << 30)) c.release_idle();
    }
    // n doubles of host memory that live until the call's stream has drained: every source of an asynchronous upload that the
    // operator builds itself comes from here
    std::vector<double> &host(size_t n, double fill = 0.0) {
        staged.emplace_back(n, fill);
        return staged.back();
    }
    template <class T>
    T *alloc(size_t n) {
        OpCache &c = g_op_cache;
        const size_t bytes = ((n ? n : 1) * sizeof(T) + 255) / 256 * 256;
        size_t best = (size_t)-1;
        for (size_t i = 0; i < c.blocks.size(); ++i) {
            const OpCache::Block &b = c.blocks[i];
            if (!b.busy && b.bytes >= bytes && b.bytes <= 4 * bytes && (best == (size_t)-1 || b.bytes < c.blocks[best].bytes)) best = i;
        }
        if (best == (size_t)-1) {
            void *p = nullptr;
            if (hipMalloc(&p, bytes) != hipSuccess) {
                (void)hipGetLastError();
                c.release_idle();                                   // make room and try once more
                mine.clear();
                for (size_t i = 0; i < c.blocks.size(); ++i) if (c.blocks[i].busy) mine.push_back(i);      // (indices moved; every busy block is this call's: one call per thread at a time)
                if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            }
            c.blocks.push_back({p, bytes, false});
            c.total += bytes;
            best = c.blocks.size() - 1;
        }
        c.blocks[best].busy = true;
        mine.push_back(best);
        // FFVD_OP_CACHE_POISON=1 (tests): every block handed out starts as NaN bytes -- nothing may rely on what a block held before
        static const bool poison = [] { const char *e = getenv("FFVD_OP_CACHE_POISON"); return e && *e && strcmp(e, "0") != 0; }();
        if (poison && stream) (void)hipMemsetAsync(c.blocks[best].p, 0xFF, c.blocks[best].bytes, stream);
        return (T *)c.blocks[best].p;
    }
    // device -> host for a large result: through the thread's page-locked block when it has (or gets) one of that size, else directly.
    // Synchronises the stream.
    bool download(void *dst, const void *src, size_t bytes) {
        if (void *pin = pinned_block(bytes)) {
            if (hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
            if (hipStreamSynchronize(stream) != hipSuccess) return false;
            memcpy(dst, pin, bytes);
            return true;
        }
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    }
    // the thread's page-locked block, grown to `bytes` (nullptr when it cannot be had or the size is outside 1 MB .. 256 MB)
    void *pinned_block(size_t bytes) {
        OpCache &c = g_op_cache;
        if (bytes < ((size_t)1 << 20) || bytes > ((size_t)256 << 20)) return nullptr;
        if (c.pinned_bytes < bytes) {
            if (c.pinned) { hipHostFree(c.pinned); c.pinned = nullptr; c.pinned_bytes = 0; }
            if (hipHostMalloc(&c.pinned, bytes, hipHostMallocDefault) == hipSuccess) c.pinned_bytes = bytes;
            else { (void)hipGetLastError(); c.pinned = nullptr; }
        }
        return c.pinned;
    }
    // host -> device, asynchronous, straight from the caller's memory.  (Measured: large uploads through the page-locked block + a
    // synchronisation made a 200-step rollout call 0.4 ms slower and changed nothing for the sweep -- the 28 ms some calls spend here in
    // tools/bench_next.py's process are a wait of the stream behind the 0.2 ms DMA, whichever memory it reads; FFVD_PG_TIMING=1 shows it.)
    double *upload(const double *src, size_t n) {
        double *d = alloc<double>(n);
        if (d && n && hipMemcpyAsync(d, src, n * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess) return nullptr;
        return d;
    }
};

// FFVD_PG_TIMING / FFVD_RG_TIMING (tools): where a call spends its wall time, one line per lap on stderr.  A lap waits for the stream
// first (so a timed call is slower) unless told not to: the time the host needed to enqueue, then the time the GPU needed after that.
struct LapTimer {
    const char *who;
    hipStream_t stream;
    bool on;
    std::chrono::steady_clock::time_point last;
    LapTimer(const char *env, const char *who_, hipStream_t s) : who(who_), stream(s), on(getenv(env) != nullptr), last(std::chrono::steady_clock::now()) {}
    void lap(const char *what, bool drain = true) {
        if (!on) return;
        if (drain) (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "%s:   %-28s %.3f ms\n", who, what, std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
};
}  // namespace

// Free what the calling thread's operator cache holds (device buffers of finished ffvd_op_* calls, their stream).
extern "C" int ffvd_op_release_cache(void) {
    g_op_cache.release_all();
    return FFVD_OK;
}

#define OP_BEGIN(name)                                                                       \
    Scratch sc;                                                                              \
    if (!sc.begin())                                                                         \
        return set_error(nullptr, FFVD_EDEVICE, name ": no usable HIP device / stream creation failed");
// the same for a body that several entry points share: `who` (a std::string) names the one that was called
#define OP_BEGIN_AS(who)                                                                     \
    Scratch sc;                                                                              \
    if (!sc.begin())                                                                         \
        return set_error(nullptr, FFVD_EDEVICE, (who) + ": no usable HIP device / stream creation failed");
#define OP_CHECK_AS(ptr, who) \
    if (!(ptr)) return set_error(nullptr, FFVD_ENOMEM, (who) + ": device allocation or upload failed");
#define OP_CHECK(ptr, name) \
    if (!(ptr)) return set_error(nullptr, FFVD_ENOMEM, name ": device allocation or upload failed");

// ---- set-up shared by the operators ------------------------------------------------------------------------------------------------
// Device-side hyper-parameters of D kernels over the inducing inputs Z: uploads Z and logvariance, runs prep_hypers.  (LinearK has no
// lengthscales: its loglen block is allocated and not written.)
static int stage_hypers(Scratch &sc, const char *who, int kind, const double *Z, int M, int Mp, int P, int D, const double *logvariance,
                        const double *loglengthscales, HyperView &hv) {
    double *dZ = sc.upload(Z, (size_t)M * P), *dlogvar = sc.upload(logvariance, D);
    double *loglen = sc.alloc<double>((size_t)D * P);
    double *variance = sc.alloc<double>(D), *len = sc.alloc<double>((size_t)D * P);
    double *Zs = sc.alloc<double>((size_t)D * Mp * P), *zz = sc.alloc<double>((size_t)D * Mp);
    if (!dZ || !dlogvar || !loglen || !variance || !len || !Zs || !zz)
        return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation or upload failed");
    if (loglengthscales)
        OP_TRY(hipMemcpyAsync(loglen, loglengthscales, (size_t)D * P * sizeof(double), hipMemcpyHostToDevice, sc.stream));
    launch_prep_hypers(sc.stream, kind, dZ, M, Mp, P, D, 0, dlogvar, loglen, variance, len, Zs, zz);
    hv = HyperView{variance, len, Zs, zz};
    return FFVD_OK;
}

// Projection arguments of an operator: one chain, all D dims, GP inputs x (T rows of P columns, no separate control block).
static ProjectArgs op_project_args(int kind, const HyperView &hv, const double *x, int T, int Tp, int P, int M, int Mp, int D,
                                   const double *W, size_t w_stride, const double *U, double *F, double *rowsq, double *fmean, int ng) {
    ProjectArgs pa{};
    pa.kind = kind; pa.x = x; pa.x_chain_stride = 0; pa.x_ld = P; pa.x_cols = P; pa.ctrl = nullptr;
    pa.T = T; pa.Tp = Tp; pa.C = 0; pa.P = P; pa.M = M; pa.Mp = Mp; pa.Dl = D; pa.d_begin = 0; pa.hv = hv;
    pa.W = W; pa.w_stride = w_stride; pa.U = U; pa.u_ld = U ? D : 0; pa.b0 = 0; pa.nb = D; pa.F = F;
    pa.rowsq = rowsq; pa.fmean = fmean; pa.ng = ng;
    return pa;
}

// Host copy (an upload source: from sc.host) of `batch` n x n matrices, each padded to np x np with an identity block; diag_add is
// added to the n live diagonal entries.
static std::vector<double> &pad_identity(Scratch &sc, const double *src, int batch, int n, int np, double diag_add = 0.0) {
    const size_t slab = (size_t)np * np;
    std::vector<double> &out = sc.host(slab * batch);
    for (int b = 0; b < batch; ++b) {
        double *S = out.data() + slab * b;
        for (int i = 0; i < np; ++i) {
            if (i < n) {
                memcpy(S + (size_t)i * np, src + ((size_t)b * n + i) * n, (size_t)n * sizeof(double));
                if (diag_add != 0.0) S[(size_t)i * np + i] += diag_add;
            } else S[(size_t)i * np + i] = 1.0;
        }
    }
    return out;
}

// upload a caller-supplied stack of D M x M matrices padded to Mp (M a multiple of the block size: nothing to pad -- the caller's
// array itself is uploaded)
static double *upload_stack(Scratch &sc, const double *src, int D, int M, int Mp) {
    if (M == Mp) return sc.upload(src, (size_t)D * M * M);
    std::vector<double> &pad = pad_identity(sc, src, D, M, Mp);
    return sc.upload(pad.data(), pad.size());
}

// n M x M matrices given as a table of host pointers -> a device stack of Mp x Mp slots.  The matrices are NOT packed on the host:
// each goes from where the caller keeps it straight into its slot (a pitched copy when M != Mp; the padding is zeroed on the device).
static double *upload_matrix_table(Scratch &sc, const double *const *src, size_t n, int M, int Mp) {
    double *dst = sc.alloc<double>(n * Mp * Mp);
    if (!dst) return nullptr;
    if (Mp != M && hipMemsetAsync(dst, 0, n * Mp * Mp * sizeof(double), sc.stream) != hipSuccess) return nullptr;
    for (size_t b = 0; b < n; ++b) {
        const hipError_t e = (Mp == M)
            ? hipMemcpyAsync(dst + b * Mp * Mp, src[b], (size_t)M * M * sizeof(double), hipMemcpyHostToDevice, sc.stream)
            : hipMemcpy2DAsync(dst + b * Mp * Mp, (size_t)Mp * sizeof(double), src[b], (size_t)M * sizeof(double),
                               (size_t)M * sizeof(double), M, hipMemcpyHostToDevice, sc.stream);
        if (e != hipSuccess) return nullptr;
    }
    return dst;
}

// FFVD_ENOTPD for matrix d of a batch whose Cholesky flag (1 + first bad pivot) is set
static int chol_not_pd(const char *who, const std::string &what, int d, int32_t flag) {
    return set_error(nullptr, FFVD_ENOTPD, std::string(who) + ": Cholesky of " + what + " failed: latent dim " + std::to_string(d) + ", pivot " +
                                               std::to_string(flag - 1) + " is not positive");
}
// read the D Cholesky flags back (synchronises the stream, so every copy enqueued before has landed too)
static int fetch_chol_info(Scratch &sc, const int32_t *dinfo, int D, const char *who, const char *what) {
    std::vector<int32_t> hinfo(D, 0);
    if (hipMemcpyAsync(hinfo.data(), dinfo, D * sizeof(int32_t), hipMemcpyDeviceToHost, sc.stream) != hipSuccess ||
        hipStreamSynchronize(sc.stream) != hipSuccess)
        return set_error(nullptr, FFVD_EDEVICE, std::string(who) + ": device error while reading Cholesky status");
    for (int d = 0; d < D; ++d)
        if (hinfo[d]) return chol_not_pd(who, what, d, hinfo[d]);
    return FFVD_OK;
}

static void launch_skinny_gemm(hipStream_t stream, const SkinnyArgs &a) {
    ffvd::launch_skinny_gemm(stream, a.A, a.a_stride, a.lda, a.B, a.b_stride, a.ldb, a.upper, a.rows, a.K, a.N, a.nb, a.Tp, a.C, a.c_stride,
                             a.ldc, a.u, a.u_stride, a.sq, a.dot, a.B2, a.b2_stride, a.ldb2, a.N2, a.sq2, a.a_trans, a.upper2);
}

extern "C" int ffvd_op_kernel_matrix(int kind, const double *X, int N, const double *X2, int N2, int P,
                                     double logvariance, const double *loglengthscales, double jitter, double *out) {
    if (!X || !out || N < 0 || P < 1 || (X2 && N2 < 0) || (kind == FFVD_KERNEL_SE && !loglengthscales) ||
        (kind != FFVD_KERNEL_SE && kind != FFVD_KERNEL_LINEAR))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_kernel_matrix: bad argument");
    OP_BEGIN("ffvd_op_kernel_matrix");
    const int same = (X2 == nullptr);
    if (same) N2 = N;
    if ((size_t)N * N2 == 0) return FFVD_OK;
    double *dX = sc.upload(X, (size_t)N * P);
    OP_CHECK(dX, "ffvd_op_kernel_matrix");
    double *dX2 = same ? dX : sc.upload(X2, (size_t)N2 * P);
    OP_CHECK(dX2, "ffvd_op_kernel_matrix");
    double *dl = sc.alloc<double>(P);
    OP_CHECK(dl, "ffvd_op_kernel_matrix");
    if (loglengthscales) OP_TRY(hipMemcpyAsync(dl, loglengthscales, P * sizeof(double), hipMemcpyHostToDevice, sc.stream));
    double *dO = sc.alloc<double>((size_t)N * N2);
    OP_CHECK(dO, "ffvd_op_kernel_matrix");
    launch_kernel_matrix(sc.stream, kind, dX, N, dX2, N2, P, logvariance, dl, jitter, same, dO);
    OP_TRY(hipMemcpyAsync(out, dO, (size_t)N * N2 * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_kernel_diag(int kind, const double *X, int N, int P, double logvariance, double *out) {
    if (!X || !out || N < 0 || P < 1) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_kernel_diag: bad argument");
    OP_BEGIN("ffvd_op_kernel_diag");
    if (N == 0) return FFVD_OK;
    double *dX = sc.upload(X, (size_t)N * P);
    OP_CHECK(dX, "ffvd_op_kernel_diag");
    double *dO = sc.alloc<double>(N);
    OP_CHECK(dO, "ffvd_op_kernel_diag");
    launch_kernel_diag(sc.stream, kind, dX, N, P, logvariance, dO);
    OP_TRY(hipMemcpyAsync(out, dO, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

// Batched Cholesky of `batch` np x np slabs (identity padded, np % NB == 0) at dA, which the caller uploaded from host_in (left
// intact); hinfo[b] <- 0 or 1 + first bad pivot.  If the one-launch (dataflow) variant gave up on a bounded wait, the batch is uploaded
// again from host_in and re-run with the launch-per-column variant, which has no inter-workgroup waits; a warning for
// ffvd_last_error(NULL) says so (an error of the caller's replaces it).
// Shared by ffvd_op_cholesky and ffvd_op_get_rand_full_cov.
static int potrf_with_stall_recovery(Scratch &sc, double *dA, const double *host_in, int np, int batch, int32_t *dinfo,
                                     double *dinv, int32_t *hinfo, const char *who) {
    const size_t slab = (size_t)np * np;
    for (int attempt = 0;; ++attempt) {
        {
            CholOverrideGuard guard;            // reset on the error returns below as well
            if (attempt == 1) {
                OP_TRY(hipMemcpyAsync(dA, host_in, slab * batch * sizeof(double), hipMemcpyHostToDevice, sc.stream));
                guard.force_left();
            }
            OP_TRY(hipMemsetAsync(dinfo, 0, batch * sizeof(int32_t), sc.stream));
            launch_potrf_ext(sc.stream, dA, np, 0, 0, batch, slab, dinfo, dinv);
        }
        OP_TRY(hipMemcpyAsync(hinfo, dinfo, batch * sizeof(int32_t), hipMemcpyDeviceToHost, sc.stream));
        OP_TRY(hipStreamSynchronize(sc.stream));
        bool stalled = false;
        for (int b = 0; b < batch; ++b) stalled = stalled || hinfo[b] < 0;
        if (!stalled) {
            if (attempt == 1)
                set_error(nullptr, FFVD_OK, "warning: " + std::string(who) + ": the one-launch (dataflow) Cholesky gave up on a bounded wait; the batch "
                                            "was re-run with the launch-per-column Cholesky and completed");
            return FFVD_OK;
        }
        if (attempt == 1)
            return set_error(nullptr, FFVD_EDEVICE, std::string(who) + ": abandoned, a block row waited more than 1 s for the row above it");
    }
}

extern "C" int ffvd_op_cholesky(const double *A, int n, int batch, double *L, int32_t *info) {
    if (!A || !L || n < 1 || batch < 0) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_cholesky: bad argument");
    OP_BEGIN("ffvd_op_cholesky");
    if (batch == 0) return FFVD_OK;
    const int np = round_up(n, NB);
    const size_t slab = (size_t)np * np;
    std::vector<double> &pad = pad_identity(sc, A, batch, n, np);
    double *dA = sc.upload(pad.data(), pad.size());
    OP_CHECK(dA, "ffvd_op_cholesky");
    int32_t *dinfo = sc.alloc<int32_t>(batch);
    OP_CHECK(dinfo, "ffvd_op_cholesky");
    double *dinv = sc.alloc<double>(potrf_scratch_doubles(np, batch));
    OP_CHECK(dinv, "ffvd_op_cholesky");
    std::vector<int32_t> hinfo(batch, 0);
    int rc = potrf_with_stall_recovery(sc, dA, pad.data(), np, batch, dinfo, dinv, hinfo.data(), "ffvd_op_cholesky");
    if (rc) return rc;
    OP_TRY(hipMemcpyAsync(pad.data(), dA, pad.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    int bad = -1;
    for (int b = 0; b < batch; ++b) {
        const double *S = pad.data() + slab * b;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) L[((size_t)b * n + i) * n + j] = (j <= i) ? S[(size_t)i * np + j] : 0.0;
        if (info) info[b] = hinfo[b];
        if (hinfo[b] != 0 && bad < 0) bad = b;
    }
    if (bad >= 0) {
        char msg[160];
        snprintf(msg, sizeof msg, "ffvd_op_cholesky: matrix %d is not positive definite (pivot %d)", bad, hinfo[bad] - 1);
        return set_error(nullptr, FFVD_ENOTPD, msg);
    }
    return FFVD_OK;
}

// shared by kernel_pre_cal / conditional: device-side hypers + K_uu + extended Cholesky
struct KuuWork {
    HyperView hv;
    double *Kuu, *dinv;
    int32_t *info;
    int Mp;
};
static int build_kuu(Scratch &sc, const char *who, int kind, const double *Z, int M, int P, int D, const double *logvariance,
                     const double *loglengthscales, double jitter, KuuWork &w) {
    const int Mp = round_up(M, NB);
    w.Mp = Mp;
    if (int rc = stage_hypers(sc, who, kind, Z, M, Mp, P, D, logvariance, loglengthscales, w.hv)) return rc;
    w.Kuu = sc.alloc<double>((size_t)D * 2 * Mp * Mp);
    w.info = sc.alloc<int32_t>(D);
    w.dinv = sc.alloc<double>(potrf_scratch_doubles(Mp, D));
    if (!w.Kuu || !w.info || !w.dinv) return FFVD_ENOMEM;
    if (hipMemsetAsync(w.info, 0, D * sizeof(int32_t), sc.stream) != hipSuccess) return FFVD_EDEVICE;
    launch_kuu_build(sc.stream, kind, w.hv, M, Mp, P, D, jitter, w.Kuu, nullptr);
    launch_potrf_ext(sc.stream, w.Kuu, Mp, Mp, Mp, D, (size_t)2 * Mp * Mp, w.info, w.dinv);
    return FFVD_OK;
}

extern "C" int ffvd_op_trsm(const double *L, int n, const double *B, int m, double *X) {
    if (!L || !B || !X || n < 1 || m < 0) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_trsm: bad argument");
    for (int i = 0; i < n; ++i)
        if (!(L[(size_t)i * n + i] != 0.0)) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_trsm: zero on the diagonal of L");
    OP_BEGIN("ffvd_op_trsm");
    if (m == 0) return FFVD_OK;
    // slab = [ L (np x np, identity padding) ; R = B^T (mp x np, zero padding) ];  X^T = R L^-T
    const int np = round_up(n, NB), mp = round_up(m, NB);
    std::vector<double> &slab = sc.host((size_t)(np + mp) * np);
    for (int i = 0; i < np; ++i) {
        if (i < n) for (int j = 0; j <= i; ++j) slab[(size_t)i * np + j] = L[(size_t)i * n + j];
        else slab[(size_t)i * np + i] = 1.0;
    }
    for (int c = 0; c < m; ++c)
        for (int i = 0; i < n; ++i) slab[(size_t)(np + c) * np + i] = B[(size_t)i * m + c];
    double *dA = sc.upload(slab.data(), slab.size());
    OP_CHECK(dA, "ffvd_op_trsm");
    double *dinv = sc.alloc<double>(DINV_STRIDE);
    OP_CHECK(dinv, "ffvd_op_trsm");
    launch_trsm_ext(sc.stream, dA, np, mp, 1, slab.size(), dinv);
    OP_TRY(hipGetLastError());
    OP_TRY(hipMemcpyAsync(slab.data(), dA, slab.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    for (int c = 0; c < m; ++c)
        for (int i = 0; i < n; ++i) X[(size_t)i * m + c] = slab[(size_t)(np + c) * np + i];
    return FFVD_OK;
}

extern "C" int ffvd_op_kernel_pre_cal(int kind, const double *Z, int M, int P, int D, const double *logvariance,
                                      const double *loglengthscales, double jitter, double *Lm_inverse_seq) {
    if (!Z || !logvariance || !Lm_inverse_seq || M < 1 || P < 1 || P > MAXP || D < 1 ||
        (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_kernel_pre_cal: bad argument");
    OP_BEGIN("ffvd_op_kernel_pre_cal");
    KuuWork w{};
    int rc = build_kuu(sc, "ffvd_op_kernel_pre_cal", kind, Z, M, P, D, logvariance, loglengthscales, jitter, w);
    if (rc) return set_error(nullptr, rc, "ffvd_op_kernel_pre_cal: device allocation or upload failed");
    const size_t Mp = w.Mp;
    std::vector<double> host((size_t)D * 2 * Mp * Mp);
    OP_TRY(hipMemcpyAsync(host.data(), w.Kuu, host.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    if ((rc = fetch_chol_info(sc, w.info, D, "ffvd_op_kernel_pre_cal", "K_uu + jitter*I"))) return rc;
    for (int d = 0; d < D; ++d) {
        const double *Wd = host.data() + (size_t)d * 2 * Mp * Mp + Mp * Mp;
        for (int i = 0; i < M; ++i)
            memcpy(Lm_inverse_seq + ((size_t)d * M + i) * M, Wd + (size_t)i * Mp, (size_t)M * sizeof(double));
    }
    return FFVD_OK;
}

extern "C" int ffvd_op_collapse(int kind, const double *Lm_inverse_seq, const double *X_combine, const double *X,
                                const double *Z, int T, int M, int P, int D, const double *logvariance,
                                const double *loglengthscales, const double *Q, double batch_size, double Y_N,
                                double out3[3]) {
    if (!Lm_inverse_seq || !X_combine || !X || !Z || !logvariance || !Q || !out3 || T < 1 || M < 1 || P < 1 ||
        P > MAXP || D < 1 || (kind == FFVD_KERNEL_SE && !loglengthscales) || !(batch_size > 0.0))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_collapse: bad argument");
    OP_BEGIN("ffvd_op_collapse");
    const int Mp = round_up(M, NB), Tp = round_up(T, STRIP), ng = (Mp + 511) / 512;
    std::vector<double> &logQ = sc.host(D);
    for (int d = 0; d < D; ++d) logQ[d] = log(Q[d]);
    HyperView hv{};
    if (int rc = stage_hypers(sc, "ffvd_op_collapse", kind, Z, M, Mp, P, D, logvariance, loglengthscales, hv)) return rc;
    double *dW = upload_stack(sc, Lm_inverse_seq, D, M, Mp);      // the caller's L^{-T} stack, padded to Mp with an identity block
    double *dXc = sc.upload(X_combine, (size_t)T * P);
    double *dX = sc.upload(X, (size_t)(T + 1) * D);
    double *dlq = sc.upload(logQ.data(), D);
    double *F = sc.alloc<double>((size_t)D * Tp * Mp);
    const size_t hstride = (size_t)(Mp + NB) * Mp;
    double *H = sc.alloc<double>((size_t)D * hstride);
    double *rowsq = sc.alloc<double>((size_t)D * ng * Tp);
    double *hterms = sc.alloc<double>((size_t)D * 2), *cterms = sc.alloc<double>(8);
    int32_t *info = sc.alloc<int32_t>(D);
    double *dinv = sc.alloc<double>(potrf_scratch_doubles(Mp, D));
    if (!dW || !dXc || !dX || !dlq || !F || !H || !rowsq || !hterms || !cterms || !info || !dinv)
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_collapse: device allocation or upload failed");
    OP_TRY(hipMemsetAsync(H, 0, (size_t)D * hstride * sizeof(double), sc.stream));
    OP_TRY(hipMemsetAsync(info, 0, D * sizeof(int32_t), sc.stream));
    launch_project(sc.stream, op_project_args(kind, hv, dXc, T, Tp, P, M, Mp, D, dW, (size_t)Mp * Mp, nullptr, F, rowsq, nullptr, ng));
    GramArgs ga{};
    ga.mode = GRAM_F; ga.A = F; ga.a_stride = (size_t)Tp * Mp; ga.rows = Tp; ga.with_row = 1;
    ga.X = dX; ga.log_Q = dlq; ga.T = T; ga.D = D; ga.Mp = Mp; ga.Dl = D; ga.d_begin = 0;
    ga.b0 = 0; ga.nb = D; ga.yn_over_batch = Y_N / batch_size; ga.H = H; ga.h_stride = hstride;
    launch_gram(sc.stream, ga);
    launch_potrf_ext(sc.stream, H, Mp, NB, 0, D, hstride, info, dinv);
    launch_h_finish(sc.stream, H, Mp, hstride, D, hterms);
    ReduceArgs ra{};
    ra.kind = kind; ra.branch = FFVD_BRANCH_B; ra.X = dX; ra.ctrl = nullptr; ra.Y = nullptr; ra.log_Q = dlq;
    ra.CC = nullptr; ra.DD = nullptr; ra.log_Rchols = nullptr; ra.variance = hv.variance; ra.T = T; ra.Tp = Tp; ra.D = D;
    ra.C = 0; ra.Ydim = 0; ra.Dl = D; ra.d_begin = 0; ra.S = 1; ra.ng = ng; ra.shared_terms = 0;
    ra.xk = dXc; ra.xk_chain_stride = 0; ra.xk_ld = P; ra.xk_cols = P; ra.rowsq = rowsq; ra.fmean = nullptr;
    ra.chain_terms = cterms;
    double *cpart = sc.alloc<double>(128);
    if (!cpart) return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_collapse: device allocation failed");
    launch_chain_reduce(sc.stream, ra, cpart);
    std::vector<double> ht((size_t)D * 2), ct(8);
    OP_TRY(hipMemcpyAsync(ht.data(), hterms, ht.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(ct.data(), cterms, 8 * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    if (int rc = fetch_chol_info(sc, info, D, "ffvd_op_collapse", "H")) return rc;
    double term1 = 0.0, term2 = 0.0;
    for (int d = 0; d < D; ++d) { term1 += -0.5 * ht[2 * d]; term2 += 0.5 * ht[2 * d + 1]; }
    out3[0] = -term1 / Y_N;
    out3[1] = -term2 / Y_N;
    out3[2] = -ct[2] / Y_N;      // chain_reduce's trace sum: sum_d sum_t -0.5 (Kdiag - |F_t|^2) / Q_d
    return FFVD_OK;
}

extern "C" int ffvd_op_conditional(int kind, const double *Xnew, int N, const double *Z, int M, int P, int D,
                                   const double *logvariance, const double *loglengthscales, const double *f,
                                   double jitter, double *mean, double *var) {
    if (!Xnew || !Z || !logvariance || !f || !mean || !var || N < 0 || M < 1 || P < 1 || P > MAXP || D < 1 ||
        (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_conditional: bad argument");
    OP_BEGIN("ffvd_op_conditional");
    if (N == 0) return FFVD_OK;
    KuuWork w{};
    int rc = build_kuu(sc, "ffvd_op_conditional", kind, Z, M, P, D, logvariance, loglengthscales, jitter, w);
    if (rc) return set_error(nullptr, rc, "ffvd_op_conditional: device allocation or upload failed");
    const int Mp = w.Mp, Tp = round_up(N, STRIP), ng = (Mp + 511) / 512;
    double *dX = sc.upload(Xnew, (size_t)N * P);
    double *dU = sc.upload(f, (size_t)M * D);
    double *rowsq = sc.alloc<double>((size_t)D * ng * Tp), *fmean = sc.alloc<double>((size_t)D * ng * Tp);
    double *dmean = sc.alloc<double>((size_t)N * D), *dvar = sc.alloc<double>((size_t)N * D);
    if (!dX || !dU || !rowsq || !fmean || !dmean || !dvar)
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_conditional: device allocation or upload failed");
    launch_project(sc.stream, op_project_args(kind, w.hv, dX, N, Tp, P, M, Mp, D, w.Kuu + (size_t)Mp * Mp, (size_t)2 * Mp * Mp, dU, nullptr,
                                              rowsq, fmean, ng));
    launch_conditional_finish(sc.stream, kind, dX, N, P, w.hv.variance, rowsq, fmean, ng, Tp, D, dmean, dvar, nullptr);
    OP_TRY(hipMemcpyAsync(mean, dmean, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(var, dvar, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    return fetch_chol_info(sc, w.info, D, "ffvd_op_conditional", "K_uu + jitter*I");
}

extern "C" int ffvd_op_predict_mean(const double *X_end, int N, int D, const double *CC, const double *DD, int Ydim,
                                    double *out) {
    if (!X_end || !CC || !DD || !out || N < 0 || D < 1 || Ydim < 1)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_predict_mean: bad argument");
    OP_BEGIN("ffvd_op_predict_mean");
    if (N == 0) return FFVD_OK;
    double *dX = sc.upload(X_end, (size_t)N * D), *dC = sc.upload(CC, (size_t)D * Ydim), *dD = sc.upload(DD, Ydim);
    double *dO = sc.alloc<double>((size_t)N * Ydim);
    if (!dX || !dC || !dD || !dO) return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_predict_mean: device allocation or upload failed");
    launch_predict_mean(sc.stream, dX, N, D, dC, dD, Ydim, dO);
    OP_TRY(hipMemcpyAsync(out, dO, (size_t)N * Ydim * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_logdensity_norm_diag(int nonvec, const double *y, const double *ymean, const double *Rchols, int N,
                                            int J, double *out) {
    if (!y || !ymean || !Rchols || !out || N < 0 || J < 1)
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_logdensity_norm_diag: bad argument");
    OP_BEGIN("ffvd_op_logdensity_norm_diag");
    if (N == 0) return FFVD_OK;
    const size_t nout = nonvec ? (size_t)N * J : (size_t)N;
    double *dy = sc.upload(y, (size_t)N * J), *dm = sc.upload(ymean, (size_t)N * J), *dR = sc.upload(Rchols, J);
    double *dO = sc.alloc<double>(nout);
    if (!dy || !dm || !dR || !dO) return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_logdensity_norm_diag: device allocation or upload failed");
    launch_logdensity(sc.stream, nonvec ? 1 : 0, dy, dm, dR, N, J, dO);
    OP_TRY(hipMemcpyAsync(out, dO, nout * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_get_rand(const double *mean, const double *var, const double *eps, int64_t n, double *out) {
    if (!mean || !var || !eps || !out || n < 0) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_get_rand: bad argument");
    OP_BEGIN("ffvd_op_get_rand");
    if (n == 0) return FFVD_OK;
    double *dm = sc.upload(mean, (size_t)n), *dv = sc.upload(var, (size_t)n), *de = sc.upload(eps, (size_t)n);
    double *dO = sc.alloc<double>((size_t)n);
    if (!dm || !dv || !de || !dO) return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_get_rand: device allocation or upload failed");
    launch_get_rand(sc.stream, dm, dv, de, (size_t)n, dO);
    OP_TRY(hipMemcpyAsync(out, dO, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_collapse_u_mean(int kind, const double *Lm_inverse_seq, const double *X_combine, const double *X,
                                       const double *Z, int T, int M, int P, int D, const double *logvariance,
                                       const double *loglengthscales, const double *Q, double *U_mean,
                                       double *H_inv_sqrt) {
    if (!Lm_inverse_seq || !X_combine || !X || !Z || !logvariance || !Q || !U_mean || !H_inv_sqrt || T < 1 || M < 1 ||
        P < 1 || P > MAXP || D < 1 || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_collapse_u_mean: bad argument");
    OP_BEGIN("ffvd_op_collapse_u_mean");
    const int Mp = round_up(M, NB), Tp = round_up(T, STRIP), ng = (Mp + 511) / 512;
    std::vector<double> &logQ = sc.host(D);
    for (int d = 0; d < D; ++d) logQ[d] = log(Q[d]);
    // slab per dim: rows [0,Mp) H, rows [Mp,2Mp) identity -> L_H^-T, row 2Mp carries b -> L_H^-1 b
    const size_t hstride = (size_t)(2 * Mp + NB) * Mp;
    std::vector<double> &Hinit = sc.host((size_t)D * hstride);
    for (int d = 0; d < D; ++d)
        for (int i = 0; i < Mp; ++i) Hinit[(size_t)d * hstride + (size_t)(Mp + i) * Mp + i] = 1.0;
    HyperView hv{};
    if (int rc = stage_hypers(sc, "ffvd_op_collapse_u_mean", kind, Z, M, Mp, P, D, logvariance, loglengthscales, hv)) return rc;
    double *dW = upload_stack(sc, Lm_inverse_seq, D, M, Mp);
    double *dXc = sc.upload(X_combine, (size_t)T * P), *dX = sc.upload(X, (size_t)(T + 1) * D);
    double *dlq = sc.upload(logQ.data(), D);
    double *F = sc.alloc<double>((size_t)D * Tp * Mp), *rowsq = sc.alloc<double>((size_t)D * ng * Tp);
    double *H = sc.upload(Hinit.data(), Hinit.size());
    double *dU = sc.alloc<double>((size_t)M * D);
    int32_t *info = sc.alloc<int32_t>(D);
    double *dinv = sc.alloc<double>(potrf_scratch_doubles(Mp, D));
    if (!dW || !dXc || !dX || !dlq || !F || !rowsq || !H || !dU || !info || !dinv)
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_collapse_u_mean: device allocation or upload failed");
    OP_TRY(hipMemsetAsync(info, 0, D * sizeof(int32_t), sc.stream));
    launch_project(sc.stream, op_project_args(kind, hv, dXc, T, Tp, P, M, Mp, D, dW, (size_t)Mp * Mp, nullptr, F, rowsq, nullptr, ng));
    GramArgs ga{};
    ga.mode = GRAM_F; ga.A = F; ga.a_stride = (size_t)Tp * Mp; ga.rows = Tp; ga.with_row = 1; ga.brow = 2 * Mp;
    ga.X = dX; ga.log_Q = dlq; ga.T = T; ga.D = D; ga.Mp = Mp; ga.Dl = D; ga.d_begin = 0;
    ga.b0 = 0; ga.nb = D; ga.yn_over_batch = 1.0; ga.H = H; ga.h_stride = hstride;     // :215,:217 (no batch rescaling)
    launch_gram(sc.stream, ga);
    launch_potrf_ext(sc.stream, H, Mp, Mp + NB, Mp, D, hstride, info, dinv);
    // U_mean[:, d] = H^-1 b = L_H^-T (L_H^-1 b)   (tf.linalg.solve, :219)
    launch_matvec(sc.stream, H + (size_t)Mp * Mp, hstride, H + (size_t)2 * Mp * Mp, hstride, Mp, dU, D, 1, M, D);
    std::vector<double> hH((size_t)D * hstride);
    OP_TRY(hipMemcpyAsync(hH.data(), H, hH.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(U_mean, dU, (size_t)M * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    if (int rc = fetch_chol_info(sc, info, D, "ffvd_op_collapse_u_mean", "H")) return rc;
    for (int d = 0; d < D; ++d)          // Lm_inverse_dd_seq = L_H^-T (:222)
        for (int i = 0; i < M; ++i)
            memcpy(H_inv_sqrt + ((size_t)d * M + i) * M, hH.data() + (size_t)d * hstride + (size_t)(Mp + i) * Mp,
                   (size_t)M * sizeof(double));
    return FFVD_OK;
}

extern "C" int ffvd_op_conditional_precalc(int kind, const double *Lm_inverse_seq, const double *Xnew, int N,
                                           const double *Z, int M, int P, int D, const double *logvariance,
                                           const double *loglengthscales, const double *f, const double *q_sqrt,
                                           double *mean, double *var) {
    if (!Lm_inverse_seq || !Xnew || !Z || !logvariance || !f || !mean || !var || N < 0 || M < 1 || M > 2048 || P < 1 ||
        P > MAXP || D < 1 || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_conditional_precalc: bad argument");
    OP_BEGIN("ffvd_op_conditional_precalc");
    if (N == 0) return FFVD_OK;
    const int Mp = round_up(M, NB), Tp = round_up(N, STRIP), ng = (Mp + 511) / 512;
    HyperView hv{};
    if (int rc = stage_hypers(sc, "ffvd_op_conditional_precalc", kind, Z, M, Mp, P, D, logvariance, loglengthscales, hv)) return rc;
    double *dW = upload_stack(sc, Lm_inverse_seq, D, M, Mp);
    double *dX = sc.upload(Xnew, (size_t)N * P), *dU = sc.upload(f, (size_t)M * D);
    double *F = sc.alloc<double>((size_t)D * Tp * Mp);
    double *rowsq = sc.alloc<double>((size_t)D * ng * Tp), *fmean = sc.alloc<double>((size_t)D * ng * Tp);
    double *dmean = sc.alloc<double>((size_t)N * D), *dvar = sc.alloc<double>((size_t)N * D);
    double *dQs = q_sqrt ? sc.upload(q_sqrt, (size_t)M * M) : nullptr;     // slice d = 0 only (the reference quirk)
    double *extra = q_sqrt ? sc.alloc<double>((size_t)D * Tp) : nullptr;
    if (!dW || !dX || !dU || !F || !rowsq || !fmean || !dmean || !dvar || (q_sqrt && (!dQs || !extra)))
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_conditional_precalc: device allocation or upload failed");
    // A^T = K_fu L^-T (:349), mean (:365), sum A^2 (:356)
    launch_project(sc.stream, op_project_args(kind, hv, dX, N, Tp, P, M, Mp, D, dW, (size_t)Mp * Mp, dU, q_sqrt ? F : nullptr, rowsq,
                                              fmean, ng));
    if (q_sqrt) launch_qsqrt_inflation(sc.stream, F, (size_t)Tp * Mp, Tp, Mp, M, dQs, extra, N, D);
    launch_conditional_finish(sc.stream, kind, dX, N, P, hv.variance, rowsq, fmean, ng, Tp, D, dmean, dvar, extra);
    OP_TRY(hipMemcpyAsync(mean, dmean, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(var, dvar, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

// Full predictive covariance / q_sqrt inflation of the conditional (ffvd_op_conditional_cov, ffvd_op_conditional_precalc_cov), once
// the stack W_d = L_d^-T (Mp x Mp, slab stride w_stride) and the hyper-parameters are on the device.  Mean and per-point variance run
// through the same launches as ffvd_op_conditional / ffvd_op_conditional_precalc (projection with F kept, conditional_finish); then
//   q_sqrt (M x M slice 0, as given):  E_d = F_d q0 (cov.hip, COV_GEN, q0^T uploaded once for all d);
//   full_cov:  Sigma_d = K_d(Xnew, Xnew) - F_d F_d^T (+ E_d E_d^T) (cov.hip, COV_SYM), var: D x N x N, its diagonal the per-point
//              variance (without q_sqrt: that of the full_cov = 0 form bit for bit; with it: the q_sqrt term summed from E's rows);
//   otherwise: var[:, d] += sum_j E_d[:, j]^2 through qsqrt_inflation (conditionals_multi_output.py:371-380), var: N x D.
static int conditional_cov_tail(Scratch &sc, const char *who, int kind, const HyperView &hv, const double *W, size_t w_stride,
                                const double *Xnew, int N, int M, int P, int D, const double *f, const double *q_sqrt, int full_cov,
                                double *mean, double *var) {
    const int Mp = round_up(M, NB), Tp = round_up(N, STRIP), ng = (Mp + 511) / 512;
    double *dX = sc.upload(Xnew, (size_t)N * P), *dU = sc.upload(f, (size_t)M * D);
    double *rowsq = sc.alloc<double>((size_t)D * ng * Tp), *fmean = sc.alloc<double>((size_t)D * ng * Tp);
    double *dmean = sc.alloc<double>((size_t)N * D), *dvar = sc.alloc<double>((size_t)N * D);
    double *F = sc.alloc<double>((size_t)D * Tp * Mp);
    if (!dX || !dU || !rowsq || !fmean || !dmean || !dvar || !F)
        return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation or upload failed");
    // F = A^T = K_fu L^-T (:34 / :349), mean (:48 / :365)
    launch_project(sc.stream, op_project_args(kind, hv, dX, N, Tp, P, M, Mp, D, W, w_stride, dU, F, rowsq, fmean, ng));
    if (!full_cov) {
        double *dQs = q_sqrt ? sc.upload(q_sqrt, (size_t)M * M) : nullptr, *extra = q_sqrt ? sc.alloc<double>((size_t)D * Tp) : nullptr;
        if (q_sqrt && (!dQs || !extra)) return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation or upload failed");
        if (q_sqrt) launch_qsqrt_inflation(sc.stream, F, (size_t)Tp * Mp, Tp, Mp, M, dQs, extra, N, D);
        launch_conditional_finish(sc.stream, kind, dX, N, P, hv.variance, rowsq, fmean, ng, Tp, D, dmean, dvar, extra);
        OP_TRY(hipMemcpyAsync(mean, dmean, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
        OP_TRY(hipMemcpyAsync(var, dvar, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
        OP_TRY(hipStreamSynchronize(sc.stream));
        return FFVD_OK;
    }
    double *E = nullptr, *extra = nullptr;
    if (q_sqrt) {
        std::vector<double> &qt = sc.host((size_t)Mp * Mp);          // q0^T, zero padded: row j = column j of q0
        for (int k = 0; k < M; ++k)
            for (int j = 0; j < M; ++j) qt[(size_t)j * Mp + k] = q_sqrt[(size_t)k * M + j];
        double *dQt = sc.upload(qt.data(), qt.size());
        E = sc.alloc<double>((size_t)D * Tp * Mp);
        extra = sc.alloc<double>((size_t)D * Tp);
        if (!dQt || !E || !extra) return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation or upload failed");
        CovArgs ea{};
        ea.mode = COV_GEN; ea.A = F; ea.a_stride = (size_t)Tp * Mp; ea.lda = Mp; ea.arows = Tp; ea.K = Mp;
        ea.B = dQt; ea.b_stride = 0; ea.ldb = Mp; ea.brows = Mp; ea.ncols = Mp;
        ea.C = E; ea.c_stride = (size_t)Tp * Mp; ea.ldc = Mp; ea.nb = D;
        launch_cov(sc.stream, ea);                                   // LTA^T = F q0 (:371-376, slice 0 for every dim)
        launch_row_sumsq(sc.stream, E, (size_t)Tp * Mp, Mp, Mp, N, D, Tp, extra);     // sum_j LTA^2 (:380)
    }
    // the per-point variance becomes the diagonal of Sigma_d
    launch_conditional_finish(sc.stream, kind, dX, N, P, hv.variance, rowsq, fmean, ng, Tp, D, dmean, dvar, extra);
    double *dS = sc.alloc<double>((size_t)D * N * N);
    if (!dS) return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation failed");
    CovArgs ca{};
    ca.mode = COV_SYM; ca.A = F; ca.E = E; ca.a_stride = (size_t)Tp * Mp; ca.lda = Mp; ca.arows = Tp; ca.K = Mp;
    ca.C = dS; ca.c_stride = (size_t)N * N; ca.ldc = N; ca.N = N; ca.kind = kind; ca.P = P; ca.x = dX;
    ca.variance = hv.variance; ca.len = hv.len; ca.diag = dvar; ca.nb = D;
    launch_cov(sc.stream, ca);                                       // K(Xnew) - A^T A (+ LTA^T LTA) (:41-44 full_cov branch)
    OP_TRY(hipGetLastError());
    OP_TRY(hipMemcpyAsync(mean, dmean, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    if (!sc.download(var, dS, (size_t)D * N * N * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, std::string(who) + ": device error while copying the covariance out");
    return FFVD_OK;
}

static bool cov_args_ok(int kind, const double *Xnew, int N, const double *Z, int M, int P, int D, const double *logvariance,
                        const double *loglengthscales, const double *f, const double *q_sqrt, int full_cov, const double *mean,
                        const double *var) {
    return Xnew && Z && logvariance && f && mean && var && N >= 0 && M >= 1 && P >= 1 && P <= MAXP && D >= 1 &&
           (kind == FFVD_KERNEL_SE || kind == FFVD_KERNEL_LINEAR) && (kind != FFVD_KERNEL_SE || loglengthscales) &&
           (full_cov == 0 || full_cov == 1) && (!q_sqrt || M <= 2048) &&
           (size_t)D * N * N <= ((size_t)1 << 40);
}

extern "C" int ffvd_op_conditional_cov(int kind, const double *Xnew, int N, const double *Z, int M, int P, int D,
                                       const double *logvariance, const double *loglengthscales, const double *f,
                                       const double *q_sqrt, int full_cov, double jitter, double *mean, double *var) {
    if (!cov_args_ok(kind, Xnew, N, Z, M, P, D, logvariance, loglengthscales, f, q_sqrt, full_cov, mean, var))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_conditional_cov: bad argument");
    OP_BEGIN("ffvd_op_conditional_cov");
    if (N == 0) return FFVD_OK;
    KuuWork w{};
    int rc = build_kuu(sc, "ffvd_op_conditional_cov", kind, Z, M, P, D, logvariance, loglengthscales, jitter, w);
    if (rc) return set_error(nullptr, rc, "ffvd_op_conditional_cov: device allocation or upload failed");
    const int Mp = w.Mp;
    rc = conditional_cov_tail(sc, "ffvd_op_conditional_cov", kind, w.hv, w.Kuu + (size_t)Mp * Mp, (size_t)2 * Mp * Mp, Xnew, N, M, P,
                              D, f, q_sqrt, full_cov, mean, var);
    if (rc) return rc;
    return fetch_chol_info(sc, w.info, D, "ffvd_op_conditional_cov", "K_uu + jitter*I");
}

extern "C" int ffvd_op_conditional_precalc_cov(int kind, const double *Lm_inverse_seq, const double *Xnew, int N, const double *Z,
                                               int M, int P, int D, const double *logvariance, const double *loglengthscales,
                                               const double *f, const double *q_sqrt, int full_cov, double *mean, double *var) {
    if (!Lm_inverse_seq || !cov_args_ok(kind, Xnew, N, Z, M, P, D, logvariance, loglengthscales, f, q_sqrt, full_cov, mean, var))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_conditional_precalc_cov: bad argument");
    OP_BEGIN("ffvd_op_conditional_precalc_cov");
    if (N == 0) return FFVD_OK;
    const int Mp = round_up(M, NB);
    HyperView hv{};
    if (int rc = stage_hypers(sc, "ffvd_op_conditional_precalc_cov", kind, Z, M, Mp, P, D, logvariance, loglengthscales, hv)) return rc;
    double *dW = upload_stack(sc, Lm_inverse_seq, D, M, Mp);
    OP_CHECK(dW, "ffvd_op_conditional_precalc_cov");
    return conditional_cov_tail(sc, "ffvd_op_conditional_precalc_cov", kind, hv, dW, (size_t)Mp * Mp, Xnew, N, M, P, D, f, q_sqrt,
                                full_cov, mean, var);
}

extern "C" int ffvd_op_get_rand_full_cov(const double *mean, const double *var, const double *eps, int N, int D, double jitter,
                                         double *out) {
    if (!mean || !var || !eps || !out || N < 0 || D < 1 || !(jitter >= 0.0) || (size_t)D * N * N > ((size_t)1 << 40))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_get_rand_full_cov: bad argument");
    OP_BEGIN("ffvd_op_get_rand_full_cov");
    if (N == 0) return FFVD_OK;
    const int np = round_up(N, NB);
    const size_t slab = (size_t)np * np;
    std::vector<double> &pad = pad_identity(sc, var, D, N, np, jitter);      // Sigma_d + jitter I, identity padded to np
    double *dA = sc.upload(pad.data(), pad.size());
    double *dm = sc.upload(mean, (size_t)N * D), *de = sc.upload(eps, (size_t)N * D), *dO = sc.alloc<double>((size_t)N * D);
    int32_t *dinfo = sc.alloc<int32_t>(D);
    double *dinv = sc.alloc<double>(potrf_scratch_doubles(np, D));
    if (!dA || !dm || !de || !dO || !dinfo || !dinv)
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_get_rand_full_cov: device allocation or upload failed");
    std::vector<int32_t> hinfo(D, 0);
    int rc = potrf_with_stall_recovery(sc, dA, pad.data(), np, D, dinfo, dinv, hinfo.data(), "ffvd_op_get_rand_full_cov");
    if (rc) return rc;
    for (int d = 0; d < D; ++d)
        if (hinfo[d]) return chol_not_pd("ffvd_op_get_rand_full_cov", "var[" + std::to_string(d) + "] + jitter*I", d, hinfo[d]);
    launch_tril_matvec(sc.stream, dA, slab, np, N, D, dm, de, dO);    // mean + L eps (utils.py:4-11, full_cov branch)
    OP_TRY(hipGetLastError());
    OP_TRY(hipMemcpyAsync(out, dO, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_adam_step(double *theta, const double *grad, double *m, double *v, int64_t n, double lr,
                                 double beta1, double beta2, double eps, int64_t t) {
    if (!theta || !grad || !m || !v || n < 0 || t < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_adam_step: bad argument");
    OP_BEGIN("ffvd_op_adam_step");
    if (n == 0) return FFVD_OK;
    double *dth = sc.upload(theta, n), *dm = sc.upload(m, n), *dv = sc.upload(v, n);
    const double *dg = sc.upload(grad, n);
    if (!dth || !dm || !dv || !dg) return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_adam_step: device allocation or upload failed");
    OptTable tab{};
    tab.count = 1;
    tab.t[0].theta = dth; tab.t[0].grad = dg; tab.t[0].s0 = dm; tab.t[0].s1 = dv; tab.t[0].n = n;
    const double lr_t = lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t));
    launch_adam(sc.stream, tab, lr_t, beta1, beta2, eps);
    OP_TRY(hipMemcpyAsync(theta, dth, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(m, dm, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(v, dv, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_sghmc_step(double *theta, const double *grad, double *xi, double *g, double *g2, double *p,
                                  const double *noise, int64_t n, double epsilon, double mdecay, double X_N, int burn_in) {
    if (!theta || !grad || !xi || !g || !g2 || !p || !noise || n < 0 || !(X_N > 0.0))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_sghmc_step: bad argument");
    OP_BEGIN("ffvd_op_sghmc_step");
    if (n == 0) return FFVD_OK;
    double *dth = sc.upload(theta, n), *dxi = sc.upload(xi, n), *dg_ = sc.upload(g, n), *dg2 = sc.upload(g2, n);
    double *dp = sc.upload(p, n);
    const double *dgrad = sc.upload(grad, n), *dnoise = sc.upload(noise, n);
    if (!dth || !dxi || !dg_ || !dg2 || !dp || !dgrad || !dnoise)
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_sghmc_step: device allocation or upload failed");
    OptTable tab{};
    tab.count = 1;
    OptTensor &t = tab.t[0];
    t.theta = dth; t.grad = dgrad; t.s0 = dxi; t.s1 = dg_; t.s2 = dg2; t.s3 = dp; t.noise = dnoise; t.n = n;
    launch_sghmc(sc.stream, tab, epsilon, mdecay, X_N, burn_in);
    OP_TRY(hipMemcpyAsync(theta, dth, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(p, dp, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    if (burn_in) {
        OP_TRY(hipMemcpyAsync(xi, dxi, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
        OP_TRY(hipMemcpyAsync(g, dg_, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
        OP_TRY(hipMemcpyAsync(g2, dg2, n * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    }
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

// ---- step loops: posterior rollouts and the particle-Gibbs sweep -----------------------------------------------------------------------
// What a rollout step and a particle-Gibbs step share.  K_fu rows once per step, then the triangular projection GEMM with fvar / fmean
// in its epilogue (one workgroup per 128-column tile and dim): 16 workgroups instead of the 4 of the fused projection kernel, whose
// single workgroup per dim made a step compute-bound on one CU.
// Few rows per step (R rollouts / particles): the skinny product (kernels.hip) with one partial sum per 16-column slab replaces the
// 128 x 128-tile projection GEMM (50 -> 7 us per step) and the per-row q_sqrt kernel (37 us).
struct StepSetup {
    int R, D, Mp, Tp, ng;
    bool skinny;
    int ngs;                                    // partial sums per row in rowsq / fmean: 16-column slabs (skinny) or 128-column tiles
    double *Kf = nullptr, *ucol = nullptr, *rowsq = nullptr, *fmean = nullptr;
    ProjectArgs pa{};                           // K(x_t, Z) rows (pa.x: the step's input rows)
    ProjGemmArgs pg{};                          // tiled step: F = K_fu L^-T
    SkinnyArgs sk{};                            // skinny step: the same product from the k-major rows of launch_kfu_build_t
    StepSetup(Scratch &sc, int R_, int M, int D_)
        : R(R_), D(D_), Mp(round_up(M, NB)), Tp(round_up(R_, STRIP)), ng((Mp + 127) / 128), skinny(R_ <= 512), ngs(skinny ? Mp / 16 : ng) {
        Kf = sc.alloc<double>((size_t)D * Tp * Mp), ucol = sc.alloc<double>((size_t)D * Mp);
        rowsq = sc.alloc<double>((size_t)D * ngs * Tp), fmean = sc.alloc<double>((size_t)D * ngs * Tp);
    }
    bool ok() const { return Kf && ucol && rowsq && fmean; }
    // x: the R start rows; W = L^-T stack, U: inducing outputs (M x D); F: where the tiled step keeps F, or null; WQ (skinny step,
    // optional): W q_sqrt as second right-hand side, its slab sums of squares into extra.  Enqueues the columns of U (ucol).
    void fill(Scratch &sc, int kind, const HyperView &hv, const double *x, int P, int M, const double *W, const double *U, double *F,
              const double *WQ, double *extra, int q_upper) {
        const size_t msq = (size_t)Mp * Mp, fst = (size_t)Tp * Mp;
        pa = op_project_args(kind, hv, x, R, Tp, P, M, Mp, D, W, msq, U, Kf, rowsq, fmean, ng);
        launch_ucols(sc.stream, U, M, Mp, D, 0, D, ucol);
        pg.Kf = Kf; pg.kf_stride = fst; pg.W = W; pg.w_stride = msq; pg.F = F; pg.f_stride = F ? fst : 0;
        pg.rowsq = rowsq; pg.fmean = fmean; pg.u = ucol; pg.u_stride = Mp; pg.Tp = Tp; pg.Mp = Mp; pg.Dl = D; pg.b0 = 0; pg.nb = D;
        sk = SkinnyArgs{Kf, fst, Tp, W, msq, Mp, 1, R, Mp, Mp, D, Tp, nullptr, 0, 0, ucol, (size_t)Mp, rowsq, fmean,
                        WQ, WQ ? msq : 0, WQ ? Mp : 0, WQ ? Mp : 0, WQ ? extra : nullptr, 1, WQ ? q_upper : 0};
    }
    // the persistent loop kernels (loops.hip) build K(x_t, Z) row-major
    SkinnyArgs loop_sk() const {
        SkinnyArgs s = sk;
        s.lda = Mp; s.a_trans = 0;
        return s;
    }
};

// the R x (D + C) input rows of step 0: a state (x_stride = 0: the same for every row) and the control row of step 0
static std::vector<double> &start_rows(Scratch &sc, const double *x, int x_stride, const double *ctrl, int R, int D, int C) {
    const int P = D + C;
    std::vector<double> &xc0 = sc.host((size_t)R * P);
    for (int r = 0; r < R; ++r) {
        for (int d = 0; d < D; ++d) xc0[(size_t)r * P + d] = x[(size_t)r * x_stride + d];
        for (int c = 0; c < C; ++c) xc0[(size_t)r * P + D + c] = ctrl[c];
    }
    return xc0;
}

// FFVD_STEP_LOOP=1: the whole loop as one persistent launch (launch_loop gets the zeroed counter block).  If a wait gave up (the grid
// was not resident at once) the start rows are uploaded again and the per-step launches run.
template <class LaunchLoop, class StepLaunches>
static int run_step_loop(Scratch &sc, const char *who, int D, double *dxc, const std::vector<double> &xc0, LaunchLoop launch_loop,
                         StepLaunches step_launches) {
    const int nwords = loop_words(D);
    int32_t *words = sc.alloc<int32_t>(nwords);
    if (!words) return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation or upload failed");
    OP_TRY(hipMemsetAsync(words, 0, (size_t)nwords * sizeof(int32_t), sc.stream));
    launch_loop(words);
    int32_t hw[4] = {0, 0, 0, 0};
    OP_TRY(hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    if (hw[1] != 0) {
        OP_TRY(hipMemcpyAsync(dxc, xc0.data(), xc0.size() * sizeof(double), hipMemcpyHostToDevice, sc.stream));
        step_launches();
    }
    return FFVD_OK;
}

// W = L^-T is upper triangular; when q_sqrt (one M x M slice) is too -- the reference hands over L_H^-T -- so is W q_sqrt, and the second
// right-hand side of a step's product stops at a slab's last row like the first (exact zeros are skipped: half of its k range)
static bool q_sqrt_is_upper(const double *q, int M) {
    for (int i = 1; i < M; ++i)
        for (int j = 0; j < i; ++j)
            if (q[(size_t)i * M + j] != 0.0) return false;
    return true;
}

extern "C" int ffvd_op_rollout_fallbacks(void) { return g_rollout_fallbacks; }

extern "C" int ffvd_op_rollout(int kind, const double *Lm_inverse_seq, const double *Z, int M, int P, int D,
                               const double *logvariance, const double *loglengthscales, const double *f,
                               const double *q_sqrt, const double *x_last, int R, const double *ctrl, int C, int steps,
                               const double *log_Q, const double *eps, double *predict_x, double *predict_var) {
    if (!Lm_inverse_seq || !Z || !logvariance || !f || !x_last || !log_Q || !eps || !predict_x || !predict_var || R < 1 ||
        steps < 0 || M < 1 || M > 2048 || D < 1 || C < 0 || P != D + C || P > MAXP || (C > 0 && !ctrl) ||
        (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_rollout: bad argument");
    OP_BEGIN("ffvd_op_rollout");
    if (steps == 0) return FFVD_OK;
    StepSetup st(sc, R, M, D);
    const int Mp = st.Mp, Tp = st.Tp, ng = st.ng, ngs = st.ngs;
    const bool skinny = st.skinny;
    std::vector<double> &xc0 = start_rows(sc, x_last, 0, ctrl, R, D, C);   // x_t = X[-1] (:226), every rollout; control row of step 0 (:293)
    HyperView hv{};
    if (int rc = stage_hypers(sc, "ffvd_op_rollout", kind, Z, M, Mp, P, D, logvariance, loglengthscales, hv)) return rc;
    double *dW = upload_stack(sc, Lm_inverse_seq, D, M, Mp);
    double *dxc = sc.upload(xc0.data(), xc0.size()), *dU = sc.upload(f, (size_t)M * D);
    double *dxc2 = sc.alloc<double>(xc0.size());          // the rows of step t + 1 (the step kernel reads one buffer and writes the other)
    double *dlq = sc.upload(log_Q, D), *deps = sc.upload(eps, (size_t)steps * R * D);
    double *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    double *F = q_sqrt ? sc.alloc<double>((size_t)D * Tp * Mp) : nullptr;
    double *dpx = sc.alloc<double>((size_t)R * steps * D), *dpv = sc.alloc<double>((size_t)R * steps * D);
    const int q_upper = (q_sqrt && skinny && q_sqrt_is_upper(q_sqrt, M)) ? 1 : 0;
    double *dQs = q_sqrt ? (skinny ? upload_stack(sc, q_sqrt, 1, M, Mp) /* (F is zero in the padded columns) */ : sc.upload(q_sqrt, (size_t)M * M)) : nullptr;   // slice d = 0 only
    double *extra = q_sqrt ? sc.alloc<double>((size_t)D * (skinny ? ngs : 1) * Tp) : nullptr;
    // skinny path: W q_sqrt once per call (D products of M^3), so that the inflation term is a second right-hand side of the
    // step's one product instead of a dependent product on F
    double *dWQ = (q_sqrt && skinny) ? sc.alloc<double>((size_t)D * Mp * Mp) : nullptr;
    if (!dW || !dxc || !dxc2 || !dU || !dlq || !deps || (C && !dctrl) || !st.ok() || !dpx || !dpv || (q_sqrt && (!dQs || !extra || !F)) ||
        (q_sqrt && skinny && !dWQ))
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_rollout: device allocation or upload failed");
    st.fill(sc, kind, hv, dxc, P, M, dW, dU, F, dWQ, extra, q_upper);
    // the whole loop is enqueued at once: steps x (K_fu rows, projection, [q_sqrt inflation], conditional, update)
    if (dWQ)
        ffvd::launch_skinny_gemm(sc.stream, dW, (size_t)Mp * Mp, Mp, dQs, 0, Mp, 0, Mp, Mp, Mp, D, Mp, dWQ, (size_t)Mp * Mp, Mp, nullptr, 0,
                                 nullptr, nullptr);
    double *xbuf[2] = {dxc, dxc2};                                           // input rows of step t in xbuf[t & 1]
    auto step_launches = [&]() {                                              // three dependent launches per step
        for (int t = 0; t < steps; ++t) {
            st.pa.x = xbuf[t & 1];
            if (skinny) {
                launch_kfu_build_t(sc.stream, st.pa, Tp);                            // K(x_t, Z) per dim, m-major (coalesced operand loads)
                // conditional_after_kernel_precalculation (:300) and, in the same launch, sum_j (F q_sqrt)_j^2 = |K (W q_sqrt)|^2 (:371-380)
                launch_skinny_gemm(sc.stream, st.sk);
            } else {
                launch_kfu_build(sc.stream, st.pa);                                  // K(x_t, Z) per dim
                launch_proj_gemm(sc.stream, st.pg);
                if (q_sqrt) launch_qsqrt_inflation(sc.stream, F, (size_t)Tp * Mp, Tp, Mp, M, dQs, extra, R, D);
            }
            // conditional epilogue + x <- x + f_mu + eps sqrt(f_var + Q) in one launch (three dependent launches per step instead of five)
            launch_rollout_finish_update(sc.stream, kind, hv.variance, st.rowsq, st.fmean, skinny ? ngs : ng, Tp, extra, skinny ? ngs : 1, dlq,
                                         deps + (size_t)t * R * D, (C && t + 1 < steps) ? dctrl + (size_t)(t + 1) * C : nullptr, R, D, C, t,
                                         steps, xbuf[t & 1], xbuf[(t + 1) & 1], dpx, dpv);
        }
    };
    // Round 4: the whole loop as ONE persistent launch (loops.hip; the same kernel bodies: bit-identical) -- first
    // with a grid-wide barrier between the phases (64.7 against 32.7 us per step at 32 rollouts: 160-512 workgroups on one counter),
    // then with one role per workgroup and per-unit counters (40.3 against 36.0; 93 against 57 at 100 rollouts).  MEASURED SLOWER both
    // times: ~170 agent-scope releases / acquires per step cost more than the three kernel boundaries they replace -- so it is opt-in:
    // FFVD_STEP_LOOP=1.
    const char *nsl = getenv("FFVD_STEP_LOOP");
    const int loop_mode = (nsl && *nsl) ? atoi(nsl) : -1;
    // Third form (loops.hip, rollout_resident_kernel; FFVD_STEP_LOOP=2): L^-T and W q_sqrt stay in LDS for the whole loop, three hand-offs
    // per step.  Measured as the slope between 200 and 800 steps at M = 512, D = 4 (tools/rollout_modes.py): 16.6-19.2 us per step at 16
    // rollouts, 19.3-23.9 at 32, 27-50 at 64 against 19.6-20.8 / 20.1-20.6 / 20.5-25.7 for the launches -- a hand-off among 32 workgroups
    // costs 4-5 us here (release 2, wait + acquire 2.5-3: FFVD_RR_STAMPS=1), three of them are what three kernel boundaries cost.
    // (Second measurement, with the hand-offs rebuilt without cache maintenance -- write-through stores and sc1 loads instead of fences, as in
    //  the Gram kernel's tail exchange: 10.1-11.8 us per step at 16 rollouts, 13.6-17.9 at 32, 20.5-27 at 64.  The default up to 32 rollouts.)
    // (Third measurement, the products' MFMA section branch-free per chunk: 10.4-12.5 / 12.5-15.4 / 17.9-22.5 us per step.  The default
    //  wherever it applies: up to 64 rollouts, M <= 512, 8 latent dims.)
    // (Round 5: with K^T operands, the XCD-mapped grid and long / short slabs paired per CU the per-step launches take 15.4-15.6 us
    //  (18.4-21.8 with q_sqrt) from 40 to 64 rollouts, the resident loop 16.6-18.6 (20.3-23.4); at 32: 15.0 / 16.6 against 12.7 / 14.9,
    //  profiles/r05_rollout_modes.txt -- the resident loop is the default up to 32 rollouts, FFVD_STEP_LOOP=2 asks for it up to 64.)
    const bool resident = skinny && rollout_resident_ok(R, D, P, Mp) && (loop_mode == 2 || (loop_mode < 0 && R <= 32));
    const bool use_loop = skinny && loop_mode == 1;
    bool resident_done = false;
    if (resident) {
        const int RT = (R + 15) / 16, RP = 16 * RT, NS = Mp / 16;
        int32_t *words = sc.alloc<int32_t>(rollout_resident_words());
        double *Kt = sc.alloc<double>((size_t)D * Mp * RP), *part = sc.alloc<double>((size_t)D * NS * RP * 4);
        double *xb = sc.alloc<double>((size_t)2 * RP * D), *dxl = sc.upload(x_last, D);
        OP_CHECK(words && Kt && part && xb && dxl, "ffvd_op_rollout");
        OP_TRY(hipMemsetAsync(words, 0, (size_t)rollout_resident_words() * sizeof(int32_t), sc.stream));
        RolloutResidentArgs ra{};
        ra.kind = kind; ra.R = R; ra.RT = RT; ra.D = D; ra.C = C; ra.P = P; ra.M = M; ra.Mp = Mp; ra.steps = steps; ra.NS = NS;
        ra.hv = hv; ra.W = dW; ra.w_stride = (size_t)Mp * Mp; ra.WQ = q_sqrt ? dWQ : nullptr; ra.wq_upper = q_sqrt ? q_upper : 0; ra.ucol = st.ucol;
        ra.log_Q = dlq; ra.eps = deps; ra.ctrl = dctrl; ra.x_last = dxl; ra.Kt = Kt; ra.part = part; ra.xbuf = xb;
        ra.predict_x = dpx; ra.predict_var = dpv; ra.words = words; ra.abort_w = words + 1;
        long long *dst = nullptr;
        if (getenv("FFVD_RR_STAMPS")) { dst = sc.alloc<long long>(32); if (dst) OP_TRY(hipMemsetAsync(dst, 0, 32 * sizeof(long long), sc.stream)); }
        ra.stamps = dst;
        ra.test_stall = getenv("FFVD_RR_TEST_STALL") ? 1 : 0;
        const int lrc = launch_rollout_resident(sc.stream, ra);
        if (lrc == 0) {
            int32_t hw[4] = {0, 0, 0, 0};
            OP_TRY(hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, sc.stream));
            OP_TRY(hipStreamSynchronize(sc.stream));
            resident_done = hw[1] == 0;          // (a wait gave up: the per-step launches below, from the initial rows)
            if (!resident_done) {
                // the two forms agree to 1e-9, not bit for bit, so a fallback decided by run-time contention must not be
                // silent -- counted (ffvd_op_rollout_fallbacks) and left as a warning for ffvd_last_error(NULL)
                ++g_rollout_fallbacks;
                set_error(nullptr, FFVD_OK,
                          "warning: ffvd_op_rollout: the resident-operand loop gave up on a bounded wait (its workgroups were not all "
                          "resident: another tenant on the GPU?); the call was completed by the per-step launches, whose results "
                          "agree to 1e-9 but are not bit-identical (FFVD_STEP_LOOP=0 selects them always)");
            }
            if (dst && steps > 10) {             // tools: where step 10 spent its time (us since its start), slab 0 (the updater) and the last slab of dim 0
                long long hs[32];
                OP_TRY(hipMemcpy(hs, dst, sizeof hs, hipMemcpyDeviceToHost));
                static const char *nm[12] = {"start", "x_t seen", "inputs staged", "K stored", "K counted", "all K seen", "products", "partials stored",
                                             "partials counted", "all partials seen", "updated", "x counted"};
                for (int w = 0; w < 2; ++w) {
                    fprintf(stderr, "rollout_resident R=%d q=%d slab %s:", R, q_sqrt ? 1 : 0, w ? "last" : "0");
                    for (int i = 1; i < 12; ++i) if (hs[16 * w + i]) fprintf(stderr, "  %s %.2f", nm[i], (double)(hs[16 * w + i] - hs[16 * w]) / 100.0);
                    fprintf(stderr, "\n");
                }
            }
        } else (void)hipGetLastError();
    }
    if (resident_done) {
    } else if (use_loop) {
        RolloutLoopArgs la{};
        la.pa = st.pa;
        la.sk = st.loop_sk();
        la.f = FinishIn{kind, D + C, ngs, Tp, D, ngs, hv.variance, st.rowsq, st.fmean, extra};
        la.log_Q = dlq; la.eps = deps; la.ctrl = dctrl; la.R = R; la.C = C; la.steps = steps;
        la.xbuf0 = xbuf[0]; la.xbuf1 = xbuf[1]; la.predict_x = dpx; la.predict_var = dpv;
        const int rc = run_step_loop(sc, "ffvd_op_rollout", D, dxc, xc0, [&](int32_t *words) {
            la.bar = reinterpret_cast<unsigned *>(words); la.abort_w = words + 1;
            launch_rollout_loop(sc.stream, la);
        }, step_launches);
        if (rc) return rc;
    } else step_launches();
    OP_TRY(hipGetLastError());
    OP_TRY(hipMemcpyAsync(predict_x, dpx, (size_t)R * steps * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipMemcpyAsync(predict_var, dpv, (size_t)R * steps * D * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

// ---- rollout summaries (predict_summary.h) --------------------------------------------------------------------------------------------
// The held-out predictive summary of base_model.py:330-348 over all rollouts of a call, formed on the device stacks.
namespace {
struct SummaryReq {
    const double *CC, *DD, *noise_std;           // D x J, J, J
    int J;
    const double *Y_test;                        // n_test x J or NULL
    int n_test;
    double *y_mean, *y_var, *y_var_total;        // steps x J, each may be NULL
    double *lpd, *lpd_gauss;                     // n_test x J, each may be NULL
};

// the checks that need no array (before the "nothing to do" return) and those that read the small arrays (after it)
bool summary_scalars_ok(const SummaryReq &q, long long N, int steps, int D) {
    if (q.J < 1 || q.J > PS_MAXJ || D < 1 || D > MAXP || N < 0 || steps < 0 || q.n_test < 0 || q.n_test > steps) return false;
    return N == 0 || steps == 0 || N <= ((1LL << 31) - 1) / steps / D;              // N * steps * D < 2^31 elements per stack
}
bool summary_arrays_ok(const SummaryReq &q) {
    if (!q.CC || !q.DD || !q.noise_std || !(q.y_mean || q.y_var || q.y_var_total || q.lpd || q.lpd_gauss)) return false;
    if ((q.n_test > 0 || q.lpd || q.lpd_gauss) && !q.Y_test) return false;
    for (int j = 0; j < q.J; ++j)
        if (!std::isfinite(q.noise_std[j]) || !(q.noise_std[j] > 0.0)) return false;
    return true;
}

// The two launches of predict_summary.h on stacks that are on the device, then the requested outputs come down (one small copy).
int run_summary(Scratch &sc, const std::string &who, const double *dpx, const double *dpv, int N, int steps, int D, const SummaryReq &q) {
    const int J = q.J;
    const size_t SJ = (size_t)steps * J, TJ = (size_t)q.n_test * J;
    PredictSummaryArgs a{};
    a.N = N; a.steps = steps; a.D = D; a.J = J; a.n_test = q.n_test; a.x = dpx; a.v = dpv;
    a.CC = sc.upload(q.CC, (size_t)D * J); a.DD = sc.upload(q.DD, J); a.sd = sc.upload(q.noise_std, J);
    a.Y = q.n_test ? sc.upload(q.Y_test, TJ) : nullptr;
    a.part = sc.alloc<double>(ps_part_doubles(N, steps, J));
    a.out = sc.alloc<double>(ps_out_doubles(steps, J));
    if (!a.CC || !a.DD || !a.sd || (q.n_test && !a.Y) || !a.part || !a.out)
        return set_error(nullptr, FFVD_ENOMEM, who + ": device allocation or upload failed");
    launch_predict_summary(sc.stream, a);
    OP_TRY(hipGetLastError());
    std::vector<double> &h = sc.host(ps_out_doubles(steps, J));
    OP_TRY(hipMemcpyAsync(h.data(), a.out, h.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    double *const dst[5] = {q.y_mean, q.y_var, q.y_var_total, q.lpd, q.lpd_gauss};
    for (int f = 0; f < 5; ++f)
        if (dst[f]) memcpy(dst[f], h.data() + f * SJ, (f < 3 ? SJ : TJ) * sizeof(double));
    return FFVD_OK;
}
}  // namespace

// base_model.py:330-348 for stacks the caller holds: they are uploaded, summarised by the same launches as in the fused calls
extern "C" int ffvd_op_rollout_summary(const double *predict_x, const double *predict_var, int N, int steps, int D, const double *CC,
                                       const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                                       double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss) {
    const char *bad = "ffvd_op_rollout_summary: bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    if (!summary_scalars_ok(q, N, steps, D)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (N == 0 || steps == 0) return FFVD_OK;
    if (!predict_x || !predict_var || !summary_arrays_ok(q)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN("ffvd_op_rollout_summary");
    const size_t n = (size_t)N * steps * D;
    double *dpx = sc.upload(predict_x, n), *dpv = sc.upload(predict_var, n);
    OP_CHECK(dpx && dpv, "ffvd_op_rollout_summary");
    return run_summary(sc, "ffvd_op_rollout_summary", dpx, dpv, N, steps, D, q);
}

// G posteriors, one launch per step for all of them (rollout_group.hip).  sum: the rollouts are also summarised where the step
// launches wrote them, before any download, and predict_x / predict_var may each be NULL (not downloaded).
static int rollout_grouped_run(const std::string &who, int kind, int G, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                               int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                               const double *const *q_sqrts, const double *x_lasts, int R, const double *ctrl, int C, int steps,
                               const double *log_Qs, const double *eps, double *predict_x, double *predict_var, const SummaryReq *sum) {
    const std::string bad = who + ": bad argument";
    if ((kind != FFVD_KERNEL_SE && kind != FFVD_KERNEL_LINEAR) || G < 0 || R < 1 || steps < 0 || M < 1 || M > 2048 || D < 1 || C < 0 ||
        P != D + C || P > MAXP)
        return set_error(nullptr, FFVD_EINVAL, bad);
    const int Mp = round_up(M, RG_SLAB), NS = Mp / RG_SLAB;
    if ((long long)G * D * Mp * Mp > (1LL << 29) || (long long)G * R > (1LL << 20) || (R + RG_RC - 1) / RG_RC > 65535 ||
        (long long)G * D * NS >= (1LL << 31))
        return set_error(nullptr, FFVD_EINVAL, bad + " (beyond the limits of rollout_group.h)");
    if (sum && !summary_scalars_ok(*sum, (long long)G * R, steps, D)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !fs || !x_lasts || !log_Qs || !eps || (!sum && (!predict_x || !predict_var)) ||
        (C > 0 && !ctrl) || (kind == FFVD_KERNEL_SE && !loglengthscales) || (sum && !summary_arrays_ok(*sum)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t GD = (size_t)G * D, out_n = (size_t)G * R * steps * D;
    for (size_t b = 0; b < GD; ++b) if (!Lm_inverse_seqs[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    if (q_sqrts)
        for (int g = 0; g < G; ++g) if (!q_sqrts[g]) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN_AS(who);
    LapTimer timer("FFVD_RG_TIMING", who.c_str(), sc.stream);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, GD, M, Mp);
    timer.lap("W uploaded");
    // W q_sqrt is upper triangular when every group's q_sqrt slice is (the reference hands over L_H^-T): the step products then stop at
    // a slab's last row for both right-hand sides.  Otherwise they walk all rows; for a group whose slice IS upper triangular the extra
    // terms are exact zeros, so its results do not depend on what the other groups hold.
    int q_upper = q_sqrts ? 1 : 0;
    for (int g = 0; q_upper && g < G; ++g) q_upper = q_sqrt_is_upper(q_sqrts[g], M) ? 1 : 0;
    timer.lap("q_sqrt scanned");
    double *dq = q_sqrts ? upload_matrix_table(sc, q_sqrts, (size_t)G, M, Mp) : nullptr;
    double *dB = q_sqrts ? sc.alloc<double>(GD * Mp * Mp) : nullptr;
    double *dZ = sc.upload(Zs, (size_t)G * M * P), *dU = sc.upload(fs, (size_t)G * M * D), *dxl = sc.upload(x_lasts, GD);
    double *dlv = sc.upload(logvariances, GD), *dll = loglengthscales ? sc.upload(loglengthscales, GD * P) : nullptr;
    double *dlq = sc.upload(log_Qs, GD), *deps = sc.upload(eps, (size_t)steps * G * R * D);
    double *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    double *variance = sc.alloc<double>(GD), *len = sc.alloc<double>(GD * P), *Zsc = sc.alloc<double>(GD * Mp * P), *zz = sc.alloc<double>(GD * Mp);
    double *part = sc.alloc<double>((size_t)2 * GD * NS * R * 4), *xbuf = sc.alloc<double>((size_t)2 * G * R * D);
    double *dpx = sc.alloc<double>(out_n), *dpv = sc.alloc<double>(out_n);
    OP_CHECK_AS(dW && dZ && dU && dxl && dlv && dlq && deps && (!C || dctrl) && (!loglengthscales || dll) && variance && len && Zsc && zz &&
             part && xbuf && dpx && dpv && (!q_sqrts || (dq && dB)), who);
    timer.lap("q_sqrt, small arrays uploaded");
    launch_rg_prep(sc.stream, kind, G, D, M, Mp, P, dZ, dlv, dll, variance, len, Zsc, zz);
    if (q_sqrts) launch_rg_wq(sc.stream, G, D, Mp, q_upper, dW, dq, dB);
    timer.lap("hyper-parameters, W q_sqrt");
    RolloutGroupArgs a{};
    a.kind = kind; a.G = G; a.R = R; a.D = D; a.C = C; a.P = P; a.M = M; a.Mp = Mp; a.NS = NS; a.steps = steps;
    a.has_q = q_sqrts ? 1 : 0; a.q_upper = q_upper;
    a.W = dW; a.B = dB; a.Zs = Zsc; a.zz = zz; a.variance = variance; a.len = len; a.f = dU; a.x_last = dxl; a.log_Q = dlq;
    a.ctrl = dctrl; a.eps = deps; a.part = part; a.xbuf = xbuf; a.predict_x = dpx; a.predict_var = dpv;
    for (int t = 0; t <= steps; ++t) launch_rg_step(sc.stream, a, t);
    OP_TRY(hipGetLastError());
    timer.lap("step launches");
    if (sum) {
        if (int rc = run_summary(sc, who, dpx, dpv, G * R, steps, D, *sum)) return rc;
        timer.lap("summary");
    }
    if ((predict_x && !sc.download(predict_x, dpx, out_n * sizeof(double))) ||
        (predict_var && !sc.download(predict_var, dpv, out_n * sizeof(double))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    timer.lap("results downloaded");
    return FFVD_OK;
}

extern "C" int ffvd_op_rollout_grouped(int kind, int G, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                                       const double *logvariances, const double *loglengthscales, const double *fs,
                                       const double *const *q_sqrts, const double *x_lasts, int R, const double *ctrl, int C, int steps,
                                       const double *log_Qs, const double *eps, double *predict_x, double *predict_var) {
    return rollout_grouped_run("ffvd_op_rollout_grouped", kind, G, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts,
                               x_lasts, R, ctrl, C, steps, log_Qs, eps, predict_x, predict_var, nullptr);
}

extern "C" int ffvd_op_rollout_grouped_summary(int kind, int G, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                               int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                               const double *const *q_sqrts, const double *x_lasts, int R, const double *ctrl, int C,
                                               int steps, const double *log_Qs, const double *eps, double *predict_x,
                                               double *predict_var, const double *CC, const double *DD, const double *noise_std, int J,
                                               const double *Y_test, int n_test, double *y_mean, double *y_var, double *y_var_total,
                                               double *lpd, double *lpd_gauss) {
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    return rollout_grouped_run("ffvd_op_rollout_grouped_summary", kind, G, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs,
                               q_sqrts, x_lasts, R, ctrl, C, steps, log_Qs, eps, predict_x, predict_var, &q);
}

extern "C" int ffvd_op_pg_sweep(int kind, const double *Lm_inverse_seq, const double *Z, int M, int P, int D,
                                const double *logvariance, const double *loglengthscales, const double *U,
                                const double *X_ref, int X_N, const double *Y, int Ydim, const double *ctrl, int C,
                                const double *CC, const double *DD, const double *Rchols, const double *log_Q, int n_free,
                                const double *x0, const double *eps, const double *unif, double *particles, int32_t *idx) {
    if (!Lm_inverse_seq || !Z || !logvariance || !U || !X_ref || !Y || !CC || !DD || !Rchols || !log_Q || !x0 || !eps ||
        !unif || !particles || !idx || n_free < 1 || n_free + 1 > 1024 || X_N < 1 || M < 1 || M > 2048 || D < 1 || C < 0 ||
        P != D + C || P > MAXP || Ydim < 1 || Ydim > 8 || (C > 0 && !ctrl) || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, "ffvd_op_pg_sweep: bad argument");
    for (int j = 0; j < Ydim; ++j)
        if (!(Rchols[(size_t)j * Ydim + j] > 0.0)) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_pg_sweep: Rchols diagonal must be positive");
    OP_BEGIN("ffvd_op_pg_sweep");
    const int R = n_free, steps = X_N - 1;
    memcpy(particles, x0, (size_t)R * D * sizeof(double));                                   // particles[0] (:87)
    if (steps == 0) return FFVD_OK;
    StepSetup st(sc, R, M, D);
    const int Mp = st.Mp, Tp = st.Tp, ngs = st.ngs;
    const bool skinny = st.skinny;
    std::vector<double> &xc0 = start_rows(sc, x0, D, ctrl, R, D, C);                          // control row of step 0 (:93)
    LapTimer timer("FFVD_PG_TIMING", "ffvd_op_pg_sweep", sc.stream);
    double *dW = upload_stack(sc, Lm_inverse_seq, D, M, Mp);
    timer.lap("L^-T uploaded");
    HyperView hv{};
    if (int rc = stage_hypers(sc, "ffvd_op_pg_sweep", kind, Z, M, Mp, P, D, logvariance, loglengthscales, hv)) return rc;
    double *dxc = sc.upload(xc0.data(), xc0.size()), *dU = sc.upload(U, (size_t)M * D);
    double *dlq = sc.upload(log_Q, D);
    double *deps = sc.upload(eps, (size_t)steps * R * D), *dun = sc.upload(unif, (size_t)steps * R);
    timer.lap("draws uploaded");
    double *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    double *dXr = sc.upload(X_ref, (size_t)X_N * D), *dY = sc.upload(Y, (size_t)steps * Ydim);
    double *dCC = sc.upload(CC, (size_t)D * Ydim), *dDD = sc.upload(DD, Ydim), *dR = sc.upload(Rchols, (size_t)Ydim * Ydim);
    double *dmean = sc.alloc<double>((size_t)R * D), *dvar = sc.alloc<double>((size_t)R * D);
    double *cand = sc.alloc<double>((size_t)(R + 1) * D);
    double *dparts = sc.alloc<double>((size_t)steps * R * D);
    int32_t *didx = sc.alloc<int32_t>((size_t)steps * R);
    if (!dW || !dxc || !dU || !dlq || !deps || !dun || (C && !dctrl) || !dXr || !dY || !dCC || !dDD || !dR || !st.ok() || !dmean || !dvar ||
        !cand || !dparts || !didx)
        return set_error(nullptr, FFVD_ENOMEM, "ffvd_op_pg_sweep: device allocation or upload failed");
    st.fill(sc, kind, hv, dxc, P, M, dW, dU, nullptr, nullptr, nullptr, 0);
    // the whole sweep is enqueued at once: steps x (K_fu rows, projection, conditional, propagate + weight + resample)
    auto step_launches = [&]() {
        for (int t = 0; t < steps; ++t) {
            if (skinny) {                               // K(x_t, Z) m-major: the skinny product's operand loads coalesce
                launch_kfu_build_t(sc.stream, st.pa, Tp);
                launch_skinny_gemm(sc.stream, st.sk);
            } else { launch_kfu_build(sc.stream, st.pa); launch_proj_gemm(sc.stream, st.pg); }                          // conditional_after_kernel_precalculation (:95-97)
            const double *ctrl_next = (C && t + 1 < steps) ? dctrl + (size_t)(t + 1) * C : nullptr;
            launch_conditional_finish(sc.stream, kind, dxc, R, P, hv.variance, st.rowsq, st.fmean, ngs, Tp, D, dmean, dvar, nullptr);
            launch_pg_step(sc.stream, dmean, dvar, dlq, deps + (size_t)t * R * D, dun + (size_t)t * R, dY + (size_t)t * Ydim,
                           dXr + (size_t)(t + 1) * D, dCC, dDD, dR, ctrl_next,
                           R, D, C, Ydim, dxc, cand, dparts + (size_t)t * R * D, didx + (size_t)t * R);
        }
    };
    // Round 4: ONE persistent launch for the sweep (loops.hip), three grid-wide barriers per step instead of four dependent launches:
    // measured slower (86 against 43 us per step with roles and per-unit counters, 151 with a grid-wide barrier; see ffvd_op_rollout), opt-in with FFVD_STEP_LOOP=1
    const char *nsl = getenv("FFVD_STEP_LOOP");
    const bool use_loop = skinny && nsl && *nsl && strcmp(nsl, "0") != 0;
    if (use_loop) {
        PgLoopArgs la{};
        la.pa = st.pa;
        la.sk = st.loop_sk();
        la.kind = kind; la.R = R; la.D = D; la.C = C; la.Ydim = Ydim; la.steps = steps; la.ngs = ngs;
        la.variance = hv.variance; la.rowsq = st.rowsq; la.fmean = st.fmean; la.mean = dmean; la.var = dvar; la.cand = cand; la.parts = dparts;
        la.idx = didx; la.log_Q = dlq; la.eps = deps; la.unif = dun; la.Y = dY; la.X_ref = dXr; la.CC = dCC; la.DD = dDD; la.Rch = dR;
        la.ctrl = dctrl;
        const int rc = run_step_loop(sc, "ffvd_op_pg_sweep", D, dxc, xc0, [&](int32_t *words) {
            la.bar = reinterpret_cast<unsigned *>(words); la.abort_w = words + 1;
            launch_pg_loop(sc.stream, la);
        }, step_launches);
        if (rc) return rc;
    } else {
        timer.lap("uploads and set-up");
        step_launches();
        timer.lap("steps enqueued", false);        // how long the host takes to enqueue the sweep ...
        timer.lap("steps drained");                // ... and how long the GPU needs after that
    }
    OP_TRY(hipGetLastError());
    if (!sc.download(particles + (size_t)R * D, dparts, (size_t)steps * R * D * sizeof(double)) ||
        !sc.download(idx, didx, (size_t)steps * R * sizeof(int32_t)))
        return set_error(nullptr, FFVD_EDEVICE, "ffvd_op_pg_sweep: copying the results to the host failed");
    timer.lap("results to the host");
    return FFVD_OK;
}

// ---- grouped collapsed posteriors (posterior_group.h) ---------------------------------------------------------------------------------
// U_mean and L_H^-T of collapse_u_mean_after_kernel_precalculation (conditionals_multi_output.py:206-227, called at
// base_model.py:243-256) for G groups over n_models (1 or G) sets of Z / hyper-parameters, with the K_uu factors of kernel_pre_cal
// (:124-169) formed in the same call.  Everything between the small uploads and the results stays on the device.
namespace {
struct PgIn {
    const char *who;
    int kind, G, n_models, M, P, D, C, T, groups_per_pass;
    const double *Zs, *logvar, *loglen, *Xs, *ctrl_fit, *log_Qs;
    double jitter;
};
struct PgWork {
    int Mp, nK;                    // M rounded up to 64; K_uu factorisations = n_models * D
    double *Kuu;                   // [nK] slabs of 2 Mp x Mp: L, then L^-T
    double *Xs, *log_Qs;           // the uploaded [G][T+1][D], [G][D]
    double *U;                     // [G][M][D]
    // optional targets, filled pass by pass
    double *q0 = nullptr;          // [G][Mp16][Mp16]: L_H^-T of each group's d = 0 (upper triangle, zero padding)
    int Mp16 = 0;
    double *Hpack = nullptr;       // [G][D][M][M]: L_H^-T as ffvd_op_collapse_u_mean returns it
    double *qall = nullptr;        // [G][D][Mp][Mp]: L_H^-T of every (group, dim) (upper triangle, zero padding)
    HyperView hv{};                // [nK] device hyper-parameters (launch_rg_prep), left for what follows the posteriors
};

// scalar-argument checks shared by the two entry points (before any device call)
bool pg_scalars_ok(int kind, int G, int n_models, int M, int P, int D, int C, int T, int groups_per_pass, double jitter) {
    return (kind == FFVD_KERNEL_SE || kind == FFVD_KERNEL_LINEAR) && G >= 0 && M >= 1 && M <= 2048 && D >= 1 && C >= 0 && P == D + C &&
           P <= MAXP && T >= 1 && groups_per_pass >= 0 && (n_models == 1 || n_models == G) && std::isfinite(jitter) &&
           (long long)G * D <= (1LL << 24);                 // (units are counted in int)
}

// Uploads the inputs, enqueues the whole posterior (K_uu chain, projection, Gram, H chain, matvec, the pass's packing kernels) and
// reads every factorisation flag in ONE download; nothing before that waits for the device.  A dataflow Cholesky launch that gave up
// on a bounded wait: everything is enqueued once more from the inputs (still on the device) with the launch-per-column variant, as
// potrf_with_stall_recovery does.  On FFVD_OK the stream is drained and w's arrays are final.
int pg_posterior(Scratch &sc, const PgIn &in, PgWork &w) {
    const int G = in.G, D = in.D, M = in.M, P = in.P, C = in.C, T = in.T, nm = in.n_models, kind = in.kind;
    const int Mp = round_up(M, NB), Tp = round_up(T, STRIP), ng = (Mp + 511) / 512, nK = nm * D, GD = G * D;
    const size_t kstride = (size_t)2 * Mp * Mp, hstride = (size_t)(2 * Mp + NB) * Mp, fstride = (size_t)Tp * Mp;
    w.Mp = Mp; w.nK = nK;
    int gpp = in.groups_per_pass > 0 ? in.groups_per_pass : pg_groups_per_pass(G, D, Tp, Mp);
    if (gpp > G) gpp = G;
    if ((long long)gpp * D > 32768) gpp = 32768 / D > 0 ? 32768 / D : 1;
    const int upp = gpp * D;                                       // units per pass
    const std::string who = in.who;

    double *dZ = sc.upload(in.Zs, (size_t)nm * M * P), *dlv = sc.upload(in.logvar, nK);
    double *dll = in.loglen ? sc.upload(in.loglen, (size_t)nK * P) : nullptr;
    double *dctrl = C ? sc.upload(in.ctrl_fit, (size_t)T * C) : nullptr;
    w.Xs = sc.upload(in.Xs, (size_t)G * (T + 1) * D);
    w.log_Qs = sc.upload(in.log_Qs, GD);
    double *variance = sc.alloc<double>(nK), *len = sc.alloc<double>((size_t)nK * P);
    double *Zsc = sc.alloc<double>((size_t)nK * Mp * P), *zz = sc.alloc<double>((size_t)nK * Mp);
    double *Xt = sc.alloc<double>((size_t)(T + 1) * GD);
    w.Kuu = sc.alloc<double>((size_t)nK * kstride);
    w.hv = HyperView{variance, len, Zsc, zz};
    double *F = sc.alloc<double>((size_t)upp * fstride), *H = sc.alloc<double>((size_t)upp * hstride);
    double *ubuf = sc.alloc<double>((size_t)upp * M);
    w.U = sc.alloc<double>((size_t)GD * M);
    const int kchunk = nK < 32768 ? nK : 32768;
    double *dinvK = sc.alloc<double>(potrf_scratch_doubles(Mp, kchunk)), *dinvH = sc.alloc<double>(potrf_scratch_doubles(Mp, upp));
    int32_t *info = sc.alloc<int32_t>((size_t)nK + GD);
    if (!dZ || !dlv || (in.loglen && !dll) || (C && !dctrl) || !w.Xs || !w.log_Qs || !variance || !len || !Zsc || !zz || !Xt || !w.Kuu ||
        !F || !H || !ubuf || !w.U || !dinvK || !dinvH || !info)
        return set_error(nullptr, FFVD_ENOMEM, who + ": device allocation or upload failed");

    std::vector<int32_t> hinfo((size_t)nK + GD, 0);
    for (int attempt = 0;; ++attempt) {
        {
            CholOverrideGuard guard;            // reset on the error returns below as well
            if (attempt == 1) guard.force_left();
            OP_TRY(hipMemsetAsync(info, 0, ((size_t)nK + GD) * sizeof(int32_t), sc.stream));
            // 1. hyper-parameters of every (model, dim): prep_hypers' arithmetic, one launch, in HyperView's layout
            launch_rg_prep(sc.stream, kind, nm, D, M, Mp, P, dZ, dlv, dll, variance, len, Zsc, zz);
            // 2. K_uu + jitter I -> L, L^-T (kernel_pre_cal, :124-169)
            for (int k0 = 0; k0 < nK; k0 += kchunk) {
                const int n = nK - k0 < kchunk ? nK - k0 : kchunk;
                const HyperView hv{variance + k0, len + (size_t)k0 * P, Zsc + (size_t)k0 * Mp * P, zz + (size_t)k0 * Mp};
                launch_kuu_build(sc.stream, kind, hv, M, Mp, P, n, in.jitter, w.Kuu + (size_t)k0 * kstride, nullptr);
                launch_potrf_ext(sc.stream, w.Kuu + (size_t)k0 * kstride, Mp, Mp, Mp, n, kstride, info + k0, dinvK);
            }
            launch_pg_stage_x(sc.stream, w.Xs, G, T, D, Xt);
            for (int g0 = 0; g0 < G; g0 += gpp) {
                const int ngp = G - g0 < gpp ? G - g0 : gpp, nb = ngp * D, b0 = g0 * D;
                // 3. F = K_fu L^-T (:212-213)
                ProjectArgs pa{};
                pa.kind = kind; pa.x_ld = D; pa.x_cols = D; pa.ctrl = dctrl; pa.T = T; pa.Tp = Tp; pa.C = C; pa.P = P; pa.M = M; pa.Mp = Mp;
                pa.Dl = D; pa.d_begin = 0; pa.w_stride = kstride; pa.ng = ng;
                if (nm == 1) {          // the ELBO's shape: chains s = b / D of one model
                    pa.x = w.Xs; pa.x_chain_stride = (size_t)(T + 1) * D; pa.hv = HyperView{variance, len, Zsc, zz};
                    pa.W = w.Kuu + (size_t)Mp * Mp; pa.b0 = b0; pa.nb = nb; pa.F = F;
                    launch_project(sc.stream, pa);
                } else {
                    for (int gl = 0; gl < ngp; ++gl) {
                        const size_t k0 = (size_t)(g0 + gl) * D;
                        pa.x = w.Xs + (size_t)(g0 + gl) * (T + 1) * D; pa.x_chain_stride = 0;
                        pa.hv = HyperView{variance + k0, len + k0 * P, Zsc + k0 * Mp * P, zz + k0 * Mp};
                        pa.W = w.Kuu + k0 * kstride + (size_t)Mp * Mp; pa.b0 = 0; pa.nb = D; pa.F = F + (size_t)gl * D * fstride;
                        launch_project(sc.stream, pa);
                    }
                }
                // 4. H = I + F^T F / Q and b = F^T delta / Q (:214-217) into zeroed slabs with a device-set identity, then the chain
                OP_TRY(hipMemsetAsync(H, 0, (size_t)nb * hstride * sizeof(double), sc.stream));
                launch_set_identity(sc.stream, H, hstride, Mp, Mp, nb);
                GramArgs ga{};
                ga.mode = GRAM_F; ga.A = F; ga.a_stride = fstride; ga.rows = Tp; ga.with_row = 1; ga.brow = 2 * Mp;
                ga.X = Xt; ga.log_Q = w.log_Qs; ga.T = T; ga.D = GD; ga.Mp = Mp; ga.Dl = GD; ga.d_begin = 0;      // one chain of G * D dims
                ga.b0 = b0; ga.nb = nb; ga.yn_over_batch = 1.0; ga.H = H; ga.h_stride = hstride;
                launch_gram(sc.stream, ga);
                launch_potrf_ext(sc.stream, H, Mp, Mp + NB, Mp, nb, hstride, info + nK + b0, dinvH);
                // 5. U_mean[:, d] = L_H^-T (L_H^-1 b) (:219)
                launch_matvec(sc.stream, H + (size_t)Mp * Mp, hstride, H + (size_t)2 * Mp * Mp, hstride, Mp, ubuf, 1, M, M, nb);
                launch_pg_unpack_u(sc.stream, ubuf, ngp, D, M, w.U + (size_t)g0 * M * D);
                if (w.q0)               // slice d = 0 of each group
                    launch_pg_pack(sc.stream, H, hstride, Mp, Mp, ngp, D, M, 1, w.q0 + (size_t)g0 * w.Mp16 * w.Mp16, w.Mp16, w.Mp16, ngp);
                if (w.qall)             // every slice (q_mode "intent" of the grouped conditionals)
                    launch_pg_pack(sc.stream, H, hstride, Mp, Mp, nb, 1, M, 1, w.qall + (size_t)b0 * Mp * Mp, Mp, Mp, nb);
                if (w.Hpack)            // Lm_inverse_dd_seq = L_H^-T (:222)
                    launch_pg_pack(sc.stream, H, hstride, Mp, Mp, nb, 1, M, 0, w.Hpack + (size_t)b0 * M * M, M, M, nb);
            }
        }
        OP_TRY(hipGetLastError());
        OP_TRY(hipMemcpyAsync(hinfo.data(), info, hinfo.size() * sizeof(int32_t), hipMemcpyDeviceToHost, sc.stream));
        if (hipStreamSynchronize(sc.stream) != hipSuccess)
            return set_error(nullptr, FFVD_EDEVICE, who + ": device error while reading Cholesky status");
        for (int k = 0; k < nK; ++k)
            if (hinfo[k] > 0)
                return set_error(nullptr, FFVD_ENOTPD, who + ": Cholesky of K_uu + jitter*I failed: group " + std::to_string(k / D) +
                                                       ", latent dim " + std::to_string(k % D) + ", pivot " + std::to_string(hinfo[k] - 1) +
                                                       " is not positive");
        bool stalled = false;
        for (int32_t f : hinfo) stalled = stalled || f < 0;
        if (stalled) {
            if (attempt == 1)
                return set_error(nullptr, FFVD_EDEVICE, who + ": abandoned, a block row waited more than 1 s for the row above it");
            continue;
        }
        for (int b = 0; b < GD; ++b)
            if (hinfo[nK + b] > 0)
                return set_error(nullptr, FFVD_ENOTPD, who + ": Cholesky of H failed: group " + std::to_string(b / D) + ", latent dim " +
                                                       std::to_string(b % D) + ", pivot " + std::to_string(hinfo[nK + b] - 1) +
                                                       " is not positive");
        if (attempt == 1)
            set_error(nullptr, FFVD_OK, "warning: " + who + ": the one-launch (dataflow) Cholesky gave up on a bounded wait; the posteriors "
                                        "were formed again with the launch-per-column Cholesky and completed");
        return FFVD_OK;
    }
}
}  // namespace

extern "C" int ffvd_op_posterior_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances,
                                         const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                                         const double *log_Qs, double jitter, int groups_per_pass, double *Lm_inverse, double *U_means,
                                         double *H_inv_sqrts) {
    const char *who = "ffvd_op_posterior_grouped", *bad = "ffvd_op_posterior_grouped: bad argument";
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0) return FFVD_OK;
    if (!Zs || !logvariances || !Xs || !log_Qs || !U_means || (C > 0 && !ctrl_fit) || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN("ffvd_op_posterior_grouped");
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const size_t GD = (size_t)G * D, MM = (size_t)M * M, nK = (size_t)n_models * D;
    if (H_inv_sqrts) { w.Hpack = sc.alloc<double>(GD * MM); OP_CHECK(w.Hpack, "ffvd_op_posterior_grouped"); }
    double *Lpack = Lm_inverse ? sc.alloc<double>(nK * MM) : nullptr;
    if (Lm_inverse) OP_CHECK(Lpack, "ffvd_op_posterior_grouped");
    if (int rc = pg_posterior(sc, in, w)) return rc;
    if (Lpack) launch_pg_pack(sc.stream, w.Kuu, (size_t)2 * w.Mp * w.Mp, w.Mp, w.Mp, (int)nK, 1, M, 0, Lpack, M, M, (int)nK);
    OP_TRY(hipGetLastError());
    if (!sc.download(U_means, w.U, GD * M * sizeof(double)) || (H_inv_sqrts && !sc.download(H_inv_sqrts, w.Hpack, GD * MM * sizeof(double))) ||
        (Lpack && !sc.download(Lm_inverse, Lpack, nK * MM * sizeof(double))))
        return set_error(nullptr, FFVD_EDEVICE, "ffvd_op_posterior_grouped: copying the results back failed");
    return FFVD_OK;
}

// The posteriors above handed to the grouped rollout loop (base_model.py:243-314 per group) without leaving the device: W, q0, f and
// x_last of RolloutGroupArgs are written by posterior_group.hip's kernels from the factorisation slabs, then launch_rg_prep /
// launch_rg_wq / launch_rg_step run as in ffvd_op_rollout_grouped.
// sum: as in rollout_grouped_run -- the summary launches follow the step launches, predict_x / predict_var may each be NULL.
static int posterior_rollout_grouped_run(const std::string &whos, int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                         const double *logvariances, const double *loglengthscales, const double *Xs,
                                         const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter, int groups_per_pass,
                                         int R, const double *ctrl_roll, int steps, const double *eps, double *predict_x,
                                         double *predict_var, double *U_means, const SummaryReq *sum) {
    const char *who = whos.c_str();
    const std::string bad = whos + ": bad argument";
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || R < 1 || steps < 0)
        return set_error(nullptr, FFVD_EINVAL, bad);
    const int Mp16 = round_up(M, RG_SLAB), NS = Mp16 / RG_SLAB;
    if ((long long)G * D * Mp16 * Mp16 > (1LL << 29) || (long long)G * R > (1LL << 20) || (R + RG_RC - 1) / RG_RC > 65535 ||
        (long long)G * D * NS >= (1LL << 31))
        return set_error(nullptr, FFVD_EINVAL, bad + " (beyond the limits of rollout_group.h)");
    if (sum && !summary_scalars_ok(*sum, (long long)G * R, steps, D)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Zs || !logvariances || !Xs || !log_Qs || !eps || (!sum && (!predict_x || !predict_var)) || (C > 0 && (!ctrl_fit || !ctrl_roll)) ||
        (kind == FFVD_KERNEL_SE && !loglengthscales) || (sum && !summary_arrays_ok(*sum)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN_AS(whos);
    LapTimer timer("FFVD_RG_TIMING", who, sc.stream);
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const size_t GD = (size_t)G * D, mm16 = (size_t)Mp16 * Mp16, out_n = (size_t)G * R * steps * D;
    w.Mp16 = Mp16;
    w.q0 = sc.alloc<double>((size_t)G * mm16);
    double *dW = sc.alloc<double>(GD * mm16), *dB = sc.alloc<double>(GD * mm16);
    OP_CHECK_AS(w.q0 && dW && dB, whos);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    timer.lap("posteriors");
    // the rollout loop's own copy of the small inputs, one row per group (a shared model is repeated: launch_rg_step indexes by group)
    const double *hZ = Zs, *hlv = logvariances, *hll = loglengthscales;
    if (n_models == 1 && G > 1) {
        std::vector<double> &rz = sc.host((size_t)G * M * P), &rv = sc.host(GD), &rl = sc.host(loglengthscales ? GD * P : 0);
        for (int g = 0; g < G; ++g) {
            memcpy(rz.data() + (size_t)g * M * P, Zs, (size_t)M * P * sizeof(double));
            memcpy(rv.data() + (size_t)g * D, logvariances, D * sizeof(double));
            if (loglengthscales) memcpy(rl.data() + (size_t)g * D * P, loglengthscales, (size_t)D * P * sizeof(double));
        }
        hZ = rz.data(); hlv = rv.data(); hll = loglengthscales ? rl.data() : nullptr;
    }
    double *dZ = sc.upload(hZ, (size_t)G * M * P), *dlv = sc.upload(hlv, GD), *dll = hll ? sc.upload(hll, GD * P) : nullptr;
    double *deps = sc.upload(eps, (size_t)steps * G * R * D), *dctrl = C ? sc.upload(ctrl_roll, (size_t)steps * C) : nullptr;
    double *dxl = sc.alloc<double>(GD);
    double *variance = sc.alloc<double>(GD), *len = sc.alloc<double>(GD * P), *Zsc = sc.alloc<double>(GD * Mp16 * P), *zz = sc.alloc<double>(GD * Mp16);
    double *part = sc.alloc<double>((size_t)2 * GD * NS * R * 4), *xbuf = sc.alloc<double>((size_t)2 * G * R * D);
    double *dpx = sc.alloc<double>(out_n), *dpv = sc.alloc<double>(out_n);
    OP_CHECK_AS(dZ && dlv && (!hll || dll) && deps && (!C || dctrl) && dxl && variance && len && Zsc && zz && part && xbuf && dpx && dpv,
             whos);
    // W[g][d] = L^-T of the group's model; with one model every group reads the same slab (the stack is still materialised)
    launch_pg_pack(sc.stream, w.Kuu, (size_t)2 * w.Mp * w.Mp, w.Mp, w.Mp, w.nK, 1, M, 1, dW, Mp16, Mp16, (int)GD);
    launch_pg_x_last(sc.stream, w.Xs, G, T, D, dxl);
    launch_rg_prep(sc.stream, kind, G, D, M, Mp16, P, dZ, dlv, dll, variance, len, Zsc, zz);
    launch_rg_wq(sc.stream, G, D, Mp16, 1, dW, w.q0, dB);
    timer.lap("operands packed, W q_sqrt");
    RolloutGroupArgs a{};
    a.kind = kind; a.G = G; a.R = R; a.D = D; a.C = C; a.P = P; a.M = M; a.Mp = Mp16; a.NS = NS; a.steps = steps;
    a.has_q = 1; a.q_upper = 1;          // q0's strict lower triangle was written as exact zeros
    a.W = dW; a.B = dB; a.Zs = Zsc; a.zz = zz; a.variance = variance; a.len = len; a.f = w.U; a.x_last = dxl; a.log_Q = w.log_Qs;
    a.ctrl = dctrl; a.eps = deps; a.part = part; a.xbuf = xbuf; a.predict_x = dpx; a.predict_var = dpv;
    for (int t = 0; t <= steps; ++t) launch_rg_step(sc.stream, a, t);
    OP_TRY(hipGetLastError());
    timer.lap("step launches");
    if (sum) {
        if (int rc = run_summary(sc, whos, dpx, dpv, G * R, steps, D, *sum)) return rc;
        timer.lap("summary");
    }
    if ((predict_x && !sc.download(predict_x, dpx, out_n * sizeof(double))) ||
        (predict_var && !sc.download(predict_var, dpv, out_n * sizeof(double))) ||
        (U_means && !sc.download(U_means, w.U, GD * M * sizeof(double))))
        return set_error(nullptr, FFVD_EDEVICE, whos + ": copying the results back failed");
    timer.lap("results downloaded");
    return FFVD_OK;
}

extern "C" int ffvd_op_posterior_rollout_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                 const double *logvariances, const double *loglengthscales, const double *Xs,
                                                 const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                 int groups_per_pass, int R, const double *ctrl_roll, int steps, const double *eps,
                                                 double *predict_x, double *predict_var, double *U_means) {
    return posterior_rollout_grouped_run("ffvd_op_posterior_rollout_grouped", kind, G, n_models, Zs, M, P, D, logvariances, loglengthscales,
                                         Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, R, ctrl_roll, steps, eps, predict_x,
                                         predict_var, U_means, nullptr);
}

extern "C" int ffvd_op_posterior_rollout_grouped_summary(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                         const double *logvariances, const double *loglengthscales, const double *Xs,
                                                         const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                         int groups_per_pass, int R, const double *ctrl_roll, int steps,
                                                         const double *eps, double *predict_x, double *predict_var, double *U_means,
                                                         const double *CC, const double *DD, const double *noise_std, int J,
                                                         const double *Y_test, int n_test, double *y_mean, double *y_var,
                                                         double *y_var_total, double *lpd, double *lpd_gauss) {
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    return posterior_rollout_grouped_run("ffvd_op_posterior_rollout_grouped_summary", kind, G, n_models, Zs, M, P, D, logvariances,
                                         loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, R, ctrl_roll, steps, eps,
                                         predict_x, predict_var, U_means, &q);
}

// ---- grouped GP conditionals (conditional_group.h) ------------------------------------------------------------------------------------
// conditional_after_kernel_precalculation (conditionals_multi_output.py:306-387, white=True, full_cov=False) for G posteriors at N
// common inputs: F = K(Xnew, Z) L^-T (:349) once per (model, dim), mean = F U_g (:365), var = Kdiag - sum F^2 (:356) + sum (F q)^2
// (:369-380), and the equal-weight mixture over the groups.
namespace {
struct CgOut { double *means, *vars, *mix_mean, *mix_var; };

// scalar-argument checks shared by the two entry points (before any device call); C = P - D
bool cg_scalars_ok(int kind, int G, int n_models, int M, int P, int D, int N, int q_mode, int rows_per_pass) {
    if (!((kind == FFVD_KERNEL_SE || kind == FFVD_KERNEL_LINEAR) && G >= 0 && M >= 1 && M <= 2048 && D >= 1 && P >= D && P <= MAXP &&
          N >= 0 && (q_mode == 0 || q_mode == 1) && rows_per_pass >= 0 && (n_models == 1 || n_models == G) &&
          (long long)G * D <= (1LL << 24)))
        return false;
    const long long Mp = round_up(M, NB);
    return (long long)G * D * Mp * Mp <= (1LL << 29) && (long long)G * D * N < (1LL << 31);
}
bool cg_outputs_ok(const CgOut &o) { return (o.means || o.vars || o.mix_mean) && (!o.mix_mean == !o.mix_var); }

// The launches of conditional_group.h on operands that are already on the device, then the requested outputs come down.
int cg_run(Scratch &sc, const std::string &who, int kind, int G, int nm, int M, int P, int D, int N, int rows_per_pass, const HyperView &hv,
           const double *W, size_t w_stride, const double *dU, const double *dq, int q_per_dim, int q_upper, const double *dX,
           const CgOut &o) {
    const int Mp = round_up(M, NB);
    const size_t out_n = (size_t)G * N * D, ND = (size_t)N * D;
    CondGroupArgs a{};
    a.kind = kind; a.G = G; a.n_models = nm; a.M = M; a.Mp = Mp; a.P = P; a.D = D; a.N = N;
    a.rows_per_pass = rows_per_pass > 0 ? rows_per_pass : cg_rows_per_pass(nm, D, Mp);
    a.hv = hv; a.W = W; a.w_stride = w_stride; a.U = dU; a.q = dq; a.q_per_dim = q_per_dim; a.q_upper = q_upper; a.x = dX;
    a.need_var = (o.vars || o.mix_var) ? 1 : 0;
    const CondGroupScratch need = cg_scratch_doubles(G, nm, D, Mp, N, a.rows_per_pass, a.need_var && dq);
    a.F = sc.alloc<double>(need.F); a.rowsq = sc.alloc<double>(need.rowsq); a.Ut = sc.alloc<double>(need.Ut); a.mbuf = sc.alloc<double>(need.mbuf);
    a.part = need.part ? sc.alloc<double>(need.part) : nullptr;
    a.mean = sc.alloc<double>(out_n);
    a.var = a.need_var ? sc.alloc<double>(out_n) : nullptr;
    double *dmm = o.mix_mean ? sc.alloc<double>(ND) : nullptr, *dmv = o.mix_mean ? sc.alloc<double>(ND) : nullptr;
    if (!a.F || !a.rowsq || !a.Ut || !a.mbuf || (need.part && !a.part) || !a.mean || (a.need_var && !a.var) || (o.mix_mean && (!dmm || !dmv)))
        return set_error(nullptr, FFVD_ENOMEM, who + ": device allocation or upload failed");
    launch_conditional_group(sc.stream, a);
    if (o.mix_mean) launch_cg_mixture(sc.stream, a.mean, a.var, G, ND, dmm, dmv);
    OP_TRY(hipGetLastError());
    if ((o.means && !sc.download(o.means, a.mean, out_n * sizeof(double))) || (o.vars && !sc.download(o.vars, a.var, out_n * sizeof(double))) ||
        (o.mix_mean && (!sc.download(o.mix_mean, dmm, ND * sizeof(double)) || !sc.download(o.mix_var, dmv, ND * sizeof(double)))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}
}  // namespace

// Posteriors given by the caller (also explicit-U models and SG-HMC samples of U: q_sqrts = NULL)
extern "C" int ffvd_op_conditional_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                           int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                           const double *const *q_sqrts, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                           double *means, double *vars, double *mix_mean, double *mix_var) {
    const char *who = "ffvd_op_conditional_grouped", *bad = "ffvd_op_conditional_grouped: bad argument";
    if (!cg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || N == 0) return FFVD_OK;
    const CgOut out{means, vars, mix_mean, mix_var};
    if (!Lm_inverse_seqs || !Zs || !logvariances || !fs || !Xnew || !cg_outputs_ok(out) || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t nK = (size_t)n_models * D, GD = (size_t)G * D, nq = q_sqrts ? (q_mode ? GD : (size_t)G) : 0;
    for (size_t b = 0; b < nK; ++b) if (!Lm_inverse_seqs[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    for (size_t b = 0; b < nq; ++b) if (!q_sqrts[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN("ffvd_op_conditional_grouped");
    const int Mp = round_up(M, NB);
    // the triangular k cut needs EVERY slice upper triangular (the reference hands over L_H^-T); a dense slice takes the full range
    int q_upper = nq ? 1 : 0;
    for (size_t b = 0; q_upper && b < nq; ++b) q_upper = q_sqrt_is_upper(q_sqrts[b], M) ? 1 : 0;
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp), *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    double *dZ = sc.upload(Zs, (size_t)n_models * M * P), *dU = sc.upload(fs, GD * M), *dX = sc.upload(Xnew, (size_t)N * P);
    double *dlv = sc.upload(logvariances, nK), *dll = loglengthscales ? sc.upload(loglengthscales, nK * P) : nullptr;
    double *variance = sc.alloc<double>(nK), *len = sc.alloc<double>(nK * P), *Zsc = sc.alloc<double>(nK * Mp * P), *zz = sc.alloc<double>(nK * Mp);
    OP_CHECK(dW && (!nq || dq) && dZ && dU && dX && dlv && (!loglengthscales || dll) && variance && len && Zsc && zz, "ffvd_op_conditional_grouped");
    launch_rg_prep(sc.stream, kind, n_models, D, M, Mp, P, dZ, dlv, dll, variance, len, Zsc, zz);
    return cg_run(sc, who, kind, G, n_models, M, P, D, N, rows_per_pass, HyperView{variance, len, Zsc, zz}, dW, (size_t)Mp * Mp, dU, dq,
                  q_mode, q_upper, dX, out);
}

// The collapsed posteriors of ffvd_op_posterior_grouped (base_model.py:243-256) evaluated at Xnew without leaving the device: L^-T is
// read in the K_uu slabs, U_mean where the matvec left it, the q slices are packed by launch_pg_pack (exact zeros in the padding and
// the strict lower triangle, so the k cut holds by construction).
extern "C" int ffvd_op_posterior_conditional_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                     const double *logvariances, const double *loglengthscales, const double *Xs,
                                                     const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                     int groups_per_pass, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                                     double *means, double *vars, double *mix_mean, double *mix_var, double *U_means) {
    const char *who = "ffvd_op_posterior_conditional_grouped", *bad = "ffvd_op_posterior_conditional_grouped: bad argument";
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) ||
        !cg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || N == 0) return FFVD_OK;
    const CgOut out{means, vars, mix_mean, mix_var};
    if (!Zs || !logvariances || !Xs || !log_Qs || !Xnew || !cg_outputs_ok(out) || (C > 0 && !ctrl_fit) ||
        (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN("ffvd_op_posterior_conditional_grouped");
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const int Mp = round_up(M, NB);
    const size_t GD = (size_t)G * D, mm = (size_t)Mp * Mp;
    const bool need_q = vars || mix_var;
    if (need_q && q_mode) w.qall = sc.alloc<double>(GD * mm);
    else if (need_q) { w.Mp16 = Mp; w.q0 = sc.alloc<double>((size_t)G * mm); }
    double *dX = sc.upload(Xnew, (size_t)N * P);
    OP_CHECK(dX && (!need_q || w.qall || w.q0), "ffvd_op_posterior_conditional_grouped");
    if (int rc = pg_posterior(sc, in, w)) return rc;
    if (int rc = cg_run(sc, who, kind, G, n_models, M, P, D, N, rows_per_pass, w.hv, w.Kuu + mm, 2 * mm, w.U, q_mode ? w.qall : w.q0, q_mode, 1,
                        dX, out))
        return rc;
    if (U_means && !sc.download(U_means, w.U, GD * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, "ffvd_op_posterior_conditional_grouped: copying the results back failed");
    return FFVD_OK;
}

// ---- moment-matched prediction (moment_group.h) ---------------------------------------------------------------------------------------
// A Gaussian state of each of G posteriors pushed through x_{t+1} = x_t + f(x_t, c_t) + noise in closed form (SE-ARD only), one launch
// per step for all groups; optionally summarised as a held-out prediction before anything comes down.
namespace {
// scalar-argument checks shared by the two entry points (before any device call)
bool mg_scalars_ok(int kind, int G, int n_models, int M, int P, int D, int C, int steps, int q_mode) {
    if (!(kind == FFVD_KERNEL_SE && G >= 0 && steps >= 0 && M >= 1 && M <= 2048 && D >= 1 && D <= MG_MAXD && C >= 0 && P == D + C &&
          P <= MAXP && (q_mode == 0 || q_mode == 1) && (n_models == 1 || n_models == G) && (long long)G * D <= (1LL << 24)))
        return false;
    const long long Mp = round_up(M, NB), NS = (M + MG_SLAB - 1) / MG_SLAB;
    return (long long)G * D * Mp * Mp <= (1LL << 29) && (long long)G * mg_npair(D) * NS < (1LL << 31) &&
           (steps == 0 || G <= ((1LL << 31) - 1) / steps / D / D);
}
// the trailing summary block of the entry points: asked for when anything in it is given
bool mg_summary_wanted(const SummaryReq &q) {
    return q.CC || q.DD || q.noise_std || q.J != 0 || q.Y_test || q.n_test != 0 || q.y_mean || q.y_var || q.y_var_total || q.lpd || q.lpd_gauss;
}

// the summary launch of moment_group.h on stacks that are on the device, then the requested outputs come down (one small copy)
int mg_summary(Scratch &sc, const std::string &who, const double *dm, const double *dS, int G, int steps, int D, const SummaryReq &q) {
    const int J = q.J;
    const size_t SJ = (size_t)steps * J, TJ = (size_t)q.n_test * J;
    MomentSummaryArgs a{};
    a.G = G; a.steps = steps; a.D = D; a.J = J; a.n_test = q.n_test; a.m = dm; a.S = dS;
    a.CC = sc.upload(q.CC, (size_t)D * J); a.DD = sc.upload(q.DD, J); a.sd = sc.upload(q.noise_std, J);
    a.Y = q.n_test ? sc.upload(q.Y_test, TJ) : nullptr;
    a.out = sc.alloc<double>(5 * SJ);
    if (!a.CC || !a.DD || !a.sd || (q.n_test && !a.Y) || !a.out)
        return set_error(nullptr, FFVD_ENOMEM, who + ": device allocation or upload failed");
    launch_moment_summary(sc.stream, a);
    OP_TRY(hipGetLastError());
    std::vector<double> &h = sc.host(5 * SJ);
    OP_TRY(hipMemcpyAsync(h.data(), a.out, h.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    double *const dst[5] = {q.y_mean, q.y_var, q.y_var_total, q.lpd, q.lpd_gauss};
    for (int f = 0; f < 5; ++f)
        if (dst[f]) memcpy(dst[f], h.data() + f * SJ, (f < 3 ? SJ : TJ) * sizeof(double));
    return FFVD_OK;
}

// The filter request of mg_run: the emission, the observations (NaN = unobserved) and the outputs, each of which may be NULL
struct FilterReq {
    const double *CC, *DD, *noise_std;           // D x J, J, J
    int J;
    const double *Y_obs;                         // steps x J
    double *m_filt, *S_filt, *cross, *lpd, *lpd_joint, *m_smooth, *S_smooth;
    double *y_mean, *y_var_total, *lpd_mix, *lpd_gauss;      // the pooled one-step summary (steps x J)
};
// the checks of a filter request that need no array, and those that read the small arrays (Y_obs: no infinity)
bool filter_scalars_ok(const FilterReq &f) { return f.J >= 1 && f.J <= MG_MAXJ; }
bool filter_arrays_ok(const FilterReq &f, int steps, const double *m_pred, const double *S_pred) {
    if (!f.CC || !f.DD || !f.noise_std || !f.Y_obs) return false;
    if (!(m_pred || S_pred || f.m_filt || f.S_filt || f.cross || f.lpd || f.lpd_joint || f.m_smooth || f.S_smooth || f.y_mean ||
          f.y_var_total || f.lpd_mix || f.lpd_gauss))
        return false;
    for (int j = 0; j < f.J; ++j)
        if (!std::isfinite(f.noise_std[j]) || !(f.noise_std[j] > 0.0)) return false;
    for (size_t e = 0; e < (size_t)steps * f.J; ++e)
        if (std::isinf(f.Y_obs[e])) return false;
    return true;
}

// Operands on the device -> beta, Gamma, the step launches, the summary, the downloads.  flt: the launches are those of the filter
// (moment_group.h), m_x / S_x are the predicted moments, the summary is the pooled one-step summary of the request.  dW: [n_models * D] slots of Mp x Mp (upper
// triangular, zero padded); dq: nullptr, or [G] (q_mode 0) / [G * D] (q_mode 1) slots of Mp x Mp; hv: variance / len per (model, dim).
int mg_run(Scratch &sc, const std::string &who, int G, int nm, int M, int P, int D, int C, int steps, const HyperView &hv, const double *dZ,
           const double *dW, const double *dq, int q_mode, const double *dU, const double *dxl, const double *dS0, const double *dlq,
           const double *dctrl, double *m_x, double *S_x, const SummaryReq *sum, const FilterReq *flt = nullptr) {
    const int Mp = round_up(M, NB), NS = (M + MG_SLAB - 1) / MG_SLAB, nK = nm * D, GD = G * D;
    const size_t mm = (size_t)Mp * Mp, nm_x = (size_t)G * steps * D, nS_x = nm_x * D;
    const int units = dq ? GD : nK, nq = dq ? (q_mode ? GD : G) : 0;
    double *beta = sc.alloc<double>((size_t)GD * Mp), *gam = sc.alloc<double>((size_t)units * mm);
    double *dN = dq ? sc.alloc<double>((size_t)nq * mm) : nullptr, *dE = dq ? sc.alloc<double>((size_t)nq * mm) : nullptr;
    double *dWE = dq ? sc.alloc<double>((size_t)GD * mm) : nullptr;
    double *unused = sc.alloc<double>((size_t)(nq > units ? nq : units));          // (cov.hip reads a variance per slot for its seed: none here)
    double *part = sc.alloc<double>((size_t)2 * G * mg_fields(D) * NS), *state = sc.alloc<double>((size_t)2 * G * (D + D * D));
    double *dm = sc.alloc<double>(nm_x), *dS = sc.alloc<double>(nS_x);
    OP_CHECK_AS(beta && gam && (!dq || (dN && dE && dWE)) && unused && part && state && dm && dS, who);
    MomentFilterArgs fa{};
    MomentSmoothArgs sa{};
    const bool smooth = flt && (flt->m_smooth || flt->S_smooth);
    const size_t nlpd = flt ? (size_t)G * steps * flt->J : 0, nlj = (size_t)G * steps;
    if (flt) {
        fa.J = flt->J;
        fa.CC = sc.upload(flt->CC, (size_t)D * flt->J); fa.DD = sc.upload(flt->DD, flt->J); fa.sd = sc.upload(flt->noise_std, flt->J);
        fa.Y = sc.upload(flt->Y_obs, (size_t)steps * flt->J);
        fa.m_filt = sc.alloc<double>(nm_x); fa.S_filt = sc.alloc<double>(nS_x); fa.cross = sc.alloc<double>(nS_x);
        fa.lpd = sc.alloc<double>(nlpd); fa.lpd_joint = sc.alloc<double>(nlj);
        OP_CHECK_AS(fa.CC && fa.DD && fa.sd && fa.Y && fa.m_filt && fa.S_filt && fa.cross && fa.lpd && fa.lpd_joint, who);
        if (smooth) {
            sa.G = G; sa.D = D; sa.steps = steps; sa.m_pred = dm; sa.S_pred = dS; sa.m_filt = fa.m_filt; sa.S_filt = fa.S_filt;
            sa.cross = fa.cross; sa.m_smooth = sc.alloc<double>(nm_x); sa.S_smooth = sc.alloc<double>(nS_x);
            OP_CHECK_AS(sa.m_smooth && sa.S_smooth, who);
        }
    }
    launch_mg_beta(sc.stream, G, D, M, Mp, nm == G, dW, dU, beta);
    // Gamma = W (I - q q^T) W^T through cov.hip's product body.  COV_GEN: C = A B^T, all Mp x Mp entries written.
    CovArgs gen{};
    gen.mode = COV_GEN; gen.a_stride = mm; gen.lda = Mp; gen.arows = Mp; gen.K = Mp; gen.ldb = Mp; gen.brows = Mp; gen.ncols = Mp;
    gen.c_stride = mm; gen.ldc = Mp;
    auto product = [&](const double *A, const double *B, size_t b_stride, double *Cdst, int n) {
        for (int u0 = 0; u0 < n; u0 += 32768) {                                       // (grid y)
            gen.A = A + (size_t)u0 * mm; gen.B = B + (size_t)u0 * b_stride; gen.b_stride = b_stride; gen.C = Cdst + (size_t)u0 * mm;
            gen.nb = n - u0 < 32768 ? n - u0 : 32768;
            launch_cov(sc.stream, gen);
        }
    };
    if (!dq) product(dW, dW, mm, gam, nK);                                            // W W^T per (model, dim)
    else {
        // E = I - q q^T as (N + N^T) - N N^T with N = I - q: no cancellation where q is close to the identity, which is where W is
        // large.  -N N^T: the symmetric product C = seed - A A^T with an empty seed (a LinearK seed over P = 0 columns is an exact zero).
        OP_TRY(hipMemsetAsync(dE, 0, (size_t)nq * mm * sizeof(double), sc.stream));
        CovArgs sym{};
        sym.mode = COV_SYM; sym.a_stride = mm; sym.lda = Mp; sym.arows = Mp; sym.K = Mp; sym.c_stride = mm; sym.ldc = Mp; sym.N = M;
        sym.kind = FFVD_KERNEL_LINEAR; sym.P = 0; sym.variance = unused; sym.len = hv.len;
        for (int u0 = 0; u0 < nq; u0 += 32768) {
            const int n = nq - u0 < 32768 ? nq - u0 : 32768;
            launch_mg_nmat(sc.stream, n, M, Mp, dq + (size_t)u0 * mm, dN + (size_t)u0 * mm);
            sym.A = dN + (size_t)u0 * mm; sym.C = dE + (size_t)u0 * mm; sym.nb = n;
            launch_cov(sc.stream, sym);
            launch_mg_emat(sc.stream, n, M, Mp, dN + (size_t)u0 * mm, dE + (size_t)u0 * mm);
        }
        // (W E) W^T per (group, dim); E is symmetric, so W E = W E^T.  One launch pair per group: a group's W and E slots are
        // contiguous whichever of them is shared
        for (int g = 0; g < G; ++g) {
            const double *Wg = dW + (nm == G ? (size_t)g * D * mm : 0);
            double *WEg = dWE + (size_t)g * D * mm;
            product(Wg, q_mode ? dE + (size_t)g * D * mm : dE + (size_t)g * mm, q_mode ? mm : 0, WEg, D);
            product(WEg, Wg, mm, gam + (size_t)g * D * mm, D);
        }
    }
    MomentGroupArgs a{};
    a.G = G; a.n_models = nm; a.D = D; a.C = C; a.P = P; a.M = M; a.Mp = Mp; a.NS = NS; a.steps = steps; a.unit_per_group = dq ? 1 : 0;
    a.Z = dZ; a.variance = hv.variance; a.len = hv.len; a.beta = beta; a.gam = gam; a.x_last = dxl; a.S0 = dS0; a.log_Q = dlq;
    a.ctrl = dctrl; a.part = part; a.state = state; a.m_x = dm; a.S_x = dS;
    if (!flt)
        for (int t = 0; t <= steps; ++t) launch_mg_step(sc.stream, a, t);
    else {
        for (int t = 0; t <= steps; ++t) launch_mg_filter_step(sc.stream, a, fa, t);
        if (smooth) launch_mg_smooth(sc.stream, sa);
    }
    OP_TRY(hipGetLastError());
    if (sum)
        if (int rc = mg_summary(sc, who, dm, dS, G, steps, D, *sum)) return rc;
    if (flt) {
        auto down = [&](double *dst, const double *src, size_t n) { return !dst || sc.download(dst, src, n * sizeof(double)); };
        if (!down(flt->m_filt, fa.m_filt, nm_x) || !down(flt->S_filt, fa.S_filt, nS_x) || !down(flt->cross, fa.cross, nS_x) ||
            !down(flt->lpd, fa.lpd, nlpd) || !down(flt->lpd_joint, fa.lpd_joint, nlj) || !down(flt->m_smooth, sa.m_smooth, nm_x) ||
            !down(flt->S_smooth, sa.S_smooth, nS_x))
            return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    }
    if ((m_x && !sc.download(m_x, dm, nm_x * sizeof(double))) || (S_x && !sc.download(S_x, dS, nS_x * sizeof(double))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}
}  // namespace

// Posteriors given by the caller (also explicit-U models and SG-HMC samples of U: q_sqrts = NULL)
extern "C" int ffvd_op_moment_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                      int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                      const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                      const double *ctrl, int C, int steps, const double *log_Qs, double *m_x, double *S_x,
                                      const double *CC, const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                                      double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string who = "ffvd_op_moment_grouped", bad = who + ": bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    const SummaryReq *sum = mg_summary_wanted(q) ? &q : nullptr;
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + " (moment matching is closed-form for the SE kernel only)");
    if (!mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) || (sum && !summary_scalars_ok(q, G, steps, D)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !x_lasts || !log_Qs || (C > 0 && !ctrl) ||
        (!sum && (!m_x || !S_x)) || (sum && !summary_arrays_ok(q)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t nK = (size_t)n_models * D, GD = (size_t)G * D, nq = q_sqrts ? (q_mode ? GD : (size_t)G) : 0;
    for (size_t b = 0; b < nK; ++b) if (!Lm_inverse_seqs[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    for (size_t b = 0; b < nq; ++b) if (!q_sqrts[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN_AS(who);
    const int Mp = round_up(M, NB);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp), *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    double *dZ = sc.upload(Zs, (size_t)n_models * M * P), *dU = sc.upload(fs, GD * M), *dxl = sc.upload(x_lasts, GD);
    double *dS0 = S0s ? sc.upload(S0s, GD * D) : nullptr, *dlq = sc.upload(log_Qs, GD), *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    double *dlv = sc.upload(logvariances, nK), *dll = sc.upload(loglengthscales, nK * P);
    double *variance = sc.alloc<double>(nK), *len = sc.alloc<double>(nK * P), *Zsc = sc.alloc<double>(nK * Mp * P), *zz = sc.alloc<double>(nK * Mp);
    OP_CHECK_AS(dW && (!nq || dq) && dZ && dU && dxl && (!S0s || dS0) && dlq && (!C || dctrl) && dlv && dll && variance && len && Zsc && zz, who);
    launch_rg_prep(sc.stream, kind, n_models, D, M, Mp, P, dZ, dlv, dll, variance, len, Zsc, zz);
    return mg_run(sc, who, G, n_models, M, P, D, C, steps, HyperView{variance, len, Zsc, zz}, dZ, dW, dq, q_mode, dU, dxl, dS0, dlq,
                  dctrl, m_x, S_x, sum);
}

// The collapsed posteriors of ffvd_op_posterior_grouped (base_model.py:243-256) propagated without leaving the device: L^-T is packed
// from the K_uu slabs, U_mean is read where the matvec left it, the q slices are packed by launch_pg_pack (exact zeros in the padding
// and the strict lower triangle), the start means are the last rows of Xs.
extern "C" int ffvd_op_posterior_moment_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                const double *logvariances, const double *loglengthscales, const double *Xs,
                                                const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                int groups_per_pass, int q_mode, const double *S0s, const double *ctrl_roll, int steps,
                                                double *m_x, double *S_x, double *U_means, const double *CC, const double *DD,
                                                const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean,
                                                double *y_var, double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string whos = "ffvd_op_posterior_moment_grouped", bad = whos + ": bad argument";
    const char *who = "ffvd_op_posterior_moment_grouped";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    const SummaryReq *sum = mg_summary_wanted(q) ? &q : nullptr;
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + " (moment matching is closed-form for the SE kernel only)");
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || !mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) ||
        (sum && !summary_scalars_ok(q, G, steps, D)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || (C > 0 && (!ctrl_fit || !ctrl_roll)) || (!sum && (!m_x || !S_x)) ||
        (sum && !summary_arrays_ok(q)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN_AS(whos);
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const int Mp = round_up(M, NB), nK = n_models * D;
    const size_t GD = (size_t)G * D, mm = (size_t)Mp * Mp;
    if (q_mode) w.qall = sc.alloc<double>(GD * mm);
    else { w.Mp16 = Mp; w.q0 = sc.alloc<double>((size_t)G * mm); }
    double *dW = sc.alloc<double>((size_t)nK * mm), *dxl = sc.alloc<double>(GD);
    OP_CHECK_AS((w.qall || w.q0) && dW && dxl, whos);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    double *dZ = sc.upload(Zs, (size_t)n_models * M * P), *dS0 = S0s ? sc.upload(S0s, GD * D) : nullptr;
    double *dctrl = C ? sc.upload(ctrl_roll, (size_t)steps * C) : nullptr;
    OP_CHECK_AS(dZ && (!S0s || dS0) && (!C || dctrl), whos);
    launch_pg_pack(sc.stream, w.Kuu, 2 * mm, Mp, Mp, nK, 1, M, 1, dW, Mp, Mp, nK);
    launch_pg_x_last(sc.stream, w.Xs, G, T, D, dxl);
    if (int rc = mg_run(sc, whos, G, n_models, M, P, D, C, steps, w.hv, dZ, dW, q_mode ? w.qall : w.q0, q_mode, w.U, dxl, dS0, w.log_Qs,
                        dctrl, m_x, S_x, sum))
        return rc;
    if (U_means && !sc.download(U_means, w.U, GD * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, whos + ": copying the results back failed");
    return FFVD_OK;
}

// ---- filtering and smoothing (moment_group.h) -------------------------------------------------------------------------------------
namespace {
// the pooled one-step summary of a filter request as a summary request on the predicted stacks (every row carries an observation
// row: NaN entries give NaN densities), or nothing when none of its outputs is asked for
bool filter_summary(const FilterReq &f, int steps, SummaryReq &q) {
    q = SummaryReq{f.CC, f.DD, f.noise_std, f.J, f.Y_obs, steps, f.y_mean, nullptr, f.y_var_total, f.lpd_mix, f.lpd_gauss};
    return f.y_mean || f.y_var_total || f.lpd_mix || f.lpd_gauss;
}
}  // namespace

// ffvd_op_moment_grouped with a measurement update after every step (posteriors given by the caller)
extern "C" int ffvd_op_filter_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                      int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                      const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                      const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                      const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                      double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                      double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss) {
    const std::string who = "ffvd_op_filter_grouped", bad = who + ": bad argument";
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + " (moment matching is closed-form for the SE kernel only)");
    if (!mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) || !filter_scalars_ok(f)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !x_lasts || !log_Qs || (C > 0 && !ctrl) ||
        !filter_arrays_ok(f, steps, m_pred, S_pred))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t nK = (size_t)n_models * D, GD = (size_t)G * D, nq = q_sqrts ? (q_mode ? GD : (size_t)G) : 0;
    for (size_t b = 0; b < nK; ++b) if (!Lm_inverse_seqs[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    for (size_t b = 0; b < nq; ++b) if (!q_sqrts[b]) return set_error(nullptr, FFVD_EINVAL, bad);
    SummaryReq q{};
    const SummaryReq *sum = filter_summary(f, steps, q) ? &q : nullptr;
    OP_BEGIN_AS(who);
    const int Mp = round_up(M, NB);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp), *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    double *dZ = sc.upload(Zs, (size_t)n_models * M * P), *dU = sc.upload(fs, GD * M), *dxl = sc.upload(x_lasts, GD);
    double *dS0 = S0s ? sc.upload(S0s, GD * D) : nullptr, *dlq = sc.upload(log_Qs, GD), *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    double *dlv = sc.upload(logvariances, nK), *dll = sc.upload(loglengthscales, nK * P);
    double *variance = sc.alloc<double>(nK), *len = sc.alloc<double>(nK * P), *Zsc = sc.alloc<double>(nK * Mp * P), *zz = sc.alloc<double>(nK * Mp);
    OP_CHECK_AS(dW && (!nq || dq) && dZ && dU && dxl && (!S0s || dS0) && dlq && (!C || dctrl) && dlv && dll && variance && len && Zsc && zz, who);
    launch_rg_prep(sc.stream, kind, n_models, D, M, Mp, P, dZ, dlv, dll, variance, len, Zsc, zz);
    return mg_run(sc, who, G, n_models, M, P, D, C, steps, HyperView{variance, len, Zsc, zz}, dZ, dW, dq, q_mode, dU, dxl, dS0, dlq,
                  dctrl, m_pred, S_pred, sum, &f);
}

// The collapsed posteriors of ffvd_op_posterior_grouped filtered without leaving the device (as ffvd_op_posterior_moment_grouped);
// x0s NULL: the start means are the last rows of Xs
extern "C" int ffvd_op_posterior_filter_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                const double *logvariances, const double *loglengthscales, const double *Xs,
                                                const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                double *lpd_gauss, double *U_means) {
    const std::string whos = "ffvd_op_posterior_filter_grouped", bad = whos + ": bad argument";
    const char *who = "ffvd_op_posterior_filter_grouped";
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + " (moment matching is closed-form for the SE kernel only)");
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || !mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) ||
        !filter_scalars_ok(f))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || (C > 0 && (!ctrl_fit || !ctrl_roll)) ||
        !filter_arrays_ok(f, steps, m_pred, S_pred))
        return set_error(nullptr, FFVD_EINVAL, bad);
    SummaryReq q{};
    const SummaryReq *sum = filter_summary(f, steps, q) ? &q : nullptr;
    OP_BEGIN_AS(whos);
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const int Mp = round_up(M, NB), nK = n_models * D;
    const size_t GD = (size_t)G * D, mm = (size_t)Mp * Mp;
    if (q_mode) w.qall = sc.alloc<double>(GD * mm);
    else { w.Mp16 = Mp; w.q0 = sc.alloc<double>((size_t)G * mm); }
    double *dW = sc.alloc<double>((size_t)nK * mm), *dxl = x0s ? sc.upload(x0s, GD) : sc.alloc<double>(GD);
    OP_CHECK_AS((w.qall || w.q0) && dW && dxl, whos);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    double *dZ = sc.upload(Zs, (size_t)n_models * M * P), *dS0 = S0s ? sc.upload(S0s, GD * D) : nullptr;
    double *dctrl = C ? sc.upload(ctrl_roll, (size_t)steps * C) : nullptr;
    OP_CHECK_AS(dZ && (!S0s || dS0) && (!C || dctrl), whos);
    launch_pg_pack(sc.stream, w.Kuu, 2 * mm, Mp, Mp, nK, 1, M, 1, dW, Mp, Mp, nK);
    if (!x0s) launch_pg_x_last(sc.stream, w.Xs, G, T, D, dxl);
    if (int rc = mg_run(sc, whos, G, n_models, M, P, D, C, steps, w.hv, dZ, dW, q_mode ? w.qall : w.q0, q_mode, w.U, dxl, dS0, w.log_Qs,
                        dctrl, m_pred, S_pred, sum, &f))
        return rc;
    if (U_means && !sc.download(U_means, w.U, GD * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, whos + ": copying the results back failed");
    return FFVD_OK;
}

// The summary of the moment-matched prediction for stacks the caller holds: they are uploaded, summarised by the same launch as in the
// two calls above
extern "C" int ffvd_op_moment_summary(const double *m_x, const double *S_x, int G, int steps, int D, const double *CC, const double *DD,
                                      const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean, double *y_var,
                                      double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string who = "ffvd_op_moment_summary", bad = who + ": bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    if (!summary_scalars_ok(q, G, steps, D) || D > MG_MAXD || (G > 0 && steps > 0 && G > ((1LL << 31) - 1) / steps / D / D))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!m_x || !S_x || !summary_arrays_ok(q)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN_AS(who);
    const size_t n = (size_t)G * steps * D;
    double *dm = sc.upload(m_x, n), *dS = sc.upload(S_x, n * D);
    OP_CHECK_AS(dm && dS, who);
    return mg_summary(sc, who, dm, dS, G, steps, D, q);
}
