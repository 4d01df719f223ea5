// What the operator sources (ops.hip, ops_loops.hip, ops_grouped.hip) share: the per-thread cache of device temporaries, a call's
// Scratch, the lap timer of the timing switches, the OP_BEGIN / OP_CHECK forms and the set-up helpers that several operators use.
#pragma once
#include "abi_internal.h"
#include "kernels.h"
#include "step_bodies.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

namespace ffvd {

// ---- operator-level entry points (temporaries per call; not the hot path) -------------------------------------------------------------
// Round 5: the temporaries come from a per-thread cache instead of hipMalloc / hipFree / hipStreamCreate per call.  A rollout call made
// ~27 allocations and as many frees around 200 steps of 15 us: 2.7 ms of host work per call (profiles/r04_next_rows.json: 27.6 us per
// step of a 200-step call against 15.3 marginal).  A block is handed out again when its size fits (smallest block that is large enough
// and at most 4 x the request); the cache is bounded (256 blocks / 8 GiB: beyond that everything idle is freed) and can be released
// with ffvd_op_release_cache().  Nothing relies on fresh memory being zero (hipMalloc never promised that).
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
// the calling thread's cache: ONE object per thread for the whole library, defined in ops.hip
OpCache &op_cache();

struct Scratch {
    std::vector<size_t> mine;           // indices into the cache of the blocks this call holds
    hipStream_t stream = nullptr;
    // host staging buffers of this call (host()).  A member, so it outlives the destructor body: an asynchronous upload may read its
    // source until the stream has been synchronised, on the early error returns as well.
    std::deque<std::vector<double>> staged;
    bool begin() {
        OpCache &c = op_cache();
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
        OpCache &c = op_cache();
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
        OpCache &c = op_cache();
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
        OpCache &c = op_cache();
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

// `who` (a std::string or a string literal) names the entry point that was called
#define OP_BEGIN(who)                                                                        \
    Scratch sc;                                                                              \
    if (!sc.begin())                                                                         \
        return set_error(nullptr, FFVD_EDEVICE, std::string(who) + ": no usable HIP device / stream creation failed");
#define OP_CHECK(ptr, who) \
    if (!(ptr)) return set_error(nullptr, FFVD_ENOMEM, std::string(who) + ": device allocation or upload failed");

// ---- set-up shared by the operators ------------------------------------------------------------------------------------------------
// Device-side hyper-parameters of D kernels over the inducing inputs Z: uploads Z and logvariance, runs prep_hypers.  (LinearK has no
// lengthscales: its loglen block is allocated and not written.)
inline int stage_hypers(Scratch &sc, const char *who, int kind, const double *Z, int M, int Mp, int P, int D, const double *logvariance,
                        const double *loglengthscales, HyperView &hv) {
    double *dZ = sc.upload(Z, (size_t)M * P), *dlogvar = sc.upload(logvariance, D);
    double *loglen = sc.alloc<double>((size_t)D * P);
    double *variance = sc.alloc<double>(D), *len = sc.alloc<double>((size_t)D * P);
    double *Zs = sc.alloc<double>((size_t)D * Mp * P), *zz = sc.alloc<double>((size_t)D * Mp);
    OP_CHECK(dZ && dlogvar && loglen && variance && len && Zs && zz, who);
    if (loglengthscales)
        OP_TRY(hipMemcpyAsync(loglen, loglengthscales, (size_t)D * P * sizeof(double), hipMemcpyHostToDevice, sc.stream));
    launch_prep_hypers(sc.stream, kind, dZ, M, Mp, P, D, 0, dlogvar, loglen, variance, len, Zs, zz);
    hv = HyperView{variance, len, Zs, zz};
    return FFVD_OK;
}

// Projection arguments of an operator: one chain, all D dims, GP inputs x (T rows of P columns, no separate control block).
inline ProjectArgs op_project_args(int kind, const HyperView &hv, const double *x, int T, int Tp, int P, int M, int Mp, int D,
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
inline std::vector<double> &pad_identity(Scratch &sc, const double *src, int batch, int n, int np, double diag_add = 0.0) {
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
inline double *upload_stack(Scratch &sc, const double *src, int D, int M, int Mp) {
    if (M == Mp) return sc.upload(src, (size_t)D * M * M);
    std::vector<double> &pad = pad_identity(sc, src, D, M, Mp);
    return sc.upload(pad.data(), pad.size());
}

// n M x M matrices given as a table of host pointers -> a device stack of Mp x Mp slots.  The matrices are NOT packed on the host:
// each goes from where the caller keeps it straight into its slot (a pitched copy when M != Mp; the padding is zeroed on the device).
inline double *upload_matrix_table(Scratch &sc, const double *const *src, size_t n, int M, int Mp) {
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
inline int chol_not_pd(const char *who, const std::string &what, int d, int32_t flag) {
    return set_error(nullptr, FFVD_ENOTPD, std::string(who) + ": Cholesky of " + what + " failed: latent dim " + std::to_string(d) + ", pivot " +
                                               std::to_string(flag - 1) + " is not positive");
}
// read the D Cholesky flags back (synchronises the stream, so every copy enqueued before has landed too)
inline int fetch_chol_info(Scratch &sc, const int32_t *dinfo, int D, const char *who, const char *what) {
    std::vector<int32_t> hinfo(D, 0);
    if (hipMemcpyAsync(hinfo.data(), dinfo, D * sizeof(int32_t), hipMemcpyDeviceToHost, sc.stream) != hipSuccess ||
        hipStreamSynchronize(sc.stream) != hipSuccess)
        return set_error(nullptr, FFVD_EDEVICE, std::string(who) + ": device error while reading Cholesky status");
    for (int d = 0; d < D; ++d)
        if (hinfo[d]) return chol_not_pd(who, what, d, hinfo[d]);
    return FFVD_OK;
}

// W = L^-T is upper triangular; when q_sqrt (one M x M slice) is too -- the reference hands over L_H^-T -- so is W q_sqrt, and the second
// right-hand side of a step's product stops at a slab's last row like the first (exact zeros are skipped: half of its k range)
inline bool q_sqrt_is_upper(const double *q, int M) {
    for (int i = 1; i < M; ++i)
        for (int j = 0; j < i; ++j)
            if (q[(size_t)i * M + j] != 0.0) return false;
    return true;
}

inline void launch_skinny_gemm(hipStream_t stream, const SkinnyArgs &a) {
    launch_skinny_gemm(stream, a.A, a.a_stride, a.lda, a.B, a.b_stride, a.ldb, a.upper, a.rows, a.K, a.N, a.nb, a.Tp, a.C, a.c_stride,
                       a.ldc, a.u, a.u_stride, a.sq, a.dot, a.B2, a.b2_stride, a.ldb2, a.N2, a.sq2, a.a_trans, a.upper2);
}

}  // namespace ffvd
