// The elementary stateless operators of the C ABI (ffvd_op_*, include/ffvd_abi.h): what the Python mirror of the reference API calls.
// Temporaries per call, not the hot path.  The step loops are in ops_loops.hip, the grouped operators in ops_grouped.hip; the three
// share op_scratch.h, and only abi_internal.h with abi.hip.
#include "op_scratch.h"
#include "grad.h"
#include "optim.h"

#include <cmath>

using namespace ffvd;

// the one operator cache of a thread (op_scratch.h): every block that ops.hip, ops_loops.hip and ops_grouped.hip hand out comes from it
OpCache &ffvd::op_cache() { thread_local OpCache cache; return cache; }

// Free what the calling thread's operator cache holds (device buffers of finished ffvd_op_* calls, their stream).
extern "C" int ffvd_op_release_cache(void) {
    op_cache().release_all();
    return FFVD_OK;
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
    double *dX = sc.upload(X, (size_t)N * P), *dX2 = same ? dX : sc.upload(X2, (size_t)N2 * P);
    double *dl = sc.alloc<double>(P), *dO = sc.alloc<double>((size_t)N * N2);
    OP_CHECK(dX && dX2 && dl && dO, "ffvd_op_kernel_matrix");
    if (loglengthscales) OP_TRY(hipMemcpyAsync(dl, loglengthscales, P * sizeof(double), hipMemcpyHostToDevice, sc.stream));
    launch_kernel_matrix(sc.stream, kind, dX, N, dX2, N2, P, logvariance, dl, jitter, same, dO);
    OP_TRY(hipMemcpyAsync(out, dO, (size_t)N * N2 * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

extern "C" int ffvd_op_kernel_diag(int kind, const double *X, int N, int P, double logvariance, double *out) {
    if (!X || !out || N < 0 || P < 1) return set_error(nullptr, FFVD_EINVAL, "ffvd_op_kernel_diag: bad argument");
    OP_BEGIN("ffvd_op_kernel_diag");
    if (N == 0) return FFVD_OK;
    double *dX = sc.upload(X, (size_t)N * P), *dO = sc.alloc<double>(N);
    OP_CHECK(dX && dO, "ffvd_op_kernel_diag");
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
    int32_t *dinfo = sc.alloc<int32_t>(batch);
    double *dinv = sc.alloc<double>(potrf_scratch_doubles(np, batch));
    OP_CHECK(dA && dinfo && dinv, "ffvd_op_cholesky");
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
    double *dA = sc.upload(slab.data(), slab.size()), *dinv = sc.alloc<double>(DINV_STRIDE);
    OP_CHECK(dA && dinv, "ffvd_op_trsm");
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
    OP_CHECK(dW && dXc && dX && dlq && F && H && rowsq && hterms && cterms && info && dinv, "ffvd_op_collapse");
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
    OP_CHECK(dX && dU && rowsq && fmean && dmean && dvar, "ffvd_op_conditional");
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
    OP_CHECK(dX && dC && dD && dO, "ffvd_op_predict_mean");
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
    OP_CHECK(dy && dm && dR && dO, "ffvd_op_logdensity_norm_diag");
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
    OP_CHECK(dm && dv && de && dO, "ffvd_op_get_rand");
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
    OP_CHECK(dW && dXc && dX && dlq && F && rowsq && H && dU && info && dinv, "ffvd_op_collapse_u_mean");
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
    OP_CHECK(dW && dX && dU && F && rowsq && fmean && dmean && dvar && (!q_sqrt || (dQs && extra)), "ffvd_op_conditional_precalc");
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
    OP_CHECK(dX && dU && rowsq && fmean && dmean && dvar && F, who);
    // F = A^T = K_fu L^-T (:34 / :349), mean (:48 / :365)
    launch_project(sc.stream, op_project_args(kind, hv, dX, N, Tp, P, M, Mp, D, W, w_stride, dU, F, rowsq, fmean, ng));
    if (!full_cov) {
        double *dQs = q_sqrt ? sc.upload(q_sqrt, (size_t)M * M) : nullptr, *extra = q_sqrt ? sc.alloc<double>((size_t)D * Tp) : nullptr;
        OP_CHECK(!q_sqrt || (dQs && extra), who);
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
        OP_CHECK(dQt && E && extra, who);
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
    OP_CHECK(dA && dm && de && dO && dinfo && dinv, "ffvd_op_get_rand_full_cov");
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
    OP_CHECK(dth && dm && dv && dg, "ffvd_op_adam_step");
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
    OP_CHECK(dth && dxi && dg_ && dg2 && dp && dgrad && dnoise, "ffvd_op_sghmc_step");
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
