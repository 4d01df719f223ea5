// The grouped operators of the C ABI: rollout summaries, grouped rollouts, grouped collapsed posteriors, grouped conditionals, and
// moment-matched prediction with filtering and rolling-origin forecasts (both under either propagation rule: moment matching or the
// linearisation at the filtered mean), and the linearised filter over many records in one call.  Each staging block (hyper-parameters, a caller's posterior,
// a posterior formed in the call, the emission of a summary) is written once and shared by the entry points.
#include "op_scratch.h"
#include "rollout_group.h"
#include "posterior_group.h"
#include "conditional_group.h"
#include "predict_summary.h"
#include "moment_group.h"
#include "moment_particle_draws.h"
#include "transition_grad.h"

#include <cmath>

using namespace ffvd;

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

// The emission of a summary or a filter on the device, from the caller's arrays: CC (D x J), DD, noise_std (J), `rows` rows of Y (0: none)
struct Emission { const double *CC, *DD, *sd, *Y; bool ok; };
Emission stage_emission(Scratch &sc, int D, int J, const double *CC, const double *DD, const double *noise_std, const double *Y, size_t rows) {
    Emission e{sc.upload(CC, (size_t)D * J), sc.upload(DD, J), sc.upload(noise_std, J), rows ? sc.upload(Y, rows * J) : nullptr, false};
    e.ok = e.CC && e.DD && e.sd && (!rows || e.Y);
    return e;
}

// The tail of a summary: its five fields (steps x J each, at dout; n_out doubles in all) come down in one small copy and go to the
// outputs that were asked for (n_test rows of the last two)
int fetch_summary(Scratch &sc, const double *dout, size_t n_out, int steps, const SummaryReq &q) {
    const size_t SJ = (size_t)steps * q.J, TJ = (size_t)q.n_test * q.J;
    OP_TRY(hipGetLastError());
    std::vector<double> &h = sc.host(n_out);
    OP_TRY(hipMemcpyAsync(h.data(), dout, h.size() * sizeof(double), hipMemcpyDeviceToHost, sc.stream));
    OP_TRY(hipStreamSynchronize(sc.stream));
    double *const dst[5] = {q.y_mean, q.y_var, q.y_var_total, q.lpd, q.lpd_gauss};
    for (int f = 0; f < 5; ++f)
        if (dst[f]) memcpy(dst[f], h.data() + f * SJ, (f < 3 ? SJ : TJ) * sizeof(double));
    return FFVD_OK;
}

// The two launches of predict_summary.h on stacks that are on the device, then the requested outputs come down.
int run_summary(Scratch &sc, const std::string &who, const double *dpx, const double *dpv, int N, int steps, int D, const SummaryReq &q) {
    const Emission e = stage_emission(sc, D, q.J, q.CC, q.DD, q.noise_std, q.Y_test, q.n_test);
    PredictSummaryArgs a{};
    a.N = N; a.steps = steps; a.D = D; a.J = q.J; a.n_test = q.n_test; a.x = dpx; a.v = dpv;
    a.CC = e.CC; a.DD = e.DD; a.sd = e.sd; a.Y = e.Y;
    a.part = sc.alloc<double>(ps_part_doubles(N, steps, q.J));
    a.out = sc.alloc<double>(ps_out_doubles(steps, q.J));
    OP_CHECK(e.ok && a.part && a.out, who);
    launch_predict_summary(sc.stream, a);
    return fetch_summary(sc, a.out, ps_out_doubles(steps, q.J), steps, q);
}

// the summary launch of moment_group.h on stacks that are on the device, then the requested outputs come down
int mg_summary(Scratch &sc, const std::string &who, const double *dm, const double *dS, int G, int steps, int D, const SummaryReq &q) {
    const Emission e = stage_emission(sc, D, q.J, q.CC, q.DD, q.noise_std, q.Y_test, q.n_test);
    MomentSummaryArgs a{};
    a.G = G; a.steps = steps; a.D = D; a.J = q.J; a.n_test = q.n_test; a.m = dm; a.S = dS;
    a.CC = e.CC; a.DD = e.DD; a.sd = e.sd; a.Y = e.Y;
    a.out = sc.alloc<double>((size_t)5 * steps * q.J);
    OP_CHECK(e.ok && a.out, who);
    launch_moment_summary(sc.stream, a);
    return fetch_summary(sc, a.out, (size_t)5 * steps * q.J, steps, q);
}

// ---- staging shared by the grouped operators -----------------------------------------------------------------------------------------
// Device hyper-parameters of n models (n * D kernels over n sets of inducing inputs), in three steps that a caller places among its
// own requests, because which cached block a buffer is handed depends on the order of a call's requests and every call keeps the
// order it always had: stage_group_hypers uploads Z; logs() uploads logvar and loglen (nullptr: no lengthscales); blocks() allocates
// what launch_rg_prep fills and says whether all three steps succeeded.  prep(): that launch, the caller's to place.
struct GroupHypers {
    int kind, n, D, M, Mp, P;
    const double *logvar, *loglen;               // the host arrays, until logs()
    double *dZ, *dlv, *dll;                      // uploaded: [n][M][P], [n][D], [n][D][P]
    double *variance, *len, *Zsc, *zz;           // HyperView's layout
    bool uploaded;
    bool logs(Scratch &sc) {
        dlv = sc.upload(logvar, (size_t)n * D); dll = loglen ? sc.upload(loglen, (size_t)n * D * P) : nullptr;
        return uploaded = dZ && dlv && (!loglen || dll);
    }
    bool blocks(Scratch &sc) {
        const size_t nK = (size_t)n * D;
        variance = sc.alloc<double>(nK); len = sc.alloc<double>(nK * P); Zsc = sc.alloc<double>(nK * Mp * P); zz = sc.alloc<double>(nK * Mp);
        return uploaded && variance && len && Zsc && zz;
    }
    HyperView hv() const { return HyperView{variance, len, Zsc, zz}; }
    void prep(hipStream_t stream) const { launch_rg_prep(stream, kind, n, D, M, Mp, P, dZ, dlv, dll, variance, len, Zsc, zz); }
};
GroupHypers stage_group_hypers(Scratch &sc, int kind, int n, int D, int M, int Mp, int P, const double *Zs, const double *logvar,
                               const double *loglen) {
    GroupHypers h{kind, n, D, M, Mp, P, logvar, loglen};
    h.dZ = sc.upload(Zs, (size_t)n * M * P);
    return h;
}

// A posterior given by the caller: nW matrices W = L^-T and nq slices of q_sqrt (none without q_sqrts) as tables of host pointers,
// each uploaded by upload_matrix_table.  given_nq / given_tables_ok read host memory only: the entry points call them before OP_BEGIN.
size_t given_nq(const double *const *q_sqrts, int q_mode, int G, int D) { return q_sqrts ? (q_mode ? (size_t)G * D : (size_t)G) : 0; }
bool given_tables_ok(const double *const *Lm_inverse_seqs, size_t nW, const double *const *q_sqrts, size_t nq) {
    for (size_t b = 0; b < nW; ++b) if (!Lm_inverse_seqs[b]) return false;
    for (size_t b = 0; b < nq; ++b) if (!q_sqrts[b]) return false;
    return true;
}
// W q_sqrt is upper triangular when EVERY slice of q_sqrt is (the reference hands over L_H^-T): the products then stop at a slab's last
// row for both right-hand sides.  Otherwise they walk all rows; for a group whose slice IS upper triangular the extra terms are exact
// zeros, so its results do not depend on what the other groups hold.  Reads every strict lower triangle: only the rollouts and the
// conditionals, whose kernels take the cut, ask -- between the two uploads, while W is on its way.
int given_q_upper(const double *const *q_sqrts, size_t nq, int M) {
    for (size_t b = 0; b < nq; ++b) if (!q_sqrt_is_upper(q_sqrts[b], M)) return 0;
    return nq ? 1 : 0;
}

// ---- grouped rollouts (rollout_group.h): the limits and the shared runner ----------------------------------------------------------------
bool rg_limits_ok(int G, int D, int R, int Mp) {
    return (long long)G * D * Mp * Mp <= (1LL << 29) && (long long)G * R <= (1LL << 20) && (R + RG_RC - 1) / RG_RC <= 65535 &&
           (long long)G * D * (Mp / RG_SLAB) < (1LL << 31);
}

// The grouped rollout on operands that are on the device: gh, the uploaded hyper-parameters of G models at Mp = M rounded up to
// RG_SLAB; dW, [G * D] slots of Mp x Mp; dq, nullptr or [G] slots of q_sqrt, with dB, [G * D] slots for W q_sqrt; dU, dxl, dlq per
// group; deps, dctrl.  Then hyper-parameters and W q_sqrt (the timer's ready_lap), one launch per step for all groups, the summary where
// the step launches wrote (sum: predict_x / predict_var may each be NULL, not downloaded), the downloads (U_means from dU).
int rg_run(Scratch &sc, const std::string &who, LapTimer &timer, const char *ready_lap, GroupHypers &gh, int R, int C, int steps,
           const double *dW, const double *dq, double *dB, int q_upper, const double *dU, const double *dxl, const double *dlq,
           const double *dctrl, const double *deps, double *predict_x, double *predict_var, double *U_means, const SummaryReq *sum) {
    const int G = gh.n, D = gh.D, M = gh.M, Mp = gh.Mp, NS = Mp / RG_SLAB;
    const size_t GD = (size_t)G * D, out_n = (size_t)G * R * steps * D;
    const bool hypers = gh.blocks(sc);
    double *part = sc.alloc<double>((size_t)2 * GD * NS * R * 4), *xbuf = sc.alloc<double>((size_t)2 * G * R * D);
    double *dpx = sc.alloc<double>(out_n), *dpv = sc.alloc<double>(out_n);
    OP_CHECK(hypers && part && xbuf && dpx && dpv, who);
    gh.prep(sc.stream);
    if (dq) launch_rg_wq(sc.stream, G, D, Mp, q_upper, dW, dq, dB);
    timer.lap(ready_lap);
    RolloutGroupArgs a{};
    a.kind = gh.kind; a.G = G; a.R = R; a.D = D; a.C = C; a.P = gh.P; a.M = M; a.Mp = Mp; a.NS = NS; a.steps = steps;
    a.has_q = dq ? 1 : 0; a.q_upper = q_upper;
    a.W = dW; a.B = dB; a.Zs = gh.Zsc; a.zz = gh.zz; a.variance = gh.variance; a.len = gh.len; a.f = dU; a.x_last = dxl; a.log_Q = dlq;
    a.ctrl = dctrl; a.eps = deps; a.part = part; a.xbuf = xbuf; a.predict_x = dpx; a.predict_var = dpv;
    for (int t = 0; t <= steps; ++t) launch_rg_step(sc.stream, a, t);
    OP_TRY(hipGetLastError());
    timer.lap("step launches");
    if (sum) {
        if (int rc = run_summary(sc, who, dpx, dpv, G * R, steps, D, *sum)) return rc;
        timer.lap("summary");
    }
    if ((predict_x && !sc.download(predict_x, dpx, out_n * sizeof(double))) ||
        (predict_var && !sc.download(predict_var, dpv, out_n * sizeof(double))) ||
        (U_means && !sc.download(U_means, dU, GD * M * sizeof(double))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    timer.lap("results downloaded");
    return FFVD_OK;
}
}  // namespace

// base_model.py:330-348 for stacks the caller holds: they are uploaded, summarised by the same launches as in the fused calls
extern "C" int ffvd_op_rollout_summary(const double *predict_x, const double *predict_var, int N, int steps, int D, const double *CC,
                                       const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                                       double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string who = "ffvd_op_rollout_summary", bad = who + ": bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    if (!summary_scalars_ok(q, N, steps, D)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (N == 0 || steps == 0) return FFVD_OK;
    if (!predict_x || !predict_var || !summary_arrays_ok(q)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    const size_t n = (size_t)N * steps * D;
    double *dpx = sc.upload(predict_x, n), *dpv = sc.upload(predict_var, n);
    OP_CHECK(dpx && dpv, who);
    return run_summary(sc, who, dpx, dpv, N, steps, D, q);
}

// G posteriors given by the caller, one launch per step for all of them (rollout_group.hip)
static int rollout_grouped_run(const std::string &who, int kind, int G, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                               int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                               const double *const *q_sqrts, const double *x_lasts, int R, const double *ctrl, int C, int steps,
                               const double *log_Qs, const double *eps, double *predict_x, double *predict_var, const SummaryReq *sum) {
    const std::string bad = who + ": bad argument";
    if ((kind != FFVD_KERNEL_SE && kind != FFVD_KERNEL_LINEAR) || G < 0 || R < 1 || steps < 0 || M < 1 || M > 2048 || D < 1 || C < 0 ||
        P != D + C || P > MAXP)
        return set_error(nullptr, FFVD_EINVAL, bad);
    const int Mp = round_up(M, RG_SLAB);
    if (!rg_limits_ok(G, D, R, Mp)) return set_error(nullptr, FFVD_EINVAL, bad + " (beyond the limits of rollout_group.h)");
    if (sum && !summary_scalars_ok(*sum, (long long)G * R, steps, D)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !fs || !x_lasts || !log_Qs || !eps || (!sum && (!predict_x || !predict_var)) ||
        (C > 0 && !ctrl) || (kind == FFVD_KERNEL_SE && !loglengthscales) || (sum && !summary_arrays_ok(*sum)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t GD = (size_t)G * D, nq = given_nq(q_sqrts, 0, G, D);
    if (!given_tables_ok(Lm_inverse_seqs, GD, q_sqrts, nq)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    LapTimer timer("FFVD_RG_TIMING", who.c_str(), sc.stream);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, GD, M, Mp);
    timer.lap("W uploaded");
    const int q_upper = given_q_upper(q_sqrts, nq, M);
    timer.lap("q_sqrt scanned");
    double *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr, *dB = nq ? sc.alloc<double>(GD * Mp * Mp) : nullptr;
    GroupHypers gh = stage_group_hypers(sc, kind, G, D, M, Mp, P, Zs, logvariances, loglengthscales);
    double *dU = sc.upload(fs, GD * M), *dxl = sc.upload(x_lasts, GD);
    const bool hypers = gh.logs(sc);
    double *dlq = sc.upload(log_Qs, GD), *deps = sc.upload(eps, (size_t)steps * G * R * D), *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    OP_CHECK(dW && (!nq || (dq && dB)) && hypers && dU && dxl && dlq && deps && (!C || dctrl), who);
    timer.lap("q_sqrt, small arrays uploaded");
    return rg_run(sc, who, timer, "hyper-parameters, W q_sqrt", gh, R, C, steps, dW, dq, dB, q_upper, dU, dxl, dlq, dctrl, deps, predict_x,
                  predict_var, nullptr, sum);
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

// ---- grouped collapsed posteriors (posterior_group.h) ---------------------------------------------------------------------------------
// U_mean and L_H^-T of collapse_u_mean_after_kernel_precalculation (conditionals_multi_output.py:206-227, called at
// base_model.py:243-256) for G groups over n_models (1 or G) sets of Z / hyper-parameters, with the K_uu factors of kernel_pre_cal
// (:124-169) formed in the same call.  Everything between the small uploads and the results stays on the device.
namespace {
struct PgIn {
    std::string who;
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

// The q_sqrt slices that a posterior hands on in slots of the block size of its factorisations, asked for before pg_posterior:
// every (group, dim) slice for q_mode 1, slice d = 0 of each group otherwise.  pg_q: what was packed.
bool pg_want_q(Scratch &sc, PgWork &w, int q_mode, int G, int D, int M) {
    const int Mp = round_up(M, NB);
    if (q_mode) w.qall = sc.alloc<double>((size_t)G * D * Mp * Mp);
    else { w.Mp16 = Mp; w.q0 = sc.alloc<double>((size_t)G * Mp * Mp); }
    return w.qall || w.q0;
}
const double *pg_q(const PgWork &w, int q_mode) { return q_mode ? w.qall : w.q0; }

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
    const std::string &who = in.who;

    GroupHypers gh = stage_group_hypers(sc, kind, nm, D, M, Mp, P, in.Zs, in.logvar, in.loglen);      // (prep: in the loop below)
    gh.logs(sc);
    double *dctrl = C ? sc.upload(in.ctrl_fit, (size_t)T * C) : nullptr;
    w.Xs = sc.upload(in.Xs, (size_t)G * (T + 1) * D);
    w.log_Qs = sc.upload(in.log_Qs, GD);
    const bool hypers = gh.blocks(sc);
    double *const variance = gh.variance, *const len = gh.len, *const Zsc = gh.Zsc, *const zz = gh.zz;
    double *Xt = sc.alloc<double>((size_t)(T + 1) * GD);
    w.Kuu = sc.alloc<double>((size_t)nK * kstride);
    w.hv = gh.hv();
    double *F = sc.alloc<double>((size_t)upp * fstride), *H = sc.alloc<double>((size_t)upp * hstride);
    double *ubuf = sc.alloc<double>((size_t)upp * M);
    w.U = sc.alloc<double>((size_t)GD * M);
    const int kchunk = nK < 32768 ? nK : 32768;
    double *dinvK = sc.alloc<double>(potrf_scratch_doubles(Mp, kchunk)), *dinvH = sc.alloc<double>(potrf_scratch_doubles(Mp, upp));
    int32_t *info = sc.alloc<int32_t>((size_t)nK + GD);
    OP_CHECK(hypers && (!C || dctrl) && w.Xs && w.log_Qs && Xt && w.Kuu && F && H && ubuf && w.U && dinvK && dinvH && info, who);

    std::vector<int32_t> hinfo((size_t)nK + GD, 0);
    for (int attempt = 0;; ++attempt) {
        {
            CholOverrideGuard guard;            // reset on the error returns below as well
            if (attempt == 1) guard.force_left();
            OP_TRY(hipMemsetAsync(info, 0, ((size_t)nK + GD) * sizeof(int32_t), sc.stream));
            // 1. hyper-parameters of every (model, dim): prep_hypers' arithmetic, one launch, in HyperView's layout
            gh.prep(sc.stream);
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
    const std::string who = "ffvd_op_posterior_grouped", bad = who + ": bad argument";
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0) return FFVD_OK;
    if (!Zs || !logvariances || !Xs || !log_Qs || !U_means || (C > 0 && !ctrl_fit) || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const size_t GD = (size_t)G * D, MM = (size_t)M * M, nK = (size_t)n_models * D;
    if (H_inv_sqrts) w.Hpack = sc.alloc<double>(GD * MM);
    double *Lpack = Lm_inverse ? sc.alloc<double>(nK * MM) : nullptr;
    OP_CHECK((!H_inv_sqrts || w.Hpack) && (!Lm_inverse || Lpack), who);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    if (Lpack) launch_pg_pack(sc.stream, w.Kuu, (size_t)2 * w.Mp * w.Mp, w.Mp, w.Mp, (int)nK, 1, M, 0, Lpack, M, M, (int)nK);
    OP_TRY(hipGetLastError());
    if (!sc.download(U_means, w.U, GD * M * sizeof(double)) || (H_inv_sqrts && !sc.download(H_inv_sqrts, w.Hpack, GD * MM * sizeof(double))) ||
        (Lpack && !sc.download(Lm_inverse, Lpack, nK * MM * sizeof(double))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    return FFVD_OK;
}

// The posteriors above handed to the grouped rollout loop (base_model.py:243-314 per group) without leaving the device: W, q0, f and
// x_last of RolloutGroupArgs are written by posterior_group.hip's kernels from the factorisation slabs, then rg_run.
static int posterior_rollout_grouped_run(const std::string &who, int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                         const double *logvariances, const double *loglengthscales, const double *Xs,
                                         const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter, int groups_per_pass,
                                         int R, const double *ctrl_roll, int steps, const double *eps, double *predict_x,
                                         double *predict_var, double *U_means, const SummaryReq *sum) {
    const std::string bad = who + ": bad argument";
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || R < 1 || steps < 0)
        return set_error(nullptr, FFVD_EINVAL, bad);
    const int Mp16 = round_up(M, RG_SLAB);
    if (!rg_limits_ok(G, D, R, Mp16)) return set_error(nullptr, FFVD_EINVAL, bad + " (beyond the limits of rollout_group.h)");
    if (sum && !summary_scalars_ok(*sum, (long long)G * R, steps, D)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Zs || !logvariances || !Xs || !log_Qs || !eps || (!sum && (!predict_x || !predict_var)) || (C > 0 && (!ctrl_fit || !ctrl_roll)) ||
        (kind == FFVD_KERNEL_SE && !loglengthscales) || (sum && !summary_arrays_ok(*sum)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    LapTimer timer("FFVD_RG_TIMING", who.c_str(), sc.stream);
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const size_t GD = (size_t)G * D, mm16 = (size_t)Mp16 * Mp16;
    w.Mp16 = Mp16; w.q0 = sc.alloc<double>((size_t)G * mm16);
    double *dW = sc.alloc<double>(GD * mm16), *dB = sc.alloc<double>(GD * mm16);
    OP_CHECK(w.q0 && dW && dB, who);
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
    GroupHypers gh = stage_group_hypers(sc, kind, G, D, M, Mp16, P, hZ, hlv, hll);
    gh.logs(sc);
    double *deps = sc.upload(eps, (size_t)steps * G * R * D), *dctrl = C ? sc.upload(ctrl_roll, (size_t)steps * C) : nullptr, *dxl = sc.alloc<double>(GD);
    OP_CHECK(gh.uploaded && deps && (!C || dctrl) && dxl, who);
    // W[g][d] = L^-T of the group's model; with one model every group reads the same slab (the stack is still materialised)
    launch_pg_pack(sc.stream, w.Kuu, (size_t)2 * w.Mp * w.Mp, w.Mp, w.Mp, w.nK, 1, M, 1, dW, Mp16, Mp16, (int)GD);
    launch_pg_x_last(sc.stream, w.Xs, G, T, D, dxl);
    // (q_upper: q0's strict lower triangle was written as exact zeros)
    return rg_run(sc, who, timer, "operands packed, W q_sqrt", gh, R, C, steps, dW, w.q0, dB, 1, w.U, dxl, w.log_Qs, dctrl, deps, predict_x,
                  predict_var, U_means, sum);
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
    OP_CHECK(a.F && a.rowsq && a.Ut && a.mbuf && (!need.part || a.part) && a.mean && (!a.need_var || a.var) && (!o.mix_mean || (dmm && dmv)), who);
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
    const std::string who = "ffvd_op_conditional_grouped", bad = who + ": bad argument";
    if (!cg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || N == 0) return FFVD_OK;
    const CgOut out{means, vars, mix_mean, mix_var};
    if (!Lm_inverse_seqs || !Zs || !logvariances || !fs || !Xnew || !cg_outputs_ok(out) || (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t nK = (size_t)n_models * D, nq = given_nq(q_sqrts, q_mode, G, D);
    if (!given_tables_ok(Lm_inverse_seqs, nK, q_sqrts, nq)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    const int Mp = round_up(M, NB);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp);
    const int q_upper = given_q_upper(q_sqrts, nq, M);
    double *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    GroupHypers gh = stage_group_hypers(sc, kind, n_models, D, M, Mp, P, Zs, logvariances, loglengthscales);
    double *dU = sc.upload(fs, (size_t)G * D * M), *dX = sc.upload(Xnew, (size_t)N * P);
    OP_CHECK(dW && (!nq || dq) && dU && dX && gh.logs(sc) && gh.blocks(sc), who);
    gh.prep(sc.stream);
    return cg_run(sc, who, kind, G, n_models, M, P, D, N, rows_per_pass, gh.hv(), dW, (size_t)Mp * Mp, dU, dq, q_mode, q_upper, dX, out);
}

// The collapsed posteriors of ffvd_op_posterior_grouped (base_model.py:243-256) evaluated at Xnew without leaving the device: L^-T is
// read in the K_uu slabs, U_mean where the matvec left it, the q slices are packed by launch_pg_pack (exact zeros in the padding and
// the strict lower triangle, so the k cut holds by construction).
extern "C" int ffvd_op_posterior_conditional_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                     const double *logvariances, const double *loglengthscales, const double *Xs,
                                                     const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                     int groups_per_pass, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                                     double *means, double *vars, double *mix_mean, double *mix_var, double *U_means) {
    const std::string who = "ffvd_op_posterior_conditional_grouped", bad = who + ": bad argument";
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) ||
        !cg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || N == 0) return FFVD_OK;
    const CgOut out{means, vars, mix_mean, mix_var};
    if (!Zs || !logvariances || !Xs || !log_Qs || !Xnew || !cg_outputs_ok(out) || (C > 0 && !ctrl_fit) ||
        (kind == FFVD_KERNEL_SE && !loglengthscales))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const size_t mm = (size_t)round_up(M, NB) * round_up(M, NB);
    const bool need_q = vars || mix_var, have_q = need_q && pg_want_q(sc, w, q_mode, G, D, M);
    double *dX = sc.upload(Xnew, (size_t)N * P);
    OP_CHECK(dX && (!need_q || have_q), who);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    if (int rc = cg_run(sc, who, kind, G, n_models, M, P, D, N, rows_per_pass, w.hv, w.Kuu + mm, 2 * mm, w.U, pg_q(w, q_mode), q_mode, 1, dX, out))
        return rc;
    if (U_means && !sc.download(U_means, w.U, (size_t)G * D * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
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
// the propagation rule of the filter's launches (mg_run)
enum { MG_METHOD_MOMENT = 0, MG_METHOD_LINEAR = 1, MG_METHOD_CUBATURE = 2, MG_METHOD_PARTICLE = 3, MG_METHOD_ADAPTED = 4, MG_METHOD_ADAPTIVE = 5 };    // (cubature and particle: the records calls and the forecasts; adapted, adaptive: the records calls)
// the trailing summary block of the entry points: asked for when anything in it is given
bool mg_summary_wanted(const SummaryReq &q) {
    return q.CC || q.DD || q.noise_std || q.J != 0 || q.Y_test || q.n_test != 0 || q.y_mean || q.y_var || q.y_var_total || q.lpd || q.lpd_gauss;
}

// The filter request of mg_run: the emission, the observations (NaN = unobserved) and the outputs, each of which may be NULL
struct FilterReq {
    const double *CC, *DD, *noise_std;           // D x J, J, J
    int J;
    const double *Y_obs;                         // steps x J
    double *m_filt, *S_filt, *cross, *lpd, *lpd_joint, *m_smooth, *S_smooth;
    double *y_mean, *y_var_total, *lpd_mix, *lpd_gauss;      // the pooled one-step summary (steps x J)
    // ... as a summary request on the predicted stacks: every row carries an observation row (NaN entries give NaN densities)
    SummaryReq pooled(int steps) const { return SummaryReq{CC, DD, noise_std, J, Y_obs, steps, y_mean, nullptr, y_var_total, lpd_mix, lpd_gauss}; }
};
// the checks of a filter request that need no array, and those that read the small arrays (Y_obs: no infinity)
bool filter_scalars_ok(const FilterReq &f) { return f.J >= 1 && f.J <= MG_MAXJ; }
bool filter_arrays_ok(const FilterReq &f, int steps, const double *m_pred, const double *S_pred, bool other_output = false) {
    if (!f.CC || !f.DD || !f.noise_std || !f.Y_obs) return false;
    if (!(other_output || m_pred || S_pred || f.m_filt || f.S_filt || f.cross || f.lpd || f.lpd_joint || f.m_smooth || f.S_smooth || f.y_mean ||
          f.y_var_total || f.lpd_mix || f.lpd_gauss))
        return false;
    for (int j = 0; j < f.J; ++j)
        if (!std::isfinite(f.noise_std[j]) || !(f.noise_std[j] > 0.0)) return false;
    for (size_t e = 0; e < (size_t)steps * f.J; ++e)
        if (std::isinf(f.Y_obs[e])) return false;
    return true;
}

// The forecast request of mg_run (with a filter request): from every origin (a row of the record, ascending) `horizon` steps of the
// propagation started at the filtered state of that row, as tracks of moment_group.h's fan launch; the outputs, each of which may be NULL
struct ForecastReq {
    int horizon, n_origins, tracks_per_pass;
    const int *origins;
    double *m_fc, *S_fc;                                     // [G][B][h][D], [G][B][h][D][D]
    double *y_mean, *y_var_total, *lpd_mix, *lpd_gauss;      // pooled over the groups, [B * h][J]: row b * h + k against Y_obs[origins[b] + 1 + k]
    bool any_output() const { return m_fc || S_fc || y_mean || y_var_total || lpd_mix || lpd_gauss; }
};
// the checks of a forecast request that need no array (G * B * h * D * D < 2^31), and the origin table: strictly ascending, every
// track inside the record so that its control rows exist
bool forecast_scalars_ok(const ForecastReq &q, int G, int steps, int D) {
    if (q.horizon < 1 || q.n_origins < 1 || q.tracks_per_pass < 0) return false;
    return G == 0 || steps == 0 || (long long)G * q.n_origins <= ((1LL << 31) - 1) / q.horizon / D / D;
}
bool forecast_origins_ok(const ForecastReq &q, int steps) {
    if (!q.origins) return false;
    for (int b = 0; b < q.n_origins; ++b)
        if (q.origins[b] < 0 || q.origins[b] > steps - 1 - q.horizon || (b > 0 && q.origins[b] <= q.origins[b - 1])) return false;
    return true;
}

// The posterior terms of the moment family and of the linearisation, on operands that are on the device: beta = W u per (group, dim)
// and Gamma = W (I - q q^T) W^T per unit -- (group, dim) with q slices, (model, dim) without (W W^T: one model shared by the groups
// is formed once).  alloc() makes the requests (a caller places them among its own), launch() enqueues the products.  want_gam =
// false: beta alone (a caller that asks for no variance).
// dW: [nm * D] slots of Mp x Mp (upper triangular, zero padded); dq: nullptr, or [G] (q_mode 0) / [G * D] (q_mode 1) slots.
struct BetaGamma {
    int units, nq;
    double *beta, *gam;                          // [G * D][Mp], [units][Mp][Mp]
    double *dN, *dE, *dWE, *unused;
    bool alloc(Scratch &sc, int G, int nm, int D, int Mp, const double *dq, int q_mode, bool want_gam = true) {
        const int GD = G * D;
        const size_t mm = (size_t)Mp * Mp;
        units = dq ? GD : nm * D; nq = dq ? (q_mode ? GD : G) : 0;
        beta = sc.alloc<double>((size_t)GD * Mp);
        if (!want_gam) return beta != nullptr;
        gam = sc.alloc<double>((size_t)units * mm);
        dN = dq ? sc.alloc<double>((size_t)nq * mm) : nullptr; dE = dq ? sc.alloc<double>((size_t)nq * mm) : nullptr;
        dWE = dq ? sc.alloc<double>((size_t)GD * mm) : nullptr;
        unused = sc.alloc<double>((size_t)(nq > units ? nq : units));          // (cov.hip reads a variance per slot for its seed: none here)
        return beta && gam && (!dq || (dN && dE && dWE)) && unused;
    }
    int launch(Scratch &sc, int G, int nm, int M, int D, int Mp, const double *len, const double *dW, const double *dq, int q_mode,
               const double *dU) const {
        const int nK = nm * D;
        const size_t mm = (size_t)Mp * Mp;
        launch_mg_beta(sc.stream, G, D, M, Mp, nm == G, dW, dU, beta);
        if (!gam) return FFVD_OK;
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
            sym.kind = FFVD_KERNEL_LINEAR; sym.P = 0; sym.variance = unused; sym.len = len;
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
        return FFVD_OK;
    }
};

// Operands on the device -> beta, Gamma, the step launches, the summary, the downloads.  flt: the launches are those of the filter
// (moment_group.h), m_x / S_x are the predicted moments, and `sum` is REPLACED by the pooled one-step summary of the request when that
// asks for one (the filter callers pass nullptr).  method: the propagation rule of the filter's launches, MG_METHOD_MOMENT (moment
// matching) or MG_METHOD_LINEAR (the linearisation at the filtered mean, moment_linear.hip; with a forecast request the tracks take
// the same rule: moment_linear_fan.hip, two launches per step and pass) or, with a forecast request only, MG_METHOD_CUBATURE (the
// filter is the cubature records launch with one record, moment_cubature_records.hip: [G][1][steps] stacks are [G][steps] stacks;
// the tracks are moment_cubature_fan.hip's; K, the partials, the mean sums and the offsets are sized for the larger stage, the tracks').
// MG_METHOD_PARTICLE, with a forecast request and a particle forecast request only: the body is mg_particle_fc_run, beside the particle
// records' driver.
// dW: [n_models * D] slots of Mp x Mp (upper triangular, zero padded); dq: nullptr, or [G] (q_mode 0) / [G * D] (q_mode 1) slots of
// Mp x Mp; hv: variance / len per (model, dim).
struct ParticleFcReq;
int mg_particle_fc_run(Scratch &sc, const std::string &who, int G, int nm, int M, int P, int D, int C, int steps, const HyperView &hv,
                       const double *dZ, const double *dW, const double *dq, int q_mode, const double *dU, const double *dxl, const double *dS0,
                       const double *dlq, const double *dctrl, double *m_x, double *S_x, const FilterReq &flt, const ForecastReq &fc,
                       const ParticleFcReq &pf);
int mg_run(Scratch &sc, const std::string &who, int G, int nm, int M, int P, int D, int C, int steps, const HyperView &hv, const double *dZ,
           const double *dW, const double *dq, int q_mode, const double *dU, const double *dxl, const double *dS0, const double *dlq,
           const double *dctrl, double *m_x, double *S_x, const SummaryReq *sum, const FilterReq *flt, const ForecastReq *fc = nullptr,
           int method = MG_METHOD_MOMENT, const ParticleFcReq *pf = nullptr) {
    if (method == MG_METHOD_PARTICLE) {
        if (!(flt && fc && pf))
            return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (the particle rule is built for the records filter and the forecasts only)");
        return mg_particle_fc_run(sc, who, G, nm, M, P, D, C, steps, hv, dZ, dW, dq, q_mode, dU, dxl, dS0, dlq, dctrl, m_x, S_x, *flt, *fc, *pf);
    }
    const int Mp = round_up(M, NB), NS = (M + MG_SLAB - 1) / MG_SLAB;
    const bool linear = method == MG_METHOD_LINEAR, cub = method == MG_METHOD_CUBATURE;
    if (linear && !flt)
        return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (the linearised rule is built for the filter and its forecasts only)");
    if (cub && !(flt && fc))
        return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (the cubature rule is built for the records filter and the forecasts only)");
    const int nrow = cub ? mg_crec_rows(D) : 1;                // rows of K per track
    const size_t nm_x = (size_t)G * steps * D, nS_x = nm_x * D;
    const SummaryReq fsum = flt ? flt->pooled(steps) : SummaryReq{};
    if (fsum.y_mean || fsum.y_var_total || fsum.lpd || fsum.lpd_gauss) sum = &fsum;
    BetaGamma bg{};
    const bool terms = bg.alloc(sc, G, nm, D, Mp, dq, q_mode);
    double *part = sc.alloc<double>(cub ? 1 : (size_t)2 * G * (linear ? mg_linear_fields(D) : mg_fields(D)) * NS), *state = sc.alloc<double>((size_t)2 * G * (D + D * D));
    double *dm = sc.alloc<double>(nm_x), *dS = sc.alloc<double>(nS_x);
    OP_CHECK(terms && part && state && dm && dS, who);
    MomentFilterArgs fa{};
    MomentSmoothArgs sa{};
    const bool smooth = flt && (flt->m_smooth || flt->S_smooth);
    const size_t nlpd = flt ? (size_t)G * steps * flt->J : 0, nlj = (size_t)G * steps;
    if (flt) {
        const Emission e = stage_emission(sc, D, flt->J, flt->CC, flt->DD, flt->noise_std, flt->Y_obs, steps);
        fa.J = flt->J; fa.CC = e.CC; fa.DD = e.DD; fa.sd = e.sd; fa.Y = e.Y;
        fa.m_filt = sc.alloc<double>(nm_x); fa.S_filt = sc.alloc<double>(nS_x); fa.cross = sc.alloc<double>(nS_x);
        fa.lpd = sc.alloc<double>(nlpd); fa.lpd_joint = sc.alloc<double>(nlj);
        OP_CHECK(e.ok && fa.m_filt && fa.S_filt && fa.cross && fa.lpd && fa.lpd_joint, who);
        if (smooth) {
            sa.G = G; sa.D = D; sa.steps = steps; sa.m_pred = dm; sa.S_pred = dS; sa.m_filt = fa.m_filt; sa.S_filt = fa.S_filt;
            sa.cross = fa.cross; sa.m_smooth = sc.alloc<double>(nm_x); sa.S_smooth = sc.alloc<double>(nS_x);
            OP_CHECK(sa.m_smooth && sa.S_smooth, who);
        }
    }
    // the forecast: stacks, the origin table and the slab sums / states of one pass of tracks (after every request the filter makes)
    const int B = fc ? fc->n_origins : 0, h = fc ? fc->horizon : 0;
    const int upg = dq ? 1 : 0;
    int Bp = !fc ? 0 : linear ? mg_lfan_tracks_per_pass(G, nm, D, Mp, upg, B) : cub ? mg_crec_records_per_pass(G, nm, D, Mp, upg, B)
                                                                                    : mg_fan_tracks_per_pass(G, D, NS, B);
    if (fc && fc->tracks_per_pass > 0 && fc->tracks_per_pass < Bp) Bp = fc->tracks_per_pass;
    const size_t nm_fc = (size_t)G * B * h * D, nS_fc = nm_fc * D;
    double *dmfc = nullptr, *dSfc = nullptr, *fpart = nullptr, *fstate = nullptr;
    int *dorg = nullptr;
    MomentLinearFanArgs lf{};                                // (linearised and cubature tracks: K, the column-tile partials and the mean sums of a pass)
    double *coff = nullptr;                                  // (cubature: the offsets of a step)
    if (fc) {
        dmfc = sc.alloc<double>(nm_fc); dSfc = sc.alloc<double>(nS_fc); dorg = sc.alloc<int>(B);
        fstate = sc.alloc<double>((size_t)2 * G * Bp * (D + D * D));
        if (linear || cub) {
            lf = mg_lfan_layout(G, nm, D, Mp, upg, Bp * nrow);
            lf.K = sc.alloc<double>((size_t)lf.units * lf.Tp * Mp); lf.vpart = sc.alloc<double>((size_t)lf.units * lf.ntj * lf.Tp);
            lf.msum = sc.alloc<double>((size_t)2 * G * Bp * D * (cub ? nrow : D + 1));
            if (cub) coff = sc.alloc<double>((size_t)2 * G * Bp * D * D);
            OP_CHECK(lf.K && lf.vpart && lf.msum && (!cub || coff), who);
            OP_TRY(hipMemsetAsync(lf.K, 0, (size_t)lf.units * lf.Tp * Mp * sizeof(double), sc.stream));      // rows no pass fills stay zeros
        } else {
            fpart = sc.alloc<double>((size_t)2 * G * Bp * mg_fields(D) * NS);
            OP_CHECK(fpart, who);
        }
        OP_CHECK(dmfc && dSfc && dorg && fstate, who);
        OP_TRY(hipMemcpyAsync(dorg, fc->origins, (size_t)B * sizeof(int), hipMemcpyHostToDevice, sc.stream));
    }
    if (int rc = bg.launch(sc, G, nm, M, D, Mp, hv.len, dW, dq, q_mode, dU)) return rc;
    MomentGroupArgs a{};
    a.G = G; a.n_models = nm; a.D = D; a.C = C; a.P = P; a.M = M; a.Mp = Mp; a.NS = NS; a.steps = steps; a.unit_per_group = upg;
    a.Z = dZ; a.variance = hv.variance; a.len = hv.len; a.beta = bg.beta; a.gam = bg.gam; a.x_last = dxl; a.S0 = dS0; a.log_Q = dlq;
    a.ctrl = dctrl; a.part = part; a.state = state; a.m_x = dm; a.S_x = dS;
    if (!flt)
        for (int t = 0; t <= steps; ++t) launch_mg_step(sc.stream, a, t);
    else {
        if (linear)
            for (int t = 0; t <= steps; ++t) launch_mg_linear_step(sc.stream, a, fa, t);
        else if (cub) {
            // one record per group through the records launch, in the buffers of the tracks with the layout of one record per group
            // (Bp >= 1: never larger than theirs); the K rows it filled are zeros again before the first pass of tracks
            const MomentRecordArgs ra{1, 1, 0};
            MomentLinearFanArgs l1 = mg_lfan_layout(G, nm, D, Mp, upg, nrow);
            l1.K = lf.K; l1.vpart = lf.vpart; l1.msum = lf.msum;
            for (int t = 0; t <= steps; ++t) launch_mg_crec_step(sc.stream, a, fa, ra, l1, coff, t);
            OP_TRY(hipMemsetAsync(lf.K, 0, (size_t)l1.units * l1.Tp * Mp * sizeof(double), sc.stream));
        } else
            for (int t = 0; t <= steps; ++t) launch_mg_filter_step(sc.stream, a, fa, t);
        if (smooth) launch_mg_smooth(sc.stream, sa);
    }
    if (fc) {
        // passes of at most Bp origins, h + 1 launches each; a track's values do not depend on the pass it is in
        MomentGroupArgs ta = a;
        ta.steps = h; ta.x_last = nullptr; ta.S0 = nullptr; ta.part = fpart; ta.state = fstate; ta.m_x = dmfc; ta.S_x = dSfc;
        MomentFanArgs fn{};
        fn.B = B; fn.n = steps; fn.origin = dorg; fn.m_filt = fa.m_filt; fn.S_filt = fa.S_filt;
        for (int b0 = 0; b0 < B; b0 += Bp) {
            fn.b0 = b0; fn.Bp = B - b0 < Bp ? B - b0 : Bp;
            ta.G = G * fn.Bp;
            if (linear) {
                lf.nr = lf.shared ? G * fn.Bp : fn.Bp;
                for (int t = 0; t <= h; ++t) launch_mg_lfan_step(sc.stream, ta, fn, lf, t);
            } else if (cub) {
                lf.nr = (lf.shared ? G * fn.Bp : fn.Bp) * nrow;
                for (int t = 0; t <= h; ++t) launch_mg_cfan_step(sc.stream, ta, fn, lf, coff, t);
            } else
                for (int t = 0; t <= h; ++t) launch_mg_fan_step(sc.stream, ta, fn, t);
        }
    }
    OP_TRY(hipGetLastError());
    if (sum)
        if (int rc = mg_summary(sc, who, dm, dS, G, steps, D, *sum)) return rc;
    if (fc && (fc->y_mean || fc->y_var_total || fc->lpd_mix || fc->lpd_gauss)) {
        // the forecast stacks as [G][B * h][D] against the targets Y_fc[b * h + k] = Y_obs[origins[b] + 1 + k]
        const int J = flt->J;
        std::vector<double> &yfc = sc.host((size_t)B * h * J);
        for (int b = 0; b < B; ++b)
            memcpy(yfc.data() + (size_t)b * h * J, flt->Y_obs + (size_t)(fc->origins[b] + 1) * J, (size_t)h * J * sizeof(double));
        const SummaryReq fq{flt->CC, flt->DD, flt->noise_std, J, yfc.data(), B * h, fc->y_mean, nullptr, fc->y_var_total, fc->lpd_mix, fc->lpd_gauss};
        if (int rc = mg_summary(sc, who, dmfc, dSfc, G, B * h, D, fq)) return rc;
    }
    if (fc && ((fc->m_fc && !sc.download(fc->m_fc, dmfc, nm_fc * sizeof(double))) || (fc->S_fc && !sc.download(fc->S_fc, dSfc, nS_fc * sizeof(double)))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
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
const char *const mg_se_only = " (moment matching is closed-form for the SE kernel only)";
const char *const mg_linear_se_only = " (the linearised filter is built for the SE kernel only: its kernel row and Jacobian are SE-ARD's)";
const char *const mg_linear_fc_se_only =
    " (the linearised forecasts are built for the SE kernel only: their kernel rows and Jacobians are SE-ARD's)";
const char *const mg_cubature_fc_se_only = " (the cubature forecasts are built for the SE kernel only: their kernel rows are SE-ARD's)";
const char *const mg_particle_fc_se_only = " (the particle forecasts are built for the SE kernel only: their kernel rows are SE-ARD's)";
const char *mg_fc_se_only(int method) {
    return method == MG_METHOD_LINEAR ? mg_linear_fc_se_only : method == MG_METHOD_CUBATURE ? mg_cubature_fc_se_only
         : method == MG_METHOD_PARTICLE ? mg_particle_fc_se_only : mg_se_only;
}

// Posteriors given by the caller (also explicit-U models, SG-HMC samples of U: q_sqrts = NULL) through mg_run, scalars and pointers checked
int mg_given_run(const std::string &who, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D,
                 const double *logvariances, const double *loglengthscales, const double *fs, const double *const *q_sqrts, int q_mode,
                 const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps, const double *log_Qs, double *m_x,
                 double *S_x, const SummaryReq *sum, const FilterReq *flt, const ForecastReq *fc = nullptr, int method = MG_METHOD_MOMENT,
                 const ParticleFcReq *pf = nullptr) {
    const size_t nK = (size_t)n_models * D, GD = (size_t)G * D, nq = given_nq(q_sqrts, q_mode, G, D);
    if (!given_tables_ok(Lm_inverse_seqs, nK, q_sqrts, nq)) return set_error(nullptr, FFVD_EINVAL, who + ": bad argument");
    OP_BEGIN(who);
    const int Mp = round_up(M, NB);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp), *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    GroupHypers gh = stage_group_hypers(sc, FFVD_KERNEL_SE, n_models, D, M, Mp, P, Zs, logvariances, loglengthscales);
    double *dU = sc.upload(fs, GD * M), *dxl = sc.upload(x_lasts, GD), *dS0 = S0s ? sc.upload(S0s, GD * D) : nullptr, *dlq = sc.upload(log_Qs, GD);
    double *dctrl = C ? sc.upload(ctrl, (size_t)steps * C) : nullptr;
    OP_CHECK(dW && (!nq || dq) && dU && dxl && (!S0s || dS0) && dlq && (!C || dctrl) && gh.logs(sc) && gh.blocks(sc), who);
    gh.prep(sc.stream);
    return mg_run(sc, who, G, n_models, M, P, D, C, steps, gh.hv(), gh.dZ, dW, dq, q_mode, dU, dxl, dS0, dlq, dctrl, m_x, S_x, sum, flt, fc,
                  method, pf);
}

// The collapsed posteriors of ffvd_op_posterior_grouped (base_model.py:243-256) through mg_run without leaving the device: L^-T is
// packed from the K_uu slabs, U_mean read where the matvec left it, the q slices packed by launch_pg_pack (exact zeros in the padding
// and the strict lower triangle); the start means are x0s or, without them, the last rows of Xs.
int mg_posterior_run(const PgIn &in, int q_mode, const double *x0s, const double *S0s, const double *ctrl_roll, int steps, double *m_x,
                     double *S_x, double *U_means, const SummaryReq *sum, const FilterReq *flt, const ForecastReq *fc = nullptr,
                     int method = MG_METHOD_MOMENT, const ParticleFcReq *pf = nullptr) {
    const std::string &who = in.who;
    OP_BEGIN(who);
    PgWork w{};
    const int G = in.G, D = in.D, M = in.M, C = in.C, nm = in.n_models, Mp = round_up(M, NB), nK = nm * D;
    const size_t GD = (size_t)G * D, mm = (size_t)Mp * Mp;
    const bool have_q = pg_want_q(sc, w, q_mode, G, D, M);
    double *dW = sc.alloc<double>((size_t)nK * mm), *dxl = x0s ? sc.upload(x0s, GD) : sc.alloc<double>(GD);
    OP_CHECK(have_q && dW && dxl, who);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    double *dZ = sc.upload(in.Zs, (size_t)nm * M * in.P), *dS0 = S0s ? sc.upload(S0s, GD * D) : nullptr;
    double *dctrl = C ? sc.upload(ctrl_roll, (size_t)steps * C) : nullptr;
    OP_CHECK(dZ && (!S0s || dS0) && (!C || dctrl), who);
    launch_pg_pack(sc.stream, w.Kuu, 2 * mm, Mp, Mp, nK, 1, M, 1, dW, Mp, Mp, nK);
    if (!x0s) launch_pg_x_last(sc.stream, w.Xs, G, in.T, D, dxl);
    if (int rc = mg_run(sc, who, G, nm, M, in.P, D, C, steps, w.hv, dZ, dW, pg_q(w, q_mode), q_mode, w.U, dxl, dS0, w.log_Qs, dctrl, m_x, S_x,
                        sum, flt, fc, method, pf))
        return rc;
    if (U_means && !sc.download(U_means, w.U, GD * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    return FFVD_OK;
}
}  // namespace

extern "C" int ffvd_op_moment_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                      int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                      const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                      const double *ctrl, int C, int steps, const double *log_Qs, double *m_x, double *S_x,
                                      const double *CC, const double *DD, const double *noise_std, int J, const double *Y_test, int n_test,
                                      double *y_mean, double *y_var, double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string who = "ffvd_op_moment_grouped", bad = who + ": bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    const SummaryReq *sum = mg_summary_wanted(q) ? &q : nullptr;
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + mg_se_only);
    if (!mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) || (sum && !summary_scalars_ok(q, G, steps, D)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !x_lasts || !log_Qs || (C > 0 && !ctrl) ||
        (!sum && (!m_x || !S_x)) || (sum && !summary_arrays_ok(q)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    return mg_given_run(who, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl,
                        C, steps, log_Qs, m_x, S_x, sum, nullptr);
}

extern "C" int ffvd_op_posterior_moment_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                const double *logvariances, const double *loglengthscales, const double *Xs,
                                                const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                int groups_per_pass, int q_mode, const double *S0s, const double *ctrl_roll, int steps,
                                                double *m_x, double *S_x, double *U_means, const double *CC, const double *DD,
                                                const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean,
                                                double *y_var, double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string who = "ffvd_op_posterior_moment_grouped", bad = who + ": bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    const SummaryReq *sum = mg_summary_wanted(q) ? &q : nullptr;
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + mg_se_only);
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || !mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) ||
        (sum && !summary_scalars_ok(q, G, steps, D)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || (C > 0 && (!ctrl_fit || !ctrl_roll)) || (!sum && (!m_x || !S_x)) ||
        (sum && !summary_arrays_ok(q)))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    return mg_posterior_run(in, q_mode, nullptr, S0s, ctrl_roll, steps, m_x, S_x, U_means, sum, nullptr);
}

// ---- filtering and smoothing (moment_group.h) -------------------------------------------------------------------------------------
// ffvd_op_moment_grouped with a measurement update after every step (posteriors given by the caller); `method`: the propagation rule
namespace {
int filter_given(const std::string &who, int method, int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs,
                 int M, int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                 const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps,
                 const double *log_Qs, double *m_pred, double *S_pred, const FilterReq &f) {
    const std::string bad = who + ": bad argument";
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + (method == MG_METHOD_LINEAR ? mg_linear_se_only : mg_se_only));
    if (!mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) || !filter_scalars_ok(f)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !x_lasts || !log_Qs || (C > 0 && !ctrl) ||
        !filter_arrays_ok(f, steps, m_pred, S_pred))
        return set_error(nullptr, FFVD_EINVAL, bad);
    return mg_given_run(who, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl,
                        C, steps, log_Qs, m_pred, S_pred, nullptr, &f, nullptr, method);
}
}  // namespace

extern "C" int ffvd_op_filter_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                      int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                      const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                      const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                      const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                      double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                      double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss) {
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    return filter_given("ffvd_op_filter_grouped", MG_METHOD_MOMENT, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances,
                        loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, m_pred, S_pred, f);
}

// The same with the linearised (extended Kalman) rule in place of moment matching (moment_linear.hip)
extern "C" int ffvd_op_filter_linear_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                             int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                             const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                             const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                             const double *DD, const double *noise_std, int J, const double *Y_obs, double *m_pred,
                                             double *S_pred, double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                             double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                             double *lpd_gauss) {
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    return filter_given("ffvd_op_filter_linear_grouped", MG_METHOD_LINEAR, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances,
                        loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, m_pred, S_pred, f);
}

// The collapsed posteriors of ffvd_op_posterior_grouped filtered without leaving the device (as ffvd_op_posterior_moment_grouped);
// x0s NULL: the start means are the last rows of Xs
namespace {
int filter_posterior(const std::string &who, int method, int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                     const double *logvariances, const double *loglengthscales, const double *Xs, const double *ctrl_fit, int C, int T,
                     const double *log_Qs, double jitter, int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                     const double *ctrl_roll, int steps, double *m_pred, double *S_pred, double *U_means, const FilterReq &f) {
    const std::string bad = who + ": bad argument";
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + (method == MG_METHOD_LINEAR ? mg_linear_se_only : mg_se_only));
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || !mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) ||
        !filter_scalars_ok(f))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || (C > 0 && (!ctrl_fit || !ctrl_roll)) ||
        !filter_arrays_ok(f, steps, m_pred, S_pred))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    return mg_posterior_run(in, q_mode, x0s, S0s, ctrl_roll, steps, m_pred, S_pred, U_means, nullptr, &f, nullptr, method);
}
}  // namespace

extern "C" int ffvd_op_posterior_filter_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                const double *logvariances, const double *loglengthscales, const double *Xs,
                                                const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                double *lpd_gauss, double *U_means) {
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    return filter_posterior("ffvd_op_posterior_filter_grouped", MG_METHOD_MOMENT, kind, G, n_models, Zs, M, P, D, logvariances,
                            loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, m_pred,
                            S_pred, U_means, f);
}

// The same with the linearised (extended Kalman) rule in place of moment matching (moment_linear.hip)
extern "C" int ffvd_op_posterior_filter_linear_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                       const double *logvariances, const double *loglengthscales, const double *Xs,
                                                       const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                       int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                       const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                       const double *noise_std, int J, const double *Y_obs, double *m_pred,
                                                       double *S_pred, double *m_filt, double *S_filt, double *cross, double *lpd,
                                                       double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean,
                                                       double *y_var_total, double *lpd_mix, double *lpd_gauss, double *U_means) {
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    return filter_posterior("ffvd_op_posterior_filter_linear_grouped", MG_METHOD_LINEAR, kind, G, n_models, Zs, M, P, D, logvariances,
                            loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, m_pred,
                            S_pred, U_means, f);
}

// ---- linearised filtering of many records (moment_group.h, MomentRecordArgs) ---------------------------------------------------------
// ffvd_op_filter_linear_grouped over R observed records in one call: a track (group, record) is an independent linearised filter on
// the posterior of its group with the observations, control rows and start state of its record.  beta and Gamma are staged once per
// call; the tracks of a pass advance in one launch pair per step (moment_linear_records.hip, the product kernel of the linearised
// forecasts), so Gamma is read once per 128 tracks of a unit and not once per record.
namespace {
// The records request beside a FilterReq whose Y_obs is [R][steps][J], whose per-track outputs are [G][R][steps]... and whose pooled
// four are [R][steps][J]
struct RecordsReq {
    int R, records_per_pass;
};
// the checks of a records request that need no array: G * R * steps * D * D < 2^31, G * R * D within the state kernel's grid x
bool records_scalars_ok(const RecordsReq &q, int G, int steps, int D) {
    if (q.R < 0 || q.records_per_pass < 0) return false;
    if (G == 0 || q.R == 0 || steps == 0) return true;
    return (long long)G * q.R <= ((1LL << 31) - 1) / steps / D / D && (long long)G * q.R * D < (1LL << 31);
}
const char *const mg_records_se_only =
    " (the linearised filter of many records is built for the SE kernel only: its kernel rows and Jacobians are SE-ARD's)";
const char *const mg_crecords_se_only =
    " (the cubature filter of many records is built for the SE kernel only: its kernel rows are SE-ARD's)";
const char *const mg_precords_se_only =
    " (the particle filter of many records is built for the SE kernel only: its kernel rows are SE-ARD's)";
const char *const mg_arecords_se_only =
    " (the adapted particle filter of many records is built for the SE kernel only: its kernel rows are SE-ARD's)";
const char *const mg_erecords_se_only =
    " (the adaptive particle filter of many records is built for the SE kernel only: its kernel rows are SE-ARD's)";
// the three rules that take a ParticleReq: the bootstrap filter, the fully adapted one (moment_particle_adapted.hip) and the bootstrap
// filter with adaptive resampling (moment_particle_adaptive.hip)
bool mg_particle_rule(int method) { return method == MG_METHOD_PARTICLE || method == MG_METHOD_ADAPTED || method == MG_METHOD_ADAPTIVE; }
// The particle request beside a RecordsReq (MG_METHOD_PARTICLE): N particles per track, the caller's draws with their (group, record)
// strides in doubles -- each 0 or the stride of a contiguous array -- and the outputs the Gaussian rules do not have
struct ParticleReq {
    int N;
    const double *eps;                           // [G or 1][R or 1][steps][N][D]
    long long eps_g, eps_r;
    const double *unif;                          // [G or 1][R or 1][steps]
    long long unif_g, unif_r;
    const double *xi0;                           // [G or 1][R or 1][N][D]; needed exactly when S0s is given
    long long xi0_g, xi0_r;
    double *ess, *log_evidence;                  // [G][R][steps], [G][R]
    double *particles;                           // [G][R][steps][N][D] or NULL
    int *ancestors;                              // [G][R][steps][N] or NULL
    // seeded: eps, unif, xi0 (and unif_bs of a ParticleBacksimReq beside it) are NULL and the driver fills their device buffers from
    // `seed` through the same strides (moment_particle_draws.hip); there is nothing on the host to check or to upload
    bool seeded = false;
    unsigned long long seed = 0;
    // MG_METHOD_ADAPTIVE: the rows whose ess falls below ess_threshold * N resample (finite, >= 0); the two outputs it adds
    double ess_threshold = 0.0;
    double *weights = nullptr;                   // [G][R][steps][N] or NULL
    int *resampled = nullptr;                    // [G][R][steps] or NULL
};
// The backward-simulation request beside a ParticleSmoothReq (moment_particle_backsim.hip): B trajectories per track from the
// caller's uniforms; with it the smoother's recursion is not run (its m_smooth .. w_smooth stay NULL)
struct ParticleBacksimReq {
    int B;
    const double *unif_bs;                       // [G or 1][R or 1][steps][B]
    long long unif_g, unif_r;
    double *trajectories;                        // [G][R][B][steps][D]
    int *traj_index;                             // [G][R][steps][B]
    double *m_traj, *S_traj, *lag_cov;           // [G][R][steps][D], [..][D][D], [..][D][D]
    bool any_output() const { return trajectories || traj_index || m_traj || S_traj || lag_cov; }
};
// The smoothing request beside a ParticleReq (moment_particle_smooth.hip): the rows of every record and the outputs, each of which
// may be NULL
struct ParticleSmoothReq {
    const int *lengths;                          // [R], each in [1, steps], or NULL (every record has `steps` rows)
    double *m_smooth, *S_smooth, *ess_smooth;    // [G][R][steps][D], [..][D][D], [G][R][steps]
    double *w_smooth, *weights;                  // [G][R][steps][N]
    double *trans_mean, *trans_var;              // [G][R][steps][N][D]
    const ParticleBacksimReq *bs = nullptr;
    bool any_output() const {
        return m_smooth || S_smooth || ess_smooth || w_smooth || weights || trans_mean || trans_var || (bs && bs->any_output());
    }
};
bool particle_smooth_ok(const ParticleSmoothReq &q, int R, int steps) {
    if (q.lengths)
        for (int r = 0; r < R; ++r)
            if (q.lengths[r] < 1 || q.lengths[r] > steps) return false;
    return true;
}
// a pair of strides over arrays of `inner` doubles per (group, record): record 0 or inner, group 0 or inner * (R or 1)
bool particle_strides_ok(long long sg, long long sr, long long inner, int R) {
    return (sr == 0 || sr == inner) && (sg == 0 || sg == inner * (sr ? R : 1));
}
size_t particle_extent(long long sg, long long sr, long long inner, int G, int R) {
    return (size_t)inner * (sr ? R : 1) * (sg ? G : 1);
}
// the checks of a backward-simulation request that need no device: B, the strides, G * R * B within the grid, unif_bs in [0, 1)
bool particle_backsim_ok(const ParticleBacksimReq &q, int G, int R, int steps, bool nothing, bool seeded) {
    if (q.B < 1 || q.B > MG_PBS_MAXB) return false;
    const long long nu = (long long)steps * q.B;
    if (!particle_strides_ok(q.unif_g, q.unif_r, nu, R)) return false;
    if (nothing) return true;
    if ((long long)G * R > ((1LL << 31) - 1) / q.B) return false;
    if (seeded)                                                                        // (the fill launch: a block below 2^31 doubles, its grid x)
        return nu < (1LL << 31) && (((nu + 1) / 2 + 255) / 256) * G * R < (1LL << 31);
    if (!q.unif_bs) return false;
    const size_t n_u = particle_extent(q.unif_g, q.unif_r, nu, G, R);
    for (size_t e = 0; e < n_u; ++e)
        if (!(q.unif_bs[e] >= 0.0 && q.unif_bs[e] < 1.0)) return false;
    return true;
}
// the checks of a particle request that need no device: N, the strides, the arrays (finite draws, unif in [0, 1))
bool particle_ok(const ParticleReq &q, int G, int R, int steps, int D, bool with_S0, bool nothing) {
    if (q.N < MG_PREC_MINN || q.N > MG_PREC_MAXN) return false;
    const long long ne = (long long)steps * q.N * D, nx = (long long)q.N * D;
    if (!particle_strides_ok(q.eps_g, q.eps_r, ne, R) || !particle_strides_ok(q.unif_g, q.unif_r, steps, R) ||
        !particle_strides_ok(q.xi0_g, q.xi0_r, nx, R))
        return false;
    if (nothing) return true;
    if ((long long)G * R > ((1LL << 31) - 1) / steps / q.N / D) return false;          // G * R * steps * N * D < 2^31
    if (q.seeded) return true;                                                         // (generated values: finite, unif in [0, 1))
    if (!q.eps || !q.unif || (with_S0 && !q.xi0)) return false;
    const size_t n_eps = particle_extent(q.eps_g, q.eps_r, ne, G, R), n_u = particle_extent(q.unif_g, q.unif_r, steps, G, R);
    for (size_t e = 0; e < n_eps; ++e)
        if (!std::isfinite(q.eps[e])) return false;
    for (size_t e = 0; e < n_u; ++e)
        if (!(q.unif[e] >= 0.0 && q.unif[e] < 1.0)) return false;
    if (with_S0) {
        const size_t n_x = particle_extent(q.xi0_g, q.xi0_r, nx, G, R);
        for (size_t e = 0; e < n_x; ++e)
            if (!std::isfinite(q.xi0[e])) return false;
    }
    return true;
}

// out[e] = log mean_g exp(lpd[g][e]), e < n, on the host: the mixture of all G * N particles' emissions, in ascending g, the largest
// exponent subtracted; NaN where the entry is unobserved (lpd [G][n], NaN in every group alike)
void lpd_mix_over_groups(const double *lpd, int G, size_t n, double *out) {
    for (size_t e = 0; e < n; ++e) {
        double mx = -INFINITY, sum = 0.0;
        for (int g = 0; g < G; ++g) mx = std::fmax(mx, lpd[(size_t)g * n + e]);
        for (int g = 0; g < G; ++g) sum += std::exp(lpd[(size_t)g * n + e] - mx);
        out[e] = std::isnan(lpd[e]) ? NAN : mx + std::log(sum / G);
    }
}

// The tail of a particle call: the pooled summary of the predicted stacks on the device (y_mean, y_var_total, lpd_gauss), the downloads
// (ea: the adaptive rule's stacks, whose `weights` and `resampled` come down with them),
// and on the host, from the stacks that came down: lpd_mix (lpd_mix_over_groups) and log_evidence = the sum of lpd_joint over the
// rows that have an observation, in ascending order
int mg_particle_finish(Scratch &sc, const std::string &who, int G, int R, int steps, int D, const double *dm, const double *dS, double *m_x,
                       double *S_x, const MomentFilterArgs &fa, const MomentParticleArgs &pa, const FilterReq &flt, const ParticleReq &pq,
                       const MomentParticleEssArgs *ea = nullptr) {
    const int J = flt.J;
    const size_t V = (size_t)G * R, nm_x = V * steps * D, nS_x = nm_x * D, nlpd = V * steps * J, nlj = V * steps, RS = (size_t)R * steps;
    SummaryReq fsum = flt.pooled(R * steps);
    fsum.lpd = nullptr;
    if (fsum.y_mean || fsum.y_var_total || fsum.lpd_gauss)
        if (int rc = mg_summary(sc, who, dm, dS, G, R * steps, D, fsum)) return rc;
    std::vector<double> hl, hj;                                                        // (host copies where the caller asks for a derived array only)
    double *lpd = flt.lpd, *lj = flt.lpd_joint;
    if (!lpd && flt.lpd_mix) { hl.resize(nlpd); lpd = hl.data(); }
    if (!lj && pq.log_evidence) { hj.resize(nlj); lj = hj.data(); }
    auto down = [&](void *dst, const void *src, size_t bytes) { return !dst || sc.download(dst, src, bytes); };
    if (!down(flt.m_filt, fa.m_filt, nm_x * sizeof(double)) || !down(flt.S_filt, fa.S_filt, nS_x * sizeof(double)) ||
        !down(lpd, fa.lpd, nlpd * sizeof(double)) || !down(lj, fa.lpd_joint, nlj * sizeof(double)) || !down(m_x, dm, nm_x * sizeof(double)) ||
        !down(S_x, dS, nS_x * sizeof(double)) || !down(pq.ess, pa.ess, nlj * sizeof(double)) ||
        !down(pq.particles, pa.particles, nm_x * pq.N * sizeof(double)) || !down(pq.ancestors, pa.ancestors, nlj * pq.N * sizeof(int)) ||
        (ea && (!down(pq.weights, ea->weights, nlj * pq.N * sizeof(double)) || !down(pq.resampled, ea->resampled, nlj * sizeof(int)))))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    OP_TRY(hipStreamSynchronize(sc.stream));
    if (flt.lpd_mix) lpd_mix_over_groups(lpd, G, RS * J, flt.lpd_mix);
    if (pq.log_evidence)
        for (size_t v = 0; v < V; ++v) {
            double sum = 0.0;
            for (int i = 0; i < steps; ++i)
                if (!std::isnan(lj[v * steps + i])) sum += lj[v * steps + i];
            pq.log_evidence[v] = sum;
        }
    return FFVD_OK;
}

// a call whose single track per group does not fit K is refused with the largest N that fits
int particle_fits(const std::string &who, int G, int nm, int D, int Mp, int upg, int N) {
    const long long fit = mg_prec_max_particles(G, nm, D, Mp, upg);
    if (N <= fit) return FFVD_OK;
    return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (the kernel rows of one record per group do not fit the scratch of a pass: "
                     "the largest N that fits is " + std::to_string(fit / 128 * 128 > MG_PREC_MAXN ? MG_PREC_MAXN : fit) + ")");
}

// Operands on the device -> beta, Gamma (BetaGamma, once per call), the passes over the records (steps + 1 launch pairs each), the
// smoother over all G * R tracks, the pooled summary per record and row, the downloads.  A sibling of mg_run's linear branch.
// dxl: [G][R][D]; dS0: nullptr or [G][R][D][D]; dctrl: nullptr or [R][steps][C]; the other operands as mg_run's.
// method: MG_METHOD_LINEAR (moment_linear_records.hip) or MG_METHOD_CUBATURE (moment_cubature_records.hip: 2D rows of K per track,
// 2D mean sums per (track, dim) and the offsets of a step beside the state; everything else is shared).
int mg_records_run(Scratch &sc, const std::string &who, int method, int G, int nm, int M, int P, int D, int C, int steps, const HyperView &hv,
                   const double *dZ, const double *dW, const double *dq, int q_mode, const double *dU, const double *dxl, const double *dS0,
                   const double *dlq, const double *dctrl, double *m_x, double *S_x, const FilterReq &flt, const RecordsReq &rq,
                   const ParticleReq *pq = nullptr, const ParticleSmoothReq *sq = nullptr) {
    const int Mp = round_up(M, NB), R = rq.R, J = flt.J, upg = dq ? 1 : 0;
    const int V = G * R;                                                               // tracks of the call (V * steps * D * D < 2^31)
    const size_t nm_x = (size_t)V * steps * D, nS_x = nm_x * D, nlpd = (size_t)V * steps * J, nlj = (size_t)V * steps;
    const bool cub = method == MG_METHOD_CUBATURE, par = mg_particle_rule(method), ada = method == MG_METHOD_ADAPTED;
    const bool esr = method == MG_METHOD_ADAPTIVE;
    if (esr && sq)                                                                     // (the smoothers assume equally weighted carried sets)
        return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (smoothing and backward simulation are not built on the adaptive rule's weighted sets)");
    const int nrow = cub ? mg_crec_rows(D) : par ? pq->N : 1;                          // rows of K per track
    if (par)
        if (int rc = particle_fits(who, G, nm, D, Mp, upg, pq->N)) return rc;
    int Rp = cub ? mg_crec_records_per_pass(G, nm, D, Mp, upg, R) : par ? mg_prec_records_per_pass(G, nm, D, Mp, upg, R, pq->N)
                                                                        : mg_lfan_tracks_per_pass(G, nm, D, Mp, upg, R);
    if (rq.records_per_pass > 0 && rq.records_per_pass < Rp) Rp = rq.records_per_pass;
    BetaGamma bg{};
    const bool terms = bg.alloc(sc, G, nm, D, Mp, dq, q_mode);
    double *state = sc.alloc<double>((size_t)2 * G * Rp * (D + D * D));
    double *dm = sc.alloc<double>(nm_x), *dS = sc.alloc<double>(nS_x);
    OP_CHECK(terms && state && dm && dS, who);
    const Emission e = stage_emission(sc, D, J, flt.CC, flt.DD, flt.noise_std, flt.Y_obs, (size_t)R * steps);
    MomentFilterArgs fa{};
    fa.J = J; fa.CC = e.CC; fa.DD = e.DD; fa.sd = e.sd; fa.Y = e.Y;
    fa.m_filt = sc.alloc<double>(nm_x); fa.S_filt = sc.alloc<double>(nS_x); fa.cross = par ? nullptr : sc.alloc<double>(nS_x);
    fa.lpd = sc.alloc<double>(nlpd); fa.lpd_joint = sc.alloc<double>(nlj);
    OP_CHECK(e.ok && fa.m_filt && fa.S_filt && (par || fa.cross) && fa.lpd && fa.lpd_joint, who);
    MomentSmoothArgs sa{};
    const bool smooth = flt.m_smooth || flt.S_smooth;
    if (smooth) {                                                                      // the stacks are [G][R][steps]...: its [G'][steps]...
        sa.G = V; sa.D = D; sa.steps = steps; sa.m_pred = dm; sa.S_pred = dS; sa.m_filt = fa.m_filt; sa.S_filt = fa.S_filt;
        sa.cross = fa.cross; sa.m_smooth = sc.alloc<double>(nm_x); sa.S_smooth = sc.alloc<double>(nS_x);
        OP_CHECK(sa.m_smooth && sa.S_smooth, who);
    }
    MomentLinearFanArgs lf = mg_lfan_layout(G, nm, D, Mp, upg, Rp * nrow);
    lf.K = sc.alloc<double>((size_t)lf.units * lf.Tp * Mp); lf.vpart = sc.alloc<double>((size_t)lf.units * lf.ntj * lf.Tp);
    lf.msum = par ? nullptr : sc.alloc<double>((size_t)2 * G * Rp * D * (cub ? nrow : D + 1));
    double *coff = cub ? sc.alloc<double>((size_t)2 * G * Rp * D * D) : nullptr;
    OP_CHECK(lf.K && lf.vpart && (par || lf.msum) && (!cub || coff), who);
    MomentParticleArgs pa{};
    // the draws of one stream on the device: the caller's, uploaded, or (seeded) a buffer of the same extent that one fill launch
    // writes through the same strides, every double of it
    bool fill_refused = false;
    auto draws = [&](const double *src, int stream_id, bool normal, long long len, long long sg, long long sr) -> const double * {
        const size_t n = particle_extent(sg, sr, len, G, R);
        if (!pq->seeded) return sc.upload(src, n);
        double *d = sc.alloc<double>(n);
        const MomentParticleDrawsArgs da{(unsigned)(pq->seed & 0xFFFFFFFFull), (unsigned)(pq->seed >> 32), stream_id, normal ? 1 : 0,
                                         sg ? G : 1, sr ? R : 1, (int)len, sg, sr, d};
        if (d && !launch_mg_pdraw_fill(sc.stream, da)) fill_refused = true;               // (its grid does not fit: not an allocation failure)
        return d;
    };
    const auto fill_error = [&] {
        return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (the fill launch of the seeded draws needs ceil(block / 512) * blocks < 2^31)");
    };
    if (par) {                                                                         // the draws, staged once; the particles of a pass
        const ParticleReq &q = *pq;
        const long long ne = (long long)steps * q.N * D, nx = (long long)q.N * D;
        pa.N = q.N; pa.eps_g = q.eps_g; pa.eps_r = q.eps_r; pa.unif_g = q.unif_g; pa.unif_r = q.unif_r; pa.xi0_g = q.xi0_g; pa.xi0_r = q.xi0_r;
        pa.eps = draws(q.eps, MG_PDRAW_EPS, true, ne, q.eps_g, q.eps_r);
        pa.unif = draws(q.unif, MG_PDRAW_UNIF, false, steps, q.unif_g, q.unif_r);
        pa.xi0 = dS0 ? draws(q.xi0, MG_PDRAW_XI0, true, nx, q.xi0_g, q.xi0_r) : nullptr;
        pa.xstate = sc.alloc<double>((size_t)2 * G * Rp * q.N * D);
        pa.pmean = sc.alloc<double>((size_t)G * Rp * D * q.N);
        pa.ess = sc.alloc<double>(nlj);
        pa.particles = q.particles || sq ? sc.alloc<double>(nm_x * q.N) : nullptr;
        pa.ancestors = q.ancestors || sq ? sc.alloc<int>(nlj * q.N) : nullptr;
        if (fill_refused) return fill_error();
        OP_CHECK(pa.eps && pa.unif && (!dS0 || pa.xi0) && pa.xstate && pa.pmean && pa.ess && (!(q.particles || sq) || pa.particles) &&
                 (!(q.ancestors || sq) || pa.ancestors), who);
        if (q.seeded) OP_TRY(hipGetLastError());
    }
    MomentParticleAdaptedArgs pd{};
    if (ada) {                                                                         // (mu, s) of the parents of the row in flight
        pd.mu = sc.alloc<double>((size_t)G * Rp * pq->N * D); pd.sv = sc.alloc<double>((size_t)G * Rp * pq->N * D);
        OP_CHECK(pd.mu && pd.sv, who);
    }
    MomentParticleEssArgs pe{};
    if (esr) {                                                                         // the carried log-weights of a pass; the two stacks
        pe.ess_threshold = pq->ess_threshold;
        pe.logw = sc.alloc<double>((size_t)G * Rp * pq->N);
        pe.weights = pq->weights ? sc.alloc<double>(nlj * pq->N) : nullptr;
        pe.resampled = sc.alloc<int>(nlj);
        OP_CHECK(pe.logw && (!pq->weights || pe.weights) && pe.resampled, who);
    }
    MomentParticleSmoothArgs ps{};
    MomentParticleBacksimArgs pb{};
    const ParticleBacksimReq *bq = par && sq ? sq->bs : nullptr;
    int n_max = steps;
    if (par && sq) {                                                                   // the smoother's stacks: (3 D + 3) N doubles per track row
        int *lens = nullptr;
        if (sq->lengths) {
            lens = sc.alloc<int>(R);
            OP_CHECK(lens, who);
            OP_TRY(hipMemcpyAsync(lens, sq->lengths, (size_t)R * sizeof(int), hipMemcpyHostToDevice, sc.stream));
            n_max = 1;
            for (int r = 0; r < R; ++r) n_max = sq->lengths[r] > n_max ? sq->lengths[r] : n_max;
        }
        ps.V = V; ps.R = R; ps.steps = steps; ps.N = pq->N; ps.D = D; ps.lens = lens; ps.particles = pa.particles; ps.ancestors = pa.ancestors;
        ps.trans_mean = sc.alloc<double>(nm_x * pq->N); ps.trans_var = sc.alloc<double>(nm_x * pq->N);
        // (the adapted rule: the filtered sets are equally weighted and particle i of a row is carried particle i of the next, so
        // there is no `weights` stack and no omega; its backward simulation does not form w_smooth either)
        ps.weights = ada ? nullptr : sc.alloc<double>(nlj * pq->N); ps.w_smooth = ada && bq ? nullptr : sc.alloc<double>(nlj * pq->N);
        OP_CHECK(ps.trans_mean && ps.trans_var && (ada || ps.weights) && ((ada && bq) || ps.w_smooth), who);
        if (!bq) {
            ps.cnorm = sc.alloc<double>(nlj * pq->N); ps.omega = ada ? nullptr : sc.alloc<double>((size_t)V * pq->N);
            ps.m_smooth = sc.alloc<double>(nm_x); ps.S_smooth = sc.alloc<double>(nS_x); ps.ess_smooth = sc.alloc<double>(nlj);
            OP_CHECK(ps.cnorm && (ada || ps.omega) && ps.m_smooth && ps.S_smooth && ps.ess_smooth, who);
        } else {                                                                       // the trajectories: B * D doubles and B ints per track row
            const long long nu = (long long)steps * bq->B;
            pb.V = V; pb.R = R; pb.steps = steps; pb.N = pq->N; pb.D = D; pb.B = bq->B; pb.lens = lens; pb.particles = pa.particles;
            pb.ancestors = pa.ancestors; pb.trans_mean = ps.trans_mean; pb.trans_var = ps.trans_var; pb.weights = ps.weights;
            pb.unif_g = bq->unif_g; pb.unif_r = bq->unif_r;
            pb.unif = draws(bq->unif_bs, MG_PDRAW_UNIF_BS, false, nu, bq->unif_g, bq->unif_r);
            pb.inv_var = sc.alloc<double>(nm_x * pq->N); pb.log_var = sc.alloc<double>(nlj * pq->N);
            pb.traj_index = sc.alloc<int>(nlj * bq->B); pb.trajectories = sc.alloc<double>(nm_x * bq->B);
            pb.m_traj = sc.alloc<double>(nm_x); pb.S_traj = sc.alloc<double>(nS_x); pb.lag_cov = sc.alloc<double>(nS_x);
            if (fill_refused) return fill_error();
            OP_CHECK(pb.unif && pb.inv_var && pb.log_var && pb.traj_index && pb.trajectories && pb.m_traj && pb.S_traj && pb.lag_cov, who);
            if (pq->seeded) OP_TRY(hipGetLastError());
        }
    }
    OP_TRY(hipMemsetAsync(lf.K, 0, (size_t)lf.units * lf.Tp * Mp * sizeof(double), sc.stream));          // rows no pass fills stay zeros
    if (int rc = bg.launch(sc, G, nm, M, D, Mp, hv.len, dW, dq, q_mode, dU)) return rc;
    MomentGroupArgs a{};
    a.n_models = nm; a.D = D; a.C = C; a.P = P; a.M = M; a.Mp = Mp; a.NS = 0; a.steps = steps; a.unit_per_group = upg;
    a.Z = dZ; a.variance = hv.variance; a.len = hv.len; a.beta = bg.beta; a.gam = bg.gam; a.x_last = dxl; a.S0 = dS0; a.log_Q = dlq;
    a.ctrl = dctrl; a.part = nullptr; a.state = state; a.m_x = dm; a.S_x = dS;
    // passes of at most Rp records, steps + 1 launch pairs each; a track's values do not depend on the pass it is in
    MomentRecordArgs ra{};
    ra.R = R;
    for (int r0 = 0; r0 < R; r0 += Rp) {
        ra.r0 = r0; ra.Rp = R - r0 < Rp ? R - r0 : Rp;
        a.G = G * ra.Rp;
        lf.nr = (lf.shared ? G * ra.Rp : ra.Rp) * nrow;
        for (int t = 0; t <= steps; ++t) {
            if (cub) launch_mg_crec_step(sc.stream, a, fa, ra, lf, coff, t);
            else if (ada) {
                launch_mg_parec_step(sc.stream, a, fa, ra, lf, pa, pd, t);
                if (sq && t < steps) launch_mg_psm_keep(sc.stream, a, ra, lf, pa, ps, t);   // the same launch: (mu, s) of the set carried into row t
            } else if (esr) launch_mg_pess_step(sc.stream, a, fa, ra, lf, pa, pe, t);
            else if (par) {
                launch_mg_prec_step(sc.stream, a, fa, ra, lf, pa, t);
                if (sq && t < steps) launch_mg_psm_keep(sc.stream, a, ra, lf, pa, ps, t);   // (mu, s) of step t, before the next weight launch
            } else launch_mg_lrec_step(sc.stream, a, fa, ra, lf, t);
        }
    }
    if (smooth) launch_mg_smooth(sc.stream, sa);
    if (bq && ada) launch_mg_pabs(sc.stream, pb);
    else if (bq) {
        launch_mg_psm_weights(sc.stream, fa, ps);
        launch_mg_pbs(sc.stream, pb);
    } else if (ada && sq) launch_mg_pasm_smooth(sc.stream, ps, n_max);
    else if (par && sq) launch_mg_psm_smooth(sc.stream, fa, ps, n_max);
    OP_TRY(hipGetLastError());
    if (bq) {
        const size_t Bn = (size_t)bq->B;
        auto down = [&](void *dst, const void *src, size_t bytes) { return !dst || sc.download(dst, src, bytes); };
        if (!down(bq->trajectories, pb.trajectories, nm_x * Bn * sizeof(double)) || !down(bq->traj_index, pb.traj_index, nlj * Bn * sizeof(int)) ||
            !down(bq->m_traj, pb.m_traj, nm_x * sizeof(double)) || !down(bq->S_traj, pb.S_traj, nS_x * sizeof(double)) ||
            !down(bq->lag_cov, pb.lag_cov, nS_x * sizeof(double)))
            return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    }
    if (par && sq) {
        const size_t N = (size_t)pq->N;
        auto down = [&](double *dst, const double *src, size_t n) { return !dst || sc.download(dst, src, n * sizeof(double)); };
        if (!down(sq->m_smooth, ps.m_smooth, nm_x) || !down(sq->S_smooth, ps.S_smooth, nS_x) || !down(sq->ess_smooth, ps.ess_smooth, nlj) ||
            !down(sq->w_smooth, ps.w_smooth, nlj * N) || !down(sq->weights, ps.weights, nlj * N) ||
            !down(sq->trans_mean, ps.trans_mean, nm_x * N) || !down(sq->trans_var, ps.trans_var, nm_x * N))
            return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    }
    if (par) return mg_particle_finish(sc, who, G, R, steps, D, dm, dS, m_x, S_x, fa, pa, flt, *pq, esr ? &pe : nullptr);
    // the pooled one-step summary per record and row: the predicted stacks as [G][R * steps] against Y as [R * steps][J]
    const SummaryReq fsum = flt.pooled(R * steps);
    if (fsum.y_mean || fsum.y_var_total || fsum.lpd || fsum.lpd_gauss)
        if (int rc = mg_summary(sc, who, dm, dS, G, R * steps, D, fsum)) return rc;
    auto down = [&](double *dst, const double *src, size_t n) { return !dst || sc.download(dst, src, n * sizeof(double)); };
    if (!down(flt.m_filt, fa.m_filt, nm_x) || !down(flt.S_filt, fa.S_filt, nS_x) || !down(flt.cross, fa.cross, nS_x) ||
        !down(flt.lpd, fa.lpd, nlpd) || !down(flt.lpd_joint, fa.lpd_joint, nlj) || !down(flt.m_smooth, sa.m_smooth, nm_x) ||
        !down(flt.S_smooth, sa.S_smooth, nS_x) || !down(m_x, dm, nm_x) || !down(S_x, dS, nS_x))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}

// The particle request beside a ForecastReq (mg_run, MG_METHOD_PARTICLE): the filter's request with one record (its record strides
// are 0), the forecast draws with their (group, origin) strides in doubles -- each 0 or the stride of a contiguous array -- and the
// outputs the Gaussian fans do not have
struct ParticleFcReq {
    ParticleReq filter;
    const double *eps_fc;                        // [G or 1][B or 1][h][N][D]
    long long eps_fc_g, eps_fc_b;
    double *fc_lpd;                              // [G][B][h][J] or NULL
    double *fc_particles;                        // [G][B][h][N][D] or NULL
    // the adapted rule (moment_particle_adapted.hip over the record, moment_particle_adapted_fan.hip for the tracks): the same
    // request, the same checks
    bool adapted = false;
    bool any_output() const { return filter.ess || filter.log_evidence || fc_lpd || fc_particles; }
};
// the checks of a particle forecast request that need no device: the filter's with R = 1, the strides and values of eps_fc,
// G * B * h * N * D < 2^31
bool particle_fc_ok(const ParticleFcReq &q, int G, int B, int h, int steps, int D, bool with_S0) {
    if (q.filter.eps_r || q.filter.unif_r || q.filter.xi0_r || q.filter.particles || q.filter.ancestors) return false;
    if (q.filter.N < MG_PREC_MINN || q.filter.N > MG_PREC_MAXN) return false;
    const long long ne = (long long)h * q.filter.N * D;
    if (!particle_strides_ok(q.eps_fc_g, q.eps_fc_b, ne, B) || !q.eps_fc) return false;
    if ((long long)G * B > ((1LL << 31) - 1) / h / q.filter.N / D) return false;          // (before any array is read)
    if (!particle_ok(q.filter, G, 1, steps, D, with_S0, false)) return false;
    const size_t n = particle_extent(q.eps_fc_g, q.eps_fc_b, ne, G, B);
    for (size_t e = 0; e < n; ++e)
        if (!std::isfinite(q.eps_fc[e])) return false;
    return true;
}

// mg_run with MG_METHOD_PARTICLE: the particle filter over the one record (the records launch with R = 1, in the buffers of the
// tracks; its device `particles` and `ancestors` stacks are always kept: the tracks start from them), then the passes over the origins
// (moment_particle_fan.hip: h + 1 launch triples each), the pooled summary of the forecast stacks on the device, the downloads, and on
// the host fc_lpd_mix = log mean_g exp(fc_lpd[g]) in ascending g, as mg_particle_finish forms the filter's.
// pf.adapted: the adapted filter over the record (launch_mg_parec_step, with the (mu, s) buffers of one record per group) and the
// adapted tracks (moment_particle_adapted_fan.hip), which start from its `particles` stack alone; everything else is shared.
int mg_particle_fc_run(Scratch &sc, const std::string &who, int G, int nm, int M, int P, int D, int C, int steps, const HyperView &hv,
                       const double *dZ, const double *dW, const double *dq, int q_mode, const double *dU, const double *dxl, const double *dS0,
                       const double *dlq, const double *dctrl, double *m_x, double *S_x, const FilterReq &flt, const ForecastReq &fc,
                       const ParticleFcReq &pf) {
    const int Mp = round_up(M, NB), J = flt.J, upg = dq ? 1 : 0, N = pf.filter.N, B = fc.n_origins, h = fc.horizon;
    const size_t nm_x = (size_t)G * steps * D, nS_x = nm_x * D, nlpd = (size_t)G * steps * J, nlj = (size_t)G * steps;
    const size_t nm_fc = (size_t)G * B * h * D, nS_fc = nm_fc * D, nl_fc = (size_t)G * B * h * J, BH = (size_t)B * h;
    if (int rc = particle_fits(who, G, nm, D, Mp, upg, N)) return rc;
    int Bp = mg_prec_records_per_pass(G, nm, D, Mp, upg, B, N);
    if (fc.tracks_per_pass > 0 && fc.tracks_per_pass < Bp) Bp = fc.tracks_per_pass;
    BetaGamma bg{};
    const bool terms = bg.alloc(sc, G, nm, D, Mp, dq, q_mode);
    double *dm = sc.alloc<double>(nm_x), *dS = sc.alloc<double>(nS_x);
    OP_CHECK(terms && dm && dS, who);
    const Emission e = stage_emission(sc, D, J, flt.CC, flt.DD, flt.noise_std, flt.Y_obs, steps);
    MomentFilterArgs fa{};
    fa.J = J; fa.CC = e.CC; fa.DD = e.DD; fa.sd = e.sd; fa.Y = e.Y;
    fa.m_filt = sc.alloc<double>(nm_x); fa.S_filt = sc.alloc<double>(nS_x); fa.lpd = sc.alloc<double>(nlpd); fa.lpd_joint = sc.alloc<double>(nlj);
    OP_CHECK(e.ok && fa.m_filt && fa.S_filt && fa.lpd && fa.lpd_joint, who);
    double *dmfc = sc.alloc<double>(nm_fc), *dSfc = sc.alloc<double>(nS_fc);
    int *dorg = sc.alloc<int>(B);
    MomentLinearFanArgs lf = mg_lfan_layout(G, nm, D, Mp, upg, Bp * N);
    lf.K = sc.alloc<double>((size_t)lf.units * lf.Tp * Mp); lf.vpart = sc.alloc<double>((size_t)lf.units * lf.ntj * lf.Tp);
    OP_CHECK(dmfc && dSfc && dorg && lf.K && lf.vpart, who);
    // the draws, uploaded once; the particles of a pass (the filter's one track per group lives in the same buffers)
    const ParticleReq &q = pf.filter;
    const long long ne = (long long)steps * N * D, nx = (long long)N * D, nf = (long long)h * N * D;
    MomentParticleArgs pa{};
    pa.N = N; pa.eps_g = q.eps_g; pa.unif_g = q.unif_g; pa.xi0_g = q.xi0_g;
    pa.eps = sc.upload(q.eps, particle_extent(q.eps_g, 0, ne, G, 1));
    pa.unif = sc.upload(q.unif, particle_extent(q.unif_g, 0, steps, G, 1));
    pa.xi0 = dS0 ? sc.upload(q.xi0, particle_extent(q.xi0_g, 0, nx, G, 1)) : nullptr;
    pa.xstate = sc.alloc<double>((size_t)2 * G * Bp * N * D);
    pa.pmean = sc.alloc<double>((size_t)G * Bp * D * N);
    pa.ess = sc.alloc<double>(nlj);
    pa.particles = sc.alloc<double>(nm_x * N);
    pa.ancestors = sc.alloc<int>(nlj * N);
    MomentParticleFanArgs ta{};
    ta.N = N; ta.eps_g = pf.eps_fc_g; ta.eps_b = pf.eps_fc_b;
    ta.eps_fc = sc.upload(pf.eps_fc, particle_extent(pf.eps_fc_g, pf.eps_fc_b, nf, G, B));
    ta.particles = pa.particles; ta.ancestors = pa.ancestors; ta.xstate = pa.xstate; ta.pmean = pa.pmean;
    ta.lpd_fc = sc.alloc<double>(nl_fc);
    ta.fc_particles = pf.fc_particles ? sc.alloc<double>(nm_fc * N) : nullptr;
    OP_CHECK(pa.eps && pa.unif && (!dS0 || pa.xi0) && pa.xstate && pa.pmean && pa.ess && pa.particles && pa.ancestors && ta.eps_fc &&
             ta.lpd_fc && (!pf.fc_particles || ta.fc_particles), who);
    MomentParticleAdaptedArgs pd{};
    if (pf.adapted) {                                                                  // (mu, s) of the parents of the filter's row in flight
        pd.mu = sc.alloc<double>((size_t)G * N * D); pd.sv = sc.alloc<double>((size_t)G * N * D);
        OP_CHECK(pd.mu && pd.sv, who);
    }
    OP_TRY(hipMemsetAsync(lf.K, 0, (size_t)lf.units * lf.Tp * Mp * sizeof(double), sc.stream));          // rows no pass fills stay zeros
    OP_TRY(hipMemcpyAsync(dorg, fc.origins, (size_t)B * sizeof(int), hipMemcpyHostToDevice, sc.stream));
    if (int rc = bg.launch(sc, G, nm, M, D, Mp, hv.len, dW, dq, q_mode, dU)) return rc;
    MomentGroupArgs a{};
    a.G = G; a.n_models = nm; a.D = D; a.C = C; a.P = P; a.M = M; a.Mp = Mp; a.NS = 0; a.steps = steps; a.unit_per_group = upg;
    a.Z = dZ; a.variance = hv.variance; a.len = hv.len; a.beta = bg.beta; a.gam = bg.gam; a.x_last = dxl; a.S0 = dS0; a.log_Q = dlq;
    a.ctrl = dctrl; a.part = nullptr; a.state = nullptr; a.m_x = dm; a.S_x = dS;
    {
        // one record per group through the records launch, in the buffers of the tracks with the layout of one record per group
        // (Bp >= 1: never larger than theirs); the K rows it filled are zeros again before the first pass of tracks
        const MomentRecordArgs ra{1, 1, 0};
        MomentLinearFanArgs l1 = mg_lfan_layout(G, nm, D, Mp, upg, N);
        l1.K = lf.K; l1.vpart = lf.vpart;
        for (int t = 0; t <= steps; ++t) {
            if (pf.adapted) launch_mg_parec_step(sc.stream, a, fa, ra, l1, pa, pd, t);
            else launch_mg_prec_step(sc.stream, a, fa, ra, l1, pa, t);
        }
        OP_TRY(hipMemsetAsync(lf.K, 0, (size_t)l1.units * l1.Tp * Mp * sizeof(double), sc.stream));
    }
    // passes of at most Bp origins, h + 1 launch triples each; a track's values do not depend on the pass it is in
    MomentGroupArgs tg = a;
    tg.steps = h; tg.x_last = nullptr; tg.S0 = nullptr; tg.m_x = dmfc; tg.S_x = dSfc;
    MomentFanArgs fn{};
    fn.B = B; fn.n = steps; fn.origin = dorg;
    for (int b0 = 0; b0 < B; b0 += Bp) {
        fn.b0 = b0; fn.Bp = B - b0 < Bp ? B - b0 : Bp;
        tg.G = G * fn.Bp;
        lf.nr = (lf.shared ? G * fn.Bp : fn.Bp) * N;
        for (int t = 0; t <= h; ++t) {
            if (pf.adapted) launch_mg_pafan_step(sc.stream, tg, fa, fn, lf, ta, t);
            else launch_mg_pfan_step(sc.stream, tg, fa, fn, lf, ta, t);
        }
    }
    OP_TRY(hipGetLastError());
    std::vector<double> hl;
    if (fc.y_mean || fc.y_var_total || fc.lpd_gauss) {
        // the forecast stacks as [G][B * h][D] against the targets Y_fc[b * h + k] = Y_obs[origins[b] + 1 + k]
        std::vector<double> &yfc = sc.host(BH * J);
        for (int b = 0; b < B; ++b)
            memcpy(yfc.data() + (size_t)b * h * J, flt.Y_obs + (size_t)(fc.origins[b] + 1) * J, (size_t)h * J * sizeof(double));
        const SummaryReq fq{flt.CC, flt.DD, flt.noise_std, J, yfc.data(), B * h, fc.y_mean, nullptr, fc.y_var_total, nullptr, fc.lpd_gauss};
        if (int rc = mg_summary(sc, who, dmfc, dSfc, G, B * h, D, fq)) return rc;
    }
    double *lfc = pf.fc_lpd;
    if (!lfc && fc.lpd_mix) { hl.resize(nl_fc); lfc = hl.data(); }
    auto down = [&](void *dst, const void *src, size_t bytes) { return !dst || sc.download(dst, src, bytes); };
    if (!down(fc.m_fc, dmfc, nm_fc * sizeof(double)) || !down(fc.S_fc, dSfc, nS_fc * sizeof(double)) || !down(lfc, ta.lpd_fc, nl_fc * sizeof(double)) ||
        !down(pf.fc_particles, ta.fc_particles, nm_fc * N * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    if (fc.lpd_mix) lpd_mix_over_groups(lfc, G, BH * J, fc.lpd_mix);
    return mg_particle_finish(sc, who, G, 1, steps, D, dm, dS, m_x, S_x, fa, pa, flt, q);
}

// the scalar-argument checks the two entry points share (before any device call); nothing: FFVD_OK without touching anything
int records_checks(const std::string &who, int method, int kind, int G, int n_models, int M, int P, int D, int C, int steps, int q_mode, const FilterReq &f,
                   const RecordsReq &rq, bool &nothing, const ParticleReq *pq = nullptr, bool with_S0 = false) {
    const std::string bad = who + ": bad argument";
    nothing = false;
    if (kind != FFVD_KERNEL_SE)
        return set_error(nullptr, FFVD_EINVAL, bad + (method == MG_METHOD_CUBATURE ? mg_crecords_se_only : method == MG_METHOD_PARTICLE
                                                      ? mg_precords_se_only : method == MG_METHOD_ADAPTED ? mg_arecords_se_only
                                                      : method == MG_METHOD_ADAPTIVE ? mg_erecords_se_only : mg_records_se_only));
    if (!mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) || !filter_scalars_ok(f)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (!records_scalars_ok(rq, G, steps, D))
        return set_error(nullptr, FFVD_EINVAL, bad + " (R >= 0, records_per_pass >= 0, G * R * steps * D * D < 2^31 and G * R * D < 2^31 are needed)");
    nothing = G == 0 || rq.R == 0 || steps == 0;
    if (mg_particle_rule(method) && (!pq || !particle_ok(*pq, G, rq.R, steps, D, with_S0, nothing)))
        return set_error(nullptr, FFVD_EINVAL, bad + " (2 <= N <= 2048, finite draws, unif in [0, 1), xi0 with S0s, strides 0 or contiguous and "
                                               "G * R * steps * N * D < 2^31 are needed)");
    if (method == MG_METHOD_ADAPTIVE && !(std::isfinite(pq->ess_threshold) && pq->ess_threshold >= 0.0))
        return set_error(nullptr, FFVD_EINVAL, bad + " (ess_threshold must be finite and >= 0)");
    return FFVD_OK;
}

// the body of ffvd_op_filter_records_grouped (MG_METHOD_LINEAR) and ffvd_op_filter_cubature_records_grouped (MG_METHOD_CUBATURE)
int records_given(const std::string &who, int method, int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                  int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                  const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                  const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                  const double *DD, const double *noise_std, int J, const double *Y_obs,
                  int records_per_pass, double *m_pred, double *S_pred, double *m_filt, double *S_filt,
                  double *cross, double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth,
                  double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss, const ParticleReq *pq = nullptr,
                  const ParticleSmoothReq *sq = nullptr) {
    const std::string bad = who + ": bad argument";
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    const RecordsReq rq{R, records_per_pass};
    bool nothing;
    if (int rc = records_checks(who, method, kind, G, n_models, M, P, D, C, steps, q_mode, f, rq, nothing, pq, S0s != nullptr)) return rc;
    if (sq && !nothing && !particle_smooth_ok(*sq, R, steps))
        return set_error(nullptr, FFVD_EINVAL, bad + " (every entry of lengths must lie in [1, steps])");
    if (sq && sq->bs && !particle_backsim_ok(*sq->bs, G, R, steps, nothing, pq && pq->seeded))
        return set_error(nullptr, FFVD_EINVAL, bad + " (1 <= B <= 4096, unif_bs in [0, 1), strides 0 or contiguous and G * R * B < 2^31 are needed)");
    if (nothing) return FFVD_OK;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !x_lasts || !log_Qs || (C > 0 && !ctrl) ||
        !filter_arrays_ok(f, R * steps, m_pred, S_pred, pq && (pq->ess || pq->log_evidence || pq->particles || pq->ancestors || pq->weights || pq->resampled || (sq && sq->any_output()))))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t nK = (size_t)n_models * D, GD = (size_t)G * D, VD = GD * R, nq = given_nq(q_sqrts, q_mode, G, D);
    if (!given_tables_ok(Lm_inverse_seqs, nK, q_sqrts, nq)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    const int Mp = round_up(M, NB);
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp), *dq = nq ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    GroupHypers gh = stage_group_hypers(sc, FFVD_KERNEL_SE, n_models, D, M, Mp, P, Zs, logvariances, loglengthscales);
    double *dU = sc.upload(fs, GD * M), *dxl = sc.upload(x_lasts, VD), *dS0 = S0s ? sc.upload(S0s, VD * D) : nullptr, *dlq = sc.upload(log_Qs, GD);
    double *dctrl = C ? sc.upload(ctrl, (size_t)R * steps * C) : nullptr;
    OP_CHECK(dW && (!nq || dq) && dU && dxl && (!S0s || dS0) && dlq && (!C || dctrl) && gh.logs(sc) && gh.blocks(sc), who);
    gh.prep(sc.stream);
    return mg_records_run(sc, who, method, G, n_models, M, P, D, C, steps, gh.hv(), gh.dZ, dW, dq, q_mode, dU, dxl, dS0, dlq, dctrl, m_pred, S_pred, f,
                          rq, pq, sq);
}

// the body of ffvd_op_posterior_filter_records_grouped and ffvd_op_posterior_filter_cubature_records_grouped
int records_posterior(const std::string &who, int method, int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                      const double *logvariances, const double *loglengthscales, const double *Xs,
                      const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                      int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                      const double *ctrl_roll, int steps, const double *CC, const double *DD,
                      const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                      double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *cross,
                      double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean,
                      double *y_var_total, double *lpd_mix, double *lpd_gauss, double *U_means, const ParticleReq *pq = nullptr,
                      const ParticleSmoothReq *sq = nullptr) {
    const std::string bad = who + ": bad argument";
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    const RecordsReq rq{R, records_per_pass};
    bool nothing;
    if (int rc = records_checks(who, method, kind, G, n_models, M, P, D, C, steps, q_mode, f, rq, nothing, pq, S0s != nullptr)) return rc;
    if (sq && !nothing && !particle_smooth_ok(*sq, R, steps))
        return set_error(nullptr, FFVD_EINVAL, bad + " (every entry of lengths must lie in [1, steps])");
    if (sq && sq->bs && !particle_backsim_ok(*sq->bs, G, R, steps, nothing, pq && pq->seeded))
        return set_error(nullptr, FFVD_EINVAL, bad + " (1 <= B <= 4096, unif_bs in [0, 1), strides 0 or contiguous and G * R * B < 2^31 are needed)");
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (nothing) return FFVD_OK;
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || (C > 0 && (!ctrl_fit || !ctrl_roll)) ||
        !filter_arrays_ok(f, R * steps, m_pred, S_pred, pq && (pq->ess || pq->log_evidence || pq->particles || pq->ancestors || pq->weights || pq->resampled || (sq && sq->any_output()))))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    OP_BEGIN(who);
    PgWork w{};
    const int nm = n_models, Mp = round_up(M, NB), nK = nm * D;
    const size_t GD = (size_t)G * D, VD = GD * R, mm = (size_t)Mp * Mp;
    const bool have_q = pg_want_q(sc, w, q_mode, G, D, M);
    double *dW = sc.alloc<double>((size_t)nK * mm), *dxl = x0s ? sc.upload(x0s, VD) : sc.alloc<double>(VD);
    double *dx1 = x0s ? nullptr : sc.alloc<double>(GD);
    OP_CHECK(have_q && dW && dxl && (x0s || dx1), who);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    double *dZ = sc.upload(Zs, (size_t)nm * M * P), *dS0 = S0s ? sc.upload(S0s, VD * D) : nullptr;
    double *dctrl = C ? sc.upload(ctrl_roll, (size_t)R * steps * C) : nullptr;
    OP_CHECK(dZ && (!S0s || dS0) && (!C || dctrl), who);
    launch_pg_pack(sc.stream, w.Kuu, 2 * mm, Mp, Mp, nK, 1, M, 1, dW, Mp, Mp, nK);
    if (!x0s) {
        launch_pg_x_last(sc.stream, w.Xs, G, T, D, dx1);
        launch_mg_lrec_spread(sc.stream, G, R, D, dx1, dxl);
    }
    if (int rc = mg_records_run(sc, who, method, G, nm, M, P, D, C, steps, w.hv, dZ, dW, pg_q(w, q_mode), q_mode, w.U, dxl, dS0, w.log_Qs, dctrl,
                                m_pred, S_pred, f, rq, pq, sq))
        return rc;
    if (U_means && !sc.download(U_means, w.U, GD * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    return FFVD_OK;
}
}  // namespace

#define FFVD_RECORDS_GIVEN_PARAMS                                                                                                            \
    int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D, const double *logvariances, \
        const double *loglengthscales, const double *fs, const double *const *q_sqrts, int q_mode, int R, const double *x_lasts,            \
        const double *S0s, const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,                  \
        const double *noise_std, int J, const double *Y_obs, int records_per_pass, double *m_pred, double *S_pred, double *m_filt,          \
        double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean,                  \
        double *y_var_total, double *lpd_mix, double *lpd_gauss
#define FFVD_RECORDS_GIVEN_ARGS                                                                                                              \
    kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts, q_mode, R, x_lasts, S0s, ctrl, C, steps,   \
        log_Qs, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth,   \
        y_mean, y_var_total, lpd_mix, lpd_gauss
#define FFVD_RECORDS_POSTERIOR_PARAMS                                                                                                        \
    int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances, const double *loglengthscales,        \
        const double *Xs, const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter, int groups_per_pass, int q_mode,       \
        int R, const double *x0s, const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,                \
        const double *noise_std, int J, const double *Y_obs, int records_per_pass, double *m_pred, double *S_pred, double *m_filt,          \
        double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth, double *S_smooth, double *y_mean,                  \
        double *y_var_total, double *lpd_mix, double *lpd_gauss, double *U_means
#define FFVD_RECORDS_POSTERIOR_ARGS                                                                                                          \
    kind, G, n_models, Zs, M, P, D, logvariances, loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, R, x0s,     \
        S0s, ctrl_roll, steps, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint,        \
        m_smooth, S_smooth, y_mean, y_var_total, lpd_mix, lpd_gauss, U_means

extern "C" int ffvd_op_filter_records_grouped(FFVD_RECORDS_GIVEN_PARAMS) {
    return records_given("ffvd_op_filter_records_grouped", MG_METHOD_LINEAR, FFVD_RECORDS_GIVEN_ARGS);
}

// The collapsed posteriors of ffvd_op_posterior_grouped filtered over the records without leaving the device (as
// ffvd_op_posterior_filter_linear_grouped); x0s NULL: every record of group g starts at the last row of Xs[g]
extern "C" int ffvd_op_posterior_filter_records_grouped(FFVD_RECORDS_POSTERIOR_PARAMS) {
    return records_posterior("ffvd_op_posterior_filter_records_grouped", MG_METHOD_LINEAR, FFVD_RECORDS_POSTERIOR_ARGS);
}

// The same two calls with the third-degree spherical cubature rule as the propagation (moment_cubature_records.hip)
extern "C" int ffvd_op_filter_cubature_records_grouped(FFVD_RECORDS_GIVEN_PARAMS) {
    return records_given("ffvd_op_filter_cubature_records_grouped", MG_METHOD_CUBATURE, FFVD_RECORDS_GIVEN_ARGS);
}

extern "C" int ffvd_op_posterior_filter_cubature_records_grouped(FFVD_RECORDS_POSTERIOR_PARAMS) {
    return records_posterior("ffvd_op_posterior_filter_cubature_records_grouped", MG_METHOD_CUBATURE, FFVD_RECORDS_POSTERIOR_ARGS);
}

// The same two calls with a bootstrap particle filter of N particles per track as the propagation and the update
// (moment_particle_records.hip): no smoother and no `cross`; the draws are the caller's
#define FFVD_PARTICLE_PARAMS                                                                                                                 \
    int N, const double *eps, long long eps_stride_g, long long eps_stride_r, const double *unif, long long unif_stride_g,                  \
        long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r
#define FFVD_PARTICLE_REQ                                                                                                                    \
    const ParticleReq pq {                                                                                                                   \
        N, eps, eps_stride_g, eps_stride_r, unif, unif_stride_g, unif_stride_r, xi0, xi0_stride_g, xi0_stride_r, ess, log_evidence,          \
            particles, ancestors                                                                                                             \
    }
extern "C" int ffvd_op_filter_particle_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                                       int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                                       const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                                       const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                                       const double *DD, const double *noise_std, int J, const double *Y_obs,
                                                       int records_per_pass, FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred,
                                                       double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                       double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                       double *log_evidence, double *particles, int *ancestors) {
    FFVD_PARTICLE_REQ;
    return records_given("ffvd_op_filter_particle_records_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                         logvariances, loglengthscales, fs, q_sqrts, q_mode, R, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs,
                         records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix,
                         lpd_gauss, &pq);
}

extern "C" int ffvd_op_posterior_filter_particle_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                                 const double *logvariances, const double *loglengthscales, const double *Xs,
                                                                 const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                                 int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                                 const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                                 const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                                 FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred, double *m_filt,
                                                                 double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                                 double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                                 double *log_evidence, double *particles, int *ancestors, double *U_means) {
    FFVD_PARTICLE_REQ;
    return records_posterior("ffvd_op_posterior_filter_particle_records_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Zs, M, P, D, logvariances,
                             loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD,
                             noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr,
                             y_mean, y_var_total, lpd_mix, lpd_gauss, U_means, &pq);
}

// The same two calls with the optimal proposal in place of the bootstrap one (moment_particle_adapted.hip): the fully adapted
// auxiliary particle filter.  The argument lists are those of the two calls above; `particles` is the equally weighted filtered set
// after every row and `ancestors` indexes the set carried into the row.  (Not ffvd_op_*: see DESIGN.md section 9, "Particle smoothing".)
extern "C" int ffvd_particle_adapted_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                                     int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                                     const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                                     const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                                     const double *DD, const double *noise_std, int J, const double *Y_obs,
                                                     int records_per_pass, FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred,
                                                     double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                     double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                     double *log_evidence, double *particles, int *ancestors) {
    FFVD_PARTICLE_REQ;
    return records_given("ffvd_particle_adapted_records_grouped", MG_METHOD_ADAPTED, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                         logvariances, loglengthscales, fs, q_sqrts, q_mode, R, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs,
                         records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix,
                         lpd_gauss, &pq);
}

extern "C" int ffvd_posterior_particle_adapted_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                               const double *logvariances, const double *loglengthscales, const double *Xs,
                                                               const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                               int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                               const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                               const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                               FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred, double *m_filt,
                                                               double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                               double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                               double *log_evidence, double *particles, int *ancestors, double *U_means) {
    FFVD_PARTICLE_REQ;
    return records_posterior("ffvd_posterior_particle_adapted_records_grouped", MG_METHOD_ADAPTED, kind, G, n_models, Zs, M, P, D, logvariances,
                             loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD,
                             noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr,
                             y_mean, y_var_total, lpd_mix, lpd_gauss, U_means, &pq);
}

// The same two calls followed by the marginal particle smoother on the carried sets (moment_particle_smooth.hip): the filter's
// launches with one more per step that keeps (mu, s), then the smoother over all tracks of the call.  The filter outputs are those of
// the two calls above bit for bit.  (Not ffvd_op_*: see DESIGN.md section 9, "Particle smoothing".)
#define FFVD_PARTICLE_SMOOTH_PARAMS                                                                                                          \
    const int *lengths, double *m_smooth, double *S_smooth, double *ess_smooth, double *w_smooth, double *weights, double *trans_mean,      \
        double *trans_var
#define FFVD_PARTICLE_SMOOTH_REQ const ParticleSmoothReq sq{lengths, m_smooth, S_smooth, ess_smooth, w_smooth, weights, trans_mean, trans_var}
extern "C" int ffvd_particle_smooth_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                                    int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                                    const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                                    const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                                    const double *DD, const double *noise_std, int J, const double *Y_obs,
                                                    int records_per_pass, FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred,
                                                    double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                    double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                    double *log_evidence, double *particles, int *ancestors, FFVD_PARTICLE_SMOOTH_PARAMS) {
    FFVD_PARTICLE_REQ;
    FFVD_PARTICLE_SMOOTH_REQ;
    return records_given("ffvd_particle_smooth_records_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                         logvariances, loglengthscales, fs, q_sqrts, q_mode, R, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs,
                         records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix,
                         lpd_gauss, &pq, &sq);
}

extern "C" int ffvd_posterior_particle_smooth_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                              const double *logvariances, const double *loglengthscales, const double *Xs,
                                                              const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                              int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                              const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                              const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                              FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred, double *m_filt,
                                                              double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                              double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                              double *log_evidence, double *particles, int *ancestors,
                                                              FFVD_PARTICLE_SMOOTH_PARAMS, double *U_means) {
    FFVD_PARTICLE_REQ;
    FFVD_PARTICLE_SMOOTH_REQ;
    return records_posterior("ffvd_posterior_particle_smooth_records_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Zs, M, P, D, logvariances,
                             loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD,
                             noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr,
                             y_mean, y_var_total, lpd_mix, lpd_gauss, U_means, &pq, &sq);
}
#undef FFVD_PARTICLE_SMOOTH_PARAMS
#undef FFVD_PARTICLE_SMOOTH_REQ

// The same two filter calls followed by the backward simulation of B joint trajectories per track (moment_particle_backsim.hip): the
// smoothing calls' launches up to the weights kernel, then one launch for all (track, trajectory) recursions and one for the moments.
// The filter outputs, weights, trans_mean and trans_var are those of the smoothing calls bit for bit.
#define FFVD_PARTICLE_BACKSIM_PARAMS                                                                                                         \
    const int *lengths, int B, const double *unif_bs, long long unif_bs_stride_g, long long unif_bs_stride_r, double *trajectories,         \
        int *traj_index, double *m_traj, double *S_traj, double *lag_cov, double *weights, double *trans_mean, double *trans_var
#define FFVD_PARTICLE_BACKSIM_REQ                                                                                                            \
    const ParticleBacksimReq bq{B, unif_bs, unif_bs_stride_g, unif_bs_stride_r, trajectories, traj_index, m_traj, S_traj, lag_cov};          \
    ParticleSmoothReq sq{lengths, nullptr, nullptr, nullptr, nullptr, weights, trans_mean, trans_var};                                       \
    sq.bs = &bq
extern "C" int ffvd_particle_backsim_records_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                                     int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                                     const double *const *q_sqrts, int q_mode, int R, const double *x_lasts, const double *S0s,
                                                     const double *ctrl, int C, int steps, const double *log_Qs, const double *CC,
                                                     const double *DD, const double *noise_std, int J, const double *Y_obs,
                                                     int records_per_pass, FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred,
                                                     double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                     double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                     double *log_evidence, double *particles, int *ancestors, FFVD_PARTICLE_BACKSIM_PARAMS) {
    FFVD_PARTICLE_REQ;
    FFVD_PARTICLE_BACKSIM_REQ;
    return records_given("ffvd_particle_backsim_records_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                         logvariances, loglengthscales, fs, q_sqrts, q_mode, R, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs,
                         records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix,
                         lpd_gauss, &pq, &sq);
}

extern "C" int ffvd_posterior_particle_backsim_records_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                               const double *logvariances, const double *loglengthscales, const double *Xs,
                                                               const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                               int groups_per_pass, int q_mode, int R, const double *x0s, const double *S0s,
                                                               const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                               const double *noise_std, int J, const double *Y_obs, int records_per_pass,
                                                               FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred, double *m_filt,
                                                               double *S_filt, double *lpd, double *lpd_joint, double *y_mean,
                                                               double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess,
                                                               double *log_evidence, double *particles, int *ancestors,
                                                               FFVD_PARTICLE_BACKSIM_PARAMS, double *U_means) {
    FFVD_PARTICLE_REQ;
    FFVD_PARTICLE_BACKSIM_REQ;
    return records_posterior("ffvd_posterior_particle_backsim_records_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Zs, M, P, D, logvariances,
                             loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD,
                             noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr,
                             y_mean, y_var_total, lpd_mix, lpd_gauss, U_means, &pq, &sq);
}
#undef FFVD_PARTICLE_BACKSIM_PARAMS
#undef FFVD_PARTICLE_BACKSIM_REQ

// The adapted filter's two calls followed by the marginal smoother, or by the backward simulation, on the ADAPTED sets
// (moment_particle_adapted_smooth.hip): the argument lists of the four calls above without `weights` -- the filtered sets are equally
// weighted.  The filter outputs are those of the adapted calls bit for bit; trans_mean[t] and trans_var[t] are the moments of the set
// carried into row t.  (Not ffvd_op_*: see DESIGN.md section 9, "Particle smoothing".)
#define FFVD_ADAPTED_SMOOTH_PARAMS                                                                                                           \
    const int *lengths, double *m_smooth, double *S_smooth, double *ess_smooth, double *w_smooth, double *trans_mean, double *trans_var
#define FFVD_ADAPTED_SMOOTH_REQ const ParticleSmoothReq sq{lengths, m_smooth, S_smooth, ess_smooth, w_smooth, nullptr, trans_mean, trans_var}
#define FFVD_ADAPTED_BACKSIM_PARAMS                                                                                                          \
    const int *lengths, int B, const double *unif_bs, long long unif_bs_stride_g, long long unif_bs_stride_r, double *trajectories,         \
        int *traj_index, double *m_traj, double *S_traj, double *lag_cov, double *trans_mean, double *trans_var
#define FFVD_ADAPTED_BACKSIM_REQ                                                                                                             \
    const ParticleBacksimReq bq{B, unif_bs, unif_bs_stride_g, unif_bs_stride_r, trajectories, traj_index, m_traj, S_traj, lag_cov};          \
    ParticleSmoothReq sq{lengths, nullptr, nullptr, nullptr, nullptr, nullptr, trans_mean, trans_var};                                       \
    sq.bs = &bq
#define FFVD_ADAPTED_GIVEN_HEAD                                                                                                              \
    int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D, const double *logvariances, \
        const double *loglengthscales, const double *fs, const double *const *q_sqrts, int q_mode, int R, const double *x_lasts,            \
        const double *S0s, const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,                  \
        const double *noise_std, int J, const double *Y_obs, int records_per_pass, FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred,    \
        double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,               \
        double *lpd_gauss, double *ess, double *log_evidence, double *particles, int *ancestors
#define FFVD_ADAPTED_GIVEN_CALL(who)                                                                                                         \
    records_given(who, MG_METHOD_ADAPTED, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts, q_mode, \
                  R, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt,   \
                  nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix, lpd_gauss, &pq, &sq)
#define FFVD_ADAPTED_POSTERIOR_HEAD                                                                                                          \
    int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances, const double *loglengthscales,        \
        const double *Xs, const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter, int groups_per_pass, int q_mode,       \
        int R, const double *x0s, const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,                \
        const double *noise_std, int J, const double *Y_obs, int records_per_pass, FFVD_PARTICLE_PARAMS, double *m_pred, double *S_pred,    \
        double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix,               \
        double *lpd_gauss, double *ess, double *log_evidence, double *particles, int *ancestors
#define FFVD_ADAPTED_POSTERIOR_CALL(who)                                                                                                     \
    records_posterior(who, MG_METHOD_ADAPTED, kind, G, n_models, Zs, M, P, D, logvariances, loglengthscales, Xs, ctrl_fit, C, T, log_Qs,    \
                      jitter, groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, \
                      S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix, lpd_gauss, U_means,  \
                      &pq, &sq)
extern "C" int ffvd_particle_adapted_smooth_records_grouped(FFVD_ADAPTED_GIVEN_HEAD, FFVD_ADAPTED_SMOOTH_PARAMS) {
    FFVD_PARTICLE_REQ;
    FFVD_ADAPTED_SMOOTH_REQ;
    return FFVD_ADAPTED_GIVEN_CALL("ffvd_particle_adapted_smooth_records_grouped");
}
extern "C" int ffvd_posterior_particle_adapted_smooth_records_grouped(FFVD_ADAPTED_POSTERIOR_HEAD, FFVD_ADAPTED_SMOOTH_PARAMS,
                                                                      double *U_means) {
    FFVD_PARTICLE_REQ;
    FFVD_ADAPTED_SMOOTH_REQ;
    return FFVD_ADAPTED_POSTERIOR_CALL("ffvd_posterior_particle_adapted_smooth_records_grouped");
}
extern "C" int ffvd_particle_adapted_backsim_records_grouped(FFVD_ADAPTED_GIVEN_HEAD, FFVD_ADAPTED_BACKSIM_PARAMS) {
    FFVD_PARTICLE_REQ;
    FFVD_ADAPTED_BACKSIM_REQ;
    return FFVD_ADAPTED_GIVEN_CALL("ffvd_particle_adapted_backsim_records_grouped");
}
extern "C" int ffvd_posterior_particle_adapted_backsim_records_grouped(FFVD_ADAPTED_POSTERIOR_HEAD, FFVD_ADAPTED_BACKSIM_PARAMS,
                                                                       double *U_means) {
    FFVD_PARTICLE_REQ;
    FFVD_ADAPTED_BACKSIM_REQ;
    return FFVD_ADAPTED_POSTERIOR_CALL("ffvd_posterior_particle_adapted_backsim_records_grouped");
}
#undef FFVD_ADAPTED_SMOOTH_PARAMS
#undef FFVD_ADAPTED_SMOOTH_REQ
#undef FFVD_ADAPTED_BACKSIM_PARAMS
#undef FFVD_ADAPTED_BACKSIM_REQ
#undef FFVD_ADAPTED_GIVEN_HEAD
#undef FFVD_ADAPTED_GIVEN_CALL
#undef FFVD_ADAPTED_POSTERIOR_HEAD
#undef FFVD_ADAPTED_POSTERIOR_CALL
#undef FFVD_PARTICLE_PARAMS
#undef FFVD_PARTICLE_REQ

// The twelve particle calls above with seeded draws generated on the device (moment_particle_draws.hip; DESIGN.md section 9, "Device
// draws"): rule 0 bootstrap / 1 adapted, stage 0 filter / 1 marginal smoother / 2 backward simulation select the entry point whose
// launches run, `seed` and `noise` (0 shared, 1 per record, 2 independent) stand in for its draw arrays and their strides.  The driver
// is mg_records_run with a seeded ParticleReq: one fill launch per stream writes the buffers the caller's arrays are uploaded into
// otherwise, so every output is that entry point's, bit for bit, on the arrays of ffvd_particle_draws(seed, noise, ..).
// (Not ffvd_op_*: see DESIGN.md section 9, "Particle smoothing".)
namespace {
constexpr int SEEDED_FILTER = 0, SEEDED_SMOOTH = 1, SEEDED_BACKSIM = 2;
// the strides of a noise mode over blocks of `inner` doubles: (group, record)
void seeded_strides(int noise, int R, long long inner, long long &sg, long long &sr) {
    sr = noise == MG_PDRAW_SHARED ? 0 : inner;
    sg = noise == MG_PDRAW_INDEPENDENT ? inner * R : 0;
}
// The three requests of a seeded call; sq_or_null() is what records_given / records_posterior take beside &pq
struct SeededReq {
    int method;
    ParticleReq pq;
    ParticleBacksimReq bq;
    ParticleSmoothReq sq;
    bool with_sq;
    const ParticleSmoothReq *sq_or_null() const { return with_sq ? &sq : nullptr; }
};
struct SeededOut {                                       // the outputs beyond the filter's, and `lengths`
    const int *lengths;
    int B;
    double *trajectories;
    int *traj_index;
    double *m_traj, *S_traj, *lag_cov, *weights, *trans_mean, *trans_var, *m_smooth, *S_smooth, *ess_smooth, *w_smooth;
};
// rule, stage, noise; the outputs (and `lengths`) that the (rule, stage) does not have must be NULL.  q is filled in place: q.sq.bs
// points into it.
int seeded_request(const std::string &who, int rule, int stage, unsigned long long seed, int noise, int R, int steps, int N, int D,
                   const SeededOut &o, double *ess, double *log_evidence, double *particles, int *ancestors, SeededReq &q) {
    const std::string bad = who + ": bad argument";
    if ((rule != 0 && rule != 1) || stage < SEEDED_FILTER || stage > SEEDED_BACKSIM || noise < MG_PDRAW_SHARED || noise > MG_PDRAW_INDEPENDENT)
        return set_error(nullptr, FFVD_EINVAL, bad + " (rule 0 or 1, stage 0, 1 or 2 and noise 0, 1 or 2 are needed)");
    std::string extra;
    auto must_be_null = [&](const void *p, const char *name) {
        if (p) extra += (extra.empty() ? "" : ", ") + std::string(name);
    };
    if (stage == SEEDED_FILTER) must_be_null(o.lengths, "lengths");
    if (stage != SEEDED_BACKSIM) {
        must_be_null(o.trajectories, "trajectories"); must_be_null(o.traj_index, "traj_index"); must_be_null(o.m_traj, "m_traj");
        must_be_null(o.S_traj, "S_traj"); must_be_null(o.lag_cov, "lag_cov");
    }
    if (stage == SEEDED_FILTER || rule == 1) must_be_null(o.weights, "weights");
    if (stage == SEEDED_FILTER) { must_be_null(o.trans_mean, "trans_mean"); must_be_null(o.trans_var, "trans_var"); }
    if (stage != SEEDED_SMOOTH) {
        must_be_null(o.m_smooth, "m_smooth"); must_be_null(o.S_smooth, "S_smooth"); must_be_null(o.ess_smooth, "ess_smooth");
        must_be_null(o.w_smooth, "w_smooth");
    }
    if (!extra.empty())
        return set_error(nullptr, FFVD_EINVAL, bad + " (rule " + std::to_string(rule) + ", stage " + std::to_string(stage) +
                                               " does not produce " + extra + ": NULL is needed there)");
    q.method = rule ? MG_METHOD_ADAPTED : MG_METHOD_PARTICLE;
    q.pq = ParticleReq{N, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, ess, log_evidence, particles, ancestors};
    q.pq.seeded = true;
    q.pq.seed = seed;
    seeded_strides(noise, R, (long long)steps * N * D, q.pq.eps_g, q.pq.eps_r);
    seeded_strides(noise, R, steps, q.pq.unif_g, q.pq.unif_r);
    seeded_strides(noise, R, (long long)N * D, q.pq.xi0_g, q.pq.xi0_r);
    q.bq = ParticleBacksimReq{o.B, nullptr, 0, 0, o.trajectories, o.traj_index, o.m_traj, o.S_traj, o.lag_cov};
    seeded_strides(noise, R, (long long)steps * o.B, q.bq.unif_g, q.bq.unif_r);
    q.sq = ParticleSmoothReq{o.lengths, o.m_smooth, o.S_smooth, o.ess_smooth, o.w_smooth, o.weights, o.trans_mean, o.trans_var};
    q.sq.bs = stage == SEEDED_BACKSIM ? &q.bq : nullptr;
    q.with_sq = stage != SEEDED_FILTER;
    return FFVD_OK;
}
}  // namespace

#define FFVD_SEEDED_TAIL_PARAMS                                                                                                              \
    int N, unsigned long long seed, int noise, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd,                 \
        double *lpd_joint, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess, double *log_evidence,      \
        double *particles, int *ancestors, const int *lengths, int B, double *trajectories, int *traj_index, double *m_traj,                \
        double *S_traj, double *lag_cov, double *weights, double *trans_mean, double *trans_var, double *m_smooth, double *S_smooth,        \
        double *ess_smooth, double *w_smooth
#define FFVD_SEEDED_REQ(who)                                                                                                                 \
    const SeededOut so{lengths, B, trajectories, traj_index, m_traj, S_traj, lag_cov, weights, trans_mean, trans_var, m_smooth, S_smooth,   \
                       ess_smooth, w_smooth};                                                                                               \
    SeededReq q;                                                                                                                             \
    if (int rc = seeded_request(who, rule, stage, seed, noise, R, steps, N, D, so, ess, log_evidence, particles, ancestors, q)) return rc
extern "C" int ffvd_particle_seeded_records_grouped(int rule, int stage, int kind, int G, int n_models, const double *const *Lm_inverse_seqs,
                                                    const double *Zs, int M, int P, int D, const double *logvariances,
                                                    const double *loglengthscales, const double *fs, const double *const *q_sqrts, int q_mode,
                                                    int R, const double *x_lasts, const double *S0s, const double *ctrl, int C, int steps,
                                                    const double *log_Qs, const double *CC, const double *DD, const double *noise_std, int J,
                                                    const double *Y_obs, int records_per_pass, FFVD_SEEDED_TAIL_PARAMS) {
    const char *who = "ffvd_particle_seeded_records_grouped";
    FFVD_SEEDED_REQ(who);
    return records_given(who, q.method, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts, q_mode, R,
                         x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt, S_filt,
                         nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix, lpd_gauss, &q.pq, q.sq_or_null());
}

extern "C" int ffvd_posterior_particle_seeded_records_grouped(int rule, int stage, int kind, int G, int n_models, const double *Zs, int M, int P,
                                                              int D, const double *logvariances, const double *loglengthscales,
                                                              const double *Xs, const double *ctrl_fit, int C, int T, const double *log_Qs,
                                                              double jitter, int groups_per_pass, int q_mode, int R, const double *x0s,
                                                              const double *S0s, const double *ctrl_roll, int steps, const double *CC,
                                                              const double *DD, const double *noise_std, int J, const double *Y_obs,
                                                              int records_per_pass, FFVD_SEEDED_TAIL_PARAMS, double *U_means) {
    const char *who = "ffvd_posterior_particle_seeded_records_grouped";
    FFVD_SEEDED_REQ(who);
    return records_posterior(who, q.method, kind, G, n_models, Zs, M, P, D, logvariances, loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter,
                             groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred,
                             S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix, lpd_gauss,
                             U_means, &q.pq, q.sq_or_null());
}
#undef FFVD_SEEDED_TAIL_PARAMS
#undef FFVD_SEEDED_REQ

// The two bootstrap particle filter calls with ADAPTIVE resampling (moment_particle_adaptive.hip; DESIGN.md section 9, "Adaptive
// resampling"): the track carries a weighted set and resamples only on the rows whose ess falls below ess_threshold * N (finite,
// >= 0: 0 never resamples, any value > 1 always does and returns the bootstrap calls' arrays bit for bit).  The argument lists are
// the bootstrap calls' with ess_threshold behind the draws and with weights [G][R][steps][N] (or NULL) and resampled [G][R][steps]
// (or NULL) behind ancestors; the seeded two take N, seed and noise where the others have N and the nine draw arguments.
// (Not ffvd_op_*: see DESIGN.md section 9, "Particle smoothing".)
#define FFVD_ADAPTIVE_GIVEN_HEAD                                                                                                             \
    int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P, int D, const double *logvariances, \
        const double *loglengthscales, const double *fs, const double *const *q_sqrts, int q_mode, int R, const double *x_lasts,            \
        const double *S0s, const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,                  \
        const double *noise_std, int J, const double *Y_obs, int records_per_pass
#define FFVD_ADAPTIVE_POSTERIOR_HEAD                                                                                                         \
    int kind, int G, int n_models, const double *Zs, int M, int P, int D, const double *logvariances, const double *loglengthscales,        \
        const double *Xs, const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter, int groups_per_pass, int q_mode,       \
        int R, const double *x0s, const double *S0s, const double *ctrl_roll, int steps, const double *CC, const double *DD,                \
        const double *noise_std, int J, const double *Y_obs, int records_per_pass
#define FFVD_ADAPTIVE_DRAWS                                                                                                                  \
    int N, const double *eps, long long eps_stride_g, long long eps_stride_r, const double *unif, long long unif_stride_g,                  \
        long long unif_stride_r, const double *xi0, long long xi0_stride_g, long long xi0_stride_r
#define FFVD_ADAPTIVE_TAIL                                                                                                                   \
    double ess_threshold, double *m_pred, double *S_pred, double *m_filt, double *S_filt, double *lpd, double *lpd_joint, double *y_mean,   \
        double *y_var_total, double *lpd_mix, double *lpd_gauss, double *ess, double *log_evidence, double *particles, int *ancestors,      \
        double *weights, int *resampled
#define FFVD_ADAPTIVE_REQ                                                                                                                    \
    ParticleReq pq{N,   eps,          eps_stride_g, eps_stride_r, unif, unif_stride_g, unif_stride_r, xi0, xi0_stride_g, xi0_stride_r,      \
                   ess, log_evidence, particles,    ancestors};                                                                              \
    pq.ess_threshold = ess_threshold; pq.weights = weights; pq.resampled = resampled
#define FFVD_ADAPTIVE_SEEDED_REQ                                                                                                             \
    if (noise < MG_PDRAW_SHARED || noise > MG_PDRAW_INDEPENDENT)                                                                             \
        return set_error(nullptr, FFVD_EINVAL, std::string(who) + ": bad argument (noise 0, 1 or 2 is needed)");                            \
    ParticleReq pq{N, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, ess, log_evidence, particles, ancestors};                                 \
    pq.seeded = true; pq.seed = seed;                                                                                                        \
    seeded_strides(noise, R, (long long)steps * N * D, pq.eps_g, pq.eps_r);                                                                  \
    seeded_strides(noise, R, steps, pq.unif_g, pq.unif_r);                                                                                   \
    seeded_strides(noise, R, (long long)N * D, pq.xi0_g, pq.xi0_r);                                                                          \
    pq.ess_threshold = ess_threshold; pq.weights = weights; pq.resampled = resampled
#define FFVD_ADAPTIVE_GIVEN_CALL(who)                                                                                                        \
    records_given(who, MG_METHOD_ADAPTIVE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts,     \
                  q_mode, R, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, S_pred, m_filt,   \
                  S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix, lpd_gauss, &pq)
#define FFVD_ADAPTIVE_POSTERIOR_CALL(who)                                                                                                    \
    records_posterior(who, MG_METHOD_ADAPTIVE, kind, G, n_models, Zs, M, P, D, logvariances, loglengthscales, Xs, ctrl_fit, C, T, log_Qs,   \
                      jitter, groups_per_pass, q_mode, R, x0s, S0s, ctrl_roll, steps, CC, DD, noise_std, J, Y_obs, records_per_pass, m_pred, \
                      S_pred, m_filt, S_filt, nullptr, lpd, lpd_joint, nullptr, nullptr, y_mean, y_var_total, lpd_mix, lpd_gauss, U_means,  \
                      &pq)
extern "C" int ffvd_particle_adaptive_records_grouped(FFVD_ADAPTIVE_GIVEN_HEAD, FFVD_ADAPTIVE_DRAWS, FFVD_ADAPTIVE_TAIL) {
    FFVD_ADAPTIVE_REQ;
    return FFVD_ADAPTIVE_GIVEN_CALL("ffvd_particle_adaptive_records_grouped");
}
extern "C" int ffvd_posterior_particle_adaptive_records_grouped(FFVD_ADAPTIVE_POSTERIOR_HEAD, FFVD_ADAPTIVE_DRAWS, FFVD_ADAPTIVE_TAIL,
                                                                double *U_means) {
    FFVD_ADAPTIVE_REQ;
    return FFVD_ADAPTIVE_POSTERIOR_CALL("ffvd_posterior_particle_adaptive_records_grouped");
}
extern "C" int ffvd_particle_adaptive_seeded_records_grouped(FFVD_ADAPTIVE_GIVEN_HEAD, int N, unsigned long long seed, int noise,
                                                             FFVD_ADAPTIVE_TAIL) {
    const char *who = "ffvd_particle_adaptive_seeded_records_grouped";
    FFVD_ADAPTIVE_SEEDED_REQ;
    return FFVD_ADAPTIVE_GIVEN_CALL(who);
}
extern "C" int ffvd_posterior_particle_adaptive_seeded_records_grouped(FFVD_ADAPTIVE_POSTERIOR_HEAD, int N, unsigned long long seed, int noise,
                                                                       FFVD_ADAPTIVE_TAIL, double *U_means) {
    const char *who = "ffvd_posterior_particle_adaptive_seeded_records_grouped";
    FFVD_ADAPTIVE_SEEDED_REQ;
    return FFVD_ADAPTIVE_POSTERIOR_CALL(who);
}
#undef FFVD_ADAPTIVE_GIVEN_HEAD
#undef FFVD_ADAPTIVE_POSTERIOR_HEAD
#undef FFVD_ADAPTIVE_DRAWS
#undef FFVD_ADAPTIVE_TAIL
#undef FFVD_ADAPTIVE_REQ
#undef FFVD_ADAPTIVE_SEEDED_REQ
#undef FFVD_ADAPTIVE_GIVEN_CALL
#undef FFVD_ADAPTIVE_POSTERIOR_CALL

// The draws a seeded call uses, generated on the device and downloaded: eps lead + [steps][N][D], unif lead + [steps], xi0 lead + [N][D],
// unif_bs lead + [steps][B], lead = (), (R,) or (G, R) for noise 0, 1 or 2.  Each output may be NULL; B may be 0 when unif_bs is.
extern "C" int ffvd_particle_draws(unsigned long long seed, int noise, int G, int R, int steps, int N, int D, int B, double *eps, double *unif,
                                   double *xi0, double *unif_bs) {
    const std::string who = "ffvd_particle_draws", bad = who + ": bad argument";
    if (noise < MG_PDRAW_SHARED || noise > MG_PDRAW_INDEPENDENT || G < 0 || R < 0 || steps < 0 || N < MG_PREC_MINN || N > MG_PREC_MAXN ||
        D < 1 || D > MG_MAXD || B < 0 || B > MG_PBS_MAXB || (unif_bs && B < 1))
        return set_error(nullptr, FFVD_EINVAL, bad + " (noise 0, 1 or 2, G, R, steps >= 0, 2 <= N <= 2048, 1 <= D <= 8 and 0 <= B <= 4096, "
                                               "B >= 1 with unif_bs, are needed)");
    if (G == 0 || R == 0 || steps == 0) return FFVD_OK;
    if ((long long)G * R > ((1LL << 31) - 1) / steps / N / D || (B && (long long)G * R > ((1LL << 31) - 1) / B) ||
        (long long)steps * B >= (1LL << 31))
        return set_error(nullptr, FFVD_EINVAL, bad + " (G * R * steps * N * D < 2^31, G * R * B < 2^31 and steps * B < 2^31 are needed)");
    OP_BEGIN(who);
    struct One { double *dst; int stream_id; bool normal; long long len; };
    const One all[4] = {{eps, MG_PDRAW_EPS, true, (long long)steps * N * D}, {unif, MG_PDRAW_UNIF, false, steps},
                        {xi0, MG_PDRAW_XI0, true, (long long)N * D}, {unif_bs, MG_PDRAW_UNIF_BS, false, (long long)steps * B}};
    for (const One &s : all) {
        if (!s.dst) continue;
        long long sg, sr;
        seeded_strides(noise, R, s.len, sg, sr);
        const size_t n = particle_extent(sg, sr, s.len, G, R);
        double *d = sc.alloc<double>(n);
        OP_CHECK(d, who);
        const MomentParticleDrawsArgs da{(unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), s.stream_id, s.normal ? 1 : 0,
                                         sg ? G : 1, sr ? R : 1, (int)s.len, sg, sr, d};
        if (!launch_mg_pdraw_fill(sc.stream, da)) return set_error(nullptr, FFVD_EINVAL, bad + " (the fill launch's grid does not fit)");
        OP_TRY(hipGetLastError());
        if (!sc.download(s.dst, d, n * sizeof(double)))
            return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    }
    return FFVD_OK;
}
#undef FFVD_RECORDS_GIVEN_PARAMS
#undef FFVD_RECORDS_GIVEN_ARGS
#undef FFVD_RECORDS_POSTERIOR_PARAMS
#undef FFVD_RECORDS_POSTERIOR_ARGS

// ---- rolling-origin forecasts (moment_group.h, MomentFanArgs) -----------------------------------------------------------------------
// ffvd_op_filter_grouped, then from every origin `horizon` steps of the propagation started at the filtered state of that row: one
// launch per forecast step for all (group, origin) tracks of a pass, and the pooled summary of every (origin, horizon).  `method`: the
// rule of the filter AND of the tracks (MG_METHOD_LINEAR: moment_linear.hip, then moment_linear_fan.hip, two launches per step;
// MG_METHOD_CUBATURE: moment_cubature_records.hip with one record, then moment_cubature_fan.hip, two launches per step)
namespace {
// the particle request of a forecast call (MG_METHOD_PARTICLE; the other rules take none): no `cross` and no smoother, the draws
int particle_fc_checks(const std::string &who, int method, const FilterReq &f, const ForecastReq &q, const ParticleFcReq *pf, int G, int steps,
                       int D, bool with_S0) {
    if (method != MG_METHOD_PARTICLE) return pf ? set_error(nullptr, FFVD_EINVAL, who + ": bad argument") : FFVD_OK;
    if (f.cross || f.m_smooth || f.S_smooth)
        return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (the particle filter has no cross covariance and no smoother: pass NULL)");
    if (!pf || !particle_fc_ok(*pf, G, q.n_origins, q.horizon, steps, D, with_S0))
        return set_error(nullptr, FFVD_EINVAL, who + ": bad argument (2 <= N <= 2048, finite draws, unif in [0, 1), xi0 with S0s, strides 0 or "
                                               "contiguous, G * steps * N * D < 2^31 and G * B * h * N * D < 2^31 are needed)");
    return FFVD_OK;
}

int forecast_given(const std::string &who, int method, int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                        int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                        const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                        const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        int horizon, const int *origins, int n_origins, int tracks_per_pass, double *m_fc, double *S_fc,
                                        double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss,
                                        const ParticleFcReq *pf = nullptr) {
    const std::string bad = who + ": bad argument";
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    const ForecastReq q{horizon, n_origins, tracks_per_pass, origins, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix, fc_lpd_gauss};
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + mg_fc_se_only(method));
    if (!mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) || !filter_scalars_ok(f) || !forecast_scalars_ok(q, G, steps, D))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (int rc = particle_fc_checks(who, method, f, q, pf, G, steps, D, S0s != nullptr)) return rc;
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !x_lasts || !log_Qs || (C > 0 && !ctrl) ||
        !filter_arrays_ok(f, steps, m_pred, S_pred, q.any_output() || (pf && pf->any_output())) || !forecast_origins_ok(q, steps))
        return set_error(nullptr, FFVD_EINVAL, bad);
    return mg_given_run(who, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl,
                        C, steps, log_Qs, m_pred, S_pred, nullptr, &f, &q, method, pf);
}

int forecast_posterior(const std::string &who, int method, int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                  const double *logvariances, const double *loglengthscales, const double *Xs,
                                                  const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                  int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                  const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                  const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                  double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                  double *lpd_gauss, double *U_means, int horizon, const int *origins, int n_origins,
                                                  int tracks_per_pass, double *m_fc, double *S_fc, double *fc_y_mean,
                                                  double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss,
                                                  const ParticleFcReq *pf = nullptr) {
    const std::string bad = who + ": bad argument";
    const FilterReq f{CC, DD, noise_std, J, Y_obs, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                      lpd_gauss};
    const ForecastReq q{horizon, n_origins, tracks_per_pass, origins, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix, fc_lpd_gauss};
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + mg_fc_se_only(method));
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) || !mg_scalars_ok(kind, G, n_models, M, P, D, C, steps, q_mode) ||
        !filter_scalars_ok(f) || !forecast_scalars_ok(q, G, steps, D))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (int rc = particle_fc_checks(who, method, f, q, pf, G, steps, D, S0s != nullptr)) return rc;
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || (C > 0 && (!ctrl_fit || !ctrl_roll)) ||
        !filter_arrays_ok(f, steps, m_pred, S_pred, q.any_output() || (pf && pf->any_output())) || !forecast_origins_ok(q, steps))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    return mg_posterior_run(in, q_mode, x0s, S0s, ctrl_roll, steps, m_pred, S_pred, U_means, nullptr, &f, &q, method, pf);
}
}  // namespace

extern "C" int ffvd_op_forecast_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                        int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                        const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                        const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        int horizon, const int *origins, int n_origins, int tracks_per_pass, double *m_fc, double *S_fc,
                                        double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss) {
    return forecast_given("ffvd_op_forecast_grouped", MG_METHOD_MOMENT, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D, logvariances,
                          loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J, Y_obs, m_pred,
                          S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix, lpd_gauss,
                          horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix, fc_lpd_gauss);
}

// The same on the collapsed posteriors of ffvd_op_posterior_grouped (as ffvd_op_posterior_filter_grouped): they never leave the device
extern "C" int ffvd_op_posterior_forecast_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                  const double *logvariances, const double *loglengthscales, const double *Xs,
                                                  const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                  int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                  const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                  const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                  double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                  double *lpd_gauss, double *U_means, int horizon, const int *origins, int n_origins,
                                                  int tracks_per_pass, double *m_fc, double *S_fc, double *fc_y_mean,
                                                  double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss) {
    return forecast_posterior("ffvd_op_posterior_forecast_grouped", MG_METHOD_MOMENT, kind, G, n_models, Zs, M, P, D, logvariances,
                              loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, CC,
                              DD, noise_std, J, Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean,
                              y_var_total, lpd_mix, lpd_gauss, U_means, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean,
                              fc_y_var_total, fc_lpd_mix, fc_lpd_gauss);
}

// The two calls above with the linearised (extended Kalman) rule for the filter and for the tracks (moment_linear_fan.hip)
extern "C" int ffvd_op_forecast_linear_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                        int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                        const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                        const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        int horizon, const int *origins, int n_origins, int tracks_per_pass, double *m_fc, double *S_fc,
                                        double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss) {
    return forecast_given("ffvd_op_forecast_linear_grouped", MG_METHOD_LINEAR, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                          logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J,
                          Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                          lpd_gauss, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix,
                          fc_lpd_gauss);
}

extern "C" int ffvd_op_posterior_forecast_linear_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                  const double *logvariances, const double *loglengthscales, const double *Xs,
                                                  const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                  int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                  const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                  const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                  double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                  double *lpd_gauss, double *U_means, int horizon, const int *origins, int n_origins,
                                                  int tracks_per_pass, double *m_fc, double *S_fc, double *fc_y_mean,
                                                  double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss) {
    return forecast_posterior("ffvd_op_posterior_forecast_linear_grouped", MG_METHOD_LINEAR, kind, G, n_models, Zs, M, P, D, logvariances,
                              loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, CC,
                              DD, noise_std, J, Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean,
                              y_var_total, lpd_mix, lpd_gauss, U_means, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean,
                              fc_y_var_total, fc_lpd_mix, fc_lpd_gauss);
}

// The same two calls with the third-degree spherical cubature rule for the filter (the cubature records launch with one record) and
// for the tracks (moment_cubature_fan.hip)
extern "C" int ffvd_op_forecast_cubature_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                        int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                        const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                        const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        int horizon, const int *origins, int n_origins, int tracks_per_pass, double *m_fc, double *S_fc,
                                        double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss) {
    return forecast_given("ffvd_op_forecast_cubature_grouped", MG_METHOD_CUBATURE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                          logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J,
                          Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                          lpd_gauss, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix,
                          fc_lpd_gauss);
}

extern "C" int ffvd_op_posterior_forecast_cubature_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                  const double *logvariances, const double *loglengthscales, const double *Xs,
                                                  const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                  int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                  const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                  const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                  double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                  double *lpd_gauss, double *U_means, int horizon, const int *origins, int n_origins,
                                                  int tracks_per_pass, double *m_fc, double *S_fc, double *fc_y_mean,
                                                  double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss) {
    return forecast_posterior("ffvd_op_posterior_forecast_cubature_grouped", MG_METHOD_CUBATURE, kind, G, n_models, Zs, M, P, D, logvariances,
                              loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, CC,
                              DD, noise_std, J, Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean,
                              y_var_total, lpd_mix, lpd_gauss, U_means, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean,
                              fc_y_var_total, fc_lpd_mix, fc_lpd_gauss);
}

// The same two calls with the bootstrap particle filter over the record (the particle records launch with one record) and N equally
// weighted particles per track, propagated without weighting or resampling (moment_particle_fan.hip).  The draws are the caller's:
// the filter's eps [G or 1][steps][N][D], unif [G or 1][steps], xi0 [G or 1][N][D] (with S0s) with a group stride each, the forecast's
// eps_fc [G or 1][B or 1][horizon][N][D] with a group and an origin stride (in doubles; 0 = shared).  cross, m_smooth and S_smooth
// must be NULL.
#define FFVD_PARTICLE_FC_PARAMS                                                                                                              \
    int N, const double *eps, long long eps_stride_g, const double *unif, long long unif_stride_g, const double *xi0,                       \
        long long xi0_stride_g, const double *eps_fc, long long eps_fc_stride_g, long long eps_fc_stride_b
#define FFVD_PARTICLE_FC_REQ                                                                                                                 \
    const ParticleFcReq pf {                                                                                                                 \
        ParticleReq{N, eps, eps_stride_g, 0, unif, unif_stride_g, 0, xi0, xi0_stride_g, 0, ess, log_evidence, nullptr, nullptr}, eps_fc,     \
            eps_fc_stride_g, eps_fc_stride_b, fc_lpd, fc_particles                                                                           \
    }
extern "C" int ffvd_op_forecast_particle_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                        int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                        const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                        const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        int horizon, const int *origins, int n_origins, int tracks_per_pass, FFVD_PARTICLE_FC_PARAMS,
                                        double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                                        double *fc_lpd_gauss, double *ess, double *log_evidence, double *fc_lpd, double *fc_particles) {
    FFVD_PARTICLE_FC_REQ;
    return forecast_given("ffvd_op_forecast_particle_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                          logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J,
                          Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                          lpd_gauss, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix,
                          fc_lpd_gauss, &pf);
}

extern "C" int ffvd_op_posterior_forecast_particle_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                  const double *logvariances, const double *loglengthscales, const double *Xs,
                                                  const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                  int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                  const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                  const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                  double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                  double *lpd_gauss, double *U_means, int horizon, const int *origins, int n_origins,
                                                  int tracks_per_pass, FFVD_PARTICLE_FC_PARAMS, double *m_fc, double *S_fc,
                                                  double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss,
                                                  double *ess, double *log_evidence, double *fc_lpd, double *fc_particles) {
    FFVD_PARTICLE_FC_REQ;
    return forecast_posterior("ffvd_op_posterior_forecast_particle_grouped", MG_METHOD_PARTICLE, kind, G, n_models, Zs, M, P, D, logvariances,
                              loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, CC,
                              DD, noise_std, J, Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean,
                              y_var_total, lpd_mix, lpd_gauss, U_means, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean,
                              fc_y_var_total, fc_lpd_mix, fc_lpd_gauss, &pf);
}

// The same two calls with the fully adapted particle filter over the record and the adapted tracks (moment_particle_adapted_fan.hip):
// the argument lists, the draws and the checks of the two calls above.  A track starts from the filter's equally weighted filtered
// set after its origin; m_fc / S_fc / fc_lpd are the filter's Rao-Blackwellised prediction expressions at every horizon.
namespace {
const char *const mg_afc_se_only =
    " (the adapted particle forecasts are built for the SE kernel only: their kernel rows are SE-ARD's)";
}
#define FFVD_PARTICLE_AFC_REQ                                                                                                                \
    ParticleFcReq pf {                                                                                                                       \
        ParticleReq{N, eps, eps_stride_g, 0, unif, unif_stride_g, 0, xi0, xi0_stride_g, 0, ess, log_evidence, nullptr, nullptr}, eps_fc,     \
            eps_fc_stride_g, eps_fc_stride_b, fc_lpd, fc_particles                                                                           \
    };                                                                                                                                       \
    pf.adapted = true;                                                                                                                       \
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, std::string(who) + ": bad argument" + mg_afc_se_only)
extern "C" int ffvd_particle_adapted_forecast_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M, int P,
                                        int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                        const double *const *q_sqrts, int q_mode, const double *x_lasts, const double *S0s,
                                        const double *ctrl, int C, int steps, const double *log_Qs, const double *CC, const double *DD,
                                        const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                        double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint, double *m_smooth,
                                        double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix, double *lpd_gauss,
                                        int horizon, const int *origins, int n_origins, int tracks_per_pass, FFVD_PARTICLE_FC_PARAMS,
                                        double *m_fc, double *S_fc, double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix,
                                        double *fc_lpd_gauss, double *ess, double *log_evidence, double *fc_lpd, double *fc_particles) {
    const char *who = "ffvd_particle_adapted_forecast_grouped";
    FFVD_PARTICLE_AFC_REQ;
    return forecast_given(who, MG_METHOD_PARTICLE, kind, G, n_models, Lm_inverse_seqs, Zs, M, P, D,
                          logvariances, loglengthscales, fs, q_sqrts, q_mode, x_lasts, S0s, ctrl, C, steps, log_Qs, CC, DD, noise_std, J,
                          Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean, y_var_total, lpd_mix,
                          lpd_gauss, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean, fc_y_var_total, fc_lpd_mix,
                          fc_lpd_gauss, &pf);
}

extern "C" int ffvd_posterior_particle_adapted_forecast_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                  const double *logvariances, const double *loglengthscales, const double *Xs,
                                                  const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                  int groups_per_pass, int q_mode, const double *x0s, const double *S0s,
                                                  const double *ctrl_roll, int steps, const double *CC, const double *DD,
                                                  const double *noise_std, int J, const double *Y_obs, double *m_pred, double *S_pred,
                                                  double *m_filt, double *S_filt, double *cross, double *lpd, double *lpd_joint,
                                                  double *m_smooth, double *S_smooth, double *y_mean, double *y_var_total, double *lpd_mix,
                                                  double *lpd_gauss, double *U_means, int horizon, const int *origins, int n_origins,
                                                  int tracks_per_pass, FFVD_PARTICLE_FC_PARAMS, double *m_fc, double *S_fc,
                                                  double *fc_y_mean, double *fc_y_var_total, double *fc_lpd_mix, double *fc_lpd_gauss,
                                                  double *ess, double *log_evidence, double *fc_lpd, double *fc_particles) {
    const char *who = "ffvd_posterior_particle_adapted_forecast_grouped";
    FFVD_PARTICLE_AFC_REQ;
    return forecast_posterior(who, MG_METHOD_PARTICLE, kind, G, n_models, Zs, M, P, D, logvariances,
                              loglengthscales, Xs, ctrl_fit, C, T, log_Qs, jitter, groups_per_pass, q_mode, x0s, S0s, ctrl_roll, steps, CC,
                              DD, noise_std, J, Y_obs, m_pred, S_pred, m_filt, S_filt, cross, lpd, lpd_joint, m_smooth, S_smooth, y_mean,
                              y_var_total, lpd_mix, lpd_gauss, U_means, horizon, origins, n_origins, tracks_per_pass, m_fc, S_fc, fc_y_mean,
                              fc_y_var_total, fc_lpd_mix, fc_lpd_gauss, &pf);
}
#undef FFVD_PARTICLE_AFC_REQ
#undef FFVD_PARTICLE_FC_PARAMS
#undef FFVD_PARTICLE_FC_REQ

// The summary of the moment-matched prediction for stacks the caller holds: they are uploaded, summarised by the same launch as in the
// calls above
extern "C" int ffvd_op_moment_summary(const double *m_x, const double *S_x, int G, int steps, int D, const double *CC, const double *DD,
                                      const double *noise_std, int J, const double *Y_test, int n_test, double *y_mean, double *y_var,
                                      double *y_var_total, double *lpd, double *lpd_gauss) {
    const std::string who = "ffvd_op_moment_summary", bad = who + ": bad argument";
    const SummaryReq q{CC, DD, noise_std, J, Y_test, n_test, y_mean, y_var, y_var_total, lpd, lpd_gauss};
    if (!summary_scalars_ok(q, G, steps, D) || D > MG_MAXD || (G > 0 && steps > 0 && G > ((1LL << 31) - 1) / steps / D / D))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || steps == 0) return FFVD_OK;
    if (!m_x || !S_x || !summary_arrays_ok(q)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    const size_t n = (size_t)G * steps * D;
    double *dm = sc.upload(m_x, n), *dS = sc.upload(S_x, n * D);
    OP_CHECK(dm && dS, who);
    return mg_summary(sc, who, dm, dS, G, steps, D, q);
}

// ---- linearisation of the transition (transition_grad.h) ------------------------------------------------------------------------------
// conditional_after_kernel_precalculation (conditionals_multi_output.py:306-387, white=True, full_cov=False) and its gradient with
// respect to the rows of Xnew, SE-ARD only: values and gradients from K(Xnew, Z), beta and Gamma (the moment family's staging).
namespace {
struct TgOut {
    double *means, *vars, *dmeans, *dvars, *mix_mean, *mix_var, *mix_dmean, *mix_dvar;
    bool var_side() const { return vars || dvars || mix_var || mix_dvar; }
};
// at least one output; the mixture values both or neither; mixture gradients only together with the mixture values
bool tg_outputs_ok(const TgOut &o) {
    return (o.means || o.vars || o.dmeans || o.dvars || o.mix_mean || o.mix_var || o.mix_dmean || o.mix_dvar) && (!o.mix_mean == !o.mix_var) &&
           (!(o.mix_dmean || o.mix_dvar) || o.mix_mean);
}
// scalar-argument checks shared by the two entry points (before any device call): cg_scalars_ok and G * D * N * P < 2^31
bool tg_scalars_ok(int kind, int G, int n_models, int M, int P, int D, int N, int q_mode, int rows_per_pass) {
    return cg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass) && (long long)G * D * N * P < (1LL << 31);
}
const char *const tg_se_only = " (the input gradients are closed-form for the SE kernel only)";

// Operands on the device -> beta, Gamma, the launches of transition_grad.h, the mixtures, the downloads.  dW: [nm * D] slots of
// Mp x Mp (zero padded); dq: nullptr or the q slots of BetaGamma; dZ: [nm][M][P]; hv per (model, dim).
int tg_run(Scratch &sc, const std::string &who, int G, int nm, int M, int P, int D, int N, int rows_per_pass, const HyperView &hv,
           const double *dZ, const double *dW, const double *dq, int q_mode, const double *dU, const double *dX, const TgOut &o) {
    const int Mp = round_up(M, NB);
    const size_t out_n = (size_t)G * N * D, ND = (size_t)N * D;
    TransitionGradArgs a{};
    a.G = G; a.n_models = nm; a.M = M; a.Mp = Mp; a.P = P; a.D = D; a.N = N;
    a.rows_per_pass = rows_per_pass > 0 ? rows_per_pass : cg_rows_per_pass(nm, D, Mp);
    a.unit_per_group = dq ? 1 : 0; a.need_var = o.var_side() ? 1 : 0;
    BetaGamma bg{};
    const bool terms = bg.alloc(sc, G, nm, D, Mp, dq, q_mode, a.need_var);
    const TransitionGradScratch need = tg_scratch_doubles(G, nm, D, P, Mp, N, a.rows_per_pass, bg.units, a.need_var);
    a.hv = hv; a.Z = dZ; a.beta = bg.beta; a.gam = bg.gam; a.x = dX;
    a.K = sc.alloc<double>(need.K); a.msum = sc.alloc<double>(need.msum); a.vpart = need.vpart ? sc.alloc<double>(need.vpart) : nullptr;
    a.mean = sc.alloc<double>(out_n); a.dmean = sc.alloc<double>(out_n * P);
    a.var = a.need_var ? sc.alloc<double>(out_n) : nullptr; a.dvar = a.need_var ? sc.alloc<double>(out_n * P) : nullptr;
    double *dmm = o.mix_mean ? sc.alloc<double>(ND) : nullptr, *dmv = o.mix_mean ? sc.alloc<double>(ND) : nullptr;
    double *dmdm = o.mix_dmean || o.mix_dvar ? sc.alloc<double>(ND * P) : nullptr, *dmdv = o.mix_dvar ? sc.alloc<double>(ND * P) : nullptr;
    OP_CHECK(terms && a.K && a.msum && (!need.vpart || a.vpart) && a.mean && a.dmean && (!a.need_var || (a.var && a.dvar)) &&
             (!o.mix_mean || (dmm && dmv)) && (!(o.mix_dmean || o.mix_dvar) || dmdm) && (!o.mix_dvar || dmdv), who);
    if (int rc = bg.launch(sc, G, nm, M, D, Mp, hv.len, dW, dq, q_mode, dU)) return rc;
    launch_transition_grad(sc.stream, a);
    if (o.mix_mean) launch_cg_mixture(sc.stream, a.mean, a.var, G, ND, dmm, dmv);
    if (dmdm) launch_tg_mixture(sc.stream, a.mean, a.dmean, a.dvar, dmm, G, ND, P, dmdm, dmdv);
    OP_TRY(hipGetLastError());
    auto down = [&](double *dst, const double *src, size_t n) { return !dst || sc.download(dst, src, n * sizeof(double)); };
    if (!down(o.means, a.mean, out_n) || !down(o.vars, a.var, out_n) || !down(o.dmeans, a.dmean, out_n * P) || !down(o.dvars, a.dvar, out_n * P) ||
        !down(o.mix_mean, dmm, ND) || !down(o.mix_var, dmv, ND) || !down(o.mix_dmean, dmdm, ND * P) || !down(o.mix_dvar, dmdv, ND * P))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    OP_TRY(hipStreamSynchronize(sc.stream));
    return FFVD_OK;
}
}  // namespace

// Posteriors given by the caller (also explicit-U models and SG-HMC samples of U: q_sqrts = NULL)
extern "C" int ffvd_op_conditional_grad_grouped(int kind, int G, int n_models, const double *const *Lm_inverse_seqs, const double *Zs, int M,
                                                int P, int D, const double *logvariances, const double *loglengthscales, const double *fs,
                                                const double *const *q_sqrts, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                                double *means, double *vars, double *dmeans, double *dvars, double *mix_mean,
                                                double *mix_var, double *mix_dmean, double *mix_dvar) {
    const std::string who = "ffvd_op_conditional_grad_grouped", bad = who + ": bad argument";
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + tg_se_only);
    if (!tg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass)) return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || N == 0) return FFVD_OK;
    const TgOut out{means, vars, dmeans, dvars, mix_mean, mix_var, mix_dmean, mix_dvar};
    if (!Lm_inverse_seqs || !Zs || !logvariances || !loglengthscales || !fs || !Xnew || !tg_outputs_ok(out))
        return set_error(nullptr, FFVD_EINVAL, bad);
    const size_t nK = (size_t)n_models * D, nq = given_nq(q_sqrts, q_mode, G, D);
    if (!given_tables_ok(Lm_inverse_seqs, nK, q_sqrts, nq)) return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    const int Mp = round_up(M, NB);
    const bool with_q = nq && out.var_side();                    // (the q slices enter the variance alone)
    double *dW = upload_matrix_table(sc, Lm_inverse_seqs, nK, M, Mp), *dq = with_q ? upload_matrix_table(sc, q_sqrts, nq, M, Mp) : nullptr;
    GroupHypers gh = stage_group_hypers(sc, kind, n_models, D, M, Mp, P, Zs, logvariances, loglengthscales);
    double *dU = sc.upload(fs, (size_t)G * D * M), *dX = sc.upload(Xnew, (size_t)N * P);
    OP_CHECK(dW && (!with_q || dq) && dU && dX && gh.logs(sc) && gh.blocks(sc), who);
    gh.prep(sc.stream);
    return tg_run(sc, who, G, n_models, M, P, D, N, rows_per_pass, gh.hv(), gh.dZ, dW, dq, q_mode, dU, dX, out);
}

// The collapsed posteriors of ffvd_op_posterior_grouped (base_model.py:243-256) linearised at Xnew without leaving the device: L^-T is
// packed from the K_uu slabs, U_mean read where the matvec left it, the q slices packed by launch_pg_pack (as the moment family)
extern "C" int ffvd_op_posterior_conditional_grad_grouped(int kind, int G, int n_models, const double *Zs, int M, int P, int D,
                                                          const double *logvariances, const double *loglengthscales, const double *Xs,
                                                          const double *ctrl_fit, int C, int T, const double *log_Qs, double jitter,
                                                          int groups_per_pass, int q_mode, const double *Xnew, int N, int rows_per_pass,
                                                          double *means, double *vars, double *dmeans, double *dvars, double *mix_mean,
                                                          double *mix_var, double *mix_dmean, double *mix_dvar, double *U_means) {
    const std::string who = "ffvd_op_posterior_conditional_grad_grouped", bad = who + ": bad argument";
    if (kind != FFVD_KERNEL_SE) return set_error(nullptr, FFVD_EINVAL, bad + tg_se_only);
    if (!pg_scalars_ok(kind, G, n_models, M, P, D, C, T, groups_per_pass, jitter) ||
        !tg_scalars_ok(kind, G, n_models, M, P, D, N, q_mode, rows_per_pass))
        return set_error(nullptr, FFVD_EINVAL, bad);
    if (G == 0 || N == 0) return FFVD_OK;
    const TgOut out{means, vars, dmeans, dvars, mix_mean, mix_var, mix_dmean, mix_dvar};
    if (!Zs || !logvariances || !loglengthscales || !Xs || !log_Qs || !Xnew || !tg_outputs_ok(out) || (C > 0 && !ctrl_fit))
        return set_error(nullptr, FFVD_EINVAL, bad);
    OP_BEGIN(who);
    const PgIn in{who, kind, G, n_models, M, P, D, C, T, groups_per_pass, Zs, logvariances, loglengthscales, Xs, ctrl_fit, log_Qs, jitter};
    PgWork w{};
    const int Mp = round_up(M, NB), nK = n_models * D;
    const size_t mm = (size_t)Mp * Mp;
    const bool need_q = out.var_side(), have_q = need_q && pg_want_q(sc, w, q_mode, G, D, M);
    double *dW = sc.alloc<double>((size_t)nK * mm), *dX = sc.upload(Xnew, (size_t)N * P);
    OP_CHECK(dW && dX && (!need_q || have_q), who);
    if (int rc = pg_posterior(sc, in, w)) return rc;
    double *dZ = sc.upload(Zs, (size_t)n_models * M * P);
    OP_CHECK(dZ, who);
    launch_pg_pack(sc.stream, w.Kuu, 2 * mm, Mp, Mp, nK, 1, M, 1, dW, Mp, Mp, nK);
    if (int rc = tg_run(sc, who, G, n_models, M, P, D, N, rows_per_pass, w.hv, dZ, dW, need_q ? pg_q(w, q_mode) : nullptr, q_mode, w.U, dX, out))
        return rc;
    if (U_means && !sc.download(U_means, w.U, (size_t)G * D * M * sizeof(double)))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    return FFVD_OK;
}
