// The step-loop operators of the C ABI: posterior rollouts (ffvd_op_rollout) and the particle-Gibbs sweep (ffvd_op_pg_sweep).
#include "op_scratch.h"
#include "grad.h"

#include <atomic>

using namespace ffvd;

static std::atomic<int> g_rollout_fallbacks{0};     // ffvd_op_rollout calls of this process that fell back from the resident loop to the per-step launches

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
    OP_CHECK(words, who);
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
    OP_CHECK(dW && dxc && dxc2 && dU && dlq && deps && (!C || dctrl) && st.ok() && dpx && dpv && (!q_sqrt || (dQs && extra && F)) &&
             (!q_sqrt || !skinny || dWQ), "ffvd_op_rollout");
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
    OP_CHECK(dW && dxc && dU && dlq && deps && dun && (!C || dctrl) && dXr && dY && dCC && dDD && dR && st.ok() && dmean && dvar && cand &&
             dparts && didx, "ffvd_op_pg_sweep");
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
