// The score operators of the C ABI (predict_score.h): CRPS, PIT and predictive quantiles of the equal-weight Gaussian mixture a
// stack of points (rollouts, particle sets) or of Gaussian states defines.  The stacks are uploaded as the caller holds them and are
// not scanned on the host: a component that is not finite makes the outputs of its targets NaN on the device and nothing else.
#include "op_scratch.h"
#include "predict_score.h"

#include <cmath>

using namespace ffvd;

namespace {
struct ScoreReq {
    const double *CC, *DD, *noise_std;           // D x J, J, J
    int J;
    const double *Y_test;                        // n_test x J or NULL
    int n_test;
    const double *levels;                        // Q or NULL
    int Q, targets_per_pass;
    double *crps, *pit, *quantiles;              // n_test x J, n_test x J, steps x J x Q; each may be NULL
};

int score_bad(const std::string &who, const std::string &what) { return set_error(nullptr, FFVD_EINVAL, who + ": bad argument: " + what); }

// the checks that read no array; K1, K2: the component axes (K = K1 * K2)
int score_scalars(const std::string &who, const ScoreReq &q, long long K1, long long K2, int steps, int D, int max_D) {
    if (K1 < 0 || K2 < 0 || K1 * K2 > PSC_MAXK || K1 > PSC_MAXK || K2 > PSC_MAXK)
        return score_bad(who, "the number of components K must lie in [1, " + std::to_string(PSC_MAXK) + "]");
    if (steps < 0) return score_bad(who, "steps must not be negative");
    if (D < 1 || D > max_D) return score_bad(who, "D must lie in [1, " + std::to_string(max_D) + "]");
    if (q.J < 1 || q.J > PSC_MAXJ) return score_bad(who, "J must lie in [1, " + std::to_string(PSC_MAXJ) + "]");
    if (q.Q < 0 || q.Q > PSC_MAXQ) return score_bad(who, "the number of levels Q must lie in [0, " + std::to_string(PSC_MAXQ) + "]");
    if (q.n_test < 0 || q.n_test > steps) return score_bad(who, "n_test must lie in [0, steps]");
    if (q.targets_per_pass < 0) return score_bad(who, "targets_per_pass must be 0 (automatic) or positive");
    const long long K = K1 * K2, lim = 1LL << 31;
    if (K > 0 && steps > 0 && ((long long)steps * q.J * K >= lim || (long long)steps * q.J * (q.Q > 0 ? q.Q : 1) >= lim))
        return score_bad(who, "steps * J * K and steps * J * Q must stay below 2^31");
    return FFVD_OK;
}

// the checks that read the small arrays (after the "nothing to do" return)
int score_arrays(const std::string &who, const ScoreReq &q) {
    if (!q.CC || !q.DD || !q.noise_std) return score_bad(who, "CC, DD and noise_std are needed");
    if (!q.crps && !q.pit && !q.quantiles) return score_bad(who, "at least one of crps, pit and quantiles is needed");
    if (q.n_test > 0 && (q.crps || q.pit) && !q.Y_test) return score_bad(who, "crps and pit need Y_test");
    if (q.quantiles && q.Q > 0 && !q.levels) return score_bad(who, "quantiles need levels");
    for (int j = 0; j < q.J; ++j)
        if (!std::isfinite(q.noise_std[j]) || !(q.noise_std[j] > 0.0)) return score_bad(who, "noise_std must be finite and positive");
    if (q.quantiles)
        for (int l = 0; l < q.Q; ++l)
            if (!(q.levels[l] >= 1e-9 && q.levels[l] <= 1.0 - 1e-9)) return score_bad(who, "every level must lie in [1e-9, 1 - 1e-9]");
    return FFVD_OK;
}

// The emission on the device, the staged mixture, then the launches of what was asked for and the downloads.  stage: fills a.mu
// (a.var, a.rs) from the uploaded stack.  Only the pair partials are bounded by passes: the staged arrays hold all steps * J * K
// entries at once (FFVD_ENOMEM before any launch when they do not fit; rows can be scored in slices, which changes no bit).
template <class Stage>
int score_run(Scratch &sc, const std::string &who, const ScoreReq &q, int K, int steps, int D, bool equal_var, Stage stage) {
    const size_t NT = (size_t)steps * q.J, TJ = (size_t)q.n_test * q.J;
    const bool want_crps = q.crps && TJ, want_pit = q.pit && TJ, want_q = q.quantiles && q.Q > 0;
    ScoreArgs a{};
    a.K = K; a.steps = steps; a.D = D; a.J = q.J; a.n_test = q.n_test; a.Q = q.Q; a.equal_var = equal_var ? 1 : 0;
    a.CC = sc.upload(q.CC, (size_t)D * q.J); a.DD = sc.upload(q.DD, q.J); a.sd = sc.upload(q.noise_std, q.J);
    a.Y = want_crps || want_pit ? sc.upload(q.Y_test, TJ) : nullptr;
    a.levels = want_q ? sc.upload(q.levels, q.Q) : nullptr;
    a.mu = sc.alloc<double>(NT * K);
    a.var = equal_var ? nullptr : sc.alloc<double>(NT * K);
    a.rs = equal_var ? nullptr : sc.alloc<double>(NT * K);
    const int tpp = psc_targets_per_pass(K, q.targets_per_pass);
    const size_t pass = TJ < (size_t)tpp ? TJ : (size_t)tpp;
    a.part = want_crps ? sc.alloc<double>(pass * psc_pairs(K)) : nullptr;
    a.crps = want_crps ? sc.alloc<double>(TJ) : nullptr;
    a.pit = want_pit ? sc.alloc<double>(TJ) : nullptr;
    a.quant = want_q ? sc.alloc<double>(NT * q.Q) : nullptr;
    OP_CHECK(a.CC && a.DD && a.sd && (!(want_crps || want_pit) || a.Y) && (!want_q || (a.levels && a.quant)) && a.mu &&
             (equal_var || (a.var && a.rs)) && (!want_crps || (a.part && a.crps)) && (!want_pit || a.pit), who);
    stage(a);
    if (want_crps)
        for (size_t first = 0; first < TJ; first += pass)
            launch_score_crps(sc.stream, a, (int)first, (int)(TJ - first < pass ? TJ - first : pass));
    if (want_pit) launch_score_pit(sc.stream, a);
    if (want_q) launch_score_quantiles(sc.stream, a);
    OP_TRY(hipGetLastError());
    auto down = [&](double *dst, const double *src, size_t n) { return sc.download(dst, src, n * sizeof(double)); };
    if ((want_crps && !down(q.crps, a.crps, TJ)) || (want_pit && !down(q.pit, a.pit, TJ)) || (want_q && !down(q.quantiles, a.quant, NT * q.Q)))
        return set_error(nullptr, FFVD_EDEVICE, who + ": copying the results back failed");
    return FFVD_OK;
}
}  // namespace

extern "C" int ffvd_score_points(const double *x, int K1, int K2, int steps, int D, long long stride_k1, long long stride_k2,
                                 long long stride_t, const double *CC, const double *DD, const double *noise_std, int J,
                                 const double *Y_test, int n_test, const double *levels, int Q, int targets_per_pass, double *crps,
                                 double *pit, double *quantiles) {
    const std::string who = "ffvd_score_points";
    const ScoreReq q{CC, DD, noise_std, J, Y_test, n_test, levels, Q, targets_per_pass, crps, pit, quantiles};
    if (int rc = score_scalars(who, q, K1, K2, steps, D, PSC_MAXD_POINTS)) return rc;
    if (stride_k1 < 0 || stride_k2 < 0 || stride_t < 0) return score_bad(who, "the strides must not be negative");
    if ((long long)K1 * K2 == 0 || steps == 0) return FFVD_OK;
    // the doubles the strides reach: the stack that is uploaded
    const long long lim = 1LL << 31;
    if (stride_k1 >= lim || stride_k2 >= lim || stride_t >= lim) return score_bad(who, "the stack's index products must stay below 2^31");
    const long long extent = (K1 - 1) * stride_k1 + (K2 - 1) * stride_k2 + (steps - 1) * stride_t + D;
    if (extent >= lim) return score_bad(who, "the stack's index products must stay below 2^31");
    if (!x) return score_bad(who, "x is needed");
    if (int rc = score_arrays(who, q)) return rc;
    OP_BEGIN(who);
    const double *dx = sc.upload(x, (size_t)extent);
    OP_CHECK(dx, who);
    return score_run(sc, who, q, K1 * K2, steps, D, true, [&](const ScoreArgs &a) {
        launch_score_stage_points(sc.stream, a, dx, K2, stride_k1, stride_k2, stride_t);
    });
}

extern "C" int ffvd_score_moments(const double *m_x, const double *S_x, int G, int steps, int D, const double *CC, const double *DD,
                                  const double *noise_std, int J, const double *Y_test, int n_test, const double *levels, int Q,
                                  int targets_per_pass, double *crps, double *pit, double *quantiles) {
    const std::string who = "ffvd_score_moments";
    const ScoreReq q{CC, DD, noise_std, J, Y_test, n_test, levels, Q, targets_per_pass, crps, pit, quantiles};
    if (int rc = score_scalars(who, q, G, 1, steps, D, PSC_MAXD_MOMENTS)) return rc;
    if (G == 0 || steps == 0) return FFVD_OK;
    if ((long long)G * steps * D * D >= (1LL << 31)) return score_bad(who, "G * steps * D * D must stay below 2^31");
    if (!m_x || !S_x) return score_bad(who, "m_x and S_x are needed");
    if (int rc = score_arrays(who, q)) return rc;
    OP_BEGIN(who);
    const size_t n = (size_t)G * steps * D;
    const double *dm = sc.upload(m_x, n), *dS = sc.upload(S_x, n * D);
    OP_CHECK(dm && dS, who);
    return score_run(sc, who, q, G, steps, D, false, [&](const ScoreArgs &a) { launch_score_stage_moments(sc.stream, a, dm, dS); });
}
