// Fully adapted particle filtering of many observed records in one call ("Adapted particle filtering"): the
// records filter of moment_particle_records.hip with the optimal proposal in place of the bootstrap one (the fully adapted auxiliary
// particle filter of Pitt & Shephard 1999).  Given the parent particle the transition is Gaussian with a diagonal covariance and the
// emission is linear-Gaussian, so p(y_t | x_{t-1}^i) and p(x_t | x_{t-1}^i, y_t) are closed forms: the parents are weighted by how
// well they predict y_t BEFORE anything is drawn, resampled, and the children are drawn from the optimal proposal; the new set is
// equally weighted.  A TRACK (group g, record r) carries N particles.  Per row s, with X the equally weighted set carried into the
// row, c the record's control row and (mean_i, v_i) the GP conditional of the group at [X_i, c]:
//   mu_i = X_i + mean_i,  s_i = v_i + Q                          (per dim; trans_mean and trans_var of the smoothing call)
//   m_pred = sum_i mu_i / N,  S_pred = sum_i (mu_i - m_pred)(mu_i - m_pred)^T / N + diag(sum_i s_i / N)    (no draw enters)
//   lpd_j = log mean_i N(y_sj; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + sd_j^2), the largest exponent subtracted
//   per particle, from (m, P) = (mu_i, diag s_i) and L_i = 0, over the OBSERVED j in ascending order (mg_update's scalar updates):
//     h = P c_j,  sig2 = c_j . h + sd_j^2,  r = y_sj - (c_j . m + DD_j),  L_i += -1/2 (log 2 pi + log sig2 + r^2 / sig2),
//     m += h (r / sig2),  P_ab -= h_a h_b / sig2 (the upper triangle; the lower is its mirror)            -> mt_i, P_i
//   lpd_joint = log mean_i exp L_i,  W_i = exp(L_i - max L),  ess = (sum W)^2 / sum W^2,
//   m_filt = sum W mt / sum W,  S_filt = sum W (P_i + (mt_i - m_filt)(mt_i - m_filt)^T) / sum W,
//   systematic resampling of the PARENTS, the bootstrap kernel's own (cdf, thresholds (u + i) / N tot, binary search, clamp): a_i,
//   X'_i = mt_{a_i} + chol(P_{a_i}) eps[s, i]                    (unpivoted lower factor, a pivot <= 0 gives a zero column).
// A row with nothing observed takes the bootstrap kernel's expression X_i + mean_i + eps[s, i] sqrt(v_i + Q) with a_i = i, W = 1,
// ess = N and (m_filt, S_filt) = (m_pred, S_pred) bit for bit; the branch is uniform per track.
// particles[s] is X' -- the equally weighted FILTERED set after row s, not the bootstrap filter's X^- -- and ancestors[s, i] indexes
// the set carried INTO row s.
//
// Three launches per step for all tracks of a pass, as the bootstrap filter: the weight kernel below, then the bootstrap unit's rows
// kernel and the fp64-MFMA product, both unchanged.
//   mg_parec_weight_kernel (VALU, 256 threads, workgroup = track of the pass): finishes step t - 1 from what the previous launches
//     left (pmean, the column-tile partials in ascending tile order) and writes the next state into the other half of xstate.
//     Between the weighting and the draw only (mu, s) of every parent are kept (2 D N doubles per track, MomentParticleAdaptedArgs);
//     the scalar updates are run again where (mt, P) are needed -- for the weighted mean, for the weighted covariance and, after
//     the gather, for the parent a_i -- instead of keeping (D + D (D + 1) / 2) N doubles per track.
// No atomics, vector stores only, nothing waits on another workgroup; every reduction and the scan run in the bootstrap kernel's
// fixed orders (a thread's particles ascending, a 64-lane butterfly, the four wavefronts ascending).  The one address that depends on
// computed values is the parent's: the ancestor index is clamped into [0, N) before it is used, whatever the weights are.
#include "moment_step.h"

namespace ffvd {
namespace {

constexpr int PAREC_RED = MG_MAXD * (MG_MAXD + 1) / 2;    // the widest reduction: the upper triangle of a covariance

// out[k] <- (the sum of v[k] over the workgroup) / div, in LDS: wavefront butterflies, then the four wavefronts in ascending order.
// The results stay in LDS, not in registers: they are uniform, and the passes between which they live are register-bound at D = 8.
template <int K>
__device__ __forceinline__ void parec_sum(const double (&v)[K], double (*red)[PAREC_RED], double *out, const double div) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = v[k];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s += __shfl_xor(s, mm);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) out[threadIdx.x] = (((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]) / div;
    __syncthreads();
}

template <int K>
__device__ __forceinline__ void parec_max(const double (&v)[K], double (*red)[PAREC_RED], double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = v[k];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s = fmax(s, __shfl_xor(s, mm));
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) out[threadIdx.x] = fmax(fmax(red[0][threadIdx.x], red[1][threadIdx.x]), fmax(red[2][threadIdx.x], red[3][threadIdx.x]));
    __syncthreads();
}

// entry (lo <= hi) of an upper triangle stored row by row
__device__ __forceinline__ constexpr int parec_tri(int D, int lo, int hi) { return lo * D - lo * (lo - 1) / 2 + (hi - lo); }

// The exact scalar updates of one particle over the observed outputs in ascending j: (m, P) <- (mu, diag s) conditioned on the row;
// returns L = log p(y | parent).  hs .. ys: the emission and the row of Y in LDS.  P is the upper triangle.
template <int D>
__device__ __forceinline__ double parec_update(const double (&mu)[D], const double (&sv)[D], const int J, const double (*hs)[MG_MAXD],
                                               const double *dds, const double *s2s, const double *ys, double (&m)[D],
                                               double (&P)[D * (D + 1) / 2]) {
#pragma unroll
    for (int k = 0; k < D * (D + 1) / 2; ++k) P[k] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        m[d] = mu[d];
        P[parec_tri(D, d, d)] = sv[d];
    }
    double L = 0.0;
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
        const double y = ys[j];
        if (y != y) continue;                                     // unobserved: skipped by the whole workgroup
        double c[D], h[D];
#pragma unroll
        for (int d = 0; d < D; ++d) c[d] = hs[j][d];
        double sig2 = 0.0, hm = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < D; ++q) v += P[r < q ? parec_tri(D, r, q) : parec_tri(D, q, r)] * c[q];
            h[r] = v;                                             // P c
        }
#pragma unroll
        for (int r = 0; r < D; ++r) {
            sig2 += c[r] * h[r];
            hm += c[r] * m[r];
        }
        sig2 += s2s[j];
        const double e = y - (hm + dds[j]);
        L += -0.5 * (LOG_2PI + log(sig2) + e * e / sig2);
        const double g = e / sig2;
#pragma unroll
        for (int r = 0; r < D; ++r) m[r] += h[r] * g;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) P[parec_tri(D, lo, hi)] -= h[lo] * h[hi] / sig2;
    }
    return L;
}

// Launch t of steps + 1.  a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout with N rows per track; p.xstate:
// [2][tracks][N][D] (step parity), p.pmean: [tracks][D][N]; q.mu, q.sv: [tracks][N][D].
template <int D>
__global__ __launch_bounds__(256) void mg_parec_weight_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentRecordArgs rc,
                                                              MomentLinearFanArgs l, MomentParticleArgs p, MomentParticleAdaptedArgs q) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double Wl[MG_PREC_MAXN], cdf[MG_PREC_MAXN];
    __shared__ double red[4][PAREC_RED], Lm[MG_MAXD][MG_MAXD], Sg[MG_MAXD][MG_MAXD];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], vard[MG_MAXD], Qd[MG_MAXD], wtot[4];
    __shared__ double mps[MG_MAXD], sbs[MG_MAXD], mfs[MG_MAXD], mxs[MG_MAXJ + 1], ses[MG_MAXJ], sws[2], sps[PAREC_RED], sfs[PAREC_RED];
    const int tid = threadIdx.x;
    const int G = a.G, steps = a.steps, N = p.N, J = f.J;
    const int v = blockIdx.x;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;                     // (r < R: the host sizes the passes)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);                                      // the track's first row in the K blocks of its units
    const size_t vg = (size_t)gq * rc.R + r, orow = vg * steps;                   // the track of the call; its first row in the stacks
    double *Xn = p.xstate + ((size_t)(t & 1) * G + v) * N * D;

    if (t == 0) {                                                 // the start: the bootstrap kernel's, by the same expressions
        if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[vg * D * D + tid] : 0.0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (tid < D) {
                double pv = Sg[j][j], s = Sg[tid][j];
                for (int k = 0; k < j; ++k) { pv -= Lm[j][k] * Lm[j][k]; s -= Lm[tid][k] * Lm[j][k]; }
                double e = 0.0;
                if (pv > 0.0 && tid >= j) {
                    const double qq = sqrt(pv);
                    e = tid == j ? qq : s / qq;
                }
                Lm[tid][j] = e;
            }
            __syncthreads();
        }
        const double *xi = a.S0 ? p.xi0 + (size_t)gq * p.xi0_g + (size_t)r * p.xi0_r : nullptr;
        for (int i = tid; i < N; i += 256) {
            double z[D];
#pragma unroll
            for (int c = 0; c < D; ++c) z[c] = xi ? xi[(size_t)i * D + c] : 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c <= k; ++c) s += Lm[k][c] * z[c];
                Xn[(size_t)i * D + k] = a.x_last[vg * D + k] + s;
            }
        }
        return;
    }

    const int s = t - 1;                                          // the step this launch finishes, the row of Y it conditions on
    const double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;              // X_s, the set carried into the row (read only)
    double *Mu = q.mu + (size_t)v * N * D, *Sv = q.sv + (size_t)v * N * D;
    if (tid < J * D) hs[tid / D][tid % D] = f.CC[(size_t)(tid % D) * J + tid / D];
    if (tid < J) {
        dds[tid] = f.DD[tid];
        s2s[tid] = f.sd[tid] * f.sd[tid];
        ys[tid] = f.Y[((size_t)r * steps + s) * J + tid];
    }
    if (tid < D) {
        vard[tid] = a.variance[(size_t)model * D + tid];
        Qd[tid] = exp(a.log_Q[(size_t)gq * D + tid]);
    }
    __syncthreads();
    bool any = false;
    for (int j = 0; j < J; ++j) any = any || ys[j] == ys[j];

    // pass A: (mu, s) of every parent, their sums, the predictive log-densities and their largest exponents; a row with nothing
    // observed draws here (a_i = i: no other particle is read)
    const double *ep = p.eps + (size_t)gq * p.eps_g + (size_t)r * p.eps_r + (size_t)s * N * D;
    const double *pm = p.pmean + (size_t)v * D * N;
    double *po = p.particles ? p.particles + (orow + s) * N * D : nullptr;
    double sm[D], ss[D], mx[MG_MAXJ + 1];
#pragma unroll
    for (int d = 0; d < D; ++d) sm[d] = ss[d] = 0.0;
#pragma unroll
    for (int j = 0; j <= MG_MAXJ; ++j) mx[j] = -__builtin_inf();
    for (int i = tid; i < N; i += 256) {
        double mu[D], sv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double *vp = l.vpart + (size_t)(l.shared ? d : gq * D + d) * l.ntj * l.Tp + row + i;
            double qf = 0.0;
            for (int tj = 0; tj < l.ntj; ++tj) qf += vp[(size_t)tj * l.Tp];        // column tiles in ascending order
            mu[d] = Xp[(size_t)i * D + d] + pm[(size_t)d * N + i];
            sv[d] = (vard[d] - qf) + Qd[d];
            Mu[(size_t)i * D + d] = mu[d];
            Sv[(size_t)i * D + d] = sv[d];
            sm[d] += mu[d];
            ss[d] += sv[d];
            if (!any) {                                           // the bootstrap kernel's X^-, by the same expression
                const double x = (Xp[(size_t)i * D + d] + pm[(size_t)d * N + i]) + ep[(size_t)i * D + d] * sqrt((vard[d] - qf) + Qd[d]);
                Xn[(size_t)i * D + d] = x;
                if (po) po[(size_t)i * D + d] = x;
            }
        }
        double L = 0.0;
        if (any) {
#pragma unroll
            for (int j = 0; j < MG_MAXJ; ++j)
                if (j < J && ys[j] == ys[j]) {
                    double hm = 0.0, s2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        hm += hs[j][d] * mu[d];
                        s2 += (hs[j][d] * hs[j][d]) * sv[d];
                    }
                    s2 += s2s[j];
                    const double e = ys[j] - (hm + dds[j]);
                    mx[j] = fmax(mx[j], -0.5 * (LOG_2PI + log(s2) + e * e / s2));
                }
            double m[D], P[NP];
            L = parec_update<D>(mu, sv, J, hs, dds, s2s, ys, m, P);
        }
        mx[MG_MAXJ] = fmax(mx[MG_MAXJ], L);
        Wl[i] = L;
    }
    parec_sum<D>(sm, red, mps, (double)N);                        // m_pred
    parec_sum<D>(ss, red, sbs, (double)N);                        // sum_i s_i / N
    parec_max<MG_MAXJ + 1>(mx, red, mxs);

    // pass B: the centred sums of S_pred and the densities
    {
        double sp[NP], se[MG_MAXJ], mp[D];
#pragma unroll
        for (int k = 0; k < NP; ++k) sp[k] = 0.0;
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j) se[j] = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) mp[d] = mps[d];
        for (int i = tid; i < N; i += 256) {
            double mu[D], sv[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                mu[d] = Mu[(size_t)i * D + d];
                sv[d] = Sv[(size_t)i * D + d];
            }
            int k = 0;
#pragma unroll
            for (int lo = 0; lo < D; ++lo)
#pragma unroll
                for (int hi = lo; hi < D; ++hi) sp[k++] += (mu[lo] - mp[lo]) * (mu[hi] - mp[hi]);
#pragma unroll
            for (int j = 0; j < MG_MAXJ; ++j)
                if (j < J && ys[j] == ys[j]) {
                    double hm = 0.0, s2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        hm += hs[j][d] * mu[d];
                        s2 += (hs[j][d] * hs[j][d]) * sv[d];
                    }
                    s2 += s2s[j];
                    const double e = ys[j] - (hm + dds[j]);
                    se[j] += exp(-0.5 * (LOG_2PI + log(s2) + e * e / s2) - mxs[j]);
                }
        }
        parec_sum<NP>(sp, red, sps, (double)N);
        parec_sum<MG_MAXJ>(se, red, ses, 1.0);
    }

    // pass C: the weights and the weighted sums of the conditioned means
    {
        double sw[2], wm[D];
#pragma unroll
        for (int d = 0; d < D; ++d) wm[d] = 0.0;
        sw[0] = sw[1] = 0.0;
        const double mxl = mxs[MG_MAXJ];
        for (int i = tid; i < N; i += 256) {
            double w = 1.0;
            if (any) {
                double mu[D], sv[D], m[D], P[NP];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    mu[d] = Mu[(size_t)i * D + d];
                    sv[d] = Sv[(size_t)i * D + d];
                }
                w = exp(Wl[i] - mxl);
                parec_update<D>(mu, sv, J, hs, dds, s2s, ys, m, P);
#pragma unroll
                for (int d = 0; d < D; ++d) wm[d] += w * m[d];
            }
            Wl[i] = w;
            sw[0] += w;
            sw[1] += w * w;
        }
        parec_sum<2>(sw, red, sws, 1.0);
        if (any) parec_sum<D>(wm, red, mfs, sws[0]);              // m_filt
    }

    // pass D: the weighted sums of S_filt (a row with nothing observed: the predicted moments, bit for bit)
    if (any) {
        double sf[NP], mf[D];
#pragma unroll
        for (int k = 0; k < NP; ++k) sf[k] = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) mf[d] = mfs[d];
        for (int i = tid; i < N; i += 256) {
            double mu[D], sv[D], m[D], P[NP];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                mu[d] = Mu[(size_t)i * D + d];
                sv[d] = Sv[(size_t)i * D + d];
            }
            parec_update<D>(mu, sv, J, hs, dds, s2s, ys, m, P);
#pragma unroll
            for (int d = 0; d < D; ++d) m[d] -= mf[d];
            const double w = Wl[i];
            int k = 0;
#pragma unroll
            for (int lo = 0; lo < D; ++lo)
#pragma unroll
                for (int hi = lo; hi < D; ++hi) {
                    sf[k] += w * (P[k] + m[lo] * m[hi]);
                    ++k;
                }
        }
        parec_sum<NP>(sf, red, sfs, sws[0]);
    }

    // the row's outputs, from the sums in LDS: thread k stores entry k; (lo, hi) and (hi, lo) store one value
    const double nan = __builtin_nan("");
    {
        const size_t o = orow + s;
        if (tid < D) {
            a.m_x[o * D + tid] = mps[tid];
            f.m_filt[o * D + tid] = any ? mfs[tid] : mps[tid];
        }
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) {
                if (tid == 64 + k) {
                    const double vp = lo == hi ? sps[k] + sbs[lo] : sps[k], vf = any ? sfs[k] : vp;
                    a.S_x[o * D * D + lo * D + hi] = vp;
                    a.S_x[o * D * D + hi * D + lo] = vp;
                    f.S_filt[o * D * D + lo * D + hi] = vf;
                    f.S_filt[o * D * D + hi * D + lo] = vf;
                }
                ++k;
            }
        if (tid >= 128 && tid < 128 + J) {
            const int j = tid - 128;
            f.lpd[o * J + j] = ys[j] == ys[j] ? mxs[j] + log(ses[j] / N) : nan;
        }
        if (tid == 192) {
            f.lpd_joint[o] = any ? mxs[MG_MAXJ] + log(sws[0] / N) : nan;
            p.ess[o] = any ? sws[0] * sws[0] / sws[1] : (double)N;
        }
    }

    // the scan: thread c sums its chunk of PT consecutive weights, the chunk totals are scanned by wavefront, then across the four
    const int PT = (N + 255) / 256, c0 = tid * PT;
    __syncthreads();
    double run = 0.0;
    for (int k = 0; k < PT; ++k)
        if (c0 + k < N) {
            run += Wl[c0 + k];
            cdf[c0 + k] = run;
        }
    const int lane = tid & 63, wave = tid >> 6;
    double inc = run;
#pragma unroll
    for (int mm = 1; mm < 64; mm <<= 1) {
        const double up = __shfl_up(inc, mm);
        if (lane >= mm) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    double base = inc - run;                                      // the chunks before this one in its wavefront
    for (int w = 0; w < wave; ++w) base += wtot[w];
    for (int k = 0; k < PT; ++k)
        if (c0 + k < N) cdf[c0 + k] += base;
    __syncthreads();                                              // (also: every (mu, s) of pass A is visible to the gather)

    // the ancestors, the gather of the parents' (mu, s) and the draw from the optimal proposal
    const double tot = cdf[N - 1];
    const double u0 = p.unif[(size_t)gq * p.unif_g + (size_t)r * p.unif_r + s];
    int *ao = p.ancestors ? p.ancestors + (orow + s) * N : nullptr;
    for (int i = tid; i < N; i += 256) {
        int an = i;
        if (any) {
            const double u = (u0 + i) / N * tot;
            int lo = 0, hi = N;
            while (lo < hi) {                                     // #{k: cdf_k <= u}: at most 12 rounds, whatever the values are
                const int mid = (lo + hi) >> 1;
                if (cdf[mid] <= u) lo = mid + 1;
                else hi = mid;
            }
            an = lo;
        }
        an = an < 0 ? 0 : an > N - 1 ? N - 1 : an;                // in [0, N) before any address is formed
        if (ao) ao[i] = an;
        if (!any) continue;                                       // (drawn in pass A)
        double mu[D], sv[D], m[D], P[NP], z[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            mu[d] = Mu[(size_t)an * D + d];
            sv[d] = Sv[(size_t)an * D + d];
            z[d] = ep[(size_t)i * D + d];
        }
        parec_update<D>(mu, sv, J, hs, dds, s2s, ys, m, P);
        // the unpivoted lower factor of P, column by column in place of the triangle: entry (lo, hi) holds L[hi][lo]
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double pv = P[parec_tri(D, j, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) pv -= P[parec_tri(D, k, j)] * P[parec_tri(D, k, j)];
            const bool ok = pv > 0.0;
            const double qq = sqrt(ok ? pv : 1.0);
#pragma unroll
            for (int c = j + 1; c < D; ++c) {
                double sc = P[parec_tri(D, j, c)];
#pragma unroll
                for (int k = 0; k < j; ++k) sc -= P[parec_tri(D, k, c)] * P[parec_tri(D, k, j)];
                P[parec_tri(D, j, c)] = ok ? sc / qq : 0.0;
            }
            P[parec_tri(D, j, j)] = ok ? qq : 0.0;
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double sc = 0.0;
#pragma unroll
            for (int c = 0; c <= k; ++c) sc += P[parec_tri(D, c, k)] * z[c];
            const double x = m[k] + sc;
            Xn[(size_t)i * D + k] = x;
            if (po) po[(size_t)i * D + k] = x;
        }
    }
}

}  // namespace

// a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout of the pass with N rows per track and its buffers
void launch_mg_parec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                          const MomentLinearFanArgs &l, const MomentParticleArgs &p, const MomentParticleAdaptedArgs &q, int t) {
    const dim3 grid((unsigned)a.G);
    switch (a.D) {
#define MG_CASE(d)                                                                                                                  \
    case d:                                                                                                                         \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_parec_weight_kernel<d>), grid, dim3(256), 0, stream, a, t, f, rc, l, p, q);           \
        break;
        MG_CASE(1) MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8)
#undef MG_CASE
        default: break;
    }
    if (t >= a.steps) return;
    launch_mg_prec_rows(stream, a, rc, l, p, t);
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

}  // namespace ffvd
