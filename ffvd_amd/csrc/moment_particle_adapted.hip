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
// No atomics, vector stores only, nothing waits on another workgroup.  The start, the transition, the scan, the search and the
// reductions are the blocks of moment_particle.h that the bootstrap kernel calls (a thread's particles ascending, a 64-lane butterfly,
// the four wavefronts ascending); the sums end in LDS (wg_sum_lds), not in registers.  The one address that depends on computed values
// is the parent's: the ancestor index is clamped into [0, N) before it is used, whatever the weights are.
#include "moment_particle.h"

namespace ffvd {
namespace {

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
    __shared__ double red[4][PARTICLE_RED], Lm[MG_MAXD][MG_MAXD], Sg[MG_MAXD][MG_MAXD];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], vard[MG_MAXD], Qd[MG_MAXD], wtot[4];
    __shared__ double mps[MG_MAXD], sbs[MG_MAXD], mfs[MG_MAXD], mxs[MG_MAXJ + 1], ses[MG_MAXJ], sws[2], sps[PARTICLE_RED], sfs[PARTICLE_RED];
    const int tid = threadIdx.x;
    const int G = a.G, steps = a.steps, N = p.N, J = f.J;
    const int v = blockIdx.x;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;                     // (r < R: the host sizes the passes)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);                                      // the track's first row in the K blocks of its units
    const size_t vg = (size_t)gq * rc.R + r, orow = vg * steps;                   // the track of the call; its first row in the stacks
    double *Xn = p.xstate + ((size_t)(t & 1) * G + v) * N * D;

    if (t == 0) {
        particle_start<D>(a, p, gq, r, vg, Xn, Sg, Lm);
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
    particle_stage_noise<D>(a, model, gq, vard, Qd);
    __syncthreads();
    const bool any = particle_any_observed(ys, J);

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
            particle_transition<D>(l, gq, d, row, i, N, Xp, pm, vard[d], Qd[d], mu[d], sv[d]);
            Mu[(size_t)i * D + d] = mu[d];
            Sv[(size_t)i * D + d] = sv[d];
            sm[d] += mu[d];
            ss[d] += sv[d];
            if (!any) {                                           // the bootstrap kernel's X^-, from the same two values
                const double x = mu[d] + ep[(size_t)i * D + d] * sqrt(sv[d]);
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
    wg_sum_lds<D>(sm, red, mps, (double)N);                        // m_pred
    wg_sum_lds<D>(ss, red, sbs, (double)N);                        // sum_i s_i / N
    wg_max_lds<MG_MAXJ + 1>(mx, red, mxs);

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
        wg_sum_lds<NP>(sp, red, sps, (double)N);
        wg_sum_lds<MG_MAXJ>(se, red, ses, 1.0);
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
        wg_sum_lds<2>(sw, red, sws, 1.0);
        if (any) wg_sum_lds<D>(wm, red, mfs, sws[0]);              // m_filt
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
        wg_sum_lds<NP>(sf, red, sfs, sws[0]);
    }

    // the row's outputs, from the sums in LDS: thread k stores entry k
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

    particle_scan(Wl, cdf, N, wtot);                              // (also: every (mu, s) of pass A is visible to the gather)

    // the ancestors, the gather of the parents' (mu, s) and the draw from the optimal proposal
    const double tot = cdf[N - 1];
    const double u0 = p.unif[(size_t)gq * p.unif_g + (size_t)r * p.unif_r + s];
    int *ao = p.ancestors ? p.ancestors + (orow + s) * N : nullptr;
    for (int i = tid; i < N; i += 256) {
        const int an = any ? particle_search(cdf, N, (u0 + i) / N * tot) : i;
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
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_parec_weight_kernel<d>), grid, dim3(256), 0, stream, a, t, f, rc, l, p, q))
    if (t >= a.steps) return;
    launch_mg_prec_rows(stream, a, rc, l, p, t);
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

}  // namespace ffvd
