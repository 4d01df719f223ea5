// Particle filtering of many records with adaptive (ESS-triggered) resampling ("Adaptive resampling"): the
// bootstrap filter of moment_particle_records.hip carrying a WEIGHTED set.  A track carries the particles X and the log-weights a,
// whose largest entry is exactly 0 (a = 0 at the start).  Per step s, with e_i = exp(a_i) and A = sum_i e_i:
//   X^-_i = X_i + m_i + eps[s, i] sqrt(v_i + Q)                                  (the bootstrap kernel's expression)
//   m_pred = sum_i e_i X^-_i / A,  S_pred = sum_i e_i (X^-_i - m_pred)(X^-_i - m_pred)^T / A
//   lpd_j = max_i (a_i + l_ij) + log(sum_i exp(a_i + l_ij - max) / A),  b_i = a_i + sum_{j observed} l_ij,
//   lpd_joint = max b + log(sum_i exp(b_i - max b) / A),  W_i = exp(b_i - max b),  m_filt, S_filt: the W-weighted moments,
//   ess = (sum W)^2 / sum W^2,  weights_i = W_i / sum W;
//   ess < ess_threshold N: the bootstrap kernel's systematic resampling, then a <- 0;  otherwise X_i <- X^-_i, a_i <- b_i - max b.
// A row with nothing observed propagates and keeps a: ess = A^2 / sum e_i^2, weights_i = e_i / A, m_filt = m_pred, S_filt = S_pred.
// With a = 0 every e_i is 1 and A is N exactly, every product by e_i and every sum a_i + l is exact, and every sum is formed in the
// bootstrap kernel's order: with ess_threshold > 1 the launch stores what mg_prec_weight_kernel stores, bit for bit.
//
// Three launches per step for all tracks of a pass, as the bootstrap unit: this weight kernel (VALU, 256 threads, workgroup = track
// of the pass; the launch at t finishes step t - 1), the rows kernel (launch_mg_prec_rows) and the product kernel
// (launch_mg_lfan_var), both unchanged.  The log-weights of a pass live in global memory beside xstate: the launch at t = 0 writes
// them, thread i alone ever reads or writes entry i.  e_i is formed once per row and kept in the LDS array that the scan fills with
// the cdf afterwards (the scan starts behind a barrier and nothing reads e after pass B), so the kernel takes the bootstrap kernel's
// LDS.  No atomics, nothing waits on another workgroup, every sum and the scan have an order fixed by N alone; the one address that
// depends on computed values is the gather's, clamped into [0, N) by particle_search.  The decision is uniform: every thread holds
// the same sums.
#include "moment_particle.h"

namespace ffvd {
namespace {

// Launch t of steps + 1.  a.G, l, p: as mg_prec_weight_kernel; q.logw: [tracks][N].
template <int D>
__global__ __launch_bounds__(256) void mg_pess_weight_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentRecordArgs rc,
                                                             MomentLinearFanArgs l, MomentParticleArgs p, MomentParticleEssArgs q) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double Wl[MG_PREC_MAXN], cdf[MG_PREC_MAXN];
    __shared__ double red[4][PARTICLE_RED], Lm[MG_MAXD][MG_MAXD], Sg[MG_MAXD][MG_MAXD];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], lcs[MG_MAXJ], vard[MG_MAXD], Qd[MG_MAXD], wtot[4];
    const int tid = threadIdx.x;
    const int G = a.G, steps = a.steps, N = p.N, J = f.J;
    const int v = blockIdx.x;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;                     // (r < R: the host sizes the passes)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);                                      // the track's first row in the K blocks of its units
    const size_t vg = (size_t)gq * rc.R + r, orow = vg * steps;                   // the track of the call; its first row in the stacks
    double *Xn = p.xstate + ((size_t)(t & 1) * G + v) * N * D;
    double *lw = q.logw + (size_t)v * N;

    if (t == 0) {
        particle_start<D>(a, p, gq, r, vg, Xn, Sg, Lm);
        for (int i = tid; i < N; i += 256) lw[i] = 0.0;
        return;
    }

    const int s = t - 1;                                          // the step this launch finishes, the row of Y it emits
    double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;    // X_s, overwritten by X^-_s particle by particle
    double *ew = cdf;                                             // e_i until the scan
    particle_stage_emission<D>(f, f.Y + ((size_t)r * steps + s) * J, hs, dds, s2s, ys, lcs);
    particle_stage_noise<D>(a, model, gq, vard, Qd);
    __syncthreads();
    const bool any = particle_any_observed(ys, J);

    // pass A: X^-, e, the weighted sums of the mean, A and sum e^2, the log-weights b and the largest exponents
    const double *ep = p.eps + (size_t)gq * p.eps_g + (size_t)r * p.eps_r + (size_t)s * N * D;
    const double *pm = p.pmean + (size_t)v * D * N;
    double *po = p.particles ? p.particles + (orow + s) * N * D : nullptr;
    double sm[D + 2], mx[MG_MAXJ + 1];                            // sm[D] = A, sm[D + 1] = sum e^2
#pragma unroll
    for (int d = 0; d < D + 2; ++d) sm[d] = 0.0;
#pragma unroll
    for (int j = 0; j <= MG_MAXJ; ++j) mx[j] = -__builtin_inf();
    for (int i = tid; i < N; i += 256) {
        const double ai = lw[i], e = exp(ai);
        ew[i] = e;
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double tm, tv;
            particle_transition<D>(l, gq, d, row, i, N, Xp, pm, vard[d], Qd[d], tm, tv);
            x[d] = tm + ep[(size_t)i * D + d] * sqrt(tv);
            Xp[(size_t)i * D + d] = x[d];
            if (po) po[(size_t)i * D + d] = x[d];
            sm[d] += e * x[d];
        }
        sm[D] += e;
        sm[D + 1] += e * e;
        double L = 0.0;
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) {
                const double lj = particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs);
                mx[j] = fmax(mx[j], ai + lj);
                L += lj;
            }
        const double b = ai + L;
        mx[MG_MAXJ] = fmax(mx[MG_MAXJ], b);
        Wl[i] = b;
    }
    wg_sum<D + 2>(sm, red);
    wg_max<MG_MAXJ + 1>(mx, red);
    const double A = sm[D];
    double mp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) mp[d] = sm[d] / A;

    // pass B: the weighted centred sums of S_pred, the densities, the weights W, the weighted sums of the mean, the carried a
    double sp[NP], se[MG_MAXJ], sw[2], wm[D];
#pragma unroll
    for (int k = 0; k < NP; ++k) sp[k] = 0.0;
#pragma unroll
    for (int j = 0; j < MG_MAXJ; ++j) se[j] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) wm[d] = 0.0;
    sw[0] = sw[1] = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double e = ew[i];
        double x[D], xe[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = Xp[(size_t)i * D + d];
            xe[d] = e * (x[d] - mp[d]);                           // (e = 1: the difference itself)
        }
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) sp[k++] += xe[lo] * (x[hi] - mp[hi]);
        if (any) {
            const double ai = lw[i];
#pragma unroll
            for (int j = 0; j < MG_MAXJ; ++j)
                if (j < J && ys[j] == ys[j]) se[j] += exp((ai + particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs)) - mx[j]);
            const double na = Wl[i] - mx[MG_MAXJ], w = exp(na);
            lw[i] = na;                                           // (a resampling row stores zeros below)
            Wl[i] = w;
            sw[0] += w;
            sw[1] += w * w;
#pragma unroll
            for (int d = 0; d < D; ++d) wm[d] += w * x[d];
        }
    }
    wg_sum<NP>(sp, red);
    double my_sp = 0.0, my_sf = 0.0;                              // thread 64 + k keeps entry k of the upper triangles
#pragma unroll
    for (int k = 0; k < NP; ++k)
        if (tid == 64 + k) my_sp = sp[k] / A;
    wg_sum<MG_MAXJ>(se, red);
    wg_sum<2>(sw, red);
    wg_sum<D>(wm, red);
    double mf[D];
#pragma unroll
    for (int d = 0; d < D; ++d) mf[d] = any ? wm[d] / sw[0] : mp[d];

    // pass C: the weighted centred sums of S_filt (a row with nothing observed: the predicted moments, bit for bit)
    double sf[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sf[k] = 0.0;
    if (any) {
        for (int i = tid; i < N; i += 256) {
            double x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = Xp[(size_t)i * D + d] - mf[d];
            const double w = Wl[i];
            int k = 0;
#pragma unroll
            for (int lo = 0; lo < D; ++lo)
#pragma unroll
                for (int hi = lo; hi < D; ++hi) sf[k++] += w * (x[lo] * x[hi]);
        }
        wg_sum<NP>(sf, red);
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (tid == 64 + k) my_sf = sf[k] / sw[0];
    }

    // the decision and the row's outputs: every thread holds every sum, thread k stores entry k
    const double ess = any ? sw[0] * sw[0] / sw[1] : A * A / sm[D + 1];
    const bool resample = any && ess < q.ess_threshold * N;
    const double nan = __builtin_nan("");
    {
        const size_t o = orow + s;
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (tid == d) {
                a.m_x[o * D + d] = mp[d];
                f.m_filt[o * D + d] = mf[d];
            }
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) {
                if (tid == 64 + k) {
                    particle_store_sym<D>(a.S_x, o, lo, hi, my_sp);
                    particle_store_sym<D>(f.S_filt, o, lo, hi, any ? my_sf : my_sp);
                }
                ++k;
            }
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && tid == 128 + j) f.lpd[o * J + j] = ys[j] == ys[j] ? mx[j] + log(se[j] / A) : nan;
        if (tid == 192) {
            f.lpd_joint[o] = any ? mx[MG_MAXJ] + log(sw[0] / A) : nan;
            p.ess[o] = ess;
            q.resampled[o] = resample ? 1 : 0;
        }
    }
    if (q.weights) {
        double *wo = q.weights + (orow + s) * N;
        for (int i = tid; i < N; i += 256) wo[i] = any ? Wl[i] / sw[0] : ew[i] / A;
    }

    int *ao = p.ancestors ? p.ancestors + (orow + s) * N : nullptr;
    if (!resample) {                                              // the set is carried: thread i moves the particle it propagated
        for (int i = tid; i < N; i += 256) {
            if (ao) ao[i] = i;
#pragma unroll
            for (int d = 0; d < D; ++d) Xn[(size_t)i * D + d] = Xp[(size_t)i * D + d];
        }
        return;
    }

    particle_scan(Wl, cdf, N, wtot);                              // (also: every X^- of pass A is visible to the gather)

    // the ancestors and the gather; the new set is equally weighted
    const double tot = cdf[N - 1];
    const double u0 = p.unif[(size_t)gq * p.unif_g + (size_t)r * p.unif_r + s];
    for (int i = tid; i < N; i += 256) {
        const int an = particle_search(cdf, N, (u0 + i) / N * tot);
        if (ao) ao[i] = an;
#pragma unroll
        for (int d = 0; d < D; ++d) Xn[(size_t)i * D + d] = Xp[(size_t)an * D + d];
        lw[i] = 0.0;
    }
}

}  // namespace

// a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout of the pass with N rows per track and its buffers
void launch_mg_pess_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, const MomentParticleArgs &p, const MomentParticleEssArgs &q, int t) {
    const dim3 grid((unsigned)a.G);
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pess_weight_kernel<d>), grid, dim3(256), 0, stream, a, t, f, rc, l, p, q))
    if (t >= a.steps) return;
    launch_mg_prec_rows(stream, a, rc, l, p, t);
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

}  // namespace ffvd
