// Particle filtering of many observed records in one call ("Particle filtering"): the records filter of
// moment_linear_records.hip with a bootstrap particle filter in place of a Gaussian rule.  A TRACK (group g, record r) carries N
// particles.  Per step s, with c the record's control row and (m_i, v_i) the mean and variance of the GP conditional of the group at
// [X_i, c]:
//   X^-_i = X_i + m_i + eps[s, i] sqrt(v_i + Q)                                  (per dim; the rollouts' recursion)
//   m_pred = sum_i X^-_i / N,  S_pred = sum_i (X^-_i - m_pred)(X^-_i - m_pred)^T / N
//   l_ij = log N(y_sj; CC[:, j] . X^-_i + DD_j, sd_j^2),  lpd_j = log(sum_i exp l_ij / N),  L_i = sum_{j observed} l_ij,
//   lpd_joint = log(sum_i exp L_i / N),  W_i = exp(L_i - max L),  m_filt, S_filt: the W-weighted mean and centred covariance,
//   ess = (sum W)^2 / sum W^2;  systematic resampling with one uniform u: cdf_k = W_0 + .. + W_k,
//   a_i = min(#{k: cdf_k <= (u + i) / N cdf_{N-1}}, N - 1),  X_i <- X^-_{a_i};  a row with nothing observed keeps its particles.
// The N kernel rows of a (track, dim) are N rows of the unit's K block, so the quadratic forms of all particles of all tracks of a
// unit are the diagonal of K Gamma K^T: the product kernel of the linearised forecasts, unchanged (launch_mg_lfan_var).
//
// Three launches per step for all tracks of a pass (the unfused form: the weight kernel needs one workgroup per track for its scan,
// the rows need (track, dim, slab) workgroups to fill the device):
//   mg_prec_weight_kernel (VALU, 256 threads, workgroup = track of the pass): finishes step t - 1 from what the previous launches
//     left (the means of pmean, the column-tile partials in ascending tile order), stores the row's outputs, scans the weights,
//     finds the ancestors by binary search and gathers the resampled particles into the other half of the double-buffered state;
//   mg_prec_rows_kernel (VALU, 256 threads, workgroup = (track, dim, slab of MG_PREC_SLAB particles)): the zero-padded kernel rows
//     of the slab's particles into K and their means;
//   mg_lfan_var_kernel (moment_linear_fan.hip).
// No atomics, nothing waits on another workgroup, every sum and the scan have an order fixed by N alone.  The one address that
// depends on computed values is the gather's: the ancestor index is clamped into [0, N) before it is used, whatever the weights are.
// The reductions, the start, the transition, the emission, the scan, the search and the rows body are the blocks of
// moment_particle.h, which the other particle units call too.
#include "moment_particle.h"

namespace ffvd {
namespace {

// Launch t of steps + 1.  a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout with N rows per track; p.xstate:
// [2][tracks][N][D] (step parity), p.pmean: [tracks][D][N].
template <int D>
__global__ __launch_bounds__(256) void mg_prec_weight_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentRecordArgs rc,
                                                             MomentLinearFanArgs l, MomentParticleArgs p) {
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

    if (t == 0) {
        particle_start<D>(a, p, gq, r, vg, Xn, Sg, Lm);
        return;
    }

    const int s = t - 1;                                          // the step this launch finishes, the row of Y it emits
    double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;    // X_s, overwritten by X^-_s particle by particle
    particle_stage_emission<D>(f, f.Y + ((size_t)r * steps + s) * J, hs, dds, s2s, ys, lcs);
    particle_stage_noise<D>(a, model, gq, vard, Qd);
    __syncthreads();
    const bool any = particle_any_observed(ys, J);

    // pass A: X^-, the sums of the mean, the log-weights and the largest exponents
    const double *ep = p.eps + (size_t)gq * p.eps_g + (size_t)r * p.eps_r + (size_t)s * N * D;
    const double *pm = p.pmean + (size_t)v * D * N;
    double *po = p.particles ? p.particles + (orow + s) * N * D : nullptr;
    double sm[D], mx[MG_MAXJ + 1];
#pragma unroll
    for (int d = 0; d < D; ++d) sm[d] = 0.0;
#pragma unroll
    for (int j = 0; j <= MG_MAXJ; ++j) mx[j] = -__builtin_inf();
    for (int i = tid; i < N; i += 256) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double tm, tv;
            particle_transition<D>(l, gq, d, row, i, N, Xp, pm, vard[d], Qd[d], tm, tv);
            x[d] = tm + ep[(size_t)i * D + d] * sqrt(tv);
            Xp[(size_t)i * D + d] = x[d];
            if (po) po[(size_t)i * D + d] = x[d];
            sm[d] += x[d];
        }
        double L = 0.0;
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) {
                const double lj = particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs);
                mx[j] = fmax(mx[j], lj);
                L += lj;
            }
        mx[MG_MAXJ] = fmax(mx[MG_MAXJ], L);
        Wl[i] = L;
    }
    wg_sum<D>(sm, red);
    wg_max<MG_MAXJ + 1>(mx, red);
    double mp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) mp[d] = sm[d] / N;

    // pass B: the centred sums of S_pred, the densities, the weights and the weighted sums of the mean
    double sp[NP], se[MG_MAXJ], sw[2], wm[D];
#pragma unroll
    for (int k = 0; k < NP; ++k) sp[k] = 0.0;
#pragma unroll
    for (int j = 0; j < MG_MAXJ; ++j) se[j] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) wm[d] = 0.0;
    sw[0] = sw[1] = 0.0;
    for (int i = tid; i < N; i += 256) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = Xp[(size_t)i * D + d];
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) sp[k++] += (x[lo] - mp[lo]) * (x[hi] - mp[hi]);
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) se[j] += exp(particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs) - mx[j]);
        const double w = any ? exp(Wl[i] - mx[MG_MAXJ]) : 1.0;
        Wl[i] = w;
        sw[0] += w;
        sw[1] += w * w;
#pragma unroll
        for (int d = 0; d < D; ++d) wm[d] += w * x[d];
    }
    wg_sum<NP>(sp, red);
    double my_sp = 0.0, my_sf = 0.0;                              // thread 64 + k keeps entry k of the upper triangles
#pragma unroll
    for (int k = 0; k < NP; ++k)
        if (tid == 64 + k) my_sp = sp[k] / N;
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

    // the row's outputs: every thread holds every sum, thread k stores entry k
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
            if (j < J && tid == 128 + j) f.lpd[o * J + j] = ys[j] == ys[j] ? mx[j] + log(se[j] / N) : nan;
        if (tid == 192) {
            f.lpd_joint[o] = any ? mx[MG_MAXJ] + log(sw[0] / N) : nan;
            p.ess[o] = any ? sw[0] * sw[0] / sw[1] : (double)N;
        }
    }

    particle_scan(Wl, cdf, N, wtot);                              // (also: every X^- of pass A is visible to the gather)

    // the ancestors and the gather
    const double tot = cdf[N - 1];
    const double u0 = p.unif[(size_t)gq * p.unif_g + (size_t)r * p.unif_r + s];
    int *ao = p.ancestors ? p.ancestors + (orow + s) * N : nullptr;
    for (int i = tid; i < N; i += 256) {
        const int an = any ? particle_search(cdf, N, (u0 + i) / N * tot) : i;
        if (ao) ao[i] = an;
#pragma unroll
        for (int d = 0; d < D; ++d) Xn[(size_t)i * D + d] = Xp[(size_t)an * D + d];
    }
}

// Launch t < steps.  Workgroup (track of the pass, dim, slab of MG_PREC_SLAB particles): the rows body for record r of group gq.
template <int D>
__global__ __launch_bounds__(256) void mg_prec_rows_kernel(MomentGroupArgs a, const int t, MomentRecordArgs rc, MomentLinearFanArgs l,
                                                           MomentParticleArgs p) {
    const int N = p.N, NSL = (N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const int sl = blockIdx.x % NSL, vd = blockIdx.x / NSL, d = vd % D, v = vd / D;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;
    particle_rows_body<D>(a, l, N, sl, d, gq, a.ctrl + ((size_t)r * a.steps + t) * a.C, p.xstate + ((size_t)(t & 1) * a.G + v) * N * D,
                          p.pmean + ((size_t)v * D + d) * N, N * (l.shared ? v : bl));
}

}  // namespace

// the rows of a unit's K block that the scratch of the linearised layout holds for one track per group: the largest particle count
long long mg_prec_max_particles(int G, int n_models, int D, int Mp, int unit_per_group) {
    const MomentLinearFanArgs one = mg_lfan_layout(G, n_models, D, Mp, unit_per_group, 1);
    const long long per_row = (long long)one.units * (Mp + one.ntj);
    const long long rows = MG_LFAN_SCRATCH_DOUBLES / per_row / 128 * 128;
    return one.shared ? rows / G : rows;
}

// records per group of a pass with N rows per track: the linearised layout's rows in whole tracks, the rows kernel's grid within
// 2^31; one record per group is always tried (the caller has checked N against mg_prec_max_particles)
int mg_prec_records_per_pass(int G, int n_models, int D, int Mp, int unit_per_group, int R, int N) {
    const long long want = (long long)R * N;
    const int rows = mg_lfan_tracks_per_pass(G, n_models, D, Mp, unit_per_group, (int)(want < (1LL << 30) ? want : (1LL << 30)));
    long long rp = rows / N;
    const long long nsl = (N + MG_PREC_SLAB - 1) / MG_PREC_SLAB, grid = ((1LL << 31) - 1) / ((long long)G * D * nsl);
    if (rp > grid) rp = grid;
    return (int)(rp < 1 ? 1 : rp);
}

// a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout of the pass with N rows per track and its buffers
void launch_mg_prec_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentRecordArgs &rc,
                         const MomentLinearFanArgs &l, const MomentParticleArgs &p, int t) {
    const dim3 grid((unsigned)a.G);
    const int nsl = (p.N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const dim3 rows((unsigned)((size_t)a.G * a.D * nsl));
    MG_DISPATCH_D(a.D, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_prec_weight_kernel<d>), grid, dim3(256), 0, stream, a, t, f, rc, l, p);
        if (t < a.steps) hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_prec_rows_kernel<d>), rows, dim3(256), 0, stream, a, t, rc, l, p);
    })
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

// the rows kernel of step t < steps alone, for a unit with a weight kernel of its own (moment_particle_adapted.hip)
void launch_mg_prec_rows(hipStream_t stream, const MomentGroupArgs &a, const MomentRecordArgs &rc, const MomentLinearFanArgs &l,
                         const MomentParticleArgs &p, int t) {
    const int nsl = (p.N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const dim3 rows((unsigned)((size_t)a.G * a.D * nsl));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_prec_rows_kernel<d>), rows, dim3(256), 0, stream, a, t, rc, l, p))
}

}  // namespace ffvd
