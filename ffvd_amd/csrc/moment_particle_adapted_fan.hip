// Rolling-origin multi-step forecasts from the adapted particle filter's sets ("Adapted particle forecasts"): the
// fan of moment_particle_fan.hip with the rows of the adapted filter (moment_particle_adapted.hip) in place of the bootstrap rows.  A
// TRACK (group, origin) starts from particles[o] of the adapted filter, the equally weighted FILTERED set after row o of the record: a
// straight copy, no ancestor is read.  Per step k = 1 .. h, with c the control row o + k and (mean_i, v_i) the GP conditional of the
// group at [X_i, c]:
//   mu_i = X_i + mean_i,  s_i = v_i + Q                          (per dim; the adapted kernel's mu / s)
//   m_fc = sum_i mu_i / N,  S_fc = sum_i (mu_i - m_fc)(mu_i - m_fc)^T / N + diag(sum_i s_i / N)           (no draw enters)
//   lpd_fc_j = log mean_i N(y_{o+k,j}; CC[:, j] . mu_i + DD_j, sum_d CC[d, j]^2 s_id + sd_j^2), the largest exponent subtracted;
//              NaN where y is
//   X_i <- mu_i + eps_fc[k - 1, i] sqrt(s_i)                     (the adapted filter's own row with nothing observed)
// so the last step's process noise is integrated in closed form at every horizon, and the row k = 1 of a track is the filter's
// one-step prediction of row o + 1.
//
// Three launches per step for all tracks of a pass:
//   mg_pafan_state_kernel (VALU, 256 threads, workgroup = track of the pass): launch 0 copies the start particles into the
//     double-buffered state; launch t > 0 finishes step t - 1 from what the previous launches left (the means of pmean, the
//     column-tile partials in ascending tile order) and stores row t - 1 of the forecast.  No scan, no search, no weights;
//   mg_pafan_rows_kernel: the rows body of moment_particle.h in an instantiation of this unit;
//   mg_lfan_var_kernel (moment_linear_fan.hip).
// No atomics, vector stores only, nothing waits on another workgroup, every sum has an order fixed by N alone.  The transition and the
// reductions are the blocks of moment_particle.h in the order the adapted weight kernel calls them (a thread's particles ascending, a
// 64-lane butterfly, the four wavefronts ascending; the sums end in LDS), and the expressions of its passes A and B are repeated here
// term by term, so a track is bit for bit what that filter computes over the record cut after the origin and continued by h all-NaN
// rows.  (mu, s) are not kept between the passes: pass B takes them from particle_transition again, from the same operands.  No
// address depends on a computed value.
#include "moment_particle.h"

namespace ffvd {
namespace {

// log N(y_j; CC[:, j] . mu + DD_j, sum_d CC[d, j]^2 s_d + sd_j^2) of one particle: the adapted weight kernel's expression
template <int D>
__device__ __forceinline__ double pafan_logpdf(const int j, const double (&mu)[D], const double (&sv)[D], const double (*hs)[MG_MAXD],
                                               const double *dds, const double *s2s, const double *ys) {
    double hm = 0.0, s2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        hm += hs[j][d] * mu[d];
        s2 += (hs[j][d] * hs[j][d]) * sv[d];
    }
    s2 += s2s[j];
    const double e = ys[j] - (hm + dds[j]);
    return -0.5 * (LOG_2PI + log(s2) + e * e / s2);
}

// Launch t of h + 1.  a.G: the tracks of the pass (groups * fn.Bp), a.steps: the horizon, a.m_x / a.S_x: the forecast stacks;
// f: the emission and the record's Y [n][J]; l: mg_lfan_layout with N rows per track; p.xstate: [2][tracks][N][D] (step parity),
// p.pmean: [tracks][D][N]; p.particles: the adapted filter's stack [groups][n][N][D]; p.ancestors is not read.
template <int D>
__global__ __launch_bounds__(256) void mg_pafan_state_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentFanArgs fn,
                                                             MomentLinearFanArgs l, MomentParticleFanArgs p) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double red[4][PARTICLE_RED];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], lcs[MG_MAXJ], vard[MG_MAXD], Qd[MG_MAXD];
    __shared__ double mps[MG_MAXD], sbs[MG_MAXD], mxs[MG_MAXJ], ses[MG_MAXJ], sps[PARTICLE_RED];
    const int tid = threadIdx.x;
    const int G = a.G, steps = a.steps, N = p.N, J = f.J;
    const int v = blockIdx.x;
    const int bl = v % fn.Bp, gq = v / fn.Bp, b = fn.b0 + bl, org = fn.origin[b];   // (the table was checked on the host: 0 <= org, org + steps < n)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);                                      // the track's first row in the K blocks of its units
    const size_t orow = ((size_t)gq * fn.B + b) * steps, srow = (size_t)gq * fn.n + org;
    double *Xn = p.xstate + ((size_t)(t & 1) * G + v) * N * D;

    if (t == 0) {                                                 // the start: the filtered set after row org, as it is stored
        const double *xs = p.particles + srow * N * D;
        for (int e = tid; e < N * D; e += 256) Xn[e] = xs[e];
        return;
    }

    const int s = t - 1;                                          // the step this launch finishes: row org + 1 + s of Y is its target
    const double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;
    particle_stage_emission<D>(f, f.Y + (size_t)(org + 1 + s) * J, hs, dds, s2s, ys, lcs);
    particle_stage_noise<D>(a, model, gq, vard, Qd);
    __syncthreads();

    // pass A: (mu, s) of every particle, their sums, the largest exponents of the mixture densities, and the next state
    const double *ep = p.eps_fc + (size_t)gq * p.eps_g + (size_t)b * p.eps_b + (size_t)s * N * D;
    const double *pm = p.pmean + (size_t)v * D * N;
    double *po = p.fc_particles ? p.fc_particles + (orow + s) * N * D : nullptr;
    {
        double sm[D], ss[D], mx[MG_MAXJ];
#pragma unroll
        for (int d = 0; d < D; ++d) sm[d] = ss[d] = 0.0;
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j) mx[j] = -__builtin_inf();
        for (int i = tid; i < N; i += 256) {
            double mu[D], sv[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                particle_transition<D>(l, gq, d, row, i, N, Xp, pm, vard[d], Qd[d], mu[d], sv[d]);
                sm[d] += mu[d];
                ss[d] += sv[d];
                const double x = mu[d] + ep[(size_t)i * D + d] * sqrt(sv[d]);
                Xn[(size_t)i * D + d] = x;
                if (po) po[(size_t)i * D + d] = x;
            }
#pragma unroll
            for (int j = 0; j < MG_MAXJ; ++j)
                if (j < J && ys[j] == ys[j]) mx[j] = fmax(mx[j], pafan_logpdf<D>(j, mu, sv, hs, dds, s2s, ys));
        }
        wg_sum_lds<D>(sm, red, mps, (double)N);                    // m_fc
        wg_sum_lds<D>(ss, red, sbs, (double)N);                    // sum_i s_i / N
        wg_max_lds<MG_MAXJ>(mx, red, mxs);
    }

    // pass B: the centred sums of S_fc and the densities, (mu, s) from the transition again
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
            for (int d = 0; d < D; ++d) particle_transition<D>(l, gq, d, row, i, N, Xp, pm, vard[d], Qd[d], mu[d], sv[d]);
            int k = 0;
#pragma unroll
            for (int lo = 0; lo < D; ++lo)
#pragma unroll
                for (int hi = lo; hi < D; ++hi) sp[k++] += (mu[lo] - mp[lo]) * (mu[hi] - mp[hi]);
#pragma unroll
            for (int j = 0; j < MG_MAXJ; ++j)
                if (j < J && ys[j] == ys[j]) se[j] += exp(pafan_logpdf<D>(j, mu, sv, hs, dds, s2s, ys) - mxs[j]);
        }
        wg_sum_lds<NP>(sp, red, sps, (double)N);
        wg_sum_lds<MG_MAXJ>(se, red, ses, 1.0);
    }

    // the row's outputs, from the sums in LDS: thread k stores entry k
    const size_t o = orow + s;
    if (tid < D) a.m_x[o * D + tid] = mps[tid];
    int k = 0;
#pragma unroll
    for (int lo = 0; lo < D; ++lo)
#pragma unroll
        for (int hi = lo; hi < D; ++hi) {
            if (tid == 64 + k) particle_store_sym<D>(a.S_x, o, lo, hi, lo == hi ? sps[k] + sbs[lo] : sps[k]);
            ++k;
        }
    if (tid >= 128 && tid < 128 + J) {
        const int j = tid - 128;
        p.lpd_fc[o * J + j] = ys[j] == ys[j] ? mxs[j] + log(ses[j] / N) : __builtin_nan("");
    }
}

// Launch t < h.  Workgroup (track of the pass, dim, slab of MG_PREC_SLAB particles): the rows body for control row org + 1 + t of
// the record.
template <int D>
__global__ __launch_bounds__(256) void mg_pafan_rows_kernel(MomentGroupArgs a, const int t, MomentFanArgs fn, MomentLinearFanArgs l,
                                                            MomentParticleFanArgs p) {
    const int N = p.N, NSL = (N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const int sl = blockIdx.x % NSL, vd = blockIdx.x / NSL, d = vd % D, v = vd / D;
    const int bl = v % fn.Bp, gq = v / fn.Bp, org = fn.origin[fn.b0 + bl];
    particle_rows_body<D>(a, l, N, sl, d, gq, a.ctrl + (size_t)(org + 1 + t) * a.C, p.xstate + ((size_t)(t & 1) * a.G + v) * N * D,
                          p.pmean + ((size_t)v * D + d) * N, N * (l.shared ? v : bl));
}

}  // namespace

// a.G: the tracks of the pass (groups * fn.Bp); l: mg_lfan_layout of the pass with N rows per track and its buffers
void launch_mg_pafan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentFanArgs &fn,
                          const MomentLinearFanArgs &l, const MomentParticleFanArgs &p, int t) {
    const dim3 grid((unsigned)a.G);
    const int nsl = (p.N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const dim3 rows((unsigned)((size_t)a.G * a.D * nsl));
    MG_DISPATCH_D(a.D, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pafan_state_kernel<d>), grid, dim3(256), 0, stream, a, t, f, fn, l, p);
        if (t < a.steps) hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pafan_rows_kernel<d>), rows, dim3(256), 0, stream, a, t, fn, l, p);
    })
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

}  // namespace ffvd
