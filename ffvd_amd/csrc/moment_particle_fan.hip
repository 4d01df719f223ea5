// Rolling-origin multi-step forecasts by particles ("Particle forecasts"): the propagation of
// moment_particle_records.hip without weighting or resampling, with a TRACK (group, origin) as its unit and the indexing of the moment
// fan (moment_group.h, MomentFanArgs).  A track starts from the particle set the filter carries AFTER row o of the record: the X^- of
// that row gathered through that row's ancestors (the identity for a row with nothing observed), N equally weighted particles.  Per
// step k = 1 .. h, with c the control row o + k and (m_i, v_i) the mean and variance of the GP conditional of the group at [X_i, c]:
//   X_i <- X_i + m_i + eps_fc[k - 1, i] sqrt(v_i + Q)                            (per dim; the filter's expression)
//   m_fc = sum_i X_i / N,  S_fc = sum_i (X_i - m_fc)(X_i - m_fc)^T / N
//   lpd_fc_j = log(sum_i N(y_{o+k,j}; CC[:, j] . X_i + DD_j, sd_j^2) / N)        (the largest exponent subtracted; NaN where y is)
// The N kernel rows of a (track, dim) are N rows of the unit's K block, so the quadratic forms of all particles of all tracks of a
// unit are the diagonal of K Gamma K^T: the product kernel of the linearised forecasts, unchanged (launch_mg_lfan_var).
//
// Three launches per step for all tracks of a pass:
//   mg_pfan_state_kernel (VALU, 256 threads, workgroup = track of the pass): launch 0 gathers the start particles into the
//     double-buffered state; launch t > 0 finishes step t - 1 from what the previous launches left (the means of pmean, the
//     column-tile partials in ascending tile order) and stores row t - 1 of the forecast.  No scan, no search, no weights;
//   mg_pfan_rows_kernel (VALU, 256 threads, workgroup = (track, dim, slab of MG_PREC_SLAB particles)): the zero-padded kernel rows
//     of the slab's particles into K and their means;
//   mg_lfan_var_kernel (moment_linear_fan.hip).
// No atomics, nothing waits on another workgroup, every sum has an order fixed by N alone.  The reductions, the transition, the
// emission and the rows body are the blocks of moment_particle.h that the records filter calls, so a track is bit for bit what that
// filter computes over the record cut after the origin and continued by h all-NaN rows.  The one address that depends on computed
// values is the start gather's: the ancestor index is clamped into [0, N) before it is used.
#include "moment_particle.h"

namespace ffvd {
namespace {

// Launch t of h + 1.  a.G: the tracks of the pass (groups * fn.Bp), a.steps: the horizon, a.m_x / a.S_x: the forecast stacks;
// f: the emission and the record's Y [n][J]; l: mg_lfan_layout with N rows per track; p.xstate: [2][tracks][N][D] (step parity),
// p.pmean: [tracks][D][N].
template <int D>
__global__ __launch_bounds__(256) void mg_pfan_state_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentFanArgs fn,
                                                            MomentLinearFanArgs l, MomentParticleFanArgs p) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double red[4][PARTICLE_RED];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], lcs[MG_MAXJ], vard[MG_MAXD], Qd[MG_MAXD];
    const int tid = threadIdx.x;
    const int G = a.G, steps = a.steps, N = p.N, J = f.J;
    const int v = blockIdx.x;
    const int bl = v % fn.Bp, gq = v / fn.Bp, b = fn.b0 + bl, org = fn.origin[b];   // (the table was checked on the host: 0 <= org, org + steps < n)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);                                      // the track's first row in the K blocks of its units
    const size_t orow = ((size_t)gq * fn.B + b) * steps, srow = (size_t)gq * fn.n + org;
    double *Xn = p.xstate + ((size_t)(t & 1) * G + v) * N * D;

    if (t == 0) {                                                 // the start: the X^- of row org through that row's ancestors
        const double *xs = p.particles + srow * N * D;
        const int *as = p.ancestors + srow * N;
        for (int i = tid; i < N; i += 256) {
            const int an = particle_clamp(as[i], N);
#pragma unroll
            for (int d = 0; d < D; ++d) Xn[(size_t)i * D + d] = xs[(size_t)an * D + d];
        }
        return;
    }

    const int s = t - 1;                                          // the step this launch finishes: row org + 1 + s of Y is its target
    const double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;
    particle_stage_emission<D>(f, f.Y + (size_t)(org + 1 + s) * J, hs, dds, s2s, ys, lcs);
    particle_stage_noise<D>(a, model, gq, vard, Qd);
    __syncthreads();

    // pass A: X^- (kept as the state of launch t: nothing is resampled), the sums of the mean and the largest exponents
    const double *ep = p.eps_fc + (size_t)gq * p.eps_g + (size_t)b * p.eps_b + (size_t)s * N * D;
    const double *pm = p.pmean + (size_t)v * D * N;
    double *po = p.fc_particles ? p.fc_particles + (orow + s) * N * D : nullptr;
    double sm[D], mx[MG_MAXJ];
#pragma unroll
    for (int d = 0; d < D; ++d) sm[d] = 0.0;
#pragma unroll
    for (int j = 0; j < MG_MAXJ; ++j) mx[j] = -__builtin_inf();
    for (int i = tid; i < N; i += 256) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double tm, tv;
            particle_transition<D>(l, gq, d, row, i, N, Xp, pm, vard[d], Qd[d], tm, tv);
            x[d] = tm + ep[(size_t)i * D + d] * sqrt(tv);
            Xn[(size_t)i * D + d] = x[d];
            if (po) po[(size_t)i * D + d] = x[d];
            sm[d] += x[d];
        }
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) mx[j] = fmax(mx[j], particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs));
    }
    wg_sum<D>(sm, red);
    wg_max<MG_MAXJ>(mx, red);
    double mp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) mp[d] = sm[d] / N;

    // pass B: the centred sums of S_fc and the densities (a thread reads the particles it wrote itself)
    double sp[NP], se[MG_MAXJ];
#pragma unroll
    for (int k = 0; k < NP; ++k) sp[k] = 0.0;
#pragma unroll
    for (int j = 0; j < MG_MAXJ; ++j) se[j] = 0.0;
    for (int i = tid; i < N; i += 256) {
        double x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = Xn[(size_t)i * D + d];
        int k = 0;
#pragma unroll
        for (int lo = 0; lo < D; ++lo)
#pragma unroll
            for (int hi = lo; hi < D; ++hi) sp[k++] += (x[lo] - mp[lo]) * (x[hi] - mp[hi]);
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) se[j] += exp(particle_emit_logpdf<D>(j, x, hs, dds, s2s, ys, lcs) - mx[j]);
    }
    wg_sum<NP>(sp, red);
    double my_sp = 0.0;                                           // thread 64 + k keeps entry k of the upper triangle
#pragma unroll
    for (int k = 0; k < NP; ++k)
        if (tid == 64 + k) my_sp = sp[k] / N;
    wg_sum<MG_MAXJ>(se, red);

    // the row's outputs: every thread holds every sum, thread k stores entry k
    const size_t o = orow + s;
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (tid == d) a.m_x[o * D + d] = mp[d];
    int k = 0;
#pragma unroll
    for (int lo = 0; lo < D; ++lo)
#pragma unroll
        for (int hi = lo; hi < D; ++hi) {
            if (tid == 64 + k) particle_store_sym<D>(a.S_x, o, lo, hi, my_sp);
            ++k;
        }
#pragma unroll
    for (int j = 0; j < MG_MAXJ; ++j)
        if (j < J && tid == 128 + j) p.lpd_fc[o * J + j] = ys[j] == ys[j] ? mx[j] + log(se[j] / N) : __builtin_nan("");
}

// Launch t < h.  Workgroup (track of the pass, dim, slab of MG_PREC_SLAB particles): the rows body for control row org + 1 + t of
// the record.
template <int D>
__global__ __launch_bounds__(256) void mg_pfan_rows_kernel(MomentGroupArgs a, const int t, MomentFanArgs fn, MomentLinearFanArgs l,
                                                           MomentParticleFanArgs p) {
    const int N = p.N, NSL = (N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const int sl = blockIdx.x % NSL, vd = blockIdx.x / NSL, d = vd % D, v = vd / D;
    const int bl = v % fn.Bp, gq = v / fn.Bp, org = fn.origin[fn.b0 + bl];
    particle_rows_body<D>(a, l, N, sl, d, gq, a.ctrl + (size_t)(org + 1 + t) * a.C, p.xstate + ((size_t)(t & 1) * a.G + v) * N * D,
                          p.pmean + ((size_t)v * D + d) * N, N * (l.shared ? v : bl));
}

}  // namespace

// a.G: the tracks of the pass (groups * fn.Bp); l: mg_lfan_layout of the pass with N rows per track and its buffers
void launch_mg_pfan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFilterArgs &f, const MomentFanArgs &fn,
                         const MomentLinearFanArgs &l, const MomentParticleFanArgs &p, int t) {
    const dim3 grid((unsigned)a.G);
    const int nsl = (p.N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const dim3 rows((unsigned)((size_t)a.G * a.D * nsl));
    MG_DISPATCH_D(a.D, {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pfan_state_kernel<d>), grid, dim3(256), 0, stream, a, t, f, fn, l, p);
        if (t < a.steps) hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_pfan_rows_kernel<d>), rows, dim3(256), 0, stream, a, t, fn, l, p);
    })
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

}  // namespace ffvd
