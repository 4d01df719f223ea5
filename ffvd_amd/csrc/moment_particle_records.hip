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
// An eighth translation unit of the family: the code of the others does not change with it.
#include "moment_step.h"

namespace ffvd {
namespace {

constexpr int PREC_RED = MG_MAXD * (MG_MAXD + 1) / 2;     // the widest reduction: the upper triangle of a covariance

// v[k] <- the sum over the workgroup, the same in every thread: wavefront butterflies, then the four wavefronts in ascending order
template <int K>
__device__ __forceinline__ void prec_sum(double (&v)[K], double (*red)[PREC_RED]) {
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
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

template <int K>
__device__ __forceinline__ void prec_max(double (&v)[K], double (*red)[PREC_RED]) {
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
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]));
}

// Launch t of steps + 1.  a.G: the tracks of the pass (groups * rc.Rp); l: mg_lfan_layout with N rows per track; p.xstate:
// [2][tracks][N][D] (step parity), p.pmean: [tracks][D][N].
template <int D>
__global__ __launch_bounds__(256) void mg_prec_weight_kernel(MomentGroupArgs a, const int t, MomentFilterArgs f, MomentRecordArgs rc,
                                                             MomentLinearFanArgs l, MomentParticleArgs p) {
    constexpr int NP = D * (D + 1) / 2;
    __shared__ double Wl[MG_PREC_MAXN], cdf[MG_PREC_MAXN];
    __shared__ double red[4][PREC_RED], Lm[MG_MAXD][MG_MAXD], Sg[MG_MAXD][MG_MAXD];
    __shared__ double hs[MG_MAXJ][MG_MAXD], dds[MG_MAXJ], s2s[MG_MAXJ], ys[MG_MAXJ], lcs[MG_MAXJ], vard[MG_MAXD], Qd[MG_MAXD], wtot[4];
    const int tid = threadIdx.x;
    const int G = a.G, steps = a.steps, N = p.N, J = f.J;
    const int v = blockIdx.x;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;                     // (r < R: the host sizes the passes)
    const int model = a.n_models == 1 ? 0 : gq;
    const int row = N * (l.shared ? v : bl);                                      // the track's first row in the K blocks of its units
    const size_t vg = (size_t)gq * rc.R + r, orow = vg * steps;                   // the track of the call; its first row in the stacks
    double *Xn = p.xstate + ((size_t)(t & 1) * G + v) * N * D;

    if (t == 0) {                                                 // the start: x0 + L0 xi0, L0 the unpivoted factor of S0 (zeros: x0)
        if (tid < D * D) Sg[tid / D][tid % D] = a.S0 ? a.S0[vg * D * D + tid] : 0.0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (tid < D) {
                double pv = Sg[j][j], s = Sg[tid][j];
                for (int k = 0; k < j; ++k) { pv -= Lm[j][k] * Lm[j][k]; s -= Lm[tid][k] * Lm[j][k]; }
                double e = 0.0;
                if (pv > 0.0 && tid >= j) {
                    const double q = sqrt(pv);
                    e = tid == j ? q : s / q;
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
            for (int q = 0; q < D; ++q) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c <= q; ++c) s += Lm[q][c] * z[c];
                Xn[(size_t)i * D + q] = a.x_last[vg * D + q] + s;
            }
        }
        return;
    }

    const int s = t - 1;                                          // the step this launch finishes, the row of Y it emits
    double *Xp = p.xstate + ((size_t)(s & 1) * G + v) * N * D;    // X_s, overwritten by X^-_s particle by particle
    if (tid < J * D) hs[tid / D][tid % D] = f.CC[(size_t)(tid % D) * J + tid / D];
    if (tid < J) {
        const double s2 = f.sd[tid] * f.sd[tid];
        dds[tid] = f.DD[tid];
        s2s[tid] = s2;
        lcs[tid] = -0.5 * (LOG_2PI + log(s2));
        ys[tid] = f.Y[((size_t)r * steps + s) * J + tid];
    }
    if (tid < D) {
        vard[tid] = a.variance[(size_t)model * D + tid];
        Qd[tid] = exp(a.log_Q[(size_t)gq * D + tid]);
    }
    __syncthreads();
    bool any = false;
    for (int j = 0; j < J; ++j) any = any || ys[j] == ys[j];

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
            const double *vp = l.vpart + (size_t)(l.shared ? d : gq * D + d) * l.ntj * l.Tp + row + i;
            double qf = 0.0;
            for (int tj = 0; tj < l.ntj; ++tj) qf += vp[(size_t)tj * l.Tp];        // column tiles in ascending order
            x[d] = (Xp[(size_t)i * D + d] + pm[(size_t)d * N + i]) + ep[(size_t)i * D + d] * sqrt((vard[d] - qf) + Qd[d]);
            Xp[(size_t)i * D + d] = x[d];
            if (po) po[(size_t)i * D + d] = x[d];
            sm[d] += x[d];
        }
        double L = 0.0;
#pragma unroll
        for (int j = 0; j < MG_MAXJ; ++j)
            if (j < J && ys[j] == ys[j]) {
                double hm = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) hm += hs[j][d] * x[d];
                const double e = (ys[j] - hm) - dds[j], lj = lcs[j] - 0.5 * e * e / s2s[j];
                mx[j] = fmax(mx[j], lj);
                L += lj;
            }
        mx[MG_MAXJ] = fmax(mx[MG_MAXJ], L);
        Wl[i] = L;
    }
    prec_sum<D>(sm, red);
    prec_max<MG_MAXJ + 1>(mx, red);
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
            if (j < J && ys[j] == ys[j]) {
                double hm = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) hm += hs[j][d] * x[d];
                const double e = (ys[j] - hm) - dds[j];
                se[j] += exp((lcs[j] - 0.5 * e * e / s2s[j]) - mx[j]);
            }
        const double w = any ? exp(Wl[i] - mx[MG_MAXJ]) : 1.0;
        Wl[i] = w;
        sw[0] += w;
        sw[1] += w * w;
#pragma unroll
        for (int d = 0; d < D; ++d) wm[d] += w * x[d];
    }
    prec_sum<NP>(sp, red);
    double my_sp = 0.0, my_sf = 0.0;                              // thread 64 + k keeps entry k of the upper triangles
#pragma unroll
    for (int k = 0; k < NP; ++k)
        if (tid == 64 + k) my_sp = sp[k] / N;
    prec_sum<MG_MAXJ>(se, red);
    prec_sum<2>(sw, red);
    prec_sum<D>(wm, red);
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
        prec_sum<NP>(sf, red);
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (tid == 64 + k) my_sf = sf[k] / sw[0];
    }

    // the row's outputs: every thread holds every sum, thread k stores entry k; (lo, hi) and (hi, lo) store one value
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
                    const double vp = my_sp, vf = any ? my_sf : vp;
                    a.S_x[o * D * D + lo * D + hi] = vp;
                    a.S_x[o * D * D + hi * D + lo] = vp;
                    f.S_filt[o * D * D + lo * D + hi] = vf;
                    f.S_filt[o * D * D + hi * D + lo] = vf;
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
    __syncthreads();                                              // (also: every X^- of pass A is visible to the gather)

    // the ancestors and the gather
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
#pragma unroll
        for (int d = 0; d < D; ++d) Xn[(size_t)i * D + d] = Xp[(size_t)an * D + d];
    }
}

// Launch t < steps.  Workgroup (track of the pass, dim, slab of MG_PREC_SLAB particles): thread = column j, one row of Z against the
// particles of the slab; the kernel rows go to rows N * (track row) + i of the unit's K block, their means to pmean.
template <int D>
__global__ __launch_bounds__(256) void mg_prec_rows_kernel(MomentGroupArgs a, const int t, MomentRecordArgs rc, MomentLinearFanArgs l,
                                                           MomentParticleArgs p) {
    constexpr int NQ = MG_PREC_SLAB;
    __shared__ double xp[NQ][MG_MAXD], xc[MAXP], il[MAXP], red[4][NQ];
    const int tid = threadIdx.x;
    const int G = a.G, C = a.C, P = a.P, M = a.M, Mp = a.Mp, steps = a.steps, N = p.N;
    const int NSL = (N + NQ - 1) / NQ;
    const int sl = blockIdx.x % NSL, vd = blockIdx.x / NSL, d = vd % D, v = vd / D;
    const int bl = v % rc.Rp, gq = v / rc.Rp, r = rc.r0 + bl;
    const int model = a.n_models == 1 ? 0 : gq;
    const int i0 = sl * NQ, ni = N - i0 < NQ ? N - i0 : NQ;
    const int row = N * (l.shared ? v : bl) + i0;
    const double *X = p.xstate + ((size_t)(t & 1) * G + v) * N * D;
    const double *lend = a.len + ((size_t)model * D + d) * P;
    if (tid < NQ * D) {
        const int i = tid / D, q = tid % D;
        xp[i][q] = i < ni ? X[(size_t)(i0 + i) * D + q] : 0.0;
    }
    if (tid >= 128 && tid < 128 + P) {
        const int q = tid - 128;
        xc[q] = q < D ? 0.0 : a.ctrl[((size_t)r * steps + t) * C + (q - D)];
        il[q] = 1.0 / lend[q];
    }
    __syncthreads();

    const double *Zm = a.Z + (size_t)model * M * P;
    const double *bed = a.beta + ((size_t)gq * D + d) * Mp;
    const double var = a.variance[(size_t)model * D + d];
    double *Kr = l.K + ((size_t)(l.shared ? d : gq * D + d) * l.Tp + row) * Mp;
    double acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
    for (int j = tid; j < Mp; j += 256) {
        const bool live = j < M;
        const double *z = Zm + (size_t)(live ? j : 0) * P;        // (a padding column reads row 0 and writes zeros)
        double zs[D], cc = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) zs[q] = z[q];
        for (int q = D; q < P; ++q) {
            const double u = (z[q] - xc[q]) * il[q];
            cc += u * u;
        }
        const double be = live ? bed[j] : 0.0, vk = live ? var : 0.0;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            if (i < ni) {
                double c = 0.0;
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    const double u = (zs[q] - xp[i][q]) * il[q];
                    c += u * u;
                }
                const double k = vk * exp(-0.5 * (c + cc));
                acc[i] += k * be;
                Kr[(size_t)i * Mp + j] = k;
            }
            __builtin_amdgcn_sched_barrier(0);                    // one particle at a time: interleaved exps cost registers
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        double s = acc[i];
#pragma unroll
        for (int mm = 32; mm > 0; mm >>= 1) s += __shfl_xor(s, mm);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (tid < ni) p.pmean[((size_t)v * D + d) * N + i0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
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
    switch (a.D) {
#define MG_CASE(d)                                                                                                                  \
    case d:                                                                                                                         \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_prec_weight_kernel<d>), grid, dim3(256), 0, stream, a, t, f, rc, l, p);               \
        if (t < a.steps) hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_prec_rows_kernel<d>), rows, dim3(256), 0, stream, a, t, rc, l, p);   \
        break;
        MG_CASE(1) MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8)
#undef MG_CASE
        default: break;
    }
    if (t >= a.steps) return;
    launch_mg_lfan_var(stream, l.K, a.gam, l.vpart, l.Tp, a.Mp, l.nr, l.units);
}

// the rows kernel of step t < steps alone, for a unit with a weight kernel of its own (moment_particle_adapted.hip)
void launch_mg_prec_rows(hipStream_t stream, const MomentGroupArgs &a, const MomentRecordArgs &rc, const MomentLinearFanArgs &l,
                         const MomentParticleArgs &p, int t) {
    const int nsl = (p.N + MG_PREC_SLAB - 1) / MG_PREC_SLAB;
    const dim3 rows((unsigned)((size_t)a.G * a.D * nsl));
    switch (a.D) {
#define MG_CASE(d)                                                                                                                  \
    case d: hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_prec_rows_kernel<d>), rows, dim3(256), 0, stream, a, t, rc, l, p); break;
        MG_CASE(1) MG_CASE(2) MG_CASE(3) MG_CASE(4) MG_CASE(5) MG_CASE(6) MG_CASE(7) MG_CASE(8)
#undef MG_CASE
        default: break;
    }
}

}  // namespace ffvd
