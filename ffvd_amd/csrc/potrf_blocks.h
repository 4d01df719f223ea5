// What the launch-per-step Cholesky variants (potrf.hip) and the dataflow Cholesky (potrf_flow.hip) share: the factorisation of one
// 64 x 64 diagonal block inside a workgroup -- by one wavefront (chol64_1w), or blocked on the matrix cores by four
// (chol64_mfma_4w) -- with the epilogue that stores L_kk and the inverses of its four 16 x 16 diagonal sub-blocks
// (diag_block_finish), the LDS strides those take, and what potrf.hip uses across the file boundary: the diagonal-block kernel,
// the dataflow launcher and its scratch size.
// Reference: conditionals_multi_output.py:159-166 (K3/K4: chol(K_uu + jitter I), L^{-T}) and :253-254 (the factor of H).
// DESIGN.md section 4 has the block algorithms, section 5 the measurements that chose between them.
#pragma once
#include "kernels.h"
#include "dev_common.h"

namespace ffvd {

// 64x64 Cholesky by ONE wavefront with no workgroup barriers: lane = row, the whole row in registers
// (a[c] = A[lane][c]), left-looking: column j <- a[j] - sum_{i<j} L[:,i] L[j][i].  Row j of L reaches every lane
// as broadcast LDS reads (16 bytes = two entries per instruction) of the copy Lr that the wavefront extends by one
// column per pivot.  Software pipeline: while the sqrt chain of pivot j is in flight, the wavefront already sums
// the terms i <= j-2 of column j+1 (all of them final and visible); when pivot j is done only two terms are
// missing -- L[j+1][j-1] from LDS and the newest one, L[j+1][j], by v_readlane.  A single wavefront issues in
// order, so without this interleaving every pivot would pay its full dependent latency.
// Entries above the diagonal carry don't-care values.
// Out: Lr[r][c] = L[r][c] for c <= r (LDS); invd[j] = 1 / L[j][j] (LDS).  Returns 0 or 1 + first bad pivot.
// PIPE = false drops the software pipeline (plain left-looking sums, the newest term by v_readlane): about 100
// VGPRs fewer, for launches whose many workgroups care about occupancy more than about one tile's latency.
constexpr int LR_LD = NB + 2;
constexpr int DV_LD = 17;       // row stride of the 16 x 16 inverse / scratch tiles (doubles)
template <bool PIPE>
__device__ __forceinline__ int chol64_1w(double (&a)[NB], double (*Lr)[LR_LD], double *invd, const int lane) {
    int bad = 0;
    if (!PIPE) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            double s0 = a[j], s1 = 0.0;
            if (j >= 2) wave_lds_sync();                     // column j-2 (and older) of Lr is visible
#pragma unroll
            for (int i = 0; i + 1 < j - 1 + (j & 1); i += 2) {          // pairs (i, i+1) with i + 1 <= j - 2
                const double2 lj = *reinterpret_cast<const double2 *>(&Lr[j][i]);
                s0 -= a[i] * lj.x;
                s1 -= a[i + 1] * lj.y;
            }
            if (j >= 2 && !(j & 1)) s0 -= a[j - 2] * Lr[j][j - 2];
            if (j >= 1) s1 -= a[j - 1] * readlane_f64(a[j - 1], j);
            const double v = s0 + s1;
            const double ajj = readlane_f64(v, j);
            if (!(ajj > 0.0) && bad == 0) bad = j + 1;
            double piv, y;
            pivot_sqrt(ajj, piv, y);
            a[j] = v * y;
            Lr[lane][j] = a[j];
            if (lane == 0) invd[j] = y;
        }
        return bad;
    }
    double nxt = 0.0;                                    // sum_{i <= j-3} L[:,i] L[j][i], formed during pivot j-1
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        double v = a[j] - nxt;                           // the two newest terms come straight from the registers
        if (j >= 2) v -= a[j - 2] * readlane_f64(a[j - 2], j);
        if (j >= 1) v -= a[j - 1] * readlane_f64(a[j - 1], j);
        const double ajj = readlane_f64(v, j);
        if (!(ajj > 0.0) && bad == 0) bad = j + 1;
        double piv, y;
        pivot_sqrt(ajj, piv, y);
        if (j + 1 < NB) {                                // terms i = 0 .. j-2 of column j+1, independent of pivot j
            if (j >= 2) wave_lds_sync();                 // columns <= j-2 of Lr (stored >= 1 pivot ago) are visible
            double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
            for (int i = 0; i + 1 <= j - 2; i += 2) {
                const double2 l2 = *reinterpret_cast<const double2 *>(&Lr[j + 1][i]);
                if (i & 2) { q2 += a[i] * l2.x; q3 += a[i + 1] * l2.y; }
                else { q0 += a[i] * l2.x; q1 += a[i + 1] * l2.y; }
            }
            if (j >= 2 && !(j & 1)) q0 += a[j - 2] * Lr[j + 1][j - 2];        // j-1 terms: odd count when j is even
            nxt = (q0 + q1) + (q2 + q3);
        }
        a[j] = v * y;                                    // lane j: ajj * y = sqrt(ajj) to an ulp
        Lr[lane][j] = a[j];
        if (lane == 0) invd[j] = y;
    }
    return bad;
}

// 64x64 Cholesky by the FOUR wavefronts of the workgroup, blocked 4 x 4 in 16 x 16 tiles, left-looking at tile level.  For tile
// column s the wavefronts form T'_is = T_is - sum_{k<s} L_ik L_sk^T of the step's tiles side by side on the matrix cores (i = s +
// wave), one barrier, then wavefront 0 runs ONE 16-pivot chain in registers with the tiles BELOW the diagonal tile riding through
// it.  The chain is right-looking -- pivot j scales column j of every row and subtracts its multiple of row j's multipliers from the
// columns right of it -- so a lane that starts from a row of T'_is comes out holding that row of L_is, exactly as the unblocked
// factorisation would produce it.  Lanes 0-15: the diagonal tile, 16-31: the rows of the identity (they come out as L_ss^-T, the
// inverted diagonal sub-block the panel kernels multiply by), 32-47 / 48-63: tiles (s+1, s), (s+2, s); step 0 has a third tile
// below, which a second wavefront takes through the same chain (it repeats the pivots for itself).  The chain as in tiny.hip's
// tiny_chol_inv: per-lane base pointers instead of an exec-masked load per element, no scalar test per pivot -- a non-positive or
// NaN pivot leaves NaN on L's diagonal from there on, looked for once behind the chain.  tools/df_trace.py: about 10.5 us per
// 64-block, i.e. per block column of every factorisation's latency chain (one wavefront with tile solves behind every chain: 15.5).
// In: Ts (lower triangle valid).  Out: Lr = L (lower triangle of every tile row, exact zeros above the diagonal inside the
// diagonal tiles), dinv_b[(16 s + r) * 16 + c] = (L_ss^-1)[r][c] in global memory.  Sc: four 16 x DV_LD scratch tiles (Sc[3]: the
// identity).  All 256 threads call; ends with the workgroup synchronised; returns 0 or 1 + first bad pivot on every thread of
// wavefront 0 (others: 0).
__device__ __forceinline__ int chol64_mfma_4w(double (*Ts)[NB + 1], double (*Lr)[LR_LD], double (*Sc)[16][DV_LD], double *dinv_b) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (threadIdx.x < 256) Sc[3][threadIdx.x >> 4][threadIdx.x & 15] = ((threadIdx.x >> 4) == (threadIdx.x & 15)) ? 1.0 : 0.0;
    __syncthreads();
    int bad = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int s0 = 16 * s;
        if (s > 0) {
            const int i = s + wave;
            if (i < 4) {                                     // T'_is in row-per-lane reach: Sc[wave]
                const int i0 = 16 * i;
                d4 acc = (d4){0.0, 0.0, 0.0, 0.0}, acc1 = acc;
                for (int k = 0; k < s; ++k)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const double av = Lr[i0 + lr][16 * k + 4 * t + lk], bv = Lr[s0 + lr][16 * k + 4 * t + lk];
                        if (t & 1) acc1 = mfma_f64(av, bv, acc1);
                        else acc = mfma_f64(av, bv, acc);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) Sc[wave][lk + 4 * r][lr] = Ts[i0 + lk + 4 * r][s0 + lr] - (acc[r] + acc1[r]);
            }
            __syncthreads();
        }
        if (wave == 0 || (s == 0 && wave == 1)) {
            __builtin_amdgcn_s_setprio(3);
            // which tile this lane's row belongs to: 0 the diagonal one, -1 the identity, t > 0: tile (s + t, s); -2: nothing (a copy of the
            // diagonal rows, not stored)
            int tl;
            if (wave == 0) tl = (lk == 0) ? 0 : (lk == 1) ? -1 : ((s + lk - 1 < 4) ? lk - 1 : -2);
            else tl = (lk == 1) ? 3 : -2;
            const double *src;
            if (tl == -1) src = &Sc[3][lr][0];
            else if (s == 0) src = &Ts[16 * (tl > 0 ? tl : 0) + lr][0];
            else src = &Sc[tl > 0 ? tl : 0][lr][0];
            double a[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = src[c];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double ajj = readlane_f64(a[j], j);
                double piv, y;
                pivot_sqrt(ajj, piv, y);
                a[j] *= y;
#pragma unroll
                for (int c = j + 1; c < 16; ++c) a[c] = fma(-a[j], readlane_f64(a[j], c), a[c]);
            }
            double diag = a[0];
#pragma unroll
            for (int c = 1; c < 16; ++c) diag = (lr == c) ? a[c] : diag;
            if (tl >= 0) {
                double *base = &Lr[s0 + 16 * tl + lr][s0];
#pragma unroll
                for (int c = 0; c < 16; ++c) base[c] = (tl > 0 || c <= lr) ? a[c] : 0.0;
            } else if (tl == -1) {
#pragma unroll
                for (int c = 0; c < 16; ++c) dinv_b[(s0 + c) * 16 + lr] = a[c];              // (L_ss^-1)[c][lr] = (L_ss^-T)[lr][c]
            }
            if (wave == 0) {
                const unsigned long long m = __ballot((lane < 16) & !(diag > 0.0));
                if (m && !bad) bad = s0 + (int)__builtin_ctzll(m) + 1;
            }
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
    }
    return bad;
}

// Factorise the diagonal block held in LDS tile `Ts` (row-major, stride NB+1): wavefront 0 runs chol64_1w, which
// leaves L in the LDS tile `Lr`; then all 256 threads publish L in place (lower triangle of the global block) and
// the four wavefronts invert the four 16x16 diagonal sub-blocks of L (lane = column, 16-step forward substitution)
// into dinv_b[4][16][16] -- what the panel kernel's blocked substitution multiplies by.
// (Sc != nullptr: the blocked matrix-core factor chol64_mfma_4w, which needs Lr and Ts in DIFFERENT memory and four scratch
// tiles, and leaves the inverted sub-blocks behind itself.)
template <bool PIPE>
__device__ __forceinline__ void diag_block_finish(double (*Ts)[NB + 1], double (*Lr)[LR_LD], double *invd, double *S, int n,
                                                   int k0, int32_t *info_b, double *dinv_b, double (*Sc)[16][DV_LD] = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (Sc) {
        const int bad = chol64_mfma_4w(Ts, Lr, Sc, dinv_b);      // (ends with the workgroup synchronised)
        if (w == 0 && bad && lane == 0 && *info_b == 0) *info_b = k0 + bad;
        for (int r = tid >> 6; r < NB; r += 4)
            if (lane <= r) S[(size_t)(k0 + r) * n + k0 + lane] = Lr[r][lane];         // coalesced rows of L
        return;
    }
    if (w == 0) {
        double a[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) a[c] = Ts[lane][c];
        // the pivot chain is one wavefront's dependent latency: it goes first whenever a wavefront of another workgroup
        // shares its SIMD
        __builtin_amdgcn_s_setprio(3);
        const int bad = chol64_1w<PIPE>(a, Lr, invd, lane);
        __builtin_amdgcn_s_setprio(0);
        if (bad && lane == 0 && *info_b == 0) *info_b = k0 + bad;
    }
    __syncthreads();
    for (int r = tid >> 6; r < NB; r += 4)
        if (lane <= r) S[(size_t)(k0 + r) * n + k0 + lane] = Lr[r][lane];         // coalesced rows of L
    if (lane < 16) {
        const int o = 16 * w;
        double x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            double acc = (lane == r) ? 1.0 : 0.0;
#pragma unroll
            for (int i = 0; i < r; ++i) acc -= Lr[o + r][o + i] * x[i];
            x[r] = acc * invd[o + r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dinv_b[(w * 16 + r) * 16 + lane] = x[r];
    }
}

// LDS row stride of the X(r,k) / L(j,k) tiles of the left-looking rows: potrf_ll_kernel and the dataflow kernel stage them alike
constexpr int LL_LD = NB + 2;

// potrf_flow.hip, for launch_potrf_ext: block (k, k) of every slab <- its factor, the inverted sub-blocks into dinv
__global__ void potrf_diag_kernel(double *A, int n, int k, size_t slab_stride, int32_t *info, double *dinv);
// potrf_flow.hip, for launch_potrf_ext and potrf_scratch_doubles (arguments as launch_potrf_ext's; scratch = its dinv)
void launch_potrf_flow(hipStream_t stream, double *A, int n, int extra_rows, int identity_rows, int batch,
                       size_t slab_stride, int32_t *info, double *scratch, double *linv_t, size_t linv_t_stride,
                       bool words_zeroed, bool tail_is_vector, double *kinv, size_t kinv_stride, const double *lt_rows,
                       size_t lt_stride, int lt_dl, bool kinv_help);
size_t potrf_flow_scratch_doubles(int n, int batch);      // progress words + the inverted sub-blocks of every (matrix, block column)

}  // namespace ffvd
