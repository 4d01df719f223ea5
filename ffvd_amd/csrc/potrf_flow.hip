// Dataflow Cholesky (gfx950, fp64): the extended left-looking factorisation of a whole batch in ONE launch, block rows handing
// finished blocks to each other through progress words in memory.  It factorises every batch of 32 or more matrices and every
// batch whose caller says that it is on the critical path (CHOL_FLOW), can leave L^-1 transposed and A^-1 = L^-T L^-1 behind in
// the same launch, and bounds every wait: a launch that gives up says so in info[] and the caller re-runs the batch with a
// launch-per-step variant (potrf.hip chooses; kernels.h, launch_potrf_ext has the arguments).
// Reference: conditionals_multi_output.py:159-166 (K3/K4: chol(K_uu + jitter I), L^{-T}), :253-254 (K9/K10: the factor of H).
// DESIGN.md section 4 describes the kernel and what happens when a bounded wait fires, section 5 has its measurements.
#include "potrf_blocks.h"
#include <cstdlib>

namespace ffvd {

// ---------------------------------------------------------------------------------------------
// Dataflow variant: the whole left-looking factorisation of a batch in ONE launch.  One workgroup per 64-row block row of
// every matrix walks its row from left to right,
//     for j < r:  X(r,j) = (A(r,j) - sum_{k<j} X(r,k) L(j,k)^T) L_jj^-T        then (main rows)  L_rr = chol(A(r,r) - sum_k X(r,k) X(r,k)^T),
// and learns from one progress word per (matrix, block row) when the row above it is ready:  prog[j] = j once the panels
// X(j,0..j-1) are in memory, j + 1 once L_jj and its inverted 16 x 16 diagonal sub-blocks are.  What the per-column launches
// of potrf_ll_kernel serialised -- the gather of column j (j block products) in front of every diagonal factor -- now runs
// beside the pivot chain of the block above: the chain of dependent work per block column is one substitution, one block
// product and the 64-pivot factor.
// Hand-off (MI355X guide, inter-workgroup visibility): producer = plain stores, every storing wavefront waits for them, a
// workgroup barrier, ONE lane's agent-scope release, its wait, a relaxed agent-scope store of the word; consumer = ONE lane
// polls the word relaxed, ONE agent-scope acquire and its wait, a workgroup barrier, then plain loads.  Results never depend on
// where or when a workgroup runs.  Progress does: a row waits for rows of the same matrix with a lower blockIdx only, which
// the dispatcher starts first; every spin is bounded all the same (wall clock; a stuck launch sets the abort word, every
// waiting workgroup leaves, info[b] = -1 says so).
// Block order (group, row, matrix-in-group): G a multiple of 8, so all rows of a matrix share blockIdx % 8 = one XCD's L2.
// ---------------------------------------------------------------------------------------------
constexpr int DF_DINV = 4 * 16 * 16;              // doubles of inverted diagonal sub-blocks per (matrix, block column)
constexpr long long DF_SPIN_TICKS = 100000000LL;  // bound of one wait: 1 s of the 100 MHz wall clock

struct DfArgs {
    double *A;
    int n, nb, next, nid, batch, G;
    size_t slab_stride;
    int32_t *info;
    double *dinv;      // [batch][nb][DF_DINV]
    int *prog;         // [batch][DF_PS], zeroed before the launch
    int *abort_w;      // one word, zeroed before the launch
    double *xt;        // optional: the identity-structured extra rows (R L^-T = L^-T) also land TRANSPOSED here, i.e. L^-1 as
    size_t xt_stride;  //   an n x n lower-triangular matrix (ld n) per slab; blocks above its diagonal are not written
    int vec_tail;      // the extra-row blocks behind the identity rows carry ONE live row each (their first): df_vector_row
    double *kinv;      // optional (identity rows = all of L^-T): (A)^-1 = L^-T L^-1, full symmetric n x n per slab (ld n), formed by
    size_t kinv_stride;//   the identity-row workgroups once their rows are complete (df_inverse_tiles)
    int defer_ext;     // block order: identity-structured rows of all groups behind the main rows of all groups (potrf_df_kernel)
    int kinv_help;     // (with kinv, every workgroup resident at once) the main-row workgroups form half of the inverse's tiles: df_inverse_tiles
    int fine;          // small batches (every block row on a CU of its own): a main row also announces every COLUMN it has solved
                       // (word 2 nb + row), and a gather waits term by term -- see df_column
    const double *lt;  // optional: the identity-structured extra rows of slab b start as L_d^T (d = b % lt_dl) instead of what
    size_t lt_stride;  //   memory holds: block (e, j) = L_d(j, e)^T, read from the lower-triangular n x n factor L_d (ld n)
    int lt_dl;
};

// Debug build only (-DFFVD_DF_TRACE, tools/df_trace.py): wall-clock stamps of matrix 0's block rows, in a buffer of their own.
#ifdef FFVD_DF_TRACE
__device__ long long df_trace_buf[64 * 64];
#define DF_STAMP(row, slot) do { if ((row) >= 0 && threadIdx.x == 0) df_trace_buf[(row) * 64 + (slot)] = wall_clock64(); } while (0)
int gram_trace_tiles(long long *out);       // gram.hip
extern "C" int ffvd_debug_df_trace(long long *out) {
    const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(df_trace_buf), sizeof(long long) * 64 * 64);
    // the Gram kernel's stamps of its first 16 units, where tools/gram_trace.py reads them.  Words 2048..2367 are also the stamps of
    // block rows 32..36 (n >= 2112): as before the two uses overlap, and now the copy replaces those rows' stamps even in a run
    // whose Gram kernel stamped nothing
    return rc ? rc : gram_trace_tiles(out + 2048);
}
#else
#define DF_STAMP(row, slot) do { } while (0)
#endif

// Thread 0 waits until *flag >= need, acquires, and hands the value it saw (or -1: gave up) to the workgroup.
__device__ __forceinline__ int df_wait(int *flag, int need, int *abort_w, int *slot) {
    if (threadIdx.x == 0) {
        int v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v < need) {
            const long long t0 = wall_clock64();
            for (;;) {
                __builtin_amdgcn_s_sleep(2);
                v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v >= need) break;
                if (__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { v = -1; break; }
                if (wall_clock64() - t0 > DF_SPIN_TICKS) {
                    __hip_atomic_store(abort_w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    v = -1;
                    break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *slot = v;
    }
    __syncthreads();
    return *slot;
}

// ONE lane, behind the workgroup barrier that follows every storing wavefront's own wait for its stores.
__device__ __forceinline__ void df_publish(int *flag, int value) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the compiler may drop the fence's own wait (guide: compiler hazard)
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // a later store to the same word (another wavefront) must not overtake
}

// One block column of one block row: X(r,j) = (A(r,j) - sum_{k0<=k<j} X(r,k) L(j,k)^T) L_jj^-T.  LAST (the column left of
// the diagonal of a main row) also loads A(r,r), sums X(r,k) X(r,k)^T over k < j into acc_d beside the gather, and leaves the
// solved tile in sm0 for the newest term.  Returns false when a wait gave up.
// EARLY (main rows in the fine mode, columns left of the LAST one): the tile just solved adds its X X^T to acc_d right away, in the
// time this row would otherwise wait for the next diagonal block, and the LAST column's gather carries L(j,k) terms only -- a late
// row's last gather is 3.6 us of matrix-pipe time per term with both sums in it, 30 us in front of row 7's factor.  Same terms
// in the same order: the result does not change by a bit.
template <bool LAST, bool EARLY = false>
__device__ __forceinline__ bool df_column(const DfArgs &a, double *S, int *pg, const double *dvb, const int row0, const int j,
                                          const int k0, double (*Xs)[LL_LD], double (*Ls)[LL_LD], double (*Dv)[16][DV_LD],
                                          int *wslot, int &wc, d4 (&cold_d)[2][2], d4 (&acc_d)[2][2], const int trow,
                                          double *xt_row = nullptr, const double *lt_src = nullptr, const int lt_e = 0) {
    const int n = a.n;
    DF_STAMP(trow, 5 * (j & 7) + 0);
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave >> 1, qc = wave & 1;
    const int sr = tid >> 5, sc = 2 * (tid & 31);
    const int j0 = j * NB;
    const bool tri = !(qr == 0 && qc == 1);                // the quadrant above the diagonal of S_rr is never read
    const bool do_d = LAST && tri && a.fine != 1;          // (fine = 1: the earlier columns have added their terms already)
    // this row's own tiles (nobody else writes them): requested first, their latency hides behind the waits and the k loop
    d4 cold_t[2][2], acc_t[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t rr = (size_t)(row0 + qr * 32 + 16 * x + lk + 4 * q), cc = (size_t)(qc * 32 + 16 * y + lr);
                if (!LAST && lt_src) {       // block (e, j) of L^T: element [il][cl] = L[j0 + cl][e NB + il], zero below its diagonal
                    const int il = qr * 32 + 16 * x + lk + 4 * q, cl = (int)cc;
                    const double v = lt_src[(size_t)(j0 + cl) * n + lt_e * NB + il];
                    cold_t[x][y][q] = (j > lt_e || cl >= il) ? v : 0.0;
                } else cold_t[x][y][q] = S[rr * n + j0 + cc];
                if (LAST) cold_d[x][y][q] = S[rr * n + row0 + cc];
            }
            acc_t[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
        }
    int seen = -2;
    if (j > k0) {
        // fine: term k of the gather needs tile (j, k) of block row j only -- in memory as soon as that row has solved its column k,
        // long before it has announced all of them (the last column of a late row otherwise starts its r - 1 terms, 5 us each, only
        // when the row above has finished its own: 30 us in front of row 7's factor where rows 1-4 need 7, tools/df_trace.py)
        int *pc = pg + 2 * a.nb + j;
        int have = 0;                                                        // columns of row j known to be in memory
        if (a.fine) {
            have = df_wait(pc, k0 + 1, a.abort_w, &wslot[wc++ & 1]);
            if (have < 0) return false;
        } else {
            seen = df_wait(pg + j, j, a.abort_w, &wslot[wc++ & 1]);          // the panels of block row j are in memory
            if (seen < 0) return false;
        }
        DF_STAMP(trow, 5 * (j & 7) + 1);
        d2 vx[8], vl[8];
        auto gload = [&](int k) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                vl[i] = *reinterpret_cast<const d2 *>(S + (size_t)(j0 + sr + 8 * i) * n + k * NB + sc);
                vx[i] = *reinterpret_cast<const d2 *>(S + (size_t)(row0 + sr + 8 * i) * n + k * NB + sc);
            }
        };
        gload(k0);
        for (int k = k0; k < j; ++k) {
            if (k > k0) __syncthreads();                    // everyone is done reading the previous tiles
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                Ls[sr + 8 * i][sc] = vl[i].x; Ls[sr + 8 * i][sc + 1] = vl[i].y;
                Xs[sr + 8 * i][sc] = vx[i].x; Xs[sr + 8 * i][sc + 1] = vx[i].y;
            }
            __syncthreads();
            if (k + 1 < j) {
                if (a.fine && have < k + 2) {
                    have = df_wait(pc, k + 2, a.abort_w, &wslot[wc++ & 1]);
                    if (have < 0) return false;
                }
                gload(k + 1);                               // in flight behind this step's MFMAs
            }
#pragma unroll 4
            for (int ks = 0; ks < NB / 4; ++ks) {
                double bl[2], ax[2], bx[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    bl[x] = Ls[qc * 32 + 16 * x + lr][4 * ks + lk];            // B[k][col] = L(j,k)[col][k]
                    ax[x] = Xs[qr * 32 + 16 * x + lr][4 * ks + lk];
                    bx[x] = do_d ? Xs[qc * 32 + 16 * x + lr][4 * ks + lk] : 0.0;
                }
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc_t[x][y] = mfma_f64(ax[x], bl[y], acc_t[x][y]);
                if (do_d) {
#pragma unroll
                    for (int x = 0; x < 2; ++x)
#pragma unroll
                        for (int y = 0; y < 2; ++y) acc_d[x][y] = mfma_f64(ax[x], bx[y], acc_d[x][y]);
                }
            }
        }
        __syncthreads();
    }
    DF_STAMP(trow, 5 * (j & 7) + 2);
    // T into sm0
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Xs[qr * 32 + 16 * x + lk + 4 * q][qc * 32 + 16 * y + lr] = cold_t[x][y][q] - acc_t[x][y][q];
    if (seen < j + 1) {                                                       // L_jj and its inverted sub-blocks are in memory
        seen = df_wait(pg + j, j + 1, a.abort_w, &wslot[wc++ & 1]);
        if (seen < 0) return false;
    }
    DF_STAMP(trow, 5 * (j & 7) + 3);
    // -L_jj (exactly zero above the diagonal: the refinement step reads the diagonal blocks) into sm1
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = sr + 8 * i;
        const d2 v = *reinterpret_cast<const d2 *>(S + (size_t)(j0 + r) * n + j0 + sc);
        Ls[r][sc] = (sc <= r) ? -v.x : 0.0;
        Ls[r][sc + 1] = (sc + 1 <= r) ? -v.y : 0.0;
    }
    {
        const double *dv = dvb + (size_t)j * DF_DINV;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            Dv[e >> 8][(e >> 4) & 15][e & 15] = dv[e];
        }
    }
    __syncthreads();
    DF_STAMP(trow, 52 + (j & 7));
    // X(r,j) = T L_jj^-T (potrf_panel_kernel has the derivation)
    d4 Rt[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rt[s4][r] = Xs[16 * wave + lr][16 * s4 + 4 * r + lk];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        d4 x = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) x = mfma_f64(Dv[s4][lr][4 * ks + lk], Rt[s4][ks], x);
        d4 res = Rt[s4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) res = mfma_f64(Ls[16 * s4 + lr][16 * s4 + 4 * ks + lk], x[ks], res);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) x = mfma_f64(Dv[s4][lr][4 * ks + lk], res[ks], x);
        Rt[s4] = x;
#pragma unroll
        for (int t = s4 + 1; t < 4; ++t)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) Rt[t] = mfma_f64(Ls[16 * t + lr][16 * s4 + 4 * ks + lk], x[ks], Rt[t]);
    }
    double *Rl = S + (size_t)(row0 + 16 * wave + lr) * n + j0 + lk;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rl[16 * s4 + 4 * r] = Rt[s4][r];
    if (!LAST && xt_row) {                                 // block (j, e) of L^-1 = X(e,j)^T: 128-byte runs along lr
        double *Tl = xt_row + (size_t)(j0 + lk) * n + 16 * wave + lr;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int r = 0; r < 4; ++r) Tl[(size_t)(16 * s4 + 4 * r) * n] = Rt[s4][r];
    }
    if (LAST) {
        // the newest term of S_rr comes from the tile just solved (each wavefront rewrites its own 16 rows of sm0, which it
        // alone has read)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int r = 0; r < 4; ++r) Xs[16 * wave + lr][16 * s4 + 4 * r + lk] = Rt[s4][r];
        // X(r,j) is in sm0 for everyone; the global stores stay in flight (the caller waits for them in front of the barrier
        // that publishes them): a barrier that orders the LDS traffic only
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    } else if (EARLY) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int r = 0; r < 4; ++r) Xs[16 * wave + lr][16 * s4 + 4 * r + lk] = Rt[s4][r];
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 64) df_publish(pg + 2 * a.nb + row0 / NB, j + 1);           // column j of this row is in memory -- say so
        if (tri) {
#pragma unroll 4
            for (int ks = 0; ks < NB / 4; ++ks) {
                double ax[2], bx[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    ax[x] = Xs[qr * 32 + 16 * x + lr][4 * ks + lk];
                    bx[x] = Xs[qc * 32 + 16 * x + lr][4 * ks + lk];
                }
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc_d[x][y] = mfma_f64(ax[x], bx[y], acc_d[x][y]);
            }
        }
        __syncthreads();                                   // sm0 / sm1 are free for the next column
    } else {
        if (a.fine && row0 < n) {                          // (a main row without the early sums: not used by the kernel below)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 64) df_publish(pg + 2 * a.nb + row0 / NB, j + 1);
        } else __syncthreads();                            // sm0 / sm1 are free for the next column
    }
    DF_STAMP(trow, 5 * (j & 7) + 4);
    return true;
}

// An extra-row block of which only the FIRST row is live (the row b of the ELBO: b <- b L^-T, of which the caller reads
// |b L^-T|^2): a vector walks the block columns instead of a 64-row panel -- per column a few 64 x 64 matrix-vector products
// (each wavefront a quarter of every term's inner range, partial sums through LDS) and a 64-step forward substitution in one
// wavefront -- 1/64 of the panel's work and operand traffic.  It keeps up with the diagonal blocks however late its workgroup
// starts (about 5 us per column), so the launch ends a substitution after the last diagonal factor instead of a 7-term panel
// gather (30 us at 128 matrices).  The other 63 rows of the block are not touched.
__device__ __forceinline__ void df_vector_row(const DfArgs &a, double *S, int *pg, const double *dvb, const int row0, const int b,
                                              double *xv /* [n] */, double (*Ls)[LL_LD], double *part /* [4][64] */,
                                              double *invd /* [64] */, int *wslot) {
    const int n = a.n, nb = a.nb, tid = threadIdx.x, c = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sr = tid >> 5, sc = 2 * (tid & 31);
    double *v = S + (size_t)row0 * n;
    int wc = 0;
    for (int j = 0; j < nb; ++j) {
        const int j0 = j * NB;
        const double vj = v[j0 + c];                        // this row is nobody else's
        double acc = 0.0;
        int seen = -2;
        if (j > 0) {
            seen = df_wait(pg + j, j, a.abort_w, &wslot[wc++ & 1]);          // the panels of block row j are in memory
            if (seen < 0) { if (tid == 0 && a.info) a.info[b] = -1; return; }
            const double *Lrow = S + (size_t)(j0 + c) * n + 16 * q;           // row c of block row j, this wavefront's quarter
            for (int k = 0; k < j; ++k) {
                const double *xp = xv + k * NB + 16 * q;
#pragma unroll
                for (int m = 0; m < 16; m += 2) {
                    const d2 l = *reinterpret_cast<const d2 *>(Lrow + k * NB + m);
                    acc = fma(xp[m], l.x, acc);
                    acc = fma(xp[m + 1], l.y, acc);
                }
            }
        }
        part[q * 64 + c] = acc;
        if (seen < j + 1) {                                                   // L_jj and its inverted sub-blocks are in memory
            seen = df_wait(pg + j, j + 1, a.abort_w, &wslot[wc++ & 1]);
            if (seen < 0) { if (tid == 0 && a.info) a.info[b] = -1; return; }
        } else __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = sr + 8 * i;
            const d2 l = *reinterpret_cast<const d2 *>(S + (size_t)(j0 + r) * n + j0 + sc);
            Ls[r][sc] = l.x; Ls[r][sc + 1] = l.y;
        }
        if (tid < 64) invd[tid] = dvb[(size_t)j * DF_DINV + ((tid >> 4) * 16 + (tid & 15)) * 16 + (tid & 15)];   // 1 / L_jj[c][c]
        __syncthreads();
        if (q == 0) {
            double t = vj - ((part[c] + part[64 + c]) + (part[128 + c] + part[192 + c]));
            double x = 0.0;
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                const double xm = readlane_f64(t, m) * invd[m];               // lane m's t is final at step m
                if (c == m) x = xm;
                if (c > m) t = fma(-xm, Ls[c][m], t);
            }
            v[j0 + c] = x;
            xv[j0 + c] = x;
        }
        __syncthreads();
    }
}

// Identity-row workgroup e, its row W(e, e..) = (L^-T)(e, .) complete: announce it, then form the tiles (e, f), f <= e, of
// A^-1 = L^-T L^-1 = W W^T:  (e,f) = sum_{j >= e} W(e,j) W(f,j)^T  (rows f < e belong to workgroups dispatched earlier).  The
// same staging loop as the panel gather; both triangles are written.  A separate product launch after the factorisation
// costs the K_uu chain 0.13-0.17 ms beside the K_fu build (its workgroups queue behind that kernel's), these tiles 0.04.
// DfArgs::kinv_help (every workgroup of the launch resident at once): main-row workgroup e, done with its own block row, takes
// the tiles (e, f) with e + f odd off identity-row workgroup e -- the most loaded one had 20 tile products behind the chain (60 us;
// half of them now), and the main rows had left the chip by then.
__device__ __forceinline__ bool df_inverse_tiles(const DfArgs &a, double *S, int *pg, const int b, const int e,
                                                 double (*Xs)[LL_LD], double (*Ls)[LL_LD], int *wslot, const bool helper = false) {
    const int n = a.n, nb = a.nb;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave >> 1, qc = wave & 1;
    const int sr = tid >> 5, sc = 2 * (tid & 31);
    int wc = 0;
    if (!helper) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wavefront's stores of the row have left it
        __syncthreads();
        if (tid == 0) df_publish(pg + nb + e, 1);
    } else if (e > 0) {                                         // (tile (0, 0) is even: row 0's helper has nothing to do)
        const int seen = df_wait(pg + nb + e, 1, a.abort_w, &wslot[wc++ & 1]);
        if (seen < 0) return false;
    }
    double *Kb = a.kinv + (size_t)b * a.kinv_stride;
    const double *We = S + (size_t)(n + e * NB) * n;
    for (int f = 0; f <= e; ++f) {
        if (a.kinv_help && (((e + f) & 1) != 0) != helper) continue;
        if (f < e) {
            const int seen = df_wait(pg + nb + f, 1, a.abort_w, &wslot[wc++ & 1]);
            if (seen < 0) return false;
        }
        const double *Wf = S + (size_t)(n + f * NB) * n;
        d4 acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
        d2 vx[8], vl[8];
        auto gload = [&](int j) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                vx[i] = *reinterpret_cast<const d2 *>(We + (size_t)(sr + 8 * i) * n + j * NB + sc);
                vl[i] = *reinterpret_cast<const d2 *>(Wf + (size_t)(sr + 8 * i) * n + j * NB + sc);
            }
        };
        gload(e);
        for (int j = e; j < nb; ++j) {
            __syncthreads();                                // everyone is done reading the previous tiles
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                Xs[sr + 8 * i][sc] = vx[i].x; Xs[sr + 8 * i][sc + 1] = vx[i].y;
                Ls[sr + 8 * i][sc] = vl[i].x; Ls[sr + 8 * i][sc + 1] = vl[i].y;
            }
            __syncthreads();
            if (j + 1 < nb) gload(j + 1);
#pragma unroll 4
            for (int ks = 0; ks < NB / 4; ++ks) {
                double ax[2], bl[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    ax[x] = Xs[qr * 32 + 16 * x + lr][4 * ks + lk];
                    bl[x] = Ls[qc * 32 + 16 * x + lr][4 * ks + lk];
                }
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = mfma_f64(ax[x], bl[y], acc[x][y]);
            }
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const size_t i = (size_t)(e * NB + qr * 32 + 16 * x + lk + 4 * q), jj = (size_t)(f * NB + qc * 32 + 16 * y + lr);
                    Kb[i * n + jj] = acc[x][y][q];
                    if (f < e) Kb[jj * n + i] = acc[x][y][q];
                }
    }
    return true;
}

template <bool PIPE>
__global__ __launch_bounds__(256, 2) void potrf_df_kernel(DfArgs a) {
    __shared__ double sm0[NB * LL_LD];      // X(r,k) tiles; then T = A(r,j) - sum and the solved X(r,j)
    __shared__ double sm1[NB * LL_LD];      // L(j,k) tiles; then -L_jj; at the end S_rr and its factor
    __shared__ double invd[NB];
    __shared__ double Dv[4][16][DV_LD];
    __shared__ int wslot[2];
    const int n = a.n, nb = a.nb;
    int grp, rem, ri;
    if (a.defer_ext) {
        // several groups with identity-structured rows: the main rows (and the tail rows) of EVERY group first, then the
        // identity-structured rows of every group -- those wait for diagonal blocks only, and behind the main rows of all matrices
        // they find them finished and hold their slot for a few microseconds per column instead of for the length of the chain
        const int rows_a = nb + a.next - a.nid, per_a = rows_a * a.G, n_a = ((a.batch + a.G - 1) / a.G) * per_a;
        if ((int)blockIdx.x < n_a) {
            grp = blockIdx.x / per_a; rem = blockIdx.x % per_a;
            const int rr = rem / a.G;
            ri = (rr < nb) ? rr : rr + a.nid;
        } else {
            const int id2 = blockIdx.x - n_a, per_b = a.nid * a.G;
            grp = id2 / per_b; rem = id2 % per_b;
            ri = nb + rem / a.G;
        }
    } else {
        const int per_group = (nb + a.next) * a.G;
        grp = blockIdx.x / per_group; rem = blockIdx.x % per_group;
        ri = rem / a.G;
    }
    const int b = grp * a.G + rem % a.G;
    if (b >= a.batch) return;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave >> 1, qc = wave & 1;
    double *S = a.A + (size_t)b * a.slab_stride;
    int *pg = a.prog + (size_t)b * DF_PS;
    double *dvb = a.dinv + (size_t)b * nb * DF_DINV;
    const bool main_row = ri < nb;
    int row0, k0 = 0, ncols;                // first row of the block row; first block column with non-zero X(r,k); columns to solve
    if (main_row) { row0 = ri * NB; ncols = ri; }
    else {
        const int e = ri - nb;
        row0 = n + e * NB; ncols = nb;
        if (e < a.nid) k0 = e;              // identity-structured rows: block e is zero left of block column e
    }
    double (*Xs)[LL_LD] = reinterpret_cast<double(*)[LL_LD]>(sm0);
    double (*Ls)[LL_LD] = reinterpret_cast<double(*)[LL_LD]>(sm1);
    if (!main_row && a.vec_tail && ri - nb >= a.nid) {
        df_vector_row(a, S, pg, dvb, row0, b, sm0, Ls, &Dv[0][0][0], invd, wslot);
        return;
    }
    int wc = 0;
    const int trow = (b == 0) ? ri : -1;
    DF_STAMP(trow, 51);
    // S_rr = A(r,r) - sum_{k<r} X(r,k) X(r,k)^T (main rows)
    d4 cold_d[2][2], acc_d[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc_d[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    {
        const int nplain = main_row ? ncols - 1 : ncols;
        double *xt_row = (a.xt && !main_row && ri - nb < a.nid) ? a.xt + (size_t)b * a.xt_stride + (size_t)(ri - nb) * NB : nullptr;
        const double *lt_src = (a.lt && !main_row && ri - nb < a.nid) ? a.lt + (size_t)(b % a.lt_dl) * a.lt_stride : nullptr;
        if (main_row && a.fine == 1) {
            for (int j = 0; j < nplain; ++j) {
                if (!df_column<false, true>(a, S, pg, dvb, row0, j, 0, Xs, Ls, Dv, wslot, wc, cold_d, acc_d, trow)) {
                    if (tid == 0 && a.info) a.info[b] = -1;
                    return;
                }
            }
        } else {
            for (int j = k0; j < nplain; ++j) {
                d4 unused_c[2][2], unused_a[2][2];
                if (!df_column<false>(a, S, pg, dvb, row0, j, k0, Xs, Ls, Dv, wslot, wc, unused_c, unused_a, trow, xt_row, lt_src,
                                      ri - nb)) {
                    if (tid == 0 && a.info) a.info[b] = -1;
                    return;
                }
            }
        }
    }
    if (!main_row) {
        if (a.kinv && ri - nb < a.nid && !df_inverse_tiles(a, S, pg, b, ri - nb, Xs, Ls, wslot)) {
            if (tid == 0 && a.info) a.info[b] = -1;
        }
        return;
    }
    if (ncols > 0) {
        if (!df_column<true>(a, S, pg, dvb, row0, ncols - 1, k0, Xs, Ls, Dv, wslot, wc, cold_d, acc_d, trow)) {
            if (tid == 0 && a.info) a.info[b] = -1;
            return;
        }
        if (!(qr == 0 && qc == 1)) {
#pragma unroll 4
            for (int ks = 0; ks < NB / 4; ++ks) {
                double ax[2], bx[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    ax[x] = Xs[qr * 32 + 16 * x + lr][4 * ks + lk];
                    bx[x] = Xs[qc * 32 + 16 * x + lr][4 * ks + lk];
                }
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc_d[x][y] = mfma_f64(ax[x], bx[y], acc_d[x][y]);
            }
        }
    } else {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    cold_d[x][y][q] = S[(size_t)(row0 + qr * 32 + 16 * x + lk + 4 * q) * n + row0 + qc * 32 + 16 * y + lr];
    }
    double (*Ts)[NB + 1] = reinterpret_cast<double(*)[NB + 1]>(sm1);     // -L_jj is no longer needed (all past the solve)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Ts[qr * 32 + 16 * x + lk + 4 * q][qc * 32 + 16 * y + lr] = cold_d[x][y][q] - acc_d[x][y][q];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's panel stores have left it (published below)
    __syncthreads();                                      // ... and everyone is done with X(r,j) in sm0: the factor goes there
    double (*Lr)[LR_LD] = reinterpret_cast<double(*)[LR_LD]>(sm0);
    DF_STAMP(trow, 48);
    // the panels of this row are published by wavefront 1 while wavefront 0 runs the pivot chain
    if (ncols > 0 && tid == 64) {
        df_publish(pg + ri, ri);
        if (a.fine) __hip_atomic_store(pg + 2 * nb + ri, ri, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (behind the release above)
    }
    diag_block_finish<PIPE>(Ts, Lr, invd, S, n, row0, a.info + b, dvb + (size_t)ri * DF_DINV, Dv);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    DF_STAMP(trow, 49);
#ifdef FFVD_DF_TEST_STALL
    if (b == 0 && ri == 0) return;      // test build (tests/test_gpu_ops.py): matrix 0 never announces its first diagonal block
#endif
    if (tid == 0) df_publish(pg + ri, ri + 1);
    DF_STAMP(trow, 50);
    if (a.kinv_help) {
        __syncthreads();                                      // (LDS of the diagonal factor is free again)
        if (!df_inverse_tiles(a, S, pg, b, ri, Xs, Ls, wslot, true)) {
            if (tid == 0 && a.info) a.info[b] = -1;
        }
    }
}

// Diagonal block k of every matrix, factorised by a launch of its own: the first launch of both launch-per-step variants
// (potrf.hip enqueues it; potrf_blocks.h declares it).  It is defined in this file on purpose.  It and the dataflow kernel are the
// callers of diag_block_finish<true>; where the dataflow kernel is that template's ONLY caller in its unit, hipcc specialises the
// template for the one call before inlining it and emits other (equivalent, 58 instructions shorter) code for the dataflow
// kernel than it did while all Cholesky kernels shared a unit.  With this second caller beside it the kernel's code is unchanged.
__global__ __launch_bounds__(256) void potrf_diag_kernel(double *A, int n, int k, size_t slab_stride, int32_t *info,
                                                         double *dinv) {
    __shared__ double Ts[NB][NB + 1];
    __shared__ double Lr[NB][LR_LD];
    __shared__ double invd[NB];
    const int b = blockIdx.x, tid = threadIdx.x;
    double *S = A + (size_t)b * slab_stride;
    const int k0 = k * NB;
    for (int r = tid >> 6; r < NB; r += 4) Ts[r][tid & 63] = S[(size_t)(k0 + r) * n + k0 + (tid & 63)];
    __syncthreads();
    diag_block_finish<true>(Ts, Lr, invd, S, n, k0, info + b, dinv + (size_t)b * DINV_STRIDE);
}

size_t potrf_flow_scratch_doubles(int n, int batch) {
    return potrf_flow_words(batch) / 2 + (size_t)batch * (size_t)(n / NB) * DF_DINV;
}

// Zero the progress words of a dataflow launch for `batch` matrices (they sit at the start of the scratch block, padded to 16
// bytes).  launch_potrf_ext does this itself unless told that the caller already has (words_zeroed).
void potrf_flow_clear(hipStream_t stream, double *scratch, int batch) {
    // our own fill kernel, not hipMemsetAsync: in front of a 16-matrix factorisation the runtime's memset started 40 us after
    // the kernel before it had finished (tools/prof_timeline.sh, SYNC_S=4)
    launch_fill(stream, scratch, potrf_flow_words(batch) / 2, 0.0);
}

void launch_potrf_flow(hipStream_t stream, double *A, int n, int extra_rows, int identity_rows, int batch,
                       size_t slab_stride, int32_t *info, double *scratch, double *linv_t, size_t linv_t_stride,
                       bool words_zeroed, bool tail_is_vector, double *kinv, size_t kinv_stride, const double *lt_rows,
                       size_t lt_stride, int lt_dl, bool kinv_help) {
    DfArgs a{};
    a.lt = lt_rows; a.lt_stride = lt_stride; a.lt_dl = lt_dl > 0 ? lt_dl : 1;
    a.xt = linv_t; a.xt_stride = linv_t_stride;
    a.vec_tail = tail_is_vector ? 1 : 0;
    if (kinv && identity_rows == n && 2 * (n / NB) <= DF_PS) { a.kinv = kinv; a.kinv_stride = kinv_stride; }
    a.A = A; a.n = n; a.nb = n / NB; a.next = extra_rows / NB; a.nid = identity_rows / NB; a.batch = batch;
    a.slab_stride = slab_stride; a.info = info;
    // the polled words sit at the start of the scratch block, padded to 16 bytes, and are zeroed before every launch
    a.prog = reinterpret_cast<int *>(scratch);
    a.abort_w = a.prog + (size_t)batch * DF_PS;
    a.dinv = scratch + potrf_flow_words(batch) / 2;
    if (!words_zeroed) potrf_flow_clear(stream, scratch, batch);
    const int R = a.nb + a.next, bp = (batch + 7) / 8 * 8;
    // all matrices in lockstep while the grid is a few rounds of the chip (rows leave early and make room); beyond that,
    // groups of about two chip-fulls of block rows, so that the rows of one matrix run together (they share L(j,k) in L2)
    a.G = ((size_t)bp * R <= 2048) ? bp : ((1024 / R + 7) / 8 * 8 < 8 ? 8 : (1024 / R + 7) / 8 * 8);
    if (a.G > bp) a.G = bp;
    const int groups = (batch + a.G - 1) / a.G;
    static const int defer_mode = [] { const char *e = getenv("FFVD_DF_DEFER"); return e ? atoi(e) : -1; }();
    a.defer_ext = (a.nid > 0 && groups > 1 && !a.xt && !a.kinv && defer_mode != 0) ? 1 : 0;
    // Few matrices (every block row finds a CU of its own): 16 KB of unused dynamic LDS keep a second workgroup off the CU --
    // a pivot chain that shares its SIMD with another row's MFMA loop takes up to twice as long (tools/df_trace.py)
    // (... and up to 640 block rows without identity-structured rows -- 64 matrices of a 16-chain rank: 1.87 vs 1.945 ms per iteration with
    //  one row per compute unit; 288 and 432 rows no difference, 864 none, 1152 rows 2 % slower: profiles/r04_ab_df_pad.txt)
    const bool one_per_cu = (size_t)batch * R <= 256 || (a.nid == 0 && (size_t)batch * R <= 640);
    a.kinv_help = (kinv_help && a.kinv && a.nid == a.nb && (size_t)batch * R <= 256) ? 1 : 0;
    const bool alone = one_per_cu;
    const int fine_mode = [] { const char *e = getenv("FFVD_DF_FINE"); return e ? atoi(e) : -1; }();      // (read per launch: tests switch it)
    a.fine = ((fine_mode >= 0 ? fine_mode != 0 : (alone && (size_t)batch * R <= 256)) && 3 * a.nb <= DF_PS) ? (fine_mode == 2 ? 2 : 1) : 0;    // (2: A/B, no early sums)
    hipLaunchKernelGGL(potrf_df_kernel<true>, dim3((unsigned)((size_t)groups * R * a.G)), dim3(256), alone ? 16384 : 0, stream, a);
}

}  // namespace ffvd
