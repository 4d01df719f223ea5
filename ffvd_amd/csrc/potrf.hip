// Extended blocked Cholesky of a batch (gfx950, fp64): the two launch-per-step variants and the choice between all three.
// "Extended": rows stored below the matrix ride through the factorisation as a right-hand side -- identity rows become L^{-T},
// the row delta^T F / Q becomes L_H^{-1} b (kernels.h, launch_potrf_ext).
//   right-looking  potrf_diag / potrf_panel / potrf_trail, two launches per block step: the few matrices of the K_uu chain
//   left-looking   potrf_ll_kernel, one launch per block column: re-runs a batch whose dataflow launch gave up, and n > 4096
//   dataflow       potrf_flow.hip, one launch per batch: wherever the factorisation is on the critical path
// Reference: conditionals_multi_output.py:159-166 (K3/K4: chol(K_uu + jitter I), L^{-T}), :253-254 (K9/K10: the factor of H).
// DESIGN.md section 4 describes the variants, section 5 has their measurements.
#include "potrf_blocks.h"
#include <cstdlib>

namespace ffvd {

// ---------------------------------------------------------------------------------------------
// Extended blocked Cholesky (right-looking, NB = 64), two launches per block step:
//   panel(k):  rows below the diagonal block  R <- R * L_kk^{-T}   (forward substitution, lane = row,
//              L_kk broadcast from LDS; one wavefront per 64 rows)
//   trail(k):  C(i,j) -= P_i P_j^T for the remaining tiles (one workgroup per 64x64 tile, MFMA); the workgroup
//              of tile (k+1,k+1) goes on to factorise that diagonal block (look-ahead inside the launch)
// The 64x64 diagonal factorisation runs in ONE workgroup (lane = row, 16 row entries per lane in registers, pivot
// column broadcast through LDS), and no other workgroup reads a diagonal block before a finished launch has
// published its factor.
// ---------------------------------------------------------------------------------------------
// (potrf_diag_kernel, the first launch of both variants, is defined in potrf_flow.hip, which says why.)

// tile bookkeeping shared by the panel and trailing kernels
// Extra-row blocks: the first `nid` blocks are identity-structured (block e is still zero in block-columns < e,
// so only e <= k is live at step k: `nlive` of them), the blocks after them are always live.
__device__ __forceinline__ int extra_block(int e, int nlive, int nid) { return (e < nlive) ? e : nid + (e - nlive); }
__device__ __forceinline__ int chunk_row0(int chunk, int k, int nmain, int n, int nlive, int nid) {
    return (chunk < nmain) ? (k + 1 + chunk) * NB : n + extra_block(chunk - nmain, nlive, nid) * NB;
}

constexpr int TR_LD = NB + 2;      // LDS row stride of the staged panel blocks (doubles)

// R <- R * L_kk^{-T} for one 64-row chunk, as a blocked substitution on the matrix cores.  With L_kk cut into 16x16
// blocks and X = R L_kk^{-T}:   X_s^T = L_ss^{-1} (R_s^T - sum_{m<s} L_sm X_m^T).
// Wavefront w owns rows 16w..16w+15 of the chunk and keeps the four TRANSPOSED 16x16 blocks R_s^T in the MFMA
// accumulator layout, which is exactly the B-operand layout of the next product, so the whole chain
// (4 multiplications by the inverted diagonal blocks from diag_block_finish + 6 block updates) runs register to
// register with the A operands (-L_ts, L_ss^{-1}) read from LDS: 40 MFMAs per wavefront instead of a 64-step scalar
// forward substitution.
__global__ __launch_bounds__(256) void potrf_panel_kernel(double *A, int n, int k, int nmain, size_t slab_stride,
                                                          int nlive, int nid, const double *dinv) {
    __shared__ double Ls[NB][TR_LD];       // -L_kk (only blocks below the block diagonal are read)
    __shared__ double Dv[4][16][DV_LD];    // inverses of the four 16x16 diagonal blocks of L_kk
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *S = A + (size_t)b * slab_stride;
    const int k0 = k * NB;
    const int row0 = chunk_row0(blockIdx.x, k, nmain, n, nlive, nid);
    // this lane's 16 entries: R[row0 + 16w + lr][k0 + 16s + 4r + lk]  (32-byte runs per row)
    double *Rl = S + (size_t)(row0 + 16 * w + lr) * n + k0 + lk;
    d4 Rt[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rt[s4][r] = Rl[16 * s4 + 4 * r];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = (tid >> 5) + 8 * i, c2 = 2 * (tid & 31);
        const double2 v = *reinterpret_cast<const double2 *>(S + (size_t)(k0 + r) * n + k0 + c2);
        Ls[r][c2] = (c2 <= r) ? -v.x : 0.0;              // the block's upper triangle holds don't-care values
        Ls[r][c2 + 1] = (c2 + 1 <= r) ? -v.y : 0.0;
    }
    {
        const double *dv = dinv + (size_t)b * DINV_STRIDE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            Dv[e >> 8][(e >> 4) & 15][e & 15] = dv[e];
        }
    }
    __syncthreads();
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        d4 x = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) x = mfma_f64(Dv[s4][lr][4 * ks + lk], Rt[s4][ks], x);
        // one step of iterative refinement: multiplying by an explicit inverse is not backward stable, a
        // substitution is; the residual B - L_ss X brings the product back to substitution accuracy
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
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rl[16 * s4 + 4 * r] = Rt[s4][r];
}

// Trailing update of step k: one workgroup (4 wavefronts, a 32x32 quadrant each) per 64x64 tile,
// C(i,j) -= P_i * P_j^T with P = solved panel, both panel blocks staged through LDS with wide coalesced loads.
// Tiles: main lower triangle (k < j <= i < nb) then extra-row tiles (e, j) for j in (k, nb).
// Tile 0 is the next diagonal block (k+1,k+1): wavefront 0 of its workgroup factorises it right away, so the
// 64-pivot chain of step k+1 overlaps with the rest of step k's trailing update (look-ahead inside one launch).
template <bool PIPE>
__global__ __launch_bounds__(256) void potrf_trail_kernel(double *A, int n, int k, int nmain_tiles, int n1,
                                                          size_t slab_stride, int32_t *info, int nlive, int nid,
                                                          double *dinv) {
    // One 34.8 KB LDS buffer: the panel blocks are staged in two 32-column halves (Pi half | Pj half), so that three
    // workgroups fit on a CU; the look-ahead tile later reuses the same memory as its 64 x 66 factor tile.
    constexpr int HLD = 34;                               // row stride of a staged half (doubles)
    __shared__ double sm[2 * NB * HLD];
    __shared__ double invd[NB];
    static_assert(2 * NB * HLD >= NB * LR_LD, "the staging buffer must hold the factor tile");
    double *Pi_h = sm, *Pj_h = sm + NB * HLD;
    const int b = blockIdx.y;
    const int tile = blockIdx.x;
    double *S = A + (size_t)b * slab_stride;
    const int k0 = k * NB;
    int rowblk0, colblk;   // first row / first col of the tile
    if (tile < nmain_tiles) {
        int i = 0;          // unrank lower triangle: tile = i(i+1)/2 + j
        while ((i + 1) * (i + 2) / 2 <= tile) ++i;
        int j = tile - i * (i + 1) / 2;
        rowblk0 = (k + 1 + i) * NB;
        colblk = (k + 1 + j) * NB;
    } else {
        int t = tile - nmain_tiles;
        int e = t / n1, j = t % n1;
        rowblk0 = n + extra_block(e, nlive, nid) * NB;
        colblk = (k + 1 + j) * NB;
    }
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave >> 1, qc = wave & 1;          // 32x32 quadrant of the tile
    const bool same = (rowblk0 == colblk);
    const double *Pi = S + (size_t)rowblk0 * n + k0;
    const double *Pj = S + (size_t)colblk * n + k0;
    // global -> registers for both halves at once: thread t moves 16 bytes of rows (t >> 4) + 16 i, columns
    // 32 h + 2 (t & 15) of each operand
    const int sr = tid >> 4, sc = 2 * (tid & 15);
    double2 vi[2][4], vj[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            vi[h][i] = *reinterpret_cast<const double2 *>(Pi + (size_t)(sr + 16 * i) * n + 32 * h + sc);
            if (!same) vj[h][i] = *reinterpret_cast<const double2 *>(Pj + (size_t)(sr + 16 * i) * n + 32 * h + sc);
        }
    const double *Bh = same ? Pi_h : Pj_h;
    // the tile itself is requested now, so that its latency hides behind the staging and the MFMAs
    double *Ct = S + (size_t)rowblk0 * n + colblk;
    d4 cold[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                cold[x][y][q] = Ct[(size_t)(qr * 32 + 16 * x + lk + 4 * q) * n + qc * 32 + 16 * y + lr];
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h) __syncthreads();                        // everyone is done reading the first half
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Pi_h[(sr + 16 * i) * HLD + sc] = vi[h][i].x; Pi_h[(sr + 16 * i) * HLD + sc + 1] = vi[h][i].y;
            if (!same) { Pj_h[(sr + 16 * i) * HLD + sc] = vj[h][i].x; Pj_h[(sr + 16 * i) * HLD + sc + 1] = vj[h][i].y; }
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < NB / 8; ++ks) {
            double af[2], bf[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                af[x] = Pi_h[(qr * 32 + 16 * x + lr) * HLD + 4 * ks + lk];     // A[row][k]
                bf[x] = Bh[(qc * 32 + 16 * x + lr) * HLD + 4 * ks + lk];       // B[k][col] = P_j[col][k]
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
        }
    }
    if (tile != 0) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const size_t off = (size_t)(qr * 32 + 16 * x + lk + 4 * q) * n + qc * 32 + 16 * y + lr;
                    Ct[off] = cold[x][y][q] - acc[x][y][q];
                }
        return;
    }
    // tile 0 = next diagonal block: assemble the updated block in LDS, factorise, publish.  The factor tile Lr
    // (stride 66) reuses the memory of the input tile Ts (stride 65): wavefront 0 has the whole input in registers
    // before it writes the first column of L.
    __syncthreads();
    double(*Ts)[NB + 1] = reinterpret_cast<double(*)[NB + 1]>(sm);
    double(*Lr)[LR_LD] = reinterpret_cast<double(*)[LR_LD]>(sm);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = qr * 32 + 16 * x + lk + 4 * q, cc = qc * 32 + 16 * y + lr;
                Ts[r][cc] = cold[x][y][q] - acc[x][y][q];
            }
    __syncthreads();
    diag_block_finish<PIPE>(Ts, Lr, invd, S, n, k0 + NB, info + b, dinv + (size_t)b * DINV_STRIDE);
}

// ---------------------------------------------------------------------------------------------
// Left-looking block column (the default since round 2; north_star: "blocked left-looking Cholesky with wavefront-level
// trsm").  After potrf_diag_kernel has factorised block (0,0): ONE launch per block column j, one workgroup per
// 64-row block r below the diagonal (main rows j+1..nb-1 and the live extra-row blocks), no dependency between the
// workgroups of a launch:
//     X(r,j) = (A(r,j) - sum_{k<j} X(r,k) L(j,k)^T) L_jj^-T        gathered from the finished block columns, then a
//                                                                  blocked substitution on the matrix cores
// and the workgroup of row j+1 goes on (look-ahead): it also sums X(j+1,k) X(j+1,k)^T over k <= j, factorises
// S = A(j+1,j+1) - sum in its first wavefront and publishes L_{j+1,j+1} for the next launch.
// Each block of the matrix is written ONCE (the right-looking variant re-reads and re-writes the whole trailing matrix at
// every step: 1.4 GB of tile traffic per factorisation of the 128 A-matrices of config 2 against 0.64 GB here) and a
// step is one launch instead of two.  Both operand tiles of step k sit in LDS whole (stride 66: conflict-free fragment
// reads); the global loads of step k+1 are issued before the MFMAs of step k.
// A first draft let EVERY workgroup factorise S_jj itself (no look-ahead, no diagonal launch): each workgroup then holds
// its slot for the 13 us pivot chain and the 5632 workgroup executions of one 128-matrix factorisation took 1.14 ms
// against the right-looking 0.63 ms.
// ---------------------------------------------------------------------------------------------
template <bool PIPE>
__global__ __launch_bounds__(256) void potrf_ll_kernel(double *A, int n, int j, int nmain, int nchunks, size_t slab_stride,
                                                       int32_t *info, int nlive, int nid, int batch, double *dinv) {
    __shared__ double sm0[NB * LL_LD];      // X(r,k) tiles; then T = A(r,j) - sum and the solved X(r,j)
    __shared__ double sm1[NB * LL_LD];      // L(j,k) tiles; then -L_jj; then (look-ahead) S_{j+1,j+1} and its factor
    __shared__ double invd[NB];
    __shared__ double Dv[4][16][DV_LD];
    // chunk-major order: the look-ahead workgroups (chunk 0) of ALL matrices are dispatched first -- their pivot chain is
    // the tail of the launch.  XCD-aware: the batch is padded to a multiple of 8, so all workgroups of one matrix share
    // blockIdx % 8, i.e. one XCD's L2 (they all read row block j).
    const int bpad = (int)(gridDim.x / nchunks);
    const int chunk = blockIdx.x / bpad, b = blockIdx.x % bpad;
    if (b >= batch) return;
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qr = wave >> 1, qc = wave & 1;
    double *S = A + (size_t)b * slab_stride;
    const int j0 = j * NB;
    const bool look = (chunk == 0 && nmain > 0);        // row block j + 1: also factorises the next diagonal block
    int row0, k0 = 0;                       // first row of this workgroup's block; first block column with non-zero X(r,k)
    if (chunk < nmain) row0 = (j + 1 + chunk) * NB;
    else {
        const int e = extra_block(chunk - nmain, nlive, nid);
        row0 = n + e * NB;
        if (e < nid) k0 = e;                // identity-structured rows: block e is zero left of block column e
    }
    double (*Xs)[LL_LD] = reinterpret_cast<double(*)[LL_LD]>(sm0);
    double (*Ls)[LL_LD] = reinterpret_cast<double(*)[LL_LD]>(sm1);
    // the output tile(s) are requested first: their latency hides behind the whole k loop
    d4 cold_t[2][2], cold_d[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t rr = (size_t)(qr * 32 + 16 * x + lk + 4 * q), cc = (size_t)(qc * 32 + 16 * y + lr);
                cold_t[x][y][q] = S[(row0 + rr) * n + j0 + cc];
                cold_d[x][y][q] = look ? S[(row0 + rr) * n + row0 + cc] : 0.0;
            }
    d4 acc_t[2][2], acc_d[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) { acc_t[x][y] = (d4){0.0, 0.0, 0.0, 0.0}; acc_d[x][y] = (d4){0.0, 0.0, 0.0, 0.0}; }
    // staging: thread moves 16 bytes of rows (tid >> 5) + 8 i, columns 2 (tid & 31) of each operand
    const int sr = tid >> 5, sc = 2 * (tid & 31);
    d2 vx[8], vl[8];
    auto gload = [&](int k) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            vl[i] = *reinterpret_cast<const d2 *>(S + (size_t)(j0 + sr + 8 * i) * n + k * NB + sc);
            vx[i] = *reinterpret_cast<const d2 *>(S + (size_t)(row0 + sr + 8 * i) * n + k * NB + sc);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            Ls[sr + 8 * i][sc] = vl[i].x; Ls[sr + 8 * i][sc + 1] = vl[i].y;
            Xs[sr + 8 * i][sc] = vx[i].x; Xs[sr + 8 * i][sc + 1] = vx[i].y;
        }
    };
    const bool do_d = look && !(qr == 0 && qc == 1);    // the quadrant above the diagonal of S is never read
    if (k0 < j) gload(k0);
    for (int k = k0; k < j; ++k) {
        if (k > k0) __syncthreads();                // everyone is done reading the previous tiles
        lstore();
        __syncthreads();
        if (k + 1 < j) gload(k + 1);                // in flight behind this step's MFMAs
#pragma unroll 4
        for (int ks = 0; ks < NB / 4; ++ks) {
            double bl[2], ax[2], bx[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                bl[x] = Ls[qc * 32 + 16 * x + lr][4 * ks + lk];        // B[k][col] = L(j,k)[col][k]
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
    if (k0 < j) __syncthreads();
    // T into sm0; -L_jj (exactly zero above the diagonal: the refinement step reads the diagonal blocks) into sm1; the
    // inverted 16 x 16 diagonal sub-blocks of L_jj, left in the scratch block by the workgroup that factorised it
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Xs[qr * 32 + 16 * x + lk + 4 * q][qc * 32 + 16 * y + lr] = cold_t[x][y][q] - acc_t[x][y][q];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = sr + 8 * i;
        const d2 v = *reinterpret_cast<const d2 *>(S + (size_t)(j0 + r) * n + j0 + sc);
        Ls[r][sc] = (sc <= r) ? -v.x : 0.0;
        Ls[r][sc + 1] = (sc + 1 <= r) ? -v.y : 0.0;
    }
    {
        // slot j & 1: the look-ahead workgroup of THIS launch writes the other slot while late workgroups still read this one
        const double *dv = dinv + (size_t)b * DINV_STRIDE + (j & 1) * (DINV_STRIDE / 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            Dv[e >> 8][(e >> 4) & 15][e & 15] = dv[e];
        }
    }
    __syncthreads();
    // X(r,j) = T L_jj^-T: wavefront w owns rows 16w..16w+15, the four transposed 16 x 16 blocks in the MFMA accumulator
    // layout (potrf_panel_kernel has the derivation): 4 multiplications by the inverted diagonal blocks, one residual
    // refinement each, 6 block updates
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
    if (!look) return;
    // look-ahead: S = A(j+1,j+1) - sum_{k<=j} X(j+1,k) X(j+1,k)^T; the newest term comes from the tile just solved
    // (each wavefront rewrites its own 16 rows of sm0, which it alone has read)
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[16 * wave + lr][16 * s4 + 4 * r + lk] = Rt[s4][r];
    __syncthreads();
    if (do_d) {
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
    double (*Ts)[NB + 1] = reinterpret_cast<double(*)[NB + 1]>(sm1);     // -L_jj is no longer needed (all past the solve:
    double (*Lr)[LR_LD] = reinterpret_cast<double(*)[LR_LD]>(sm1);        //  the barrier above)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Ts[qr * 32 + 16 * x + lk + 4 * q][qc * 32 + 16 * y + lr] = cold_d[x][y][q] - acc_d[x][y][q];
    __syncthreads();
    diag_block_finish<PIPE>(Ts, Lr, invd, S, n, j0 + NB, info + b, dinv + (size_t)b * DINV_STRIDE + ((j + 1) & 1) * (DINV_STRIDE / 2));
}

// Inverses of the four 16 x 16 diagonal sub-blocks of the GIVEN factor block L_jj into scratch slot j & 1 (what
// diag_block_finish leaves behind when it has just factorised the block): lets the block-column kernel run as a plain
// triangular solve against a factor that already exists (launch_trsm_ext).
__global__ __launch_bounds__(256) void diag_inv_kernel(const double *A, int n, int j, size_t slab_stride, double *dinv) {
    __shared__ double Lr[NB][NB + 1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *S = A + (size_t)b * slab_stride;
    const int j0 = j * NB;
    for (int r = tid >> 6; r < NB; r += 4) Lr[r][lane] = S[(size_t)(j0 + r) * n + j0 + lane];
    __syncthreads();
    if (lane < 16) {
        const int o = 16 * w;
        double x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            double acc = (lane == r) ? 1.0 : 0.0;
#pragma unroll
            for (int i = 0; i < r; ++i) acc -= Lr[o + r][o + i] * x[i];
            x[r] = acc / Lr[o + r][o + r];
        }
        double *dv = dinv + (size_t)b * DINV_STRIDE + (j & 1) * (DINV_STRIDE / 2);
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[(w * 16 + r) * 16 + lane] = x[r];
    }
}

// R <- R L^-T for `extra_rows` rows stored below an n x n lower-triangular factor L in every slab (ld n): the
// block-column kernel without its factorisation part, one launch pair per block column.
void launch_trsm_ext(hipStream_t stream, double *A, int n, int extra_rows, int batch, size_t slab_stride, double *dinv) {
    const int nb = n / NB, ntail = extra_rows / NB;
    if (ntail == 0) return;
    const int groups = (batch + 7) / 8;
    for (int j = 0; j < nb; ++j) {
        hipLaunchKernelGGL(diag_inv_kernel, dim3(batch), dim3(256), 0, stream, A, n, j, slab_stride, dinv);
        hipLaunchKernelGGL(potrf_ll_kernel<false>, dim3(groups * 8 * ntail), dim3(256), 0, stream, A, n, j, 0, ntail,
                           slab_stride, (int32_t *)nullptr, 0, 0, batch, dinv);
    }
}

// Which blocked variant factorises a batch: the dataflow kernel (one launch, rows handing blocks to each other) wherever the
// factorisation sits on the critical path; the right-looking launches for the few matrices of the K_uu chain, whose small
// workgroups slip in beside the Gram kernel when the chain runs on the side stream (the 76.8 KB / 256-VGPR row workgroups of the
// other two variants would wait for that kernel to drain).  The per-column left-looking launches (round 2's first variant)
// stay selectable.  FFVD_CHOL=flow|left|right forces one (read once).
static int chol_mode() {                    // 0 = auto, 1 = left-looking launches, 2 = right-looking launches, 3 = dataflow
    static const int v = [] {
        const char *e = getenv("FFVD_CHOL");
        if (!e) return 0;
        return (e[0] == 'l') ? 1 : ((e[0] == 'r') ? 2 : ((e[0] == 'f') ? 3 : 0));
    }();
    return v;
}
// Per-thread override (0 = none): the caller re-runs a batch whose dataflow launch gave up (a bounded wait fired) with one of
// the launch-per-step variants, which have no inter-workgroup waits and therefore cannot stall (abi.hip, stall recovery).
static thread_local int g_chol_override = 0;
void potrf_override_variant(int variant) { g_chol_override = variant; }
int potrf_override_current() { return g_chol_override; }
static int chol_variant(int batch, int nb, int hint);
bool potrf_flow_selected(int n, int batch, int hint) { return chol_variant(batch, n / NB, hint) == 3; }
bool potrf_flow_forms_inverse(int n, int batch, int hint) { return potrf_flow_selected(n, batch, hint) && 2 * (n / NB) <= DF_PS; }
static int chol_variant(int batch, int nb, int hint) {
    int m = g_chol_override ? g_chol_override : chol_mode();
    if (m == 0) m = (hint == CHOL_FLOW || batch >= 32) ? 3 : 2;
    if (m == 3 && nb > DF_PS) m = 1;
    return m;
}

size_t potrf_scratch_doubles(int n, int batch) {
    const int bt = batch > 0 ? batch : 1;
    const size_t flow = potrf_flow_scratch_doubles(n, bt);
    const size_t step = (size_t)bt * DINV_STRIDE;
    return flow > step ? flow : step;
}

void launch_potrf_ext(hipStream_t stream, double *A, int n, int extra_rows, int identity_rows, int batch,
                      size_t slab_stride, int32_t *info, double *dinv, int hint, double *linv_t, size_t linv_t_stride,
                      bool words_zeroed, bool tail_is_vector, double *kinv, size_t kinv_stride, const double *lt_rows,
                      size_t lt_stride, int lt_dl, bool kinv_help) {
    const int nb = n / NB;
    const int nid = identity_rows / NB, ntail = extra_rows / NB - nid;
    const int variant = chol_variant(batch, nb, hint);
    if (variant == 3) {
        launch_potrf_flow(stream, A, n, extra_rows, identity_rows, batch, slab_stride, info, dinv, linv_t, linv_t_stride, words_zeroed,
                          tail_is_vector, kinv, kinv_stride, lt_rows, lt_stride, lt_dl, kinv_help);
        return;
    }
    if (variant == 1) {
        const int groups = (batch + 7) / 8;
        hipLaunchKernelGGL(potrf_diag_kernel, dim3(batch), dim3(256), 0, stream, A, n, 0, slab_stride, info, dinv);
        for (int j = 0; j < nb; ++j) {
            const int nmain = nb - j - 1;
            const int nlive = (j + 1 < nid) ? j + 1 : nid;
            const int nchunks = nmain + nlive + ntail;
            if (nchunks == 0) continue;
            // few workgroups: the launch lasts as long as the look-ahead workgroup's 64-pivot chain -> pipelined factor variant
            if ((size_t)nchunks * batch <= 512)
                hipLaunchKernelGGL(potrf_ll_kernel<true>, dim3(groups * 8 * nchunks), dim3(256), 0, stream, A, n, j, nmain,
                                   nchunks, slab_stride, info, nlive, nid, batch, dinv);
            else
                hipLaunchKernelGGL(potrf_ll_kernel<false>, dim3(groups * 8 * nchunks), dim3(256), 0, stream, A, n, j, nmain,
                                   nchunks, slab_stride, info, nlive, nid, batch, dinv);
        }
        return;
    }
    hipLaunchKernelGGL(potrf_diag_kernel, dim3(batch), dim3(256), 0, stream, A, n, 0, slab_stride, info, dinv);
    for (int k = 0; k < nb; ++k) {
        const int nmain = nb - k - 1;
        const int nlive = (k + 1 < nid) ? k + 1 : nid;
        const int nextra = nlive + ntail;
        const int nchunks = nmain + nextra;
        if (nchunks > 0)
            hipLaunchKernelGGL(potrf_panel_kernel, dim3(nchunks, batch), dim3(256), 0, stream, A, n, k, nmain,
                               slab_stride, nlive, nid, dinv);
        const int n1 = nmain;
        if (n1 > 0) {
            const int nmain_tiles = n1 * (n1 + 1) / 2;
            const int ntiles = nmain_tiles + nextra * n1;
            // few workgroups: the launch lasts as long as tile 0's look-ahead factorisation -> pipelined variant
            // (256 VGPRs, one workgroup per CU); many: the leaner variant keeps two workgroups per CU
            if ((size_t)ntiles * batch <= 512)
                hipLaunchKernelGGL(potrf_trail_kernel<true>, dim3(ntiles, batch), dim3(256), 0, stream, A, n, k,
                                   nmain_tiles, n1, slab_stride, info, nlive, nid, dinv);
            else
                hipLaunchKernelGGL(potrf_trail_kernel<false>, dim3(ntiles, batch), dim3(256), 0, stream, A, n, k,
                                   nmain_tiles, n1, slab_stride, info, nlive, nid, dinv);
        }
    }
}

// rows [row0, row0 + n) of every slab <- identity (n x n), used to re-arm the extra rows that become L^-T
__global__ void set_identity_kernel(double *A, size_t slab_stride, int row0, int n) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx % n);
    A[(size_t)blockIdx.y * slab_stride + (size_t)(row0 + i) * n + j] = (i == j) ? 1.0 : 0.0;
}
void launch_set_identity(hipStream_t stream, double *A, size_t slab_stride, int row0, int n, int batch) {
    hipLaunchKernelGGL(set_identity_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256), batch), dim3(256), 0, stream, A,
                       slab_stride, row0, n);
}

// rows [row0, row0 + n) of slab b <- L_d^T (upper triangular, zeros left of the diagonal), d = b % Dl, from the lower-triangular
// n x n factor L_d (ld n).  Training forward of the Gram route: with L^T instead of I in the extension rows, the factorisation of
// A = K + K_uf K_fu / Q leaves  L^T L_A^-T = L_H^-T  there, L_H = L^-1 L_A being the Cholesky factor of H = L^-1 A L^-T -- the
// whitened quantities of the backward pass without forming H.  64 x 64 tiles through LDS.
__global__ __launch_bounds__(256) void set_lt_rows_kernel(const double *L, size_t l_stride, int Dl, double *A, size_t slab_stride,
                                                          int row0, int n) {
    __shared__ double tile[64][65];
    const int nt = n / 64, tr = blockIdx.x / nt, tc = blockIdx.x % nt, b = blockIdx.y;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    double *Ab = A + (size_t)b * slab_stride + (size_t)(row0 + tr * 64) * n + tc * 64;
    if (tc < tr) {
        for (int r = ty; r < 64; r += 4) Ab[(size_t)r * n + tx] = 0.0;
        return;
    }
    // out[r][c] = L[tc * 64 + c][tr * 64 + r]
    const double *Lb = L + (size_t)(b % Dl) * l_stride + (size_t)(tc * 64) * n + tr * 64;
    for (int c = ty; c < 64; c += 4) tile[c][tx] = Lb[(size_t)c * n + tx];
    __syncthreads();
    for (int r = ty; r < 64; r += 4) Ab[(size_t)r * n + tx] = (tc > tr || tx >= r) ? tile[tx][r] : 0.0;
}
void launch_set_lt_rows(hipStream_t stream, const double *L, size_t l_stride, int Dl, double *A, size_t slab_stride, int row0,
                        int n, int batch) {
    const int nt = n / 64;
    hipLaunchKernelGGL(set_lt_rows_kernel, dim3(nt * nt, batch), dim3(256), 0, stream, L, l_stride, Dl, A, slab_stride, row0, n);
}

}  // namespace ffvd
