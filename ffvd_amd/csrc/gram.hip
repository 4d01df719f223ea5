// Gram kernels (gfx950, fp64 MFMA): C = A^T A over the rows of a stored A, lower-triangular 128 x 128 tiles, batched -- the
// dominant kernel of an iteration.  H = F^T F / Q + I and b = delta^T F / Q (K6/K7: conditionals_multi_output.py:246-248), or
// A_d = K_uu + K_uf K_fu / Q from the stored K_fu with the partial sums of tr(K^-1 K_uf K_fu), or a plain
// A^T A (K^-1 = L^-T L^-1).  Also here: the pair combos of the diagonal tiles, the two-half tail of the last round with its
// exchange, the split-K pass with gram_combine_kernel, and the host-side planning (gram_ksplit, gram_tail_wg, launch_gram).
// kernels.h, GramArgs has the arguments; DESIGN.md section 4 describes the kernel, section 5 has its measurements.
#include "kernels.h"
#include "dev_common.h"
#include <cstdlib>

namespace ffvd {

// ---------------------------------------------------------------------------------------------
// Gram:  C = A^T A over the rows of A (T x Mp), lower-triangular tiles only, batched.
//   mode GRAM_F   : H = F^T F * (Y_N / (batch Q_d)) + I            (conditionals_multi_output.py:246)
//   mode GRAM_KFU : A_d = K_uf K_fu * (Y_N / (batch Q_d)) + (K_uu + jitter I)     (collapsed bound in the
//                   K_uu + K_uf K_fu / Q form) plus the partial sums of tr(K^-1 K_uf K_fu)
//   mode GRAM_PLAIN: C = A^T A (used for K^-1 = L^-T L^-1)
//   with_row != 0 : extra row Mp = delta^T A * (Y_N / (batch Q_d))                 (conditionals_multi_output.py:247-248)
// Workgroup = 128 x 128 output tile of the lower triangle, 8 wavefronts of 64 x 32 (8 accumulator tiles = 64
// VGPRs), two workgroups per CU = four resident wavefronts per SIMD -- one fp64 MFMA wavefront can use at most
// about half of a SIMD's matrix pipe (tools/mfma_probe2), so the pipe only saturates with several MFMA-ready
// wavefronts per SIMD, and a second workgroup covers the first one's barrier / staging bubbles.
// (Measured alternatives at M = 512, T = 4096, 128 units: 4 wavefronts of 64x64 3.45 ms; 16 wavefronts of 32x32,
//  one workgroup per CU 3.36 ms; 128x64 tiles, 8 wavefronts of 32x32 3.27 ms; this layout 2.98 ms.)
// ---------------------------------------------------------------------------------------------
constexpr int GT = 16;              // rows of A per LDS chunk
constexpr int G_LD = 128 + 16;      // LDS row stride (doubles): lanes l and l+16 land in different bank halves

// Debug build only (-DFFVD_DF_TRACE): wall-clock stamps of the tile pass's workgroups.
#ifdef FFVD_DF_TRACE
__device__ long long gram_trace_buf[128 * 10 * 4];      // start, end, HW_ID, blockIdx of every Gram tile (<= 128 units of 10 tiles)
__device__ long long gram_tile_buf[16 * 10 * 2];        // start, end of the tiles of the first 16 units, by tile index
extern "C" int ffvd_debug_gram_trace(long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(gram_trace_buf), sizeof(long long) * 128 * 10 * 4);
}
// (ffvd_debug_df_trace hands these out at offset 2048 of its buffer: potrf_flow.hip)
int gram_trace_tiles(long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(gram_tile_buf), sizeof(long long) * 16 * 10 * 2);
}
#endif

// 64x32 sub-block (row half, column quarter) of each wavefront.  Diagonal tiles only need the 6 sub-blocks that
// touch the lower triangle; they go to wavefronts 0..5 (SIMDs 0,1 get two, SIMDs 2,3 one); 6 and 7 do the gemv.
__device__ __constant__ unsigned char GRAM_DIAG_WR[8] = {1, 1, 1, 1, 0, 0, 0, 0};
__device__ __constant__ unsigned char GRAM_DIAG_WC[8] = {0, 1, 2, 3, 0, 1, 2, 3};

template <int N>
__device__ __forceinline__ bool gram_tail_exchange(const GramArgs &a, const int tail_id, const int half, const bool active,
                                                   d4 (&acc)[N], double &bs0, double &bs1, int *tail_slot);

template <int MODE, bool DIAG>
__device__ __forceinline__ void gram_body(const GramArgs a, const int bz, const int ti, const int tj, const int tile,
                                          const int kpart, const int ksplit, double (*As)[GT][G_LD],
                                          double (*Bs)[GT][G_LD], double (*dls)[GT], double *red, const int tail_id = -1,
                                          int *tail_slot = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = DIAG ? GRAM_DIAG_WR[wave] : (wave >> 2), wc = DIAG ? GRAM_DIAG_WC[wave] : (wave & 3);
    const int lr = lane & 15, lk = lane >> 4;
    const int Mp = a.Mp;
    const int b = a.b0 + bz, s = b / a.Dl, dl = b % a.Dl, dg = a.d_begin + dl;
    const int I0 = ti * 128 + wr * 64, J0 = tj * 128 + wc * 32;
    const bool active = (I0 < Mp) && (J0 < Mp) && (J0 < I0 + 64);
    const bool gemv = DIAG && a.with_row && tid >= 384;          // wavefronts 6, 7: no sub-block in diagonal tiles

    const double *Ab = a.A + (size_t)bz * a.a_stride;
    const double *Xs = (a.with_row && !(MODE == GRAM_PLAIN && a.rvec)) ? a.X + (size_t)s * (a.T + 1) * a.D : nullptr;
    // global -> register staging: thread (rowl, lane) moves 16 bytes of rows rowl and rowl + 8 per operand.
    // Out-of-range columns (odd number of 64-blocks) are read from a clamped valid address and zeroed.
    const int colA = ti * 128 + 2 * lane, colB = tj * 128 + 2 * lane;
    const bool okA = colA < Mp, okB = colB < Mp;
    const int colAc = okA ? colA : 0, colBc = okB ? colB : 0;
    const int rowl = tid >> 6;   // 0..7

    // The loaded registers are only touched again in lstore() (masking included), so the global loads of chunk
    // c + 1 stay in flight behind the whole MFMA phase of chunk c.
    double2 ra[2], rb[2];
    double d1 = 0.0, d0 = 0.0;
    bool dok = false;
    auto gload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const size_t t = (size_t)c * GT + rowl + 8 * i;
            ra[i] = *reinterpret_cast<const double2 *>(Ab + t * Mp + colAc);
            if (!DIAG) rb[i] = *reinterpret_cast<const double2 *>(Ab + t * Mp + colBc);
        }
        if (DIAG && a.with_row) {
            const int tt = c * GT + (tid & (GT - 1));
            if (MODE == GRAM_PLAIN && a.rvec) {                // a caller-supplied vector (residuals, backward pass)
                d1 = a.rvec[(size_t)bz * a.rows + tt];
                d0 = 0.0;
                dok = true;
            } else {
                const int tc = tt < a.T ? tt : a.T - 1;
                d1 = Xs[(size_t)(tc + 1) * a.D + dg];
                d0 = Xs[(size_t)tc * a.D + dg];
                dok = tt < a.T;
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double2 va = ra[i];
            va.x = okA ? va.x : 0.0;
            va.y = okA ? va.y : 0.0;
            *reinterpret_cast<double2 *>(&As[buf][rowl + 8 * i][2 * lane]) = va;
            if (!DIAG) {
                double2 vb = rb[i];
                vb.x = okB ? vb.x : 0.0;
                vb.y = okB ? vb.y : 0.0;
                *reinterpret_cast<double2 *>(&Bs[buf][rowl + 8 * i][2 * lane]) = vb;
            }
        }
        if (DIAG && a.with_row && tid < GT) dls[buf][tid] = dok ? d1 - d0 : 0.0;     // :247
    };

    d4 acc[4][2];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    double bsum = 0.0;

    const int nchunk_all = a.rows / GT;
    const int nrange = (tail_id >= 0) ? 2 : ksplit;                   // a tail workgroup is one of two row halves (kpart = the half)
    const int per = (nchunk_all + nrange - 1) / nrange;
    const int cbeg = kpart * per;
    const int nchunk = (cbeg + per <= nchunk_all) ? cbeg + per : nchunk_all;      // this range: chunks [cbeg, nchunk)
    gload(cbeg);
    lstore(cbeg & 1);
    __syncthreads();
    for (int c = cbeg; c < nchunk; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunk) gload(c + 1);
        if (active) {
            const double(*Bp)[G_LD] = DIAG ? As[buf] : Bs[buf];
            double af[4], bf[2], afn[4], bfn[2];
#pragma unroll
            for (int x = 0; x < 4; ++x) af[x] = As[buf][lk][wr * 64 + 16 * x + lr];
#pragma unroll
            for (int y = 0; y < 2; ++y) bf[y] = Bp[lk][wc * 32 + 16 * y + lr];
#pragma unroll
            for (int ks = 0; ks < GT / 4; ++ks) {
                if (ks + 1 < GT / 4) {       // fragments of the next k-step are requested before this step's MFMAs
#pragma unroll
                    for (int x = 0; x < 4; ++x) afn[x] = As[buf][4 * (ks + 1) + lk][wr * 64 + 16 * x + lr];
#pragma unroll
                    for (int y = 0; y < 2; ++y) bfn[y] = Bp[4 * (ks + 1) + lk][wc * 32 + 16 * y + lr];
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
#pragma unroll
                for (int x = 0; x < 4; ++x) af[x] = afn[x];
#pragma unroll
                for (int y = 0; y < 2; ++y) bf[y] = bfn[y];
            }
        }
        if (gemv) {
#pragma unroll
            for (int r = 0; r < GT; ++r) bsum += As[buf][r][tid - 384] * dls[buf][r];
        }
        if (c + 1 < nchunk) lstore(buf ^ 1);
        __syncthreads();
    }

    if (tail_id >= 0) {
        double unused = 0.0;
        if (!gram_tail_exchange(a, tail_id, kpart, active, reinterpret_cast<d4(&)[8]>(acc), bsum, unused, tail_slot)) return;
    }
    if (ksplit > 1) {            // raw partial sums of this row range; gram_combine finishes the job
        double *Pb = a.part + ((size_t)kpart * a.nb + bz) * ((size_t)(Mp + 1) * Mp);
        if (active) {
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        Pb[(size_t)(I0 + 16 * x + lk + 4 * q) * Mp + J0 + 16 * y + lr] = acc[x][y][q];
        }
        if (gemv) {
            const int col = ti * 128 + tid - 384;
            if (col < Mp) Pb[(size_t)Mp * Mp + col] = bsum;
        }
        return;
    }
    const double scale = (MODE == GRAM_PLAIN) ? 1.0 : a.yn_over_batch / exp(a.log_Q[dg]);
    double *Hb = a.H + (size_t)bz * a.h_stride;
    const double *Kadd = (MODE == GRAM_KFU || MODE == GRAM_KFU_RAW) ? a.Kadd + (size_t)dl * a.kadd_stride : nullptr;
    const double *Kinv = (MODE == GRAM_KFU) ? a.Kinv + (size_t)dl * a.kinv_stride : nullptr;
    double *Rb = (MODE == GRAM_KFU_RAW) ? a.part + (size_t)bz * ((size_t)(Mp + 1) * Mp) : nullptr;
    double *Cb2 = ((MODE == GRAM_KFU_RAW || MODE == GRAM_KFU) && a.Hcopy) ? a.Hcopy + (size_t)bz * a.hcopy_stride : nullptr;
    double trp = 0.0;
    if (active) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = I0 + 16 * x + lk + 4 * q, j = J0 + 16 * y + lr;
                    const double g = acc[x][y][q];
                    double v;
                    if (MODE == GRAM_F) v = g * scale + ((i == j) ? 1.0 : 0.0);
                    else if (MODE == GRAM_KFU_RAW) {
                        v = g * scale + Kadd[(size_t)i * Mp + j];
                        Rb[(size_t)i * Mp + j] = g;
                        if (Cb2 && j <= i) {                    // the copy holds the lower triangle (its readers sum over the chains first and mirror the sum: a mirror here was 64 cache lines per store)
                            Cb2[(size_t)i * Mp + j] = v;
                        }
                    } else if (MODE == GRAM_KFU) {
                        v = g * scale + Kadd[(size_t)i * Mp + j];
                        if (Cb2 && j <= i) {                    // second copy, lower triangle (the backward pass keeps A)
                            Cb2[(size_t)i * Mp + j] = v;
                        }
                        const double w = (i > j) ? 2.0 : ((i == j) ? 1.0 : 0.0);
                        trp += w * (Kinv[(size_t)i * Mp + j] * g);
                    } else v = g;
                    Hb[(size_t)i * Mp + j] = v;
                }
    }
    if (gemv) {
        const int col = ti * 128 + tid - 384;
        if (col < Mp) Hb[(size_t)a.brow * Mp + col] = bsum * scale;
    }
    if (MODE == GRAM_KFU) {      // deterministic workgroup reduction of the trace partial
        red[tid] = trp;
        __syncthreads();
        for (int st = 256; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) a.trpart[(size_t)b * a.ntiles + tile] = red[0];
    }
}

// Row half of a tail workgroup (GramArgs::tail_wg): leave the accumulators in memory, count in, and -- if the other half has
// counted in before -- add its values and carry on (returns true); else done (returns false).  Nobody waits.  The blocks are
// stored WRITE-THROUGH (sc1, relaxed agent-scope atomic stores) so that no release fence is needed -- an agent-scope release
// writes back the XCD L2's dirty lines, which with 135 KB per half and the chip streaming K_fu made a half last twice its time;
// the reader's ONE acquire invalidates its CU's L1 and then loads plainly (MI355X guide, inter-workgroup visibility: sc1 payload
// stores, every storing wavefront's vmcnt(0), the workgroup's barrier, one lane's relaxed agent-scope add).
// TARGET-SPECIFIC hand-off: the partial block is published with relaxed agent-scope stores + s_waitcnt vmcnt(0) + barrier +
// a relaxed fetch_add, with NO release fence (an agent-scope release writes back the XCD L2's dirty lines and doubled the time of
// a half).  That is sound on gfx942 / gfx950 only: stores are counted in vmcnt, the atomic stores are emitted
// with sc1 (write-through to memory-side coherence) and a CU's L1 is not shared across workgroups' hand-off.  Targets that track
// stores in vscnt (gfx10+) or another compiler lowering of the atomic stores would break it silently -- so the build refuses them.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "gram_tail_exchange relies on gfx942/gfx950 store semantics (vmcnt-counted sc1 write-through stores); build for gfx950"
#endif
template <int N>
__device__ __forceinline__ bool gram_tail_exchange(const GramArgs &a, const int tail_id, const int half, const bool active,
                                                   d4 (&acc)[N], double &bs0, double &bs1, int *tail_slot) {
    static_assert((N * 4 + 2) * 512 <= GRAM_TAIL_DOUBLES, "tail block too small");
    typedef __attribute__((address_space(1))) double gdouble;
    const int tid = threadIdx.x;
    gdouble *Pm = (gdouble *)(a.tail_part + ((size_t)tail_id * 2 + half) * GRAM_TAIL_DOUBLES);
    const double *Po = a.tail_part + ((size_t)tail_id * 2 + (half ^ 1)) * GRAM_TAIL_DOUBLES;
    if (active) {
#pragma unroll
        for (int x = 0; x < N; ++x)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                __hip_atomic_store(Pm + (size_t)(x * 4 + q) * 512 + tid, acc[x][q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(Pm + (size_t)(4 * N) * 512 + tid, bs0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(Pm + (size_t)(4 * N + 1) * 512 + tid, bs1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wavefront's block has left it
    __syncthreads();
    if (tid == 0) {
        const int seen = __hip_atomic_fetch_add(a.tail_cnt + tail_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 1) {                                         // the other half is complete and in memory
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(a.tail_cnt + tail_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch
        }
        *tail_slot = seen;
    }
    __syncthreads();
    if (*tail_slot != 1) return false;
    // (a + b is the same number whichever half is `a`: the result does not depend on the order of arrival)
    if (active) {
#pragma unroll
        for (int x = 0; x < N; ++x)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[x][q] += Po[(size_t)(x * 4 + q) * 512 + tid];
    }
    bs0 += Po[(size_t)(4 * N) * 512 + tid];
    bs1 += Po[(size_t)(4 * N + 1) * 512 + tid];
    return true;
}

// "Pair" combos (round 4): 16-granular triangle.  A diagonal 128-tile has 8 x 9 / 2 = 36 MFMA tiles on or below its diagonal; row
// block i (16 rows) owns i + 1 of them, so the row blocks i and 7 - i together own NINE whatever i -- four wavefronts per diagonal
// tile, each with nine MFMAs per k-step, and no MFMA tile above the diagonal is executed.  A workgroup takes the diagonal tiles of
// two neighbouring panels (both staged as before); it lasts 9 / 8 of an off-diagonal tile, and the four panels of M = 512 cost
// 2 x 1.125 workgroup-times instead of 3: executed flops 1.03 x the triangle's instead of 1.125 x.  Operands: on a diagonal tile
// the A fragment of row block i IS the B fragment of column block i, so role R reads the 8 - R column fragments 0 .. 7 - R and
// nothing else (8, 7, 6, 5 fragment reads for 9 MFMAs; the 64 x 32 sub-blocks read 6 for 8).  Earlier attempts at the triangle
// (1 x 4 row roles with 5 reads per 4 MFMAs, evenly dealt tiles) lost to their read / MFMA ratio.
// The unwritten above-diagonal MFMA tiles INSIDE the diagonal 64-blocks are mirrored from below in the epilogue (bit for bit what
// the sub-blocks used to compute there: the same products in the same order), so the buffers look as they always did.
template <int R>
__device__ __forceinline__ void gram_pair_ksteps(const double (*Sp)[G_LD], const int lr, const int lk, d4 (&acc)[9]) {
    // Registers: nine accumulator tiles are 72 of the 128 VGPRs, so the next k-step's fragments cannot have an array of their own
    // (the 64 x 32 sub-blocks keep 6 + 6): column fragment c is re-loaded into its own register right after its last MFMA of this
    // step, and only the two row operands -- f[R], f[7 - R], needed by every MFMA of the step -- are held in copies.
    constexpr int NF = 8 - R;
    double f[NF];
#pragma unroll
    for (int c = 0; c < NF; ++c) f[c] = Sp[lk][16 * c + lr];
    double aR = f[R], aS = f[7 - R];
#pragma unroll
    for (int ks = 0; ks < GT / 4; ++ks) {
#pragma unroll
        for (int c = 0; c < NF; ++c) {
            acc[R + 1 + c] = mfma_f64(aS, f[c], acc[R + 1 + c]);             // row block 7 - R, columns 0 .. 7 - R
            if (c <= R) acc[c] = mfma_f64(aR, f[c], acc[c]);                 // row block R, columns 0 .. R
            if (ks + 1 < GT / 4) f[c] = Sp[4 * (ks + 1) + lk][16 * c + lr];
            __builtin_amdgcn_sched_barrier(0);          // (keep the re-load behind the MFMAs that free its register: hoisted loads need eight more)
        }
        if (ks + 1 < GT / 4) { aR = f[R]; aS = f[7 - R]; }
    }
}

// (the whole body is instantiated per role: with the role switch inside the chunk loop the nine accumulator tiles crossed a four-way
//  merge every chunk and the register allocator kept them in scratch)
template <int MODE, int R>
__device__ __forceinline__ void gram_pair_role(const GramArgs a, const int bz, const int pa, const int tail_id,
                                               const int half /* row range: tail half or split-K part */, const int ksplit,
                                               double (*As)[GT][G_LD], double (*Bs)[GT][G_LD], double *red, int *tail_slot) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    const int Mp = a.Mp;
    const int b = a.b0 + bz, dl = b % a.Dl, dg = a.d_begin + dl;
    const int pb = pa + 1;                                               // the two panels this workgroup stages
    const int rbuf = wave >> 2;                                          // wavefronts w and w + 4 share a SIMD: the same role R = w & 3 on both panels
    const int P0 = (rbuf ? pb : pa) * 128;

    const double *Ab = a.A + (size_t)bz * a.a_stride;
    const int rowl = tid >> 6;   // 0..7
    // Staging: LDS-DMA (global_load_lds_dwordx4: one wavefront-instruction = one 1 KiB row of a panel, lane l -> bytes 16 l of the
    // row), no staging registers -- nine accumulator tiles + eight fragments leave no room for the sixteen the register-staged
    // bodies hold across the MFMA phase.  Uniform 64-bit bases per chunk (SGPRs) + ONE 32-bit byte offset per thread.  Written as asm: hipcc waits vmcnt(0) in front of the first ds_read that follows a DMA it
    // knows about (it cannot tell the two buffers apart), i.e. before the MFMA phase the DMA is meant to run behind; the loads
    // it does not count are waited for by hand in front of the barrier.
    const unsigned voff = (unsigned)((rowl * Mp + pa * 128 + 2 * lane) * (int)sizeof(double));
    typedef __attribute__((address_space(3))) void lvoid;
    auto glds = [&](const double *base, const void *lds_row) {
        const unsigned dst = (unsigned)(uintptr_t)(lvoid *)lds_row;
        unsigned keep;
        // (no immediate offset: the instruction adds it to the LDS address as well as to the global one)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(dst), "s"(base) : "memory");
    };
    auto gload = [&](int c, int buf) {
        const double *base0 = Ab + (size_t)c * GT * Mp, *base1 = base0 + (size_t)8 * Mp;
        glds(base0, &As[buf][wave][0]);
        glds(base0 + 128, &Bs[buf][wave][0]);
        glds(base1, &As[buf][wave + 8][0]);
        glds(base1 + 128, &Bs[buf][wave + 8][0]);
    };

    d4 acc[9];
#pragma unroll
    for (int x = 0; x < 9; ++x) acc[x] = (d4){0.0, 0.0, 0.0, 0.0};
    const int nchunk_all = a.rows / GT;
    const int nrange = (tail_id >= 0) ? 2 : ksplit;
    const int per = (nchunk_all + nrange - 1) / nrange;
    const int cbeg = half * per;
    const int nchunk = (cbeg + per <= nchunk_all) ? cbeg + per : nchunk_all;
    gload(cbeg, cbeg & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int c = cbeg; c < nchunk; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunk) gload(c + 1, buf ^ 1);                       // the buffer nobody reads until the barrier below
        {
            const double(*Sp)[G_LD] = rbuf ? Bs[buf] : As[buf];          // this wavefront's panel holds both of its operands
            gram_pair_ksteps<R>(Sp, lr, lk, acc);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the next chunk has landed (the DMAs are invisible to hipcc's counting)
        __syncthreads();
    }
    double bs0 = 0.0, bs1 = 0.0;           // (no delta^T A row here: launch_gram gives combos only to launches without one)
    if (tail_id >= 0 && !gram_tail_exchange(a, tail_id, half, true, acc, bs0, bs1, tail_slot)) return;
    if (ksplit > 1) {            // raw partial sums of this row range; gram_combine finishes the job (it reads whole 64 x 32 sub-blocks:
                                 // the tiles above the diagonal inside the diagonal 64-blocks are mirrored here as well)
        double *Pb = a.part + ((size_t)half * a.nb + bz) * ((size_t)(Mp + 1) * Mp);
#pragma unroll
        for (int x = 0; x < 9; ++x) {
            const int rb = (x <= R) ? R : 7 - R, cb = (x <= R) ? x : x - R - 1;
            const bool mirror = cb < rb && (rb >> 2) == (cb >> 2);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = P0 + 16 * rb + lk + 4 * q, j = P0 + 16 * cb + lr;
                Pb[(size_t)i * Mp + j] = acc[x][q];
                if (mirror) Pb[(size_t)j * Mp + i] = acc[x][q];
            }
        }
        return;
    }

    const double scale = (MODE == GRAM_PLAIN) ? 1.0 : a.yn_over_batch / exp(a.log_Q[dg]);
    double *Hb = a.H + (size_t)bz * a.h_stride;
    const double *Kadd = (MODE == GRAM_KFU || MODE == GRAM_KFU_RAW) ? a.Kadd + (size_t)dl * a.kadd_stride : nullptr;
    const double *Kinv = (MODE == GRAM_KFU) ? a.Kinv + (size_t)dl * a.kinv_stride : nullptr;
    double *Rb = (MODE == GRAM_KFU_RAW) ? a.part + (size_t)bz * ((size_t)(Mp + 1) * Mp) : nullptr;
    double *Cb2 = ((MODE == GRAM_KFU_RAW || MODE == GRAM_KFU) && a.Hcopy) ? a.Hcopy + (size_t)bz * a.hcopy_stride : nullptr;
    double trp = 0.0;
#pragma unroll
    for (int x = 0; x < 9; ++x) {
        const int rb = (x <= R) ? R : 7 - R, cb = (x <= R) ? x : x - R - 1;        // (accumulator x: row block, column block)
        const bool mirror = cb < rb && (rb >> 2) == (cb >> 2);                     // below the diagonal of a diagonal 64-block
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = P0 + 16 * rb + lk + 4 * q, j = P0 + 16 * cb + lr;
            const double g = acc[x][q];
            double v;
            if (MODE == GRAM_F) v = g * scale + ((i == j) ? 1.0 : 0.0);
            else if (MODE == GRAM_KFU_RAW || MODE == GRAM_KFU) {
                v = g * scale + Kadd[(size_t)i * Mp + j];
                if (MODE == GRAM_KFU_RAW) Rb[(size_t)i * Mp + j] = g;
                if (Cb2 && j <= i) {                    // the copy holds the lower triangle (its readers sum over the chains first and mirror the sum: a mirror here was 64 cache lines per store)
                    Cb2[(size_t)i * Mp + j] = v;
                }
                if (MODE == GRAM_KFU) {
                    const double w = (i > j) ? 2.0 : ((i == j) ? 1.0 : 0.0);
                    trp += w * (Kinv[(size_t)i * Mp + j] * g);
                }
            } else v = g;
            Hb[(size_t)i * Mp + j] = v;
            if (mirror) {
                if (MODE == GRAM_KFU_RAW) Rb[(size_t)j * Mp + i] = g;
                Hb[(size_t)j * Mp + i] = (MODE == GRAM_KFU_RAW || MODE == GRAM_KFU) ? g * scale + Kadd[(size_t)j * Mp + i] : v;
            }
        }
    }
    if (MODE == GRAM_KFU) {      // deterministic workgroup reduction of the trace partial; slot of the first panel's diagonal tile
        red[tid] = trp;
        __syncthreads();
        for (int st = 256; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) {
            a.trpart[(size_t)b * a.ntiles + pa * (pa + 1) / 2 + pa] = red[0];
            a.trpart[(size_t)b * a.ntiles + pb * (pb + 1) / 2 + pb] = 0.0;          // (one workgroup, two slots)
        }
    }
}
template <int MODE>
__device__ __forceinline__ void gram_pair_body(const GramArgs a, const int bz, const int pa, const int tail_id,
                                               const int half, const int ksplit, double (*As)[GT][G_LD], double (*Bs)[GT][G_LD],
                                               double *red, int *tail_slot) {
    const int R = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 3;
    if (R == 0) gram_pair_role<MODE, 0>(a, bz, pa, tail_id, half, ksplit, As, Bs, red, tail_slot);
    else if (R == 1) gram_pair_role<MODE, 1>(a, bz, pa, tail_id, half, ksplit, As, Bs, red, tail_slot);
    else if (R == 2) gram_pair_role<MODE, 2>(a, bz, pa, tail_id, half, ksplit, As, Bs, red, tail_slot);
    else gram_pair_role<MODE, 3>(a, bz, pa, tail_id, half, ksplit, As, Bs, red, tail_slot);
}

template <int MODE>
__global__ __launch_bounds__(512, 4) void gram_kernel(GramArgs a) {
    __shared__ double As[2][GT][G_LD];
    __shared__ double Bs[2][GT][G_LD];
    __shared__ double dls[2][GT];
    __shared__ double red[512];
    // XCD-aware mapping: all tiles of one (chain, dim) share blockIdx % 8, i.e. one XCD's L2 (speed only)
    __shared__ int tail_slot;
    const int id = blockIdx.x;
    const int xcd = id & 7;
    int loc = id >> 3;
    const int ksplit = (a.ksplit > 1 && a.part) ? a.ksplit : 1;
    const int per_unit = a.wg_per_unit;                  // ntiles * ksplit, or (combos) off-diagonal tiles + one per pair of panels, * ksplit
    // tail split: the last tail_wg / 8 workgroup slots of every XCD's list appear twice, first all their first row halves, then
    // all their second ones (workgroups that run together then read the same rows of K_fu)
    int tail_id = -1, tail_half = 0;
    if (a.tail_wg > 0) {
        const int ntl = a.tail_wg / 8, lfull = ((a.nb + 7) / 8) * per_unit - ntl;
        if (loc >= lfull) {
            const int q = loc - lfull;
            tail_id = (q % ntl) * 8 + xcd;
            tail_half = q / ntl;
            loc = lfull + q % ntl;
        }
    }
    // (pair combos last 9 / 8 of an off-diagonal tile; dealing them FIRST in the launch, one per CU while the chip fills, changed
    //  nothing against this unit-major order: 3.12 vs 3.12 ms, profiles/r04_ab_gram_pair.txt)
    int unit_l = loc / per_unit, wsel = loc % per_unit;
    int bz = unit_l * 8 + xcd;
    // Fewer units than XCDs (1-4 units of a one- or two-chain rank, split-K): a unit's row ranges are dealt to 8 / nb XCDs instead of all to
    // one -- the ranges read disjoint rows of K_fu, so nothing is shared that an L2 could keep; half of the chip idled otherwise
    // (one chain: 220 us of tile pass on four XCDs)
    const int spread = (ksplit > 1 && a.combo && a.nb <= 4 && 8 % a.nb == 0 && ksplit % (8 / a.nb) == 0) ? 8 / a.nb : 1;
    if (spread > 1) {
        const int sub = per_unit / spread;                   // workgroups of a unit on this XCD
        if (loc >= sub) return;
        bz = xcd % a.nb;
        const int rsub = xcd / a.nb, kper = ksplit / spread;
        wsel = (loc / kper) * ksplit + (loc % kper) * spread + rsub;     // (tile w = loc / kper, row range (loc % kper) * spread + rsub)
    }
    if (bz >= a.nb) return;
    int tile, kpart;
    if (a.combo) {
        const int n128 = a.Mp / 128, noff = n128 * (n128 - 1) / 2, w = wsel / ksplit;      // (split-K: the row ranges of a workgroup are neighbours in the list)
        const int cpart = (tail_id >= 0) ? tail_half : wsel % ksplit;
        if (w >= noff) {                                 // a pair combo: the diagonal tiles of two neighbouring panels
#ifdef FFVD_DF_TRACE
            const long long tc0 = wall_clock64();
#endif
            gram_pair_body<MODE>(a, bz, 2 * (w - noff), tail_id, cpart, ksplit, As, Bs, red, &tail_slot);
#ifdef FFVD_DF_TRACE
            if (threadIdx.x == 0 && bz < 128 && per_unit <= 10 && MODE == GRAM_KFU) {
                long long *g = gram_trace_buf + (size_t)(bz * 10 + w) * 4;
                g[0] = tc0; g[1] = wall_clock64(); g[2] = 1; g[3] = (long long)blockIdx.x;
            }
#endif
            return;
        }
        int ti = 1;                                      // off-diagonal tile w = ti (ti - 1) / 2 + tj,  tj < ti
        while (ti * (ti + 1) / 2 <= w) ++ti;
        tile = ti * (ti + 1) / 2 + (w - ti * (ti - 1) / 2);
        kpart = cpart;
    } else {
        tile = (loc % per_unit) / ksplit;
        kpart = (tail_id >= 0) ? tail_half : loc % ksplit;
    }
    int ti = 0;                       // tile = ti (ti + 1) / 2 + tj,  tj <= ti
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    const int tj = tile - ti * (ti + 1) / 2;
#ifdef FFVD_DF_TRACE
    const long long tw0 = wall_clock64();     // debug build (tools/gram_trace.py): start and end of the tiles of the first 16 units
#endif
    if (ti == tj) gram_body<MODE, true>(a, bz, ti, tj, tile, kpart, ksplit, As, Bs, dls, red, tail_id, &tail_slot);
    else gram_body<MODE, false>(a, bz, ti, tj, tile, kpart, ksplit, As, Bs, dls, red, tail_id, &tail_slot);
#ifdef FFVD_DF_TRACE
    if (threadIdx.x == 0 && bz < 16 && ksplit == 1 && a.ntiles <= 10 && MODE == GRAM_KFU) {
        gram_tile_buf[(bz * 10 + tile) * 2] = tw0;
        gram_tile_buf[(bz * 10 + tile) * 2 + 1] = wall_clock64();
    }
    if (threadIdx.x == 0 && bz < 128 && ksplit == 1 && a.ntiles <= 10 && MODE == GRAM_KFU) {     // every workgroup of the launch (tools/gram_rounds.py)
        long long *g = gram_trace_buf + (size_t)(bz * 10 + (a.combo ? wsel : tile)) * 4;   // (a tail workgroup: the half that ends last)
        g[0] = tw0; g[1] = wall_clock64(); g[2] = (ti == tj) ? 1 : 0; g[3] = (long long)blockIdx.x;
    }
#endif
}

// Second pass of a split-K Gram launch: one workgroup per (unit, tile) adds the `ksplit` partial tiles in fixed
// order and applies the epilogue of gram_body (scaling, + I / + K_uu, trace partial, the delta^T A row).
template <int MODE>
__global__ __launch_bounds__(1024) void gram_combine_kernel(GramArgs a) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const int bz = blockIdx.y, tile = blockIdx.x;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    const int tj = tile - ti * (ti + 1) / 2;
    const int Mp = a.Mp;
    const int b = a.b0 + bz, dl = b % a.Dl, dg = a.d_begin + dl;
    const size_t pstride = (size_t)(Mp + 1) * Mp;
    const double *P0 = a.part + (size_t)bz * pstride;
    const size_t ks_stride = (size_t)a.nb * pstride;
    const double scale = (MODE == GRAM_PLAIN) ? 1.0 : a.yn_over_batch / exp(a.log_Q[dg]);
    double *Hb = a.H + (size_t)bz * a.h_stride;
    const double *Kadd = (MODE == GRAM_KFU) ? a.Kadd + (size_t)dl * a.kadd_stride : nullptr;
    const double *Kinv = (MODE == GRAM_KFU) ? a.Kinv + (size_t)dl * a.kinv_stride : nullptr;
    double trp = 0.0;
    const bool want_tr = (MODE == GRAM_KFU) && a.trace_mode != 1, want_out = a.trace_mode != 2;
    // one pair of columns per thread and 64 x 32 sub-block (the sub-blocks gram_body writes): 16-byte accesses, the
    // eight sub-blocks unrolled so that all their loads are in flight together
    const int ri = tid >> 4, cj = 2 * (tid & 15);
#pragma unroll
    for (int sb = 0; sb < 8; ++sb) {
        const int wr = sb >> 2, wc = sb & 3;
        const int I0 = ti * 128 + wr * 64, J0 = tj * 128 + wc * 32;
        if (!((I0 < Mp) && (J0 < Mp) && (J0 < I0 + 64))) continue;
        const int i = I0 + ri, j = J0 + cj;
        const size_t off = (size_t)i * Mp + j;
        double2 g = {0.0, 0.0};
        const int nks = (a.raw_summed && a.trace_mode == 2) ? 1 : a.ksplit;
        for (int ks = 0; ks < nks; ++ks) {
            const double2 q = *reinterpret_cast<const double2 *>(P0 + (size_t)ks * ks_stride + off);
            g.x += q.x; g.y += q.y;
        }
        if (a.raw_summed && a.trace_mode == 1) *reinterpret_cast<double2 *>(const_cast<double *>(P0) + off) = g;      // (this thread alone reads and writes the element)
        double2 v = {0.0, 0.0};
        if (MODE == GRAM_F) {
            v.x = g.x * scale + ((i == j) ? 1.0 : 0.0);
            v.y = g.y * scale + ((i == j + 1) ? 1.0 : 0.0);
        } else if (MODE == GRAM_KFU) {
            if (want_out) {
                const double2 ka = *reinterpret_cast<const double2 *>(Kadd + off);
                v.x = g.x * scale + ka.x;
                v.y = g.y * scale + ka.y;
            }
            if (want_tr) {
                const double2 ki = *reinterpret_cast<const double2 *>(Kinv + off);
                const double w0 = (i > j) ? 2.0 : ((i == j) ? 1.0 : 0.0);
                const double w1 = (i > j + 1) ? 2.0 : ((i == j + 1) ? 1.0 : 0.0);
                trp += w0 * (ki.x * g.x);
                trp += w1 * (ki.y * g.y);
            }
        } else v = g;
        if (want_out) *reinterpret_cast<double2 *>(Hb + off) = v;
    }
    if (want_out && a.with_row && ti == tj && tid < 128) {
        const int col = ti * 128 + tid;
        if (col < Mp) {
            double bs = 0.0;
            for (int ks = 0; ks < a.ksplit; ++ks) bs += P0[(size_t)ks * ks_stride + (size_t)Mp * Mp + col];
            Hb[(size_t)a.brow * Mp + col] = bs * scale;
        }
    }
    if (want_tr) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) trp += __shfl_xor(trp, m);      // fixed order: reproducible
        if ((tid & 63) == 0) red[tid >> 6] = trp;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < 16; ++w) t += red[w];
            a.trpart[(size_t)b * a.ntiles + tile] = t;
        }
    }
}

int gram_ntiles(int Mp) {
    const int n128 = (Mp / NB + 1) / 2;
    return n128 * (n128 + 1) / 2;
}

static bool gram_uses_combos(int Mp, int with_row);
static int gram_wg_per_unit(int Mp, int ksplit, int with_row);
// Few tiles cannot fill the 512 workgroup slots (256 CUs x 2), and 1-2 tiles per slot balance badly (640 tiles take
// 1.56 x the time of 512).  Measured at M = 512, T = 4096: 160 tiles 0.60 ms unsplit / 0.48 ms in 3 row ranges (one
// full round) / 0.55-0.62 ms in 2, 4, 6, 8; 320 tiles 1.10 -> 0.86 ms in 3-4 ranges; 640 tiles 1.67 -> 1.52 ms in 2.
int gram_ksplit(int Mp, int nb, int rows, int with_row, bool fill_slots) {
    if (const char *e = getenv("FFVD_GSPLIT")) return atoi(e) > 0 ? atoi(e) : 1;       // tuning override
    const int nchunk = rows / GT;
    if (fill_slots && gram_uses_combos(Mp, with_row)) {
        // Nothing beside the launch (the K_uu chain runs behind it): the ranges that give every slot of the chip one workgroup --
        // tools/gsplit_s1.sh: 4 chains 320 us in four ranges against 382 in three, 2 chains 157 against 202, 1 chain 150 in eight
        // Measured per-rank iterations, side chain behind the pass vs beside it in three ranges (tools/sync_step.py, same box,
        // profiles/r04_ab_side_late.txt): 8 chains 1.07 vs 1.20 ms (two ranges), 4 chains 0.688 vs 0.705 (four; 0.750 vs 0.734 before the
        // main-row workgroups of the chain's launch helped with its inverse), 1-2 chains 0.44 / 0.53 vs 0.54 / 0.56 (eight ranges)
        const int n = nb * gram_wg_per_unit(Mp, 1, with_row);
        // (other chain counts, whole rounds of the 512 slots: 6 / 12 / 24 chains = three rounds in 8 / 4 / 2 ranges 0.887 / 1.43 / 2.47 vs
        //  0.911 / 1.47 / 2.60 ms; 20 chains = five rounds in four ranges 2.275 vs 2.176: not beyond three rounds)
        if (n > 0 && n % 512 == 0) return 0;                                         // (whole rounds unsplit: the caller's unsplit schedule)
        for (int ks = 2; ks <= 8; ++ks)
            if (n > 0 && (n * ks) % 512 == 0 && n * ks <= 1536 && nchunk / ks >= 8) return ks;
        if (n > 0 && n <= 64 && nchunk / 8 >= 8) return 8;
        return 0;                                                                   // (the caller keeps the first-half schedule)
    }
    if (gram_uses_combos(Mp, with_row)) {
        // pair combos: 8 workgroups per unit at M = 512.  Measured per-rank iteration times at config 2's shape, 1 .. 24 chains and
        // 1, 2, 3, 4, 6, 8 row ranges (tools/gram_split_sweep.sh, profiles/r04_gram_split.txt): three ranges are the best or within
        // 1 % of it everywhere (few units: 0.55 ms against 0.63 in 2, 4 or 8) -- except when the unsplit launch is exactly whole
        // rounds of the chip's 512 slots (16 chains: 1.97 unsplit, 2.00 in three)
        const int n = nb * gram_wg_per_unit(Mp, 1, with_row);
        if (n <= 0 || n >= 1024 || n % 512 == 0) return 1;
        int ks = 3;
        while (ks > 1 && nchunk / ks < 8) --ks;
        return ks;
    }
    const int n = nb * gram_ntiles(Mp);
    if (n <= 0 || n >= 1024) return 1;
    // one full round; three row ranges up to 640 tiles (re-measured with the 1024-thread combine pass: 160 tiles 1.05 ms per
    // iteration in 3 ranges / 1.08-1.09 in 2, 4; 320 tiles 1.49 in 3 / 1.53 in 2 / 1.58 in 4; 640 tiles 2.46 in 3 / 2.53 in 2)
    int ks = (n <= 256) ? 512 / n : ((n <= 704) ? 3 : (1280 + n / 2) / n);
    if (ks > 8) ks = 8;
    while (ks > 1 && nchunk / ks < 8) --ks;          // keep at least 128 rows per range
    return ks;
}
size_t gram_part_doubles(int Mp, int nb, int ksplit) {
    return ksplit > 1 ? (size_t)ksplit * nb * (size_t)(Mp + 1) * Mp : 0;
}

// workgroups per unit of a launch: with Mp a multiple of 256 the diagonal tiles of every two panels become one pair combo, also in
// a split-K launch (and only when the kernel has no delta^T A row to form: the combos have no idle wavefront for it)
static bool gram_uses_combos(int Mp, int with_row) {
    return Mp % 256 == 0 && !with_row;
}
static int gram_wg_per_unit(int Mp, int ksplit, int with_row) {
    const int n128 = (Mp / NB + 1) / 2;
    if (gram_uses_combos(Mp, with_row))
        return (n128 * (n128 - 1) / 2 + n128 / 2) * (ksplit > 1 ? ksplit : 1);
    return gram_ntiles(Mp) * (ksplit > 1 ? ksplit : 1);
}
// Which workgroups of an unsplit launch are cut in two row halves: those of the last, partial round, when their halves still fit
// into half of the chip's slots (two per CU) -- then the halves take the slots that free up FIRST at the end of the last full
// round and run beside its stragglers.  tools/gram_rounds.py (128 units): a round's tiles end 0.5-0.7 ms apart (the workgroup
// that arrived first on a CU keeps the matrix pipe), a workgroup alone on its CU reaches 57-65 % of what two reach together,
// and a 2-way split of a whole half round (256 tiles -> 512 halves) ended LATER than no split because the last halves start
// when the last slot frees up; with combos the remainder is 128 workgroups -> 256 halves -> the 256 slots that free up first.
int gram_tail_wg(int Mp, int nb, int ksplit, int with_row) {
    if (ksplit > 1) return 0;
    static const int slots = [] {
        int dev = 0, cus = 256;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
        return 2 * cus;
    }();
    const int n = ((nb + 7) / 8) * 8 * gram_wg_per_unit(Mp, ksplit, with_row);
    if (n < 2 * slots) return 0;                                 // small launches have their own split-K path
    const int r = n % slots;
    return (r > 0 && 4 * r <= slots && r % 8 == 0) ? r : 0;
}
size_t gram_tail_doubles(int tail_wg) {
    return tail_wg > 0 ? (size_t)tail_wg * 2 * GRAM_TAIL_DOUBLES + ((size_t)tail_wg + 1) / 2 : 0;
}

// phase: 0 = everything, 1 = the tile pass only, 2 = the combine pass only (split-K launches: the tile pass writes
// raw partials and needs neither K_uu nor K^-1, so the caller may run it before those exist and combine afterwards)
void launch_gram(hipStream_t stream, GramArgs a, int phase) {
    a.ntiles = gram_ntiles(a.Mp);
    if (a.brow <= 0) a.brow = a.Mp;
    if (!a.part || a.ksplit < 1) a.ksplit = 1;
    const int groups = (a.nb + 7) / 8;
    a.combo = gram_uses_combos(a.Mp, a.with_row) ? 1 : 0;
    a.wg_per_unit = gram_wg_per_unit(a.Mp, a.ksplit, a.with_row);
    if (a.ksplit > 1 || !a.tail_part || a.tail_wg != gram_tail_wg(a.Mp, a.nb, a.ksplit, a.with_row)) a.tail_wg = 0;
    if (a.tail_wg > 0) a.tail_cnt = reinterpret_cast<int *>(a.tail_part + (size_t)a.tail_wg * 2 * GRAM_TAIL_DOUBLES);
    const dim3 grid(groups * 8 * a.wg_per_unit + a.tail_wg);
    if (phase != 2 && phase != 3 && phase != 4) {
        if (a.mode == GRAM_F) hipLaunchKernelGGL(gram_kernel<GRAM_F>, grid, dim3(512), 0, stream, a);
        else if (a.mode == GRAM_KFU) hipLaunchKernelGGL(gram_kernel<GRAM_KFU>, grid, dim3(512), 0, stream, a);
        else if (a.mode == GRAM_KFU_RAW) hipLaunchKernelGGL(gram_kernel<GRAM_KFU_RAW>, grid, dim3(512), 0, stream, a);
        else hipLaunchKernelGGL(gram_kernel<GRAM_PLAIN>, grid, dim3(512), 0, stream, a);
    }
    if (phase == 3) a.trace_mode = 2;
    if ((a.ksplit > 1 && phase != 1) || phase == 3 || phase == 4) {
        const dim3 cgrid(a.ntiles, a.nb);
        if (a.mode == GRAM_KFU_RAW) a.mode = GRAM_KFU;
        if (a.mode == GRAM_F) hipLaunchKernelGGL(gram_combine_kernel<GRAM_F>, cgrid, dim3(1024), 0, stream, a);
        else if (a.mode == GRAM_KFU) hipLaunchKernelGGL(gram_combine_kernel<GRAM_KFU>, cgrid, dim3(1024), 0, stream, a);
        else hipLaunchKernelGGL(gram_combine_kernel<GRAM_PLAIN>, cgrid, dim3(1024), 0, stream, a);
    }
}

}  // namespace ffvd
