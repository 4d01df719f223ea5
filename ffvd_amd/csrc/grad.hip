// Backward pass of the collapsed-U nll (SE kernel, K_uu + K_uf K_fu / Q form) for gfx950, fp64.
//
// The reference differentiates `nll` with TensorFlow autodiff (tf.gradients, base_model.py:148;
// AdamOptimizer.minimize, dgp_model.py:303-305).  Here the gradient is evaluated in closed form
// (CPU twin: oracle/ffvd_grad_oracle.py).  Per (chain s, latent dim d):
//   alpha = 1/Q, K = K_uu + jitter I, Kf = K_fu, G = Kf^T Kf, g = Kf^T delta, A = K + alpha G, u = A^-1 (alpha g)
//   Gamma = 1/2 alpha (K^-1 - A^-1 - u u^T)              (dl/dG)
//   dl/dKf = 2 Kf Gamma + delta (alpha u)^T,  dl/ddelta = alpha Kf u
//   Psi = Gamma / alpha - 1/2 alpha K^-1 G K^-1          (dl/dK)
//   dl/dalpha = -1/2 tr(A^-1 G) + u^T g - 1/2 u^T G u - 1/2 (T sigma^2 - tr(K^-1 G))
// and E = dl/dK(.,.) o K(.,.) is pushed through the SE kernel:  dx = -(x r - E z)/l^2, dz = (E^T x - z c)/l^2,
// dlog l = (sum r x^2 - 2 sum z (E^T x) + sum c z^2)/l^2, dlog sigma^2 = sum E   (r, c: row / column sums of E).
// Dense contractions run on the fp64 MFMA through one general batched C = A^T B kernel.
#include "kernels.h"
#include "grad.h"
#include "gemm_rowmajor.h"
#include <cstdint>

namespace ffvd {

__device__ __forceinline__ double block_sum(double v, double *scratch /*[blockDim.x]*/) {
    const int tid = threadIdx.x, n = blockDim.x;
    scratch[tid] = v;
    __syncthreads();
    for (int s = n >> 1; s > 0; s >>= 1) {
        if (tid < s) scratch[tid] += scratch[tid + s];
        __syncthreads();
    }
    const double r = scratch[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------
// General batched C = A^T B:  A [rows x lda] (first nA columns), B [rows x ldb] (first nB columns),
// C [nA x nB] (ld ldc).  128x128 output tile per workgroup, 8 wavefronts of 64x32, two workgroups per CU,
// register-staged double-buffered LDS (the layout of the forward Gram kernel, full rectangular tiling).
// Epilogues:
//   ATB_PLAIN : C = acc
//   ATB_GAMMA : (A = B = L_A^-1)  C = 1/2 alpha (Kinv - acc - u_i u_j);  partial sums of sum_ij acc * K_ij
//   ATB_BWD_E : (A = Kf^T, B = Gamma)  C[t][m] = (2 acc + alpha delta_t u_m) * Kf[t][m]
// ---------------------------------------------------------------------------------------------
// LDS hand-off between the lanes of ONE wavefront
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// (wave_lds_order: dev_common.h; row16_sum, AT, A_LD and the shared row-major main loop: gemm_rowmajor.h)

// AROW: the left operand is stored [i][k] (row-major over the OUTPUT rows, e.g. K_fu itself with i = t) instead of
// [k][i]; its 128 x 16 chunk is transposed on the way into LDS, so no transposed copy of K_fu has to exist in HBM.
template <int MODE, bool AROW>
__global__ __launch_bounds__(512, 4) void atb_kernel(AtbArgs a) {
    __shared__ double As[2][AT][A_LD];
    __shared__ double Bs[2][AT][A_LD];
    __shared__ double red[512];
    // XCD-aware mapping: workgroup ids go round-robin over the 8 XCDs, so all tiles of one unit take ids of the same
    // residue: the unit's operands (2 x 2 MB at M = 512) are then read through ONE 4 MB L2 instead of all eight
    // (these M^3-sized batched products are bound by operand re-reads, not by the matrix pipe)
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int bz = (loc / a.ntile) * 8 + xcd;
    if (bz >= a.nb) return;
    const int tile = loc % a.ntile;
    const int ntj = (a.nB + 127) / 128;
    int ti = tile / ntj, tj = tile % ntj;
    if ((MODE == ATB_GAMMA || MODE == ATB_PLAIN) && a.sym) {   // lower-triangular tile list: tile = ti (ti + 1) / 2 + tj
        ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
        tj = tile - ti * (ti + 1) / 2;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const int I0 = ti * 128 + wr * 64, J0 = tj * 128 + wc * 32;
    const bool active = (I0 < a.nA) && (J0 < a.nB);
    const double *Ab = a.A + (size_t)(a.a_per_dim ? (bz % a.Dl) : bz) * a.a_stride;
    const double *Bb = a.B + (size_t)(a.b_per_dim ? (bz % a.Dl) : bz) * a.b_stride;
    const int colA = ti * 128 + 2 * lane, colB = tj * 128 + 2 * lane;
    const bool okA = colA < a.nA, okB = colB < a.nB;
    const int colAc = okA ? colA : 0, colBc = okB ? colB : 0;
    const int rowl = tid >> 6;

    double2 ra[2], rb[2];
    // AROW: thread -> output row ti*128 + (tid >> 2), k-values 4 (tid & 3) .. + 3 of the chunk (32 contiguous bytes)
    const int arow = ti * 128 + (tid >> 2), aseg = 4 * (tid & 3);
    const bool okAr = arow < a.nA;
    const double *Arow = Ab + (size_t)(okAr ? arow : 0) * a.lda + aseg;
    auto gload = [&](int c) {
        if (AROW) {
            ra[0] = *reinterpret_cast<const double2 *>(Arow + (size_t)c * AT);
            ra[1] = *reinterpret_cast<const double2 *>(Arow + (size_t)c * AT + 2);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const size_t t = (size_t)c * AT + rowl + 8 * i;
            if (!AROW) ra[i] = *reinterpret_cast<const double2 *>(Ab + t * a.lda + colAc);
            rb[i] = *reinterpret_cast<const double2 *>(Bb + t * a.ldb + colBc);
        }
    };
    auto lstore = [&](int buf) {
        if (AROW) {
            const int il = tid >> 2;
            As[buf][aseg + 0][il] = okAr ? ra[0].x : 0.0;
            As[buf][aseg + 1][il] = okAr ? ra[0].y : 0.0;
            As[buf][aseg + 2][il] = okAr ? ra[1].x : 0.0;
            As[buf][aseg + 3][il] = okAr ? ra[1].y : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double2 va = ra[i], vb = rb[i];
            va.x = okA ? va.x : 0.0; va.y = okA ? va.y : 0.0;
            vb.x = okB ? vb.x : 0.0; vb.y = okB ? vb.y : 0.0;
            if (!AROW) *reinterpret_cast<double2 *>(&As[buf][rowl + 8 * i][2 * lane]) = va;
            *reinterpret_cast<double2 *>(&Bs[buf][rowl + 8 * i][2 * lane]) = vb;
        }
    };
    d4 acc[4][2];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    int nchunk = a.rows / AT;
    int c0 = (!AROW && a.k_lower) ? ((ti > tj ? ti : tj) * 128) / AT : 0;
    if (!AROW && a.krange) {
        int k0 = 0, k1 = a.rows;
        if ((a.krange & 1) && ti * 128 > k0) k0 = ti * 128;
        if ((a.krange & 2) && tj * 128 > k0) k0 = tj * 128;
        if ((a.krange & 4) && (ti + 1) * 128 < k1) k1 = (ti + 1) * 128;
        if ((a.krange & 8) && (tj + 1) * 128 < k1) k1 = (tj + 1) * 128;
        if (k0 / AT > c0) c0 = k0 / AT;
        if (k1 / AT < nchunk) nchunk = k1 / AT;
    }
    gload(c0);
    lstore(c0 & 1);
    __syncthreads();
    for (int c = c0; c < nchunk; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunk) gload(c + 1);
        if (active) {
#pragma unroll
            for (int ks = 0; ks < AT / 4; ++ks) {
                double af[4], bf[2];
#pragma unroll
                for (int x = 0; x < 4; ++x) af[x] = As[buf][4 * ks + lk][wr * 64 + 16 * x + lr];
#pragma unroll
                for (int y = 0; y < 2; ++y) bf[y] = Bs[buf][4 * ks + lk][wc * 32 + 16 * y + lr];
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
            }
        }
        if (c + 1 < nchunk) lstore(buf ^ 1);
        __syncthreads();
    }

    const int b = a.b0 + bz, s = b / a.Dl, dl = b % a.Dl, dg = a.d_begin + dl;
    double *Cb = a.C + (size_t)bz * a.c_stride;
    double part = 0.0;
    if (active) {
        double alpha = 1.0;
        if (MODE != ATB_PLAIN) alpha = 1.0 / exp(a.log_Q[dg]);
        const double *ub = (MODE != ATB_PLAIN) ? a.u + (size_t)((MODE == ATB_BWD_E && a.u_per_dim) ? dl : bz) * a.u_stride : nullptr;
        const double *rv = (MODE == ATB_BWD_E && a.rvec) ? a.rvec + (size_t)bz * a.nA : nullptr;
        const double *Xs = (MODE == ATB_BWD_E) ? a.X + (size_t)s * (a.T + 1) * a.D : nullptr;
        const double *Kf = (MODE == ATB_BWD_E) ? a.Kf + (size_t)bz * a.kf_stride : nullptr;
        const double *Kinv = (MODE == ATB_GAMMA) ? a.Kinv + (size_t)dl * a.k_stride : nullptr;
        const double *Kc = (MODE == ATB_GAMMA) ? a.Kcopy + (size_t)dl * a.k_stride : nullptr;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = I0 + 16 * x + lk + 4 * q;
                if (i >= a.nA) continue;
                double rowv = 0.0;
                if (MODE == ATB_GAMMA) rowv = ub[i];
                if (MODE == ATB_BWD_E) rowv = (i < a.T) ? alpha * (rv ? rv[i] : Xs[(size_t)(i + 1) * a.D + dg] - Xs[(size_t)i * a.D + dg]) : 0.0;
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const int j = J0 + 16 * y + lr;
                    if (j >= a.nB) continue;
                    const double g = acc[x][y][q];
                    double v = g;
                    if (MODE == ATB_GAMMA) {
                        v = 0.5 * alpha * (Kinv[(size_t)i * a.ldk + j] - g - rowv * ub[j]);
                        const bool mirror = a.sym && ti != tj;
                        part += (mirror ? 2.0 : 1.0) * (g * Kc[(size_t)i * a.ldk + j]);
                        if (mirror) Cb[(size_t)j * a.ldc + i] = v;       // K^-1, A^-1, u u^T are all symmetric
                    } else if (MODE == ATB_BWD_E) {
                        v = 2.0 * g + rowv * ub[j];
                        if (!a.no_hadamard) v *= Kf[(size_t)i * a.ldkf + j];
                    } else if (MODE == ATB_PLAIN) {
                        if (a.sym && ti != tj) Cb[(size_t)j * a.ldc + i] = v;      // symmetric product: mirrored tile
                    }
                    Cb[(size_t)i * a.ldc + j] = v;
                }
            }
    }
    if (MODE == ATB_GAMMA) {
        red[tid] = part;
        __syncthreads();
        for (int st = 256; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) a.part[(size_t)bz * a.ntile + tile] = red[0];
    }
}

// ---------------------------------------------------------------------------------------------
// Small-product variant of the plain A^T B (ATB_PLAIN only): 64 x 64 tile per 256-thread workgroup (four wavefronts of
// 32 x 32), four workgroups per CU.  The M x M x M products of the whitened backward pass have 8-32 k-chunks per
// workgroup; with 128 x 128 tiles and two workgroups per CU prologue, epilogue and the lockstep of equal workgroups left
// the matrix pipe 35-50 % busy.  Four times as many, four times smaller workgroups overlap those phases, and the
// triangular k-ranges are cut at 64 instead of 128.
// ---------------------------------------------------------------------------------------------
constexpr int S_LD = 64 + 8;
template <int MODE>
__global__ __launch_bounds__(256, 4) void atb64_kernel(AtbArgs a) {
    __shared__ double As[2][AT][S_LD];
    __shared__ double Bs[2][AT][S_LD];
    __shared__ double red64[4];
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int bz = (loc / a.ntile) * 8 + xcd;
    if (bz >= a.nb) return;
    const int tile = loc % a.ntile;
    const int ntj = (a.nB + 63) / 64;
    int ti = tile / ntj, tj = tile % ntj;
    if (a.sym) {
        ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
        tj = tile - ti * (ti + 1) / 2;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lr = lane & 15, lk = lane >> 4;
    const int I0 = ti * 64 + wr * 32, J0 = tj * 64 + wc * 32;
    const double *Ab = a.A + (size_t)(a.a_per_dim ? (bz % a.Dl) : bz) * a.a_stride;
    const double *Bb = a.B + (size_t)(a.b_per_dim ? (bz % a.Dl) : bz) * a.b_stride;
    // staging: thread t moves 16 bytes of rows (t >> 5) and (t >> 5) + 8, columns 2 (t & 31) of each operand
    const int srow = tid >> 5, scol = 2 * (tid & 31);
    const int colA = ti * 64 + scol, colB = tj * 64 + scol;
    const bool okA = colA < a.nA, okB = colB < a.nB;
    const int colAc = okA ? colA : 0, colBc = okB ? colB : 0;
    double2 ra[2], rb[2];
    auto gload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const size_t t = (size_t)c * AT + srow + 8 * i;
            ra[i] = *reinterpret_cast<const double2 *>(Ab + t * a.lda + colAc);
            rb[i] = *reinterpret_cast<const double2 *>(Bb + t * a.ldb + colBc);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double2 va = ra[i], vb = rb[i];
            va.x = okA ? va.x : 0.0; va.y = okA ? va.y : 0.0;
            vb.x = okB ? vb.x : 0.0; vb.y = okB ? vb.y : 0.0;
            *reinterpret_cast<double2 *>(&As[buf][srow + 8 * i][scol]) = va;
            *reinterpret_cast<double2 *>(&Bs[buf][srow + 8 * i][scol]) = vb;
        }
    };
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    int k0 = 0, k1 = a.rows;
    if ((a.krange & 1) && ti * 64 > k0) k0 = ti * 64;
    if ((a.krange & 2) && tj * 64 > k0) k0 = tj * 64;
    if ((a.krange & 4) && (ti + 1) * 64 < k1) k1 = (ti + 1) * 64;
    if ((a.krange & 8) && (tj + 1) * 64 < k1) k1 = (tj + 1) * 64;
    if (a.k_lower && (ti > tj ? ti : tj) * 64 > k0) k0 = (ti > tj ? ti : tj) * 64;
    const int c0 = k0 / AT, nchunk = k1 / AT;
    if (c0 < nchunk) {
        gload(c0);
        lstore(c0 & 1);
        __syncthreads();
        for (int c = c0; c < nchunk; ++c) {
            const int buf = c & 1;
            if (c + 1 < nchunk) gload(c + 1);
#pragma unroll
            for (int ks = 0; ks < AT / 4; ++ks) {
                double af[2], bf[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) af[x] = As[buf][4 * ks + lk][wr * 32 + 16 * x + lr];
#pragma unroll
                for (int y = 0; y < 2; ++y) bf[y] = Bs[buf][4 * ks + lk][wc * 32 + 16 * y + lr];
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
            }
            if (c + 1 < nchunk) lstore(buf ^ 1);
            __syncthreads();
        }
    }
    double *Cb = a.C + (size_t)bz * a.c_stride;
    const bool mirror = a.sym && ti != tj;
    double alpha = 1.0, part = 0.0;
    const double *ub = nullptr, *Kinv = nullptr, *Kc = nullptr;
    if (MODE == ATB_GAMMA) {
        const int dl = (a.b0 + bz) % a.Dl;
        alpha = 1.0 / exp(a.log_Q[a.d_begin + dl]);
        ub = a.u + (size_t)bz * a.u_stride;
        Kinv = a.Kinv + (size_t)dl * a.k_stride;
        Kc = a.Kcopy + (size_t)dl * a.k_stride;
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = I0 + 16 * x + lk + 4 * q;
            if (i >= a.nA) continue;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const int j = J0 + 16 * y + lr;
                if (j >= a.nB) continue;
                const double g = acc[x][y][q];
                double v = g;
                if (MODE == ATB_GAMMA) {
                    v = 0.5 * alpha * (Kinv[(size_t)i * a.ldk + j] - g - ub[i] * ub[j]);
                    part += (mirror ? 2.0 : 1.0) * (g * Kc[(size_t)i * a.ldk + j]);
                }
                Cb[(size_t)i * a.ldc + j] = v;
                if (mirror) Cb[(size_t)j * a.ldc + i] = v;
            }
        }
    if (MODE == ATB_GAMMA) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) part += __shfl_xor(part, m);
        if (lane == 0) red64[wave] = part;
        __syncthreads();
        if (tid == 0) a.part[(size_t)bz * a.ntile + tile] = (red64[0] + red64[1]) + (red64[2] + red64[3]);
    }
}

void launch_atb(hipStream_t stream, const AtbArgs &a_in) {
    AtbArgs a = a_in;
    // few units (the per-dim products of the K_uu side): 128 x 128 tiles would leave most CUs without a workgroup
    const bool few = (size_t)a.nb * ((a.nA + 127) / 128) * ((a.nB + 127) / 128) <= 512;
    if (a.mode == ATB_PLAIN && (a.small_tiles || few)) {
        const int n64i = (a.nA + 63) / 64, n64j = (a.nB + 63) / 64;
        a.ntile = a.sym ? n64i * (n64i + 1) / 2 : n64i * n64j;
        hipLaunchKernelGGL(atb64_kernel<ATB_PLAIN>, dim3((unsigned)(((a.nb + 7) / 8) * 8 * a.ntile)), dim3(256), 0, stream, a);
        return;
    }
    if (a.mode == ATB_GAMMA && a.small_tiles && a.sym) {
        const int n64 = (a.nA + 63) / 64;
        a.ntile = n64 * (n64 + 1) / 2;
        hipLaunchKernelGGL(atb64_kernel<ATB_GAMMA>, dim3((unsigned)(((a.nb + 7) / 8) * 8 * a.ntile)), dim3(256), 0, stream, a);
        return;
    }
    const int nti = (a.nA + 127) / 128, ntj = (a.nB + 127) / 128;
    a.ntile = nti * ntj;
    if ((a.mode == ATB_GAMMA || a.mode == ATB_PLAIN) && a.sym) a.ntile = nti * (nti + 1) / 2;
    dim3 grid((unsigned)(((a.nb + 7) / 8) * 8 * a.ntile));
    if (a.mode == ATB_PLAIN) hipLaunchKernelGGL((atb_kernel<ATB_PLAIN, false>), grid, dim3(512), 0, stream, a);
    else if (a.mode == ATB_GAMMA) hipLaunchKernelGGL((atb_kernel<ATB_GAMMA, false>), grid, dim3(512), 0, stream, a);
    else if (a.a_rowmajor) hipLaunchKernelGGL((atb_kernel<ATB_BWD_E, true>), grid, dim3(512), 0, stream, a);
    else hipLaunchKernelGGL((atb_kernel<ATB_BWD_E, false>), grid, dim3(512), 0, stream, a);
}
int atb_ntiles(int nA, int nB) { return ((nA + 127) / 128) * ((nB + 127) / 128); }
int atb_ntiles_sym(int n) { const int nt = (n + 127) / 128; return nt * (nt + 1) / 2; }
int atb_ntiles_sym64(int n) { const int nt = (n + 63) / 64; return nt * (nt + 1) / 2; }


// ---------------------------------------------------------------------------------------------
// Fused backward product (see grad.h BwdFusedArgs).  Main loop = gemm_rowmajor_a (above): the 128 x 128 tile
// g = (K_fu Gamma)[t][m] in 8 wavefronts of 64 x 32.  Epilogue, all in registers / LDS:
//   e = (2 g + alpha delta_t u_m) K_fu[t][m]                         (overwrites the accumulators)
//   columns: [cs; etx] = [1; x^T] e      -- the accumulator layout of e IS the MFMA B-operand layout (k = rows), so
//            the column sums and e^T x are 32 more MFMAs per wavefront against a [1, x] fragment from LDS;
//   rows:    [rsum, ez] = e [1, z]       -- needs e as an A operand: each wavefront transposes its 16 x 32 strips
//            through a private LDS patch (no workgroup barrier), again 32 MFMAs; the four column-quarter
//            wavefronts are then added in LDS;  kfu = K_fu u by a 16-lane shuffle reduction.
// Row partials go out per column tile (rp), column partials per 64-row block; row_combine_kernel adds the former.
// ---------------------------------------------------------------------------------------------
constexpr int XW_LD = 128 + 4;
// Debug build only (-DFFVD_BWD_TRACE, variant `bwdtrace`, tools/bwd_trace.py): per workgroup of the last bwd_fused launch the wall clock
// at its start, after the main loop, at the epilogue's phases and at its end, and where it ran (HW_ID, XCC_ID).
#ifdef FFVD_BWD_TRACE
__device__ long long bwd_trace_buf[16384 * 12];
}  // namespace ffvd
extern "C" int ffvd_debug_bwd_trace(long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ffvd::bwd_trace_buf), sizeof(long long) * 16384 * 12);
}
namespace ffvd {
#define BWD_STAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x < 16384) bwd_trace_buf[blockIdx.x * 12 + (slot)] = wall_clock64(); } while (0)
#define BWD_WHERE() do { if (threadIdx.x == 0 && blockIdx.x < 16384) bwd_trace_buf[blockIdx.x * 12 + 3] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf) << 32); } while (0)
#else
#define BWD_STAMP(slot) do { } while (0)
#define BWD_WHERE() do { } while (0)
#endif
__global__ __launch_bounds__(512, 4) void bwd_fused_kernel(BwdFusedArgs a) {
    __shared__ double As[2][AT][A_LDT];
    __shared__ double Bs[2][AT][A_LD];
    BWD_STAMP(0); BWD_WHERE();
    // XCD-aware order (speed only): consecutive workgroup ids go to the 8 XCDs round-robin, each with its own L2.  The ntj column
    // tiles of one 128-row panel of K_fu (they read the same 128 x Mp rows) take ids 8 apart, i.e. the same XCD, back to back
    // (5.24-5.33 against 5.29-5.35 ms at config 2, alternating runs on one box).
    const int ntj = (a.Mp + 127) / 128, nti = (a.Tp + 127) / 128;
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int panel = (q / ntj) * 8 + xcd, tj = q % ntj;
    if (panel >= nti * a.nb) return;
    const int bz = panel / nti, ti = panel % nti;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const int I0 = ti * 128 + wr * 64, J0 = tj * 128 + wc * 32;
    const int Mp = a.Mp, Tp = a.Tp, P = a.P;
    const double *Kfb = a.Kf + (size_t)bz * a.kf_stride;
    const int unit_or_dim = a.per_dim ? (a.b0 + bz) % a.Dl : bz;
    const double *Gb = a.Gamma + (size_t)unit_or_dim * a.g_stride;
    const RowMajorTile rt{ti, tj, tid, lane, wr, wc, lr, lk};
    TileAcc res = gemm_rowmajor_a(As, Bs, rt, Kfb, Tp, Gb, Mp, Mp, 1 << 30);
    d4 (&acc)[4][2] = res.v;
    BWD_STAMP(1);

    // ---------------- epilogue ----------------
    const int b = a.b0 + bz, s = b / a.Dl, dl = b % a.Dl, dg = a.d_begin + dl;
    const double alpha = 1.0 / exp(a.log_Q[dg]);
    const double *ub = a.u + (size_t)unit_or_dim * a.u_stride;
    const double *Xs = a.X + (size_t)s * (a.T + 1) * a.D;
    const double *rv = a.rvec ? a.rvec + (size_t)bz * Tp : nullptr;
    // LDS map (doubles; both operand buffers are free once the main loop has synchronised):
    //   As region: XW [8][XW_LD] | Vs [8][XW_LD] | dl_s [128] | row partials of the column quarters 2, 3  [2][128][8]
    //   Bs region: per-wavefront transpose patches [8][16][17]  | row partials of the column quarters 0, 1  [2][128][8]
    // row partial slots: 0 rsum, 1..P ez, 7 kfu.  Nothing aliases, so the epilogue needs two workgroup barriers: one after the
    // staging, one before the final sum over the column quarters.
    double *sm = &As[0][0][0], *sb = &Bs[0][0][0];
    double *XW = sm, *Vs = sm + 8 * XW_LD, *dl_s = sm + 16 * XW_LD, *RPhi = dl_s + 128, *RPlo = sb + 8 * (16 * 17);
    static_assert(16 * XW_LD + 128 + 2 * 128 * 8 <= 2 * AT * A_LD && 8 * 16 * 17 + 2 * 128 * 8 <= 2 * AT * A_LD, "epilogue LDS map");
    double *RPw = ((wc & 2) ? RPhi : RPlo) + (size_t)(wc & 1) * (128 * 8);      // this wavefront's column quarter
    // K_fu values of the accumulator positions: unconditional loads from clamped addresses, one 64 x 32 strip row (x) ahead of its use
    const int jc[2] = {(J0 + lr < Mp) ? J0 + lr : Mp - 1, (J0 + 16 + lr < Mp) ? J0 + 16 + lr : Mp - 1};
    const bool jok[2] = {J0 + lr < Mp, J0 + 16 + lr < Mp};
    double kf[2][4];
    auto kload = [&](int x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = I0 + 16 * x + lk + 4 * q;
            const double *row = Kfb + (size_t)((i < Tp) ? i : Tp - 1) * Mp;
#pragma unroll
            for (int y = 0; y < 2; ++y) kf[y][q] = row[jc[y]];
        }
    };
    kload(0);
    for (int idx = tid; idx < 8 * 128; idx += 512) {
        const int p = idx >> 7, r = idx & 127;
        const int t = ti * 128 + r, j = tj * 128 + r;
        double xv = 0.0, zv = 0.0;
        if (p == 0) { xv = 1.0; zv = 1.0; }
        else if (p <= P) {
            const int pp = p - 1;
            if (t < a.T) xv = (pp < a.D) ? Xs[(size_t)t * a.D + pp] : a.ctrl[(size_t)t * a.C + (pp - a.D)];
            if (j < a.M) zv = a.Z[(size_t)j * P + pp];
        }
        XW[p * XW_LD + r] = xv;
        Vs[p * XW_LD + r] = zv;
    }
    if (tid < 128) {
        const int t = ti * 128 + tid;
        dl_s[tid] = (t < a.T) ? alpha * (rv ? rv[t] : Xs[(size_t)(t + 1) * a.D + dg] - Xs[(size_t)t * a.D + dg]) : 0.0;
    }
    double uj[2];
#pragma unroll
    for (int y = 0; y < 2; ++y) uj[y] = jok[y] ? ub[jc[y]] : 0.0;
    __syncthreads();
    BWD_STAMP(4);
    // One 16-row strip (x) of the wavefront's 64 x 32 block at a time, so that its accumulators die as the loop advances:
    //   e in place of g, the kfu partial over the wavefront's 32 columns (16-lane DPP sum);
    //   columns: [cs; etx] += [1; x^T] e -- the accumulator layout of e IS the B-operand layout with k = rows;
    //   rows: [rsum, ez] = e [1, z] -- needs e as an A operand, i.e. transposed: each 16 x 16 block goes through a private LDS
    //   patch.  LDS serves one wavefront's accesses in order, so only the compiler needs a fence (a workgroup-scope fence would
    //   also wait for outstanding global accesses).
    // The K_fu values of strip x + 1 are requested before the matrix work of strip x.
    d4 ac[2] = {(d4){0.0, 0.0, 0.0, 0.0}, (d4){0.0, 0.0, 0.0, 0.0}};
    double *Tw = sb + wave * (16 * 17);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        // the strip's four [1; x^T] fragments are requested first: an LDS read takes hundreds of cycles beside the other workgroup's main
        // loop (stamps: 8 MFMAs behind 8 reads took 2.3 us), the e pass below covers them
        double xwf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) xwf[ks] = (lr < 8) ? XW[lr * XW_LD + wr * 64 + 16 * x + 4 * ks + lk] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int il = wr * 64 + 16 * x + lk + 4 * q;
            const bool iok = ti * 128 + il < Tp;
            const double rowv = dl_s[il];
            double v = 0.0;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const bool ok = iok && jok[y];
                const double k = ok ? kf[y][q] : 0.0;
                acc[x][y][q] = (2.0 * acc[x][y][q] + rowv * uj[y]) * (a.linear ? (ok ? 1.0 : 0.0) : k);
                v += k * uj[y];
            }
            v = row16_sum(v);
            if (lr == 0) RPw[il * 8 + 7] = v;
        }
        if (x == 0) BWD_STAMP(7);
        if (x + 1 < 4) kload(x + 1);
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) ac[y] = mfma_f64(xwf[ks], acc[x][y][ks], ac[y]);
        if (x == 0) BWD_STAMP(8);
        d4 r4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int y = 0; y < 2; ++y) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Tw[(lk + 4 * q) * 17 + lr] = acc[x][y][q];
            wave_lds_order();
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const double af = Tw[lr * 17 + 4 * ks + lk];
                const double bf = (lr < 8) ? Vs[lr * XW_LD + wc * 32 + 16 * y + 4 * ks + lk] : 0.0;
                r4 = mfma_f64(af, bf, r4);
            }
            wave_lds_order();
        }
        if (lr < 7) {
#pragma unroll
            for (int q = 0; q < 4; ++q) RPw[(wr * 64 + 16 * x + lk + 4 * q) * 8 + lr] = r4[q];
        }
        if (x == 0) BWD_STAMP(9);
    }
    BWD_STAMP(5);
    {       // column partials of the 64-row block (ti, wr)
        const int nblk = Tp / 64, blk = ti * 2 + wr;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int j = J0 + 16 * y + lr;
            if (j < Mp && blk < nblk) {
                const size_t pb = ((size_t)bz * nblk + blk) * Mp + j;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int p = lk + 4 * q;
                    if (p == 0) a.cs_part[pb] = ac[y][q];
                    else if (p <= P) a.etx_part[pb * P + (p - 1)] = ac[y][q];
                }
            }
        }
    }
    __syncthreads();
    BWD_STAMP(6);
    for (int idx = tid; idx < 128 * 8; idx += 512) {
        const int row = idx >> 3, c = idx & 7;
        const int t = ti * 128 + row;
        if (t >= Tp) continue;
        const double v = (RPlo[row * 8 + c] + RPlo[128 * 8 + row * 8 + c]) + (RPhi[row * 8 + c] + RPhi[128 * 8 + row * 8 + c]);
        a.rp[(((size_t)tj * a.nb + bz) * Tp + t) * 8 + c] = v;
    }
    BWD_STAMP(2);
}

// Adds the row partials of the column tiles and forms the per-block sums rx2[p] = sum_t r_t x_tp^2.
__global__ __launch_bounds__(256) void row_combine_kernel(BwdFusedArgs a) {
    __shared__ double scratch[256];
    __shared__ double rs[64];
    const int blk = blockIdx.x, bz = blockIdx.y, tid = threadIdx.x;
    const int ntj = (a.Mp + 127) / 128, P = a.P, Tp = a.Tp;
    const int b = a.b0 + bz, s = b / a.Dl;
    for (int idx = tid; idx < 64 * 8; idx += 256) {
        const int r = idx >> 3, c = idx & 7, t = blk * 64 + r;
        double v = 0.0;
        for (int j = 0; j < ntj; ++j) v += a.rp[(((size_t)j * a.nb + bz) * Tp + t) * 8 + c];
        if (c == 0) { a.rsum[(size_t)bz * Tp + t] = v; rs[r] = v; }
        else if (c <= P) a.ez[((size_t)bz * Tp + t) * P + (c - 1)] = v;
        else if (c == 7) a.kfu[(size_t)bz * Tp + t] = v;
    }
    __syncthreads();
    const double *Xs = a.X + (size_t)s * (a.T + 1) * a.D;
    const int nblk = Tp / 64;
    for (int p = 0; p < P; ++p) {
        double v = 0.0;
        if (tid < 64) {
            const int t = blk * 64 + tid;
            if (t < a.T) {
                const double xv = (p < a.D) ? Xs[(size_t)t * a.D + p] : a.ctrl[(size_t)t * a.C + (p - a.D)];
                v = rs[tid] * xv * xv;
            }
        }
        v = block_sum(v, scratch);
        if (tid == 0) a.rx2_part[((size_t)bz * nblk + blk) * P + p] = v;
    }
}

size_t bwd_fused_rp_doubles(int Mp, int Tp, int nb) { return (size_t)((Mp + 127) / 128) * nb * Tp * 8; }
void launch_bwd_fused(hipStream_t stream, const BwdFusedArgs &a) {
    const int nti = (a.Tp + 127) / 128, ntj = (a.Mp + 127) / 128;
    const unsigned ngroups = (unsigned)(((size_t)nti * a.nb + 7) / 8);
    hipLaunchKernelGGL(bwd_fused_kernel, dim3(ngroups * 8 * ntj), dim3(512), 0, stream, a);
    hipLaunchKernelGGL(row_combine_kernel, dim3(a.Tp / 64, a.nb), dim3(256), 0, stream, a);
}

// ---------------------------------------------------------------------------------------------
// proj_gemm_kernel (see grad.h ProjGemmArgs): same tiling and staging as the backward product (128 x 128 tile, 8
// wavefronts of 64 x 32, K_fu chunk transposed into LDS), depth limited to k < (tj + 1) * 128 because W is upper
// triangular; inside that last block a wavefront stops at its own last column.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 4) void proj_gemm_kernel(ProjGemmArgs a) {
    __shared__ double As[2][AT][A_LDT];
    __shared__ double Bs[2][AT][A_LD];
    const int bz = blockIdx.y;
    const int ntj = (a.Mp + 127) / 128;
    // heavy column tiles (long k range) first: blockIdx.x / nti counts tj downwards
    const int nti = (a.Tp + 127) / 128;
    const int tj = ntj - 1 - (int)(blockIdx.x / nti), ti = blockIdx.x % nti;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lr = lane & 15, lk = lane >> 4;
    const int I0 = ti * 128 + wr * 64, J0 = tj * 128 + wc * 32;
    const int Mp = a.Mp, Tp = a.Tp;
    const int b = a.b0 + bz, dl = b % a.Dl;
    const double *Kfb = a.Kf + (size_t)bz * a.kf_stride;
    const double *Wb = a.W + (size_t)dl * a.w_stride;
    const int kend = ((tj + 1) * 128 < Mp) ? (tj + 1) * 128 : Mp;       // W[k][j] = 0 for k > j
    const RowMajorTile rt{ti, tj, tid, lane, wr, wc, lr, lk};
    TileAcc res = gemm_rowmajor_a(As, Bs, rt, Kfb, Tp, Wb, Mp, kend, (J0 + 31) / AT);
    d4 (&acc)[4][2] = res.v;
    // epilogue: F (if wanted), the row sums of F^2 and (explicit-U branch) of F u over this tile's columns
    double *Fb = a.F ? a.F + (size_t)bz * a.f_stride : nullptr;
    const double *ub = a.u ? a.u + (size_t)dl * a.u_stride : nullptr;
    const bool tile_inside = (ti + 1) * 128 <= Tp && (tj + 1) * 128 <= Mp;       // uniform: the stores of F need no per-element test
    double *rs_s = &As[0][0][0];                     // [4 wc][128 rows]
    double *fm_s = &Bs[0][0][0];
    double *dl_s = rs_s + 512, *cp_s = rs_s + 640;   // delta of the tile's 128 rows; [8 wavefronts][4 lk][32 columns] partials
    if (a.gpart) {
        if (tid < 128) {
            const int t = ti * 128 + tid, s = b / a.Dl, dg = a.d_begin + dl;
            const double *Xs = a.X + (size_t)s * (a.T + 1) * a.D;
            dl_s[tid] = (t < a.T) ? Xs[(size_t)(t + 1) * a.D + dg] - Xs[(size_t)t * a.D + dg] : 0.0;
        }
        __syncthreads();
        double cp[2] = {0.0, 0.0};
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double dv = dl_s[wr * 64 + 16 * x + lk + 4 * q];
#pragma unroll
                for (int y = 0; y < 2; ++y) cp[y] = fma(dv, acc[x][y][q], cp[y]);
            }
#pragma unroll
        for (int y = 0; y < 2; ++y) cp_s[(wave * 4 + lk) * 32 + 16 * y + lr] = cp[y];
    }
    double uj[2];
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        const int j = J0 + 16 * y + lr;
        uj[y] = (ub && j < Mp) ? ub[j] : 0.0;
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = I0 + 16 * x + lk + 4 * q;
            double v = 0.0, w = 0.0;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const int j = J0 + 16 * y + lr;
                const double f = acc[x][y][q];
                if (Fb && (tile_inside || (i < Tp && j < Mp))) Fb[(size_t)i * Mp + j] = f;
                v += f * f;
                w += f * uj[y];
            }
            v = row16_sum(v);               // DPP (__shfl_xor is an LDS round trip per step)
            if (ub) w = row16_sum(w);
            if (lr == 0) {
                rs_s[wc * 128 + wr * 64 + 16 * x + lk + 4 * q] = v;
                fm_s[wc * 128 + wr * 64 + 16 * x + lk + 4 * q] = w;
            }
        }
    __syncthreads();
    if (tid < 128) {
        const int t = ti * 128 + tid;
        if (t < Tp) {
            const size_t o = ((size_t)b * ntj + tj) * Tp + t;
            a.rowsq[o] = (rs_s[tid] + rs_s[128 + tid]) + (rs_s[256 + tid] + rs_s[384 + tid]);
            if (a.fmean) a.fmean[o] = (fm_s[tid] + fm_s[128 + tid]) + (fm_s[256 + tid] + fm_s[384 + tid]);
        }
    } else if (a.gpart && tid < 256) {       // column c of the tile: wavefronts (wr, wc = c / 32), four lk partials each, fixed order
        const int c = tid - 128, wq = c >> 5, cc = c & 31, j = tj * 128 + c;
        if (j < Mp) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) v += cp_s[((r * 4 + wq) * 4 + k) * 32 + cc];
            a.gpart[((size_t)bz * ((Tp + 127) / 128) + ti) * Mp + j] = v;
        }
    }
}
void launch_proj_gemm(hipStream_t stream, const ProjGemmArgs &a) {
    const int nti = (a.Tp + 127) / 128, ntj = (a.Mp + 127) / 128;
    hipLaunchKernelGGL(proj_gemm_kernel, dim3(nti * ntj, a.nb), dim3(512), 0, stream, a);
}

// ---------------------------------------------------------------------------------------------
// small dense helpers
// ---------------------------------------------------------------------------------------------
// out[b] = u_b^T K_d u_b   (K = K_uu + jitter I with identity padding)
__global__ __launch_bounds__(256) void uku_kernel(const double *u, size_t u_stride, const double *K, size_t k_stride,
                                                  int Mp, int Dl, double *out) {
    __shared__ double scratch[256];
    const int bz = blockIdx.x, tid = threadIdx.x;
    const double *ub = u + (size_t)bz * u_stride, *Kd = K + (size_t)(bz % Dl) * k_stride;
    double acc = 0.0;
    for (int i = tid; i < Mp; i += 256) {
        double row = 0.0;
        for (int j = 0; j < Mp; ++j) row += Kd[(size_t)i * Mp + j] * ub[j];
        acc += ub[i] * row;
    }
    acc = block_sum(acc, scratch);
    if (tid == 0) out[bz] = acc;
}
void launch_uku(hipStream_t stream, const double *u, size_t u_stride, const double *K, size_t k_stride, int Mp, int Dl,
                int nb, double *out) {
    hipLaunchKernelGGL(uku_kernel, dim3(nb), dim3(256), 0, stream, u, u_stride, K, k_stride, Mp, Dl, out);
}
// out[b] = u_b^T u_b: what uku_kernel computes against the identity (the whitened backward pass wants w^T w), with the same
// partition of the sum over the threads -- bit-identical -- and without walking an M x M identity matrix row by row per thread
// (0.93 ms for 128 units at M = 512, the head of the side chain of the training step: VERDICT r3 W11).
__global__ __launch_bounds__(256) void utu_kernel(const double *u, size_t u_stride, int Mp, double *out) {
    __shared__ double scratch[256];
    const int bz = blockIdx.x, tid = threadIdx.x;
    const double *ub = u + (size_t)bz * u_stride;
    double acc = 0.0;
    for (int i = tid; i < Mp; i += 256) {
        double row = 0.0;
        row += ub[i];                       // (the identity's row i: exact zeros elsewhere)
        acc += ub[i] * row;
    }
    acc = block_sum(acc, scratch);
    if (tid == 0) out[bz] = acc;
}
void launch_utu(hipStream_t stream, const double *u, size_t u_stride, int Mp, int nb, double *out) {
    hipLaunchKernelGGL(utu_kernel, dim3(nb), dim3(256), 0, stream, u, u_stride, Mp, out);
}

// out[dl][e] = sum_s in[(s*Dl + dl)][e]  (fixed order over chains: deterministic)
__global__ void chain_sum_kernel(const double *in, size_t in_stride, int S, int Dl, size_t n, double *out, size_t out_stride) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int dl = blockIdx.y;
    if (e >= n) return;
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += in[(size_t)(s * Dl + dl) * in_stride + e];
    out[(size_t)dl * out_stride + e] = acc;
}
void launch_chain_sum(hipStream_t stream, const double *in, size_t in_stride, int S, int Dl, size_t n, double *out,
                      size_t out_stride) {
    hipLaunchKernelGGL(chain_sum_kernel, dim3((unsigned)((n + 255) / 256), Dl), dim3(256), 0, stream, in, in_stride, S,
                       Dl, n, out, out_stride);
}

// E'[dl] = ( GamSum/alpha_sum_form - 1/2 Kinv (Asum - S K) Kinv ) o K_uu(no jitter)  where the caller provides
//   gsum = sum_s Gamma_s / alpha  (already divided),  kgk = Kinv (Asum - S K) Kinv
__global__ void psi_e_kernel(const double *gsum, const double *kgk, const double *Kcopy, int M, int Mp, double jitter,
                             double *Eout, int kind) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int dl = blockIdx.y;
    if (idx >= (size_t)Mp * Mp) return;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    const size_t o = (size_t)dl * Mp * Mp + idx;
    double v = 0.0;
    if (i < M && j < M) {
        const double kuu = (kind != 0) ? 1.0 : Kcopy[o] - ((i == j) ? jitter : 0.0);     // LinearK: no Hadamard product (as epsi_a_kernel)
        v = (gsum[o] - 0.5 * kgk[o]) * kuu;
    }
    Eout[o] = v;
}
void launch_psi_e(hipStream_t stream, const double *gsum, const double *kgk, const double *Kcopy, int M, int Mp, int Dl,
                  double jitter, double *Eout, int kind) {
    hipLaunchKernelGGL(psi_e_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, gsum, kgk,
                       Kcopy, M, Mp, jitter, Eout, kind);
}

// xsq_unit[s * Dl + dl] = sum_t |x_t|^2 over the GP inputs x_t = [X_s[t], ctrl[t]] of chain s (LinearK: Kdiag_t = variance |x_t|^2 sits
// in the trace term of the collapsed bound; the explicit-U branch gets the same sums from resid_a_kernel)
__global__ __launch_bounds__(256) void xsq_unit_kernel(const double *X, const double *ctrl, int T, int D, int C, int Dl, double *xsq_unit) {
    __shared__ double scratch[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const double *Xs = X + (size_t)s * (T + 1) * D;
    double acc = 0.0;
    for (int t = tid; t < T; t += 256) {
        double xsq = 0.0;
        for (int p = 0; p < D; ++p) xsq += Xs[(size_t)t * D + p] * Xs[(size_t)t * D + p];
        for (int p = 0; p < C; ++p) xsq += ctrl[(size_t)t * C + p] * ctrl[(size_t)t * C + p];
        acc += xsq;
    }
    acc = block_sum(acc, scratch);
    if (tid < Dl) xsq_unit[(size_t)s * Dl + tid] = acc;
}
void launch_xsq_unit(hipStream_t stream, const double *X, const double *ctrl, int T, int D, int C, int S, int Dl, double *xsq_unit) {
    hipLaunchKernelGGL(xsq_unit_kernel, dim3(S), dim3(256), 0, stream, X, ctrl, T, D, C, Dl, xsq_unit);
}

// in-place: upper triangle <- lower triangle (the forward Gram kernel only writes lower-triangular tiles)
__global__ void symmetrize_kernel(double *A, int Mp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    double *Ad = A + (size_t)blockIdx.y * Mp * Mp;
    if (j > i) Ad[idx] = Ad[(size_t)j * Mp + i];
}
void launch_symmetrize(hipStream_t stream, double *A, int Mp, int batch) {
    hipLaunchKernelGGL(symmetrize_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), batch), dim3(256), 0, stream, A, Mp);
}

// y = a*x + b*z elementwise on Dl matrices (used for Asum - S K and Gamma sums scaled by 1/alpha_d)
__global__ void axpby_kernel(const double *x, const double *z, double a, double bcoef, const double *log_Q, int d_begin,
                             int scale_mode, size_t n, double *out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int dl = blockIdx.y;
    if (e >= n) return;
    double aa = a;
    if (scale_mode == 1) aa = a * exp(log_Q[d_begin + dl]);      // multiply by Q_d = 1/alpha_d
    const size_t o = (size_t)dl * n + e;
    out[o] = aa * x[o] + (z ? bcoef * z[o] : 0.0);
}
void launch_axpby(hipStream_t stream, const double *x, const double *z, double a, double bcoef, const double *log_Q,
                  int d_begin, int scale_mode, size_t n, int Dl, double *out) {
    hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)((n + 255) / 256), Dl), dim3(256), 0, stream, x, z, a, bcoef, log_Q,
                       d_begin, scale_mode, n, out);
}

// out = x - s I on Dl matrices (reference-route backward: sum_s H_s - S I = W^T (alpha sum_s G_s) W)
__global__ void sub_identity_kernel(const double *x, double sc, int Mp, double *out) {
    const size_t n = (size_t)Mp * Mp, e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const size_t o = (size_t)blockIdx.y * n + e;
    out[o] = x[o] - ((e / Mp == e % Mp) ? sc : 0.0);
}
void launch_sub_identity(hipStream_t stream, const double *x, double sc, int Mp, int Dl, double *out) {
    const size_t n = (size_t)Mp * Mp;
    hipLaunchKernelGGL(sub_identity_kernel, dim3((unsigned)((n + 255) / 256), Dl), dim3(256), 0, stream, x, sc, Mp, out);
}

// ---------------------------------------------------------------------------------------------
// E-reduction, stage 1: one workgroup per (64-row block, unit); accumulators stay in registers, the inducing
// inputs of the current column slice and the x rows of the block sit in LDS.  For its rows t it produces
//   rsum[t] = sum_m E_tm,  ez[t][p] = sum_m E_tm z_mp,  kfu[t] = sum_m Kf_tm u_m   (kfu only if Kf != null)
// and the block partials over its rows:  cs[m] = sum_t E_tm,  etx[m][p] = sum_t E_tm x_tp,  rx2[p] = sum_t r_t x_tp^2.
// x rows: [ x[t][0:x_cols] | ctrl[t][0:C] ] or, for the K_uu side, the inducing inputs themselves.
// ---------------------------------------------------------------------------------------------
template <int PM, bool F32>      // PM: compile-time bound on P (8 or MAXP) so that the per-thread accumulators live in registers
__global__ __launch_bounds__(512) void e_reduce_kernel(EReduceArgs a) {
    constexpr int NT = 512, RW = 8;           // threads, rows per wavefront (8 wavefronts x 8 rows = 64 rows)
    __shared__ double xs[64][PM + 1];
    __shared__ double zsm[NT][PM + 1];          // inducing inputs of the current 512-column slice
    __shared__ double racc[64];
    __shared__ double scratch[NT];
    const int blk = blockIdx.x, bz = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = a.b0 + bz, s = b / a.Dl;
    const int t0 = blk * 64, P = a.P, Mp = a.Mp;
    const double *E = F32 ? nullptr : a.E + (size_t)bz * a.e_stride;
    const double *Kf = (!F32 && a.Kf) ? a.Kf + (size_t)bz * a.e_stride : nullptr;
    const double *ub = a.u ? a.u + (size_t)(a.u_per_dim ? b % a.Dl : bz) * a.u_stride : nullptr;
    // fp32 form: E_tm = (2 R_tm + alpha delta_t u_m) K_tm from the fp32 product and the fp32 K_fu (never stored)
    const float *R32 = F32 ? a.R32 + (size_t)bz * a.e_stride : nullptr;
    const float *K32 = F32 ? a.Kf32 + (size_t)bz * a.e_stride : nullptr;
    const int dgf = F32 ? a.d_begin + b % a.Dl : 0;
    const double alphaf = F32 ? 1.0 / exp(a.log_Q[dgf]) : 0.0;
    const double *Xdf = F32 ? a.Xd + (size_t)s * (a.T + 1) * a.D : nullptr;
    auto adelta = [&](int t) { return alphaf * (Xdf[(size_t)(t + 1) * a.D + dgf] - Xdf[(size_t)t * a.D + dgf]); };
    auto e32 = [&](int t, int m, double ad) {
        return (2.0 * (double)R32[(size_t)t * Mp + m] + ad * ub[m]) * (double)K32[(size_t)t * Mp + m];
    };
    const double *Zd = a.Z;                                          // unscaled inducing inputs M x P
    for (int idx = tid; idx < 64 * P; idx += NT) {                   // x rows of this block
        const int r = idx / P, p = idx % P, t = t0 + r;
        double v = 0.0;
        if (t < a.T) {
            if (a.x_is_z) v = Zd[(size_t)t * P + p];
            else v = (p < a.x_cols) ? a.x[(size_t)s * a.x_chain_stride + (size_t)t * a.x_ld + p] : a.ctrl[(size_t)t * a.C + (p - a.x_cols)];
        }
        xs[r][p] = v;
    }
    // row accumulators: wavefront w owns rows 8w..8w+7; lane-strided over the columns of each slice
    double rs[RW], kf[RW], ez[RW][PM];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        rs[rr] = 0.0; kf[rr] = 0.0;
#pragma unroll
        for (int p = 0; p < PM; ++p) ez[rr][p] = 0.0;
    }
    const size_t pbase = ((size_t)bz * a.nblk + blk) * Mp;
    for (int m0 = 0; m0 < Mp; m0 += NT) {
        __syncthreads();
        for (int idx = tid; idx < NT * P; idx += NT) {
            const int mm = idx / P, p = idx % P, m = m0 + mm;
            zsm[mm][p] = (m < a.M) ? Zd[(size_t)m * P + p] : 0.0;
        }
        __syncthreads();
        // ---- rows ----
#pragma unroll
        for (int rr = 0; rr < RW; ++rr) {
            const int t = t0 + wave * RW + rr;
            if (t < a.T) {
                const double adt = F32 ? adelta(t) : 0.0;
#pragma unroll
                for (int q = 0; q < NT / 64; ++q) {
                    const int mm = lane + 64 * q, m = m0 + mm;
                    if (m < a.M) {
                        const double e = F32 ? e32(t, m, adt) : E[(size_t)t * Mp + m];
                        rs[rr] += e;
                        if (F32) kf[rr] += (double)K32[(size_t)t * Mp + m] * ub[m];
                        else if (Kf) kf[rr] += Kf[(size_t)t * Mp + m] * ub[m];
#pragma unroll
                        for (int p = 0; p < PM; ++p)
                            if (p < P) ez[rr][p] += e * zsm[mm][p];
                    }
                }
            }
        }
        // ---- columns: thread tid owns column m0 + tid of this slice ----
        {
            const int m = m0 + tid;
            double cs = 0.0, etx[PM];
#pragma unroll
            for (int p = 0; p < PM; ++p) etx[p] = 0.0;
            if (m < a.M) {
                for (int r0 = 0; r0 < 64; r0 += 8) {        // eight independent loads in flight per thread
                    double e8[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int t = t0 + r0 + k, tc = t < a.T ? t : t0;
                        e8[k] = F32 ? e32(tc, m, adelta(tc)) : E[(size_t)tc * Mp + m];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const double e = (t0 + r0 + k < a.T) ? e8[k] : 0.0;
                        cs += e;
#pragma unroll
                        for (int p = 0; p < PM; ++p)
                            if (p < P) etx[p] += e * xs[r0 + k][p];
                    }
                }
            }
            if (m < Mp) {
                a.cs_part[pbase + m] = cs;
#pragma unroll
                for (int p = 0; p < PM; ++p)
                    if (p < P) a.etx_part[(pbase + m) * P + p] = etx[p];
            }
        }
    }
    // finish the rows: reduce over the 64 lanes
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int r = wave * RW + rr, t = t0 + r;
        double v = rs[rr], w = kf[rr];
        for (int off = 32; off > 0; off >>= 1) { v += __shfl_xor(v, off); w += __shfl_xor(w, off); }
#pragma unroll
        for (int p = 0; p < PM; ++p) {
            if (p < P) {
                double z = ez[rr][p];
                for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off);
                if (lane == 0) a.ez[((size_t)bz * a.Tp + t) * P + p] = z;
            }
        }
        if (lane == 0) {
            a.rsum[(size_t)bz * a.Tp + t] = v;
            if (a.kfu) a.kfu[(size_t)bz * a.Tp + t] = w;
            racc[r] = v;
        }
    }
    __syncthreads();
    for (int p = 0; p < P; ++p) {          // rx2[p] = sum_t r_t x_tp^2 over the block
        double v = 0.0;
        if (tid < 64 && t0 + tid < a.T) v = racc[tid] * xs[tid][p] * xs[tid][p];
        v = block_sum(v, scratch);
        if (tid == 0) a.rx2_part[((size_t)bz * a.nblk + blk) * P + p] = v;
    }
}
void launch_e_reduce(hipStream_t stream, const EReduceArgs &a) {
    if (a.R32) {
        if (a.P <= 8) hipLaunchKernelGGL((e_reduce_kernel<8, true>), dim3(a.nblk, a.nb), dim3(512), 0, stream, a);
        else hipLaunchKernelGGL((e_reduce_kernel<MAXP, true>), dim3(a.nblk, a.nb), dim3(512), 0, stream, a);
    } else if (a.P <= 8) hipLaunchKernelGGL((e_reduce_kernel<8, false>), dim3(a.nblk, a.nb), dim3(512), 0, stream, a);
    else hipLaunchKernelGGL((e_reduce_kernel<MAXP, false>), dim3(a.nblk, a.nb), dim3(512), 0, stream, a);
}

// E-reduction, stage 2: one workgroup per unit.  Sums the block partials in fixed order and forms
//   dz[m][p] = (etx[m][p] - z_mp cs_m) / l_p^2,  dlogl[p] = (rx2[p] - 2 sum_m z_mp etx[m][p] + sum_m cs_m z_mp^2) / l_p^2,
//   dlogs2 = sum_m cs_m,   and (K_uu side, x_is_z) dz += -(z_mp r_m - ez[m][p]) / l_p^2.
// Outputs are per unit: dz_unit [nb][M][P], dll_unit [nb][P], dls_unit [nb].
// 256 NG threads: thread (g = tid >> 8, r = tid & 255) sums block partials blk = g, g + NG, ... for rows m = r, r + 256, ...;
// the NG groups are added in fixed order through LDS (NG = 1 for large P, where that buffer would not fit).  PM bounds P at compile time so the per-thread arrays stay in
// registers (a run-time-indexed [MAXP] array goes to scratch).
template <int PM, int NG>
__global__ __launch_bounds__(256 * NG) void e_finish_kernel(EReduceArgs a, double *dz_unit, double *dll_unit, double *dls_unit) {
    __shared__ double scratch[256 * NG];
    __shared__ double grp[NG > 1 ? NG - 1 : 1][NG > 1 ? 256 : 1][PM + 1];
    const int bz = blockIdx.x, tid = threadIdx.x;
    const int g = tid >> 8, r = tid & 255;
    const int b = a.b0 + bz, dl = b % a.Dl;
    const int P = a.P, Mp = a.Mp;
    const double *len = a.len + (size_t)dl * P;
    double dls = 0.0;
    double llacc[PM];
#pragma unroll
    for (int p = 0; p < PM; ++p) llacc[p] = 0.0;
    for (int m0 = 0; m0 < a.M; m0 += 256) {
        const int m = m0 + r;
        const bool okm = m < a.M;
        double cs = 0.0;
        double etx[PM];
#pragma unroll
        for (int p = 0; p < PM; ++p) etx[p] = 0.0;
        if (okm) {
            for (int blk = g; blk < a.nblk; blk += NG) {
                const size_t pb = ((size_t)bz * a.nblk + blk) * Mp + m;
                cs += a.cs_part[pb];
#pragma unroll
                for (int p = 0; p < PM; ++p)
                    if (p < P) etx[p] += a.etx_part[pb * P + p];
            }
        }
        if (NG > 1 && g > 0) {
            grp[g - 1][r][PM] = cs;
#pragma unroll
            for (int p = 0; p < PM; ++p) grp[g - 1][r][p] = etx[p];
        }
        __syncthreads();
        if (g == 0 && okm) {
#pragma unroll
            for (int q = 0; q < NG - 1; ++q) {
                cs += grp[q][r][PM];
#pragma unroll
                for (int p = 0; p < PM; ++p) etx[p] += grp[q][r][p];
            }
            if (a.kind != 0) {
                // LinearK, K = s2 x z^T (kernels.py:276): dz_m = s2 (E^T x)_m (+ s2 (E z)_m on the K_uu side, where both
                // arguments are Z); d logvariance = sum E o K = s2 sum_mp z_mp (E^T x)_mp (K_fu side) / s2 sum z o (E z) (K_uu side)
                const double s2 = a.variance[dl];
#pragma unroll
                for (int p = 0; p < PM; ++p) {
                    if (p < P) {
                        const double z = a.Z[(size_t)m * P + p];
                        const double ezv = a.x_is_z ? a.ez[((size_t)bz * a.Tp + m) * P + p] : 0.0;
                        dz_unit[((size_t)bz * a.M + m) * P + p] = s2 * (etx[p] + ezv);
                        dls += s2 * z * (a.x_is_z ? ezv : etx[p]);
                    }
                }
            } else {
            dls += cs;
#pragma unroll
            for (int p = 0; p < PM; ++p) {
                if (p < P) {
                    const double z = a.Z[(size_t)m * P + p], inv2 = 1.0 / (len[p] * len[p]);
                    double dz = (etx[p] - z * cs) * inv2;
                    if (a.x_is_z) dz += -(z * a.rsum[(size_t)bz * a.Tp + m] - a.ez[((size_t)bz * a.Tp + m) * P + p]) * inv2;
                    dz_unit[((size_t)bz * a.M + m) * P + p] = dz;
                    llacc[p] += (-2.0 * z * etx[p] + cs * z * z) * inv2;
                }
            }
            }
        }
        __syncthreads();
    }
    dls = block_sum(dls, scratch);
#pragma unroll
    for (int p = 0; p < PM; ++p) {
        if (p < P) {                                     // uniform across the workgroup
            double v = block_sum(llacc[p], scratch);
            if (tid == 0) {
                double rx2 = 0.0;
                for (int blk = 0; blk < a.nblk; ++blk) rx2 += a.rx2_part[((size_t)bz * a.nblk + blk) * P + p];
                dll_unit[(size_t)bz * P + p] = (a.kind != 0) ? 0.0 : v + rx2 / (len[p] * len[p]);
            }
        }
    }
    if (tid == 0) dls_unit[bz] = dls;
}
void launch_e_finish(hipStream_t stream, const EReduceArgs &a, double *dz_unit, double *dll_unit, double *dls_unit) {
    if (a.P <= 8) hipLaunchKernelGGL((e_finish_kernel<8, 4>), dim3(a.nb), dim3(1024), 0, stream, a, dz_unit, dll_unit, dls_unit);
    else hipLaunchKernelGGL((e_finish_kernel<MAXP, 1>), dim3(a.nb), dim3(256), 0, stream, a, dz_unit, dll_unit, dls_unit);
}

// ---------------------------------------------------------------------------------------------
// Gradient w.r.t. the latent trajectories:  dX[s][t][p]  (everything that touches X, per chain)
//   likelihood (dgp_model.py:248-250,264), transition prior (:283-284), prior_x_0 (:252),
//   collapsed terms through x_comb (rows t < T) and through delta_t = x_{t+1,d} - x_{t,d}.
// One thread per (s, t, p); the sum over the local latent dims is in fixed order.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dx_kernel(DxArgs a) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int T = a.T, D = a.D;
    const size_t per = (size_t)(T + 1) * D;
    if (idx >= (size_t)a.S * per) return;
    const int s = (int)(idx / per), t = (int)((idx % per) / D), p = (int)(idx % D);
    const double *Xs = a.X + (size_t)s * per;
    const double Tn = (double)(a.T_norm > 0 ? a.T_norm : T);
    double g = 0.0;
    if (a.shared_terms) {
        if (t >= 1) {                                   // likelihood: row t-1 of Y sees X[t]
            double acc = 0.0;
            for (int j = 0; j < a.Ydim; ++j) {
                double ym = a.DD[j];
                for (int d = 0; d < D; ++d) ym += Xs[(size_t)t * D + d] * a.CC[(size_t)d * a.Ydim + j];
                const double R = exp(a.log_Rchols[j]);
                const double r = (a.Y[(size_t)(t - 1) * a.Ydim + j] - ym) / R;
                acc += (r / R) * a.CC[(size_t)p * a.Ydim + j];
            }
            g += -acc / Tn;
        }
        if (t == 0 && !a.skip_x0) g += Xs[p] / Tn;      // prior_x_0
    }
    // terms tied to latent dim p itself (delta_{t,p}) -- only if p is one of this handle's dims
    const int dl_p = p - a.d_begin;
    if (dl_p >= 0 && dl_p < a.Dl) {
        const double Q = exp(a.log_Q[p]);
        const size_t bb = ((size_t)s * a.Dl + dl_p) * a.Tp;
        if (t >= 1) {       // x_{t} is the "x_{t+1}" of transition t-1
            const double dlt = Xs[(size_t)t * D + p] - Xs[(size_t)(t - 1) * D + p];
            g += dlt / Q / Tn;                                      // transition prior
            g += -(a.kfu[bb + (t - 1)] / Q) / Tn;                   // -1/T * dl/ddelta_{t-1} (alpha Kf u)
        }
        if (t < T) {
            const double dlt = Xs[(size_t)(t + 1) * D + p] - Xs[(size_t)t * D + p];
            g -= dlt / Q / Tn;
            g -= -(a.kfu[bb + t] / Q) / Tn;
        }
    }
    // through the GP inputs x_comb[t][p] (rows t < T), summed over the local dims
    if (t < T) {
        double acc = 0.0;
        for (int dl = 0; dl < a.Dl; ++dl) {
            const size_t bb = (size_t)s * a.Dl + dl;
            if (a.kind != 0) {
                // LinearK: d K_fu / d x = s2 z, and Kdiag_t = s2 |x_t|^2 sits in the trace term: -1/2 alpha (Kdiag_t - |F_t|^2)
                const double s2 = a.variance[dl], alpha = 1.0 / exp(a.log_Q[a.d_begin + dl]);
                acc += s2 * a.ez[(bb * a.Tp + t) * a.P + p] - alpha * s2 * Xs[(size_t)t * D + p];
                continue;
            }
            const double l = a.len[(size_t)dl * a.P + p];
            acc += -(Xs[(size_t)t * D + p] * a.rsum[bb * a.Tp + t] - a.ez[(bb * a.Tp + t) * a.P + p]) / (l * l);
        }
        g += -acc / Tn;
    }
    a.dX[idx] = g / (double)a.S_total;
}
void launch_dx(hipStream_t stream, const DxArgs &a) {
    const size_t n = (size_t)a.S * (a.T + 1) * a.D;
    hipLaunchKernelGGL(dx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
}

// ---------------------------------------------------------------------------------------------
// Per-chain partial sums of the likelihood / transition-prior gradients w.r.t. the shared parameters:
//   out[s][0 : D*Ydim] dCC, [.. + Ydim] dDD, [.. + Ydim] dlogR(row 0), [.. + D] dlogQ (transition part)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void shared_partials_kernel(DxArgs a, double *out, int stride) {
    __shared__ double scratch[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int T = a.T, D = a.D, J = a.Ydim;
    const double Tn = (double)(a.T_norm > 0 ? a.T_norm : T);
    const double *Xs = a.X + (size_t)s * (T + 1) * D;
    double *o = out + (size_t)s * stride;
    for (int j = 0; j < J; ++j) {
        const double R = exp(a.log_Rchols[j]);
        double dd = 0.0, dr = 0.0;
        for (int d = 0; d < D; ++d) {
            double dc = 0.0;
            for (int t = tid; t < T; t += 256) {
                double ym = a.DD[j];
                for (int e = 0; e < D; ++e) ym += Xs[(size_t)(t + 1) * D + e] * a.CC[(size_t)e * J + j];
                const double r = (a.Y[(size_t)t * J + j] - ym) / R;
                dc += (r / R) * Xs[(size_t)(t + 1) * D + d];
                if (d == 0) { dd += r / R; dr += r * r - 1.0; }
            }
            dc = block_sum(dc, scratch);
            if (tid == 0) o[d * J + j] = -dc / Tn;
        }
        dd = block_sum(dd, scratch);
        dr = block_sum(dr, scratch);
        if (tid == 0) { o[D * J + j] = -dd / Tn; o[D * J + J + j] = -dr / Tn; }
    }
    for (int dl = 0; dl < a.Dl; ++dl) {
        const int d = a.d_begin + dl;
        const double Q = exp(a.log_Q[d]);
        double acc = 0.0;
        for (int t = tid; t < T; t += 256) {
            const double dlt = Xs[(size_t)(t + 1) * D + d] - Xs[(size_t)t * D + d];
            acc += 0.5 - 0.5 * dlt * dlt / Q;
        }
        acc = block_sum(acc, scratch);
        if (tid == 0) o[D * J + 2 * J + dl] = acc / Tn;
    }
}
void launch_shared_partials(hipStream_t stream, const DxArgs &a, double *out, int stride) {
    hipLaunchKernelGGL(shared_partials_kernel, dim3(a.S), dim3(256), 0, stream, a, out, stride);
}

// ---------------------------------------------------------------------------------------------
// Final assembly of the shared-parameter gradients (one workgroup; fixed summation order).
// ---------------------------------------------------------------------------------------------
// One workgroup per local latent dim; every sum over the chains is a strided per-thread partial followed by one
// multi-value workgroup reduction (a single thread walking S x (ngam + ntr) dependent loads took 0.12 ms).
__global__ __launch_bounds__(256) void grad_finalize_kernel(GradFinalArgs a) {
    __shared__ double scratch[4][8];
    const int tid = threadIdx.x, dl = blockIdx.x, dg = a.d_begin + dl;
    const int D = a.D, P = a.P, J = a.Ydim, Dl = a.Dl, S = a.S;
    const double Tloc = (double)a.T, Tn = (double)(a.T_norm > 0 ? a.T_norm : a.T), Sn = (double)a.S_total;
    const double rep = a.replicated_skip ? 0.0 : 1.0;      // T-shards: terms every shard computes identically count on the first only
    // prior gradients are weighted by this handle's share of the chains, so that the sum over chain shards
    // (and over dim shards, where S == S_total and every dim has one owner) is the whole-job gradient
    const double w = rep * (double)S / Sn;
    // loglengthscales of this dim, eight components at a time
    for (int p0 = 0; p0 < P; p0 += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0.0;
        for (int s = tid; s < S; s += 256) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (p0 + q < P) v[q] += a.dll_unit[(size_t)(s * Dl + dl) * P + p0 + q];
        }
        block_sum_multi_256<8>(v, scratch);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (tid == q && p0 + q < P) {
                const int p = p0 + q;
                const double acc = v[q] + rep * a.dll_kuu[(size_t)dl * P + p];
                // LinearK has no lengthscales: neither a data term nor the prior_hyper term (dgp_model.py:123-130)
                a.dloglen[(size_t)dg * P + p] = (a.kind != 0) ? 0.0 : -acc / Tn / Sn + w * a.loglen[(size_t)dg * P + p] / Tn;
            }
    }
    // logvariance, log_Q
    {
        const double alpha = 1.0 / exp(a.log_Q[dg]), s2 = exp(a.logvar[dg]);
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0.0;
        for (int s = tid; s < S; s += 256) {
            const size_t bb = (size_t)s * Dl + dl;
            // K_fu side + direct Kdiag term (SE: Kdiag = s2; LinearK: Kdiag_t = s2 |x_t|^2)
            v[0] += a.dls_unit[bb] - 0.5 * alpha * s2 * ((a.kind != 0) ? a.xsq_unit[bb] : Tloc);
            if (a.branch_a) {                                        // explicit U: dl/dalpha comes per unit from resid_a
                v[1] += a.dalpha_unit[bb] * (-alpha);
                continue;
            }
            // dl/dalpha = -1/2 tr(A^-1 G) + u^T g - 1/2 u^T G u - 1/2 (sum_t Kdiag_t - tr(K^-1 G)),  G = (A - K)/alpha;  sum_t Kdiag_t = T s2 (SE), s2 sum_t |x_t|^2 (LinearK)
            double trAK = 0.0;
            for (int t = 0; t < a.ngam; ++t) trAK += a.gam_part[bb * a.ngam + t];
            double fsq = 0.0;
            for (int t = 0; t < a.ntr; ++t) fsq += a.trpart[bb * a.ntr + t];
            const double quad = a.hterms[2 * bb + 1];
            const double trAinvG = ((double)a.Mp - trAK) / alpha;
            const double uGu = (quad - a.uku[bb]) / alpha;
            const double kdsum = ((a.kind != 0) ? a.xsq_unit[bb] : Tloc) * s2;      // sum_t Kdiag_t over THIS handle's rows
            // (T-shards: tr(A^-1 G), u^T g, u^T G u and tr(K^-1 G) are the job's -- the same on every shard, counted on the first;
            //  sum_t Kdiag_t is this shard's share.  Otherwise the expression as it always was.)
            const double dalpha = (a.T_norm > 0) ? rep * (-0.5 * trAinvG + quad / alpha - 0.5 * uGu + 0.5 * fsq) - 0.5 * kdsum
                                                 : -0.5 * trAinvG + quad / alpha - 0.5 * uGu - 0.5 * (kdsum - fsq);
            v[1] += dalpha * (-alpha);
            v[2] += a.shared_part[(size_t)s * a.sp_stride + D * J + 2 * J + dl];
        }
        block_sum_multi_256<8>(v, scratch);
        if (tid == 0) {
            const double ls = v[0] + rep * a.dls_kuu[dl];
            a.dlogvar[dg] = -ls / Tn / Sn + w * (a.logvar[dg] - (a.kind == 0 ? LOG_PRIOR_VARIANCE_SE : LOG_PRIOR_VARIANCE_LIN)) / Tn;
            a.dlogQ[dg] = -v[1] / Tn / Sn + (a.branch_a ? 0.0 : v[2] / Sn) + w * a.log_Q[dg] / Tn;
        }
    }
    if (a.shared_terms && dl == 0) {
        // C, d and row 0 of log_Rchols: D J + J + J per-chain partials, eight at a time
        const int nitem = D * J + 2 * J;
        for (int i0 = 0; i0 < nitem; i0 += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = 0.0;
            for (int s = tid; s < S; s += 256) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (i0 + q < nitem) v[q] += a.shared_part[(size_t)s * a.sp_stride + i0 + q];
            }
            block_sum_multi_256<8>(v, scratch);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (tid == q && i0 + q < nitem) {
                    const int idx = i0 + q;
                    const double acc = v[q] / Sn;
                    if (idx < D * J) a.dCC[idx] = acc + w * a.CC[idx] / Tn;
                    else if (idx < D * J + J) a.dDD[idx - D * J] = acc + w * a.DD[idx - D * J] / Tn;
                    else a.dlogR[idx - D * J - J] = acc + w * a.log_Rchols[idx - D * J - J] / Tn;
                }
        }
        for (int idx = J + tid; idx < J * J; idx += 256)       // only row 0 of log_Rchols enters the likelihood
            a.dlogR[idx] = w * a.log_Rchols[idx] / Tn;
    }
}
// explicit-U branch: dU[m][d] = -(alpha_d (W^T g_r)[m]) / T / S_total + (S / S_total) U[m][d] / T   (prior_U, choice 1)
__global__ void grad_du_kernel(GradFinalArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.M * a.D) return;
    const int m = idx / a.D, d = idx % a.D, dl = d - a.d_begin;
    double g = 0.0;
    if (dl >= 0 && dl < a.Dl) {
        const double alpha = 1.0 / exp(a.log_Q[d]);
        g = -(alpha * a.du_dim[(size_t)dl * a.Mp + m]) / (double)a.T / (double)a.S_total
            + ((double)a.S / (double)a.S_total) * a.U[idx] / (double)a.T;
    }
    a.dU[idx] = g;
}
// dZ[m][p]: fixed-order sum over units of the K_fu-side parts (scaled -1/T, mean over chains) + K_uu side + prior
__global__ __launch_bounds__(256) void grad_dz_kernel(GradFinalArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int M = a.M, P = a.P, Dl = a.Dl, S = a.S;
    if (idx >= M * P) return;
    const double Tn = (double)(a.T_norm > 0 ? a.T_norm : a.T), Sn = (double)a.S_total;
    const double rep = a.replicated_skip ? 0.0 : 1.0;
    double acc = 0.0;
    for (int s = 0; s < S; ++s)
        for (int dl = 0; dl < Dl; ++dl) acc += a.dz_unit[((size_t)(s * Dl + dl) * M * P) + idx];
    double kk = 0.0;
    for (int dl = 0; dl < Dl; ++dl) kk += a.dz_kuu[(size_t)dl * M * P + idx];
    double g = -(acc + rep * kk) / Tn / Sn;
    if (a.shared_terms && a.prior_type == 1) g += rep * ((double)S / Sn) * a.Z[idx] / Tn;
    a.dZ[idx] = g;
}
void launch_grad_finalize(hipStream_t stream, const GradFinalArgs &a) {
    hipLaunchKernelGGL(grad_dz_kernel, dim3((a.M * a.P + 255) / 256), dim3(256), 0, stream, a);
    if (a.branch_a && a.dU) hipLaunchKernelGGL(grad_du_kernel, dim3((a.M * a.D + 255) / 256), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(grad_finalize_kernel, dim3(a.Dl), dim3(256), 0, stream, a);
}

// ---------------------------------------------------------------------------------------------
// Explicit-U branch (dgp_model.py:289-297, conditional/base_conditional): small kernels of its backward pass.
// Closed form and notation: oracle/ffvd_grad_oracle.py nll_grad_explicit_u.
// ---------------------------------------------------------------------------------------------
// ucol[dl][m] = U[m][d_begin + dl]  (zero padded to Mp)
__global__ void ucols_kernel(const double *U, int M, int Mp, int D, int d_begin, double *ucol) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x, dl = blockIdx.y;
    if (m < Mp) ucol[(size_t)dl * Mp + m] = (m < M) ? U[(size_t)m * D + d_begin + dl] : 0.0;
}
void launch_ucols(hipStream_t stream, const double *U, int M, int Mp, int D, int d_begin, int Dl, double *ucol) {
    hipLaunchKernelGGL(ucols_kernel, dim3((Mp + 255) / 256, Dl), dim3(256), 0, stream, U, M, Mp, D, d_begin, ucol);
}
// r[b][t] = delta_t - mean_t (0 for t >= T);  dalpha[b] = -1/2 sum r^2 - 1/2 sum_t (Kdiag_t - |F_t|^2) + T / (2 alpha);
// Kdiag_t = sigma^2 (SE) or sigma^2 |x_comb_t|^2 (LinearK, kernels.py:278-281), whose sum over t goes to xsq[b]
__global__ __launch_bounds__(256) void resid_a_kernel(int kind, const double *X, const double *ctrl, int C, const double *fmean,
                                                      const double *rowsq, const double *variance, const double *log_Q, int T,
                                                      int Tp, int D, int Dl, int d_begin, int ng, double *r,
                                                      double *dalpha_unit, double *xsq_unit) {
    __shared__ double scratch[256];
    const int b = blockIdx.x, tid = threadIdx.x, s = b / Dl, dl = b % Dl, dg = d_begin + dl;
    const double *Xs = X + (size_t)s * (T + 1) * D;
    const double s2 = variance[dl];
    double sr = 0.0, sv = 0.0, sx = 0.0;
    for (int t = tid; t < Tp; t += 256) {
        double rt = 0.0;
        if (t < T) {
            double fm = 0.0, rs = 0.0;
            for (int g = 0; g < ng; ++g) {
                fm += fmean[((size_t)b * ng + g) * Tp + t];
                rs += rowsq[((size_t)b * ng + g) * Tp + t];
            }
            rt = (Xs[(size_t)(t + 1) * D + dg] - Xs[(size_t)t * D + dg]) - fm;
            sr += rt * rt;
            double kd = s2;
            if (kind != 0) {
                double xsq = 0.0;
                for (int p = 0; p < D; ++p) xsq += Xs[(size_t)t * D + p] * Xs[(size_t)t * D + p];
                for (int p = 0; p < C; ++p) xsq += ctrl[(size_t)t * C + p] * ctrl[(size_t)t * C + p];
                sx += xsq;
                kd = xsq * s2;
            }
            sv += kd - rs;
        }
        r[(size_t)b * Tp + t] = rt;
    }
    sr = block_sum(sr, scratch);
    sv = block_sum(sv, scratch);
    sx = block_sum(sx, scratch);
    if (tid == 0) {
        dalpha_unit[b] = -0.5 * sr - 0.5 * sv + 0.5 * (double)T * exp(log_Q[dg]);
        if (xsq_unit) xsq_unit[b] = sx;
    }
}
void launch_resid_a(hipStream_t stream, int kind, const double *X, const double *ctrl, int C, const double *fmean,
                    const double *rowsq, const double *variance, const double *log_Q, int T, int Tp, int D, int Dl, int d_begin,
                    int ng, int nb, double *r, double *dalpha_unit, double *xsq_unit) {
    hipLaunchKernelGGL(resid_a_kernel, dim3(nb), dim3(256), 0, stream, kind, X, ctrl, C, fmean, rowsq, variance, log_Q, T, Tp, D,
                       Dl, d_begin, ng, r, dalpha_unit, xsq_unit);
}
// out = 1/2 alpha_d K^-1   (plays the role of Gamma in the fused backward product)
__global__ void scale_kinv_kernel(const double *Kinv, const double *log_Q, int Mp, int d_begin, double *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int dl = blockIdx.y;
    const size_t o = (size_t)dl * Mp * Mp + idx;
    out[o] = 0.5 / exp(log_Q[d_begin + dl]) * Kinv[o];
}
void launch_scale_kinv(hipStream_t stream, const double *Kinv, const double *log_Q, int Mp, int Dl, int d_begin, double *out) {
    hipLaunchKernelGGL(scale_kinv_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, Kinv,
                       log_Q, Mp, d_begin, out);
}
// dW[k][j] = alpha (g_r[k] u[j] + (G W)[k][j])
__global__ void dw_a_kernel(const double *T1, const double *grs, size_t grs_stride, const double *ucol, const double *log_Q,
                            int Mp, int d_begin, double *dW) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int dl = blockIdx.y, k = (int)(idx / Mp), j = (int)(idx % Mp);
    const double alpha = 1.0 / exp(log_Q[d_begin + dl]);
    const size_t o = (size_t)dl * Mp * Mp + idx;
    dW[o] = alpha * (grs[(size_t)dl * grs_stride + k] * ucol[(size_t)dl * Mp + j] + T1[o]);
}
void launch_dw_a(hipStream_t stream, const double *T1, const double *grs, size_t grs_stride, const double *ucol,
                 const double *log_Q, int Mp, int Dl, int d_begin, double *dW) {
    hipLaunchKernelGGL(dw_a_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, T1, grs,
                       grs_stride, ucol, log_Q, Mp, d_begin, dW);
}
// out = -tril(P)
__global__ void tril_neg_kernel(const double *P, int Mp, double *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    const size_t o = (size_t)blockIdx.y * Mp * Mp + idx;
    out[o] = (j <= i) ? -P[o] : 0.0;
}
void launch_tril_neg(hipStream_t stream, const double *P, int Mp, int Dl, double *out) {
    hipLaunchKernelGGL(tril_neg_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, P, Mp, out);
}
// out = tril(L) from the factor slab (whose upper triangle holds don't-care values)
__global__ void tril_copy_kernel(const double *L, size_t l_stride, int Mp, double *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    out[(size_t)blockIdx.y * Mp * Mp + idx] = (j <= i) ? L[(size_t)blockIdx.y * l_stride + idx] : 0.0;
}
void launch_tril_copy(hipStream_t stream, const double *L, size_t l_stride, int Mp, int Dl, double *out) {
    hipLaunchKernelGGL(tril_copy_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, L,
                       l_stride, Mp, out);
}
// Phi = sym(tril(S) with the diagonal halved)   (Cholesky adjoint)
__global__ void phi_kernel(const double *S, int Mp, double *Phi) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    const double *Sd = S + (size_t)blockIdx.y * Mp * Mp;
    const double lo = (i >= j) ? Sd[(size_t)i * Mp + j] : Sd[(size_t)j * Mp + i];      // tril entry of the pair (i, j)
    Phi[(size_t)blockIdx.y * Mp * Mp + idx] = 0.5 * lo;       // off-diagonal: (t_ij + 0)/2; diagonal: (s_ii/2 + s_ii/2)/2
}
void launch_phi(hipStream_t stream, const double *S, int Mp, int Dl, double *Phi) {
    hipLaunchKernelGGL(phi_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, S, Mp, Phi);
}
// E = dK o K_uu (without the jitter on the diagonal; SE chain rule) or dK itself (LinearK), zero in the padding
__global__ void epsi_a_kernel(int kind, const double *dK, const double *Kcopy, int M, int Mp, double jitter, double *E) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Mp * Mp) return;
    const int i = (int)(idx / Mp), j = (int)(idx % Mp);
    const size_t o = (size_t)blockIdx.y * Mp * Mp + idx;
    const double k = (kind != 0) ? 1.0 : Kcopy[o] - ((i == j) ? jitter : 0.0);
    E[o] = (i < M && j < M) ? dK[o] * k : 0.0;
}
void launch_epsi_a(hipStream_t stream, int kind, const double *dK, const double *Kcopy, int M, int Mp, int Dl, double jitter,
                   double *E) {
    hipLaunchKernelGGL(epsi_a_kernel, dim3((unsigned)(((size_t)Mp * Mp + 255) / 256), Dl), dim3(256), 0, stream, kind, dK, Kcopy,
                       M, Mp, jitter, E);
}

}  // namespace ffvd
