// Seeded draws of the particle calls, generated where they are consumed ("Device draws").  The generator is
// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011), written out here: ten rounds of
//   c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   then  k += (W0, W1)
// with M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85 (the bump after the tenth round is formed and not used).
//
// Addressing: the key is the two words of the caller's 64-bit seed; the counter of a block of four words is (p, g, r, stream): p the
// pair of consecutive elements 2p, 2p + 1 inside the block of one track, (g, r) the group and the record of the block -- 0 where the
// noise mode shares the axis -- and stream 0 eps, 1 unif, 2 xi0, 3 unif_bs.  So an element is a pure function of (seed, stream, g, r,
// index in the block): it does not depend on G, R, steps, the order of the passes or records_per_pass, and the draws of a shorter
// call are a prefix of a longer one's.
//
// From the four words w0..w3: k1 = (w0 >> 5) 2^26 + (w1 >> 6), k2 = (w2 >> 5) 2^26 + (w3 >> 6), both below 2^53, so every product
// with 2^-53 below is exact.
//   uniform streams:  k1 2^-53 and k2 2^-53, in [0, 1)
//   normal streams:   u1 = (k1 + 1) 2^-53 in (0, 1], u2 = k2 2^-53, rho = sqrt(-2 ln u1); rho cospi(2 u2) and rho sinpi(2 u2): 2 u2 is
//                     exact and the argument of the circular functions is never rounded; always finite, |z| <= sqrt(106 ln 2) < 8.58
//
// Kernel (256 threads): thread = pair, workgroup = (chunk of 256 pairs, block), blockIdx.x = block * chunks + chunk.  The pair goes
// out in one 16-byte store where the block's base is 16-byte aligned -- uniform over the workgroup, the offset of a pair being
// even -- and in two 8-byte stores otherwise; the last element of an odd block alone.  No LDS, no atomics, vector stores only.
#include "moment_particle_draws.h"

namespace ffvd {
namespace {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
        const unsigned hi1 = __umulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
}

__global__ __launch_bounds__(256) void mg_pdraw_fill_kernel(MomentParticleDrawsArgs a) {
    const int pairs = (a.len + 1) / 2, chunks = (pairs + 255) / 256;
    const int blk = blockIdx.x / chunks, p = (blockIdx.x % chunks) * 256 + threadIdx.x;
    if (p >= pairs) return;
    const int g = blk / a.Rb, r = blk % a.Rb;
    unsigned c[4] = {(unsigned)p, (unsigned)g, (unsigned)r, (unsigned)a.stream};
    philox4x32_10(c, a.key0, a.key1);
    const unsigned long long k1 = ((unsigned long long)(c[0] >> 5) << 26) + (c[1] >> 6);
    const unsigned long long k2 = ((unsigned long long)(c[2] >> 5) << 26) + (c[3] >> 6);
    constexpr double TWO_M53 = 1.0 / 9007199254740992.0;
    double e0, e1;
    if (a.normal) {
        const double u1 = (double)(k1 + 1) * TWO_M53, u2 = (double)k2 * TWO_M53;
        const double rho = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincospi(2.0 * u2, &sn, &cs);
        e0 = rho * cs;
        e1 = rho * sn;
    } else {
        e0 = (double)k1 * TWO_M53;
        e1 = (double)k2 * TWO_M53;
    }
    double *dst = a.out + (size_t)g * a.stride_g + (size_t)r * a.stride_r + 2 * (size_t)p;
    if (2 * p + 1 >= a.len) dst[0] = e0;
    else if (((size_t)dst & 15) == 0) *reinterpret_cast<double2 *>(dst) = make_double2(e0, e1);
    else {
        dst[0] = e0;
        dst[1] = e1;
    }
}

}  // namespace

bool launch_mg_pdraw_fill(hipStream_t stream, const MomentParticleDrawsArgs &a) {
    const long long chunks = ((long long)(a.len + 1) / 2 + 255) / 256, grid = chunks * a.Gb * a.Rb;
    if (a.len < 1 || a.Gb < 1 || a.Rb < 1 || grid >= (1LL << 31)) return false;
    hipLaunchKernelGGL(mg_pdraw_fill_kernel, dim3((unsigned)grid), dim3(256), 0, stream, a);
    return true;
}

}  // namespace ffvd
