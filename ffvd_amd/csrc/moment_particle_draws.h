// Seeded draws of the particle calls, generated on the device (moment_particle_draws.hip; DESIGN.md section 9, "Device draws").  A header
// of its own: no other moment_* unit includes it, so none of them is rebuilt differently because of it.
#pragma once
#include <hip/hip_runtime.h>

namespace ffvd {

// the streams of a seed: word 3 of the Philox counter
constexpr int MG_PDRAW_EPS = 0, MG_PDRAW_UNIF = 1, MG_PDRAW_XI0 = 2, MG_PDRAW_UNIF_BS = 3;
// the noise modes: which of (group, record) a block depends on
constexpr int MG_PDRAW_SHARED = 0, MG_PDRAW_PER_RECORD = 1, MG_PDRAW_INDEPENDENT = 2;

// One stream of a call: block (g, r), g < Gb, r < Rb, of `len` doubles at out + g * stride_g + r * stride_r; its counter words are
// (pair, g, r, stream) -- Gb = 1 (Rb = 1) where the mode shares the axis, so that the word is 0 there.
// Limits: 1 <= len < 2^31; ceil(len / 512) * Gb * Rb < 2^31 (grid x).  Every double of the Gb * Rb blocks is written, nothing else.
struct MomentParticleDrawsArgs {
    unsigned key0, key1;             // the low and the high word of the seed
    int stream, normal;              // MG_PDRAW_*; 1: Box-Muller pairs, 0: uniforms in [0, 1)
    int Gb, Rb, len;
    long long stride_g, stride_r;
    double *out;
};
// false: the grid does not fit (ceil(len / 2 / 256) * Gb * Rb >= 2^31); nothing is launched
bool launch_mg_pdraw_fill(hipStream_t stream, const MomentParticleDrawsArgs &a);

}  // namespace ffvd
