// Rolling-origin multi-step forecasts from the filtered states ("Rolling-origin forecasts"): the step kernel of
// the moment-matched prediction (moment_step.h) instantiated with a TRACK as its unit of work.  A track is a (group, origin) pair: it
// borrows beta, Gamma, the hyper-parameters and log_Q of its group and takes its start state and its control rows from its origin
// (moment_group.h, MomentFanArgs).  Workgroup (track, pair a <= b, slab s); the expressions on the values, every sum order and the
// final reductions are those of the propagation, so a track is bit-identical to the propagation started from the same filtered state.
// A third translation unit: the code of the propagation and of the filter does not change with this one.
#include "moment_step.h"

namespace ffvd {

int mg_fan_tracks_per_pass(int G, int D, int NS, int B) {
    const long long per = (long long)G * mg_npair(D) * NS, words = 2LL * G * mg_fields(D) * NS;
    long long bp = ((1LL << 31) - 1) / per;
    if (MG_FAN_PART_DOUBLES / words < bp) bp = MG_FAN_PART_DOUBLES / words;
    return (int)(bp < 1 ? 1 : bp > B ? B : bp);
}

// a.G: the tracks of the pass (groups * f.Bp)
void launch_mg_fan_step(hipStream_t stream, const MomentGroupArgs &a, const MomentFanArgs &f, int t) {
    const dim3 grid((unsigned)((size_t)a.G * mg_npair(a.D) * a.NS));
    MG_DISPATCH_D(a.D, hipLaunchKernelGGL(HIP_KERNEL_NAME(mg_step_kernel<d, false, MomentFanArgs>), grid, dim3(256), 0, stream, a, t, f))
}

}  // namespace ffvd
