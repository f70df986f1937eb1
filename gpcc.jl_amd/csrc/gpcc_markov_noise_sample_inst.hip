// gpcc_markov_noise_sample_inst.hip -- the instantiations of gpcc_markov_noise_draw<P, NOFF> that ship (GpccMkShipsNoiseSample of
// gpcc_markov_noise_sample.hip.h: none spills or uses scratch memory, profiles/markov/kernel_resources_noise_sample.log) and their
// launch, as an object of their own (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_noise_sample.hip.h"

hipError_t gpcc_mksn_launch_draw(const GpccMkLaunch &g, const GpccMarkovNoiseDrawArgs &a)
{
    if ((long)g.blocks * g.threads > a.lstride || a.lanes < 1 || a.lanes > a.lstride) return hipErrorInvalidValue;   // the scratch's columns
    return gpcc_mk_dispatch<GpccMkShipsNoiseSample>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_noise_draw<P(), NOFF()>, g, 1, a);
    });
}
