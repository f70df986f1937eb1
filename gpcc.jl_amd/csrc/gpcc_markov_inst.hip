// gpcc_markov_inst.hip -- the instantiations of gpcc_markov_eval<P, NOFF> that ship (GpccMkShipsAll of gpcc_markov.hip.h) and their
// launch, as an object of their own (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov.hip.h"

hipError_t gpcc_markov_launch(const GpccMkLaunch &g, const GpccMarkovArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsAll>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_eval<P(), NOFF()>, g, 1, a);
    });
}
