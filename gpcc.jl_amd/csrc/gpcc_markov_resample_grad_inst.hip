// gpcc_markov_resample_grad_inst.hip -- the instantiations of gpcc_markov_resample_grad<P, NOFF> that ship (GpccMkShipsResampleGrad of
// gpcc_markov_resample_grad.hip.h) for one P = GPCC_INST_P, and their launch; with P = 1 also the launch of the family, which picks
// the object and runs gpcc_markov_grad's finish kernel: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_resample_grad.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_resample_grad<P, g.noff> on the grid (g.blocks, slots): each object defines its own P's
template <int P>
hipError_t gpcc_markov_resample_grad_launch_p(const GpccMkLaunch &g, int slots, const GpccMarkovResampleGradArgs &a);

template <>
hipError_t gpcc_markov_resample_grad_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int slots, const GpccMarkovResampleGradArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsResampleGrad, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_resample_grad<P(), NOFF()>, g, slots, a);
    });
}

#if GPCC_INST_P == 1
template <> hipError_t gpcc_markov_resample_grad_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovResampleGradArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_resample_grad_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovResampleGradArgs &);

hipError_t gpcc_markov_resample_grad_launch(const GpccMkLaunch &g, int slots, const GpccMarkovResampleGradArgs &a)
{
    if (slots < 1) return hipErrorInvalidValue;
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsResampleGrad>(g.p, g.noff, [&](auto P, auto) {
        return gpcc_markov_resample_grad_launch_p<P()>(g, slots, a);
    });
    return e != hipSuccess ? e : gpcc_markov_grad_finish_launch(g.s, a);
}
#endif
