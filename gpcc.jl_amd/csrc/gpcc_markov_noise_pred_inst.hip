// gpcc_markov_noise_pred_inst.hip -- the instantiations of gpcc_markov_noise_taps<P, NOFF, MODE>, gpcc_markov_noise_loo_taps<P, NOFF> and
// of gpcc_markov_loo_combine<P, NOFF> on the noise model's Args that ship (GpccMkShipsNoisePred of gpcc_markov_noise_pred.hip.h: none
// spills or uses scratch memory, profiles/markov/kernel_resources_noise_pred.log) and their launches, as an object of their own
// (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_noise_pred.hip.h"

hipError_t gpcc_mknp_launch_taps(const GpccMkLaunch &g, int mode, int ny, const GpccMarkovNoisePredArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsNoisePred>(g.p, g.noff, [&](auto P, auto NOFF) {
        return mode == GPCC_MKP_TAP ? gpcc_mk_launch_kernel(gpcc_markov_noise_taps<P(), NOFF(), GPCC_MKP_TAP>, g, ny, a)
                                    : gpcc_mk_launch_kernel(gpcc_markov_noise_taps<P(), NOFF(), GPCC_MKP_UPDATE>, g, ny, a);
    });
}

hipError_t gpcc_mknl_launch_taps(const GpccMkLaunch &g, const GpccMarkovNoiseLooArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsNoisePred>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_noise_loo_taps<P(), NOFF()>, g, 2, a);
    });
}

hipError_t gpcc_mknl_launch_combine(int p, int noff, const GpccMarkovNoiseLooCombineArgs &a, hipStream_t s)
{
    return gpcc_mk_dispatch<GpccMkShipsNoisePred>(p, noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_loo_combine<P(), NOFF(), GpccMarkovNoiseLooCombineArgs>, dim3(a.N, (a.rows + 63) / 64), 64,
                                     0, s, false, a);
    });
}
