// gpcc_markov_noise_hess_inst.hip -- the instantiations of gpcc_markov_noise_hess<P, NOFF> that ship (GpccMkShipsNoiseHess of
// gpcc_markov_noise_hess.hip.h; each holds the eight bodies of the kinds of pair) for one P = GPCC_INST_P, and their launch; with P = 1
// also the finish kernel and the launch of the family, which picks the object: three objects (gpcc.jl_amd/build.py compiles the objects
// side by side).
#include "gpcc_markov_noise_hess.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_noise_hess<P, g.noff> on the grid (g.blocks, slots): each object defines its own P's
template <int P>
hipError_t gpcc_markov_noise_hess_launch_p(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessArgs &a);

template <>
hipError_t gpcc_markov_noise_hess_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsNoiseHess, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_noise_hess<P(), NOFF()>, g, slots, a);
    });
}

#if GPCC_INST_P == 1
// the M blocks from the slots: every pair (a, b), a <= b, to both halves of its row's block; NaN blocks where info != 0
static __global__ void __launch_bounds__(64) gpcc_markov_noise_hess_finish(const GpccMarkovNoiseHessArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int n = 3 * a.L + 1;
    const bool bad = a.out_info[m] != 0;
    double *H = a.hess + m * n * n;
    int slot = 0;
    for (int i = 0; i < n; ++i)
        for (int k = i; k < n; ++k, ++slot) H[i * n + k] = H[k * n + i] = bad ? __builtin_nan("") : a.slot[(long)slot * a.M + m];
}

template <> hipError_t gpcc_markov_noise_hess_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovNoiseHessArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_noise_hess_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovNoiseHessArgs &);

hipError_t gpcc_markov_noise_hess_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessArgs &a)
{
    if (slots != gpcc_markov_noise_hess_slots(a.L)) return hipErrorInvalidValue;
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsNoiseHess>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_noise_hess_launch_p<P()>(g, slots, a); });
    if (e != hipSuccess) return e;
    gpcc_markov_noise_hess_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, g.s>>>(a);
    return hipGetLastError();
}
#endif
