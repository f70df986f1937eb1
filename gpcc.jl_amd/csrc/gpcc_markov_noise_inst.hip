// gpcc_markov_noise_inst.hip -- the instantiations of gpcc_markov_noise_eval<P, NOFF> and gpcc_markov_noise_grad<P, NOFF> that ship
// (GpccMkShipsNoise of gpcc_markov_noise.hip.h) for one P = GPCC_INST_P, and their launch; with P = 1 also the finish kernel and the
// launches of the family, which pick the object: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_noise.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_noise_eval<P, g.noff> (slots == 0) or gpcc_markov_noise_grad<P, g.noff> on the grid (g.blocks, slots): each object
// defines its own P's
template <int P>
hipError_t gpcc_markov_noise_launch_p(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseArgs &a);

template <>
hipError_t gpcc_markov_noise_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsNoise, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        if (slots == 0) return gpcc_mk_launch_kernel(gpcc_markov_noise_eval<P(), NOFF()>, g, 1, a);
        return gpcc_mk_launch_kernel(gpcc_markov_noise_grad<P(), NOFF()>, g, slots, a);
    });
}

#if GPCC_INST_P == 1
// the M x (4L + 1) rows from the slots: [alpha_1..L, rho, tau_1..L, kappa_1..L, nu_1..L], the tau pairs of OU averaged (first + last,
// in this order), NaN rows where info != 0
static __global__ void __launch_bounds__(64) gpcc_markov_noise_grad_finish(const GpccMarkovNoiseArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int L = a.L, W = 4 * L + 1, ntau = a.twice ? 2 * L : L;
    const bool bad = a.out_info[m] != 0;
    double *g = a.grad + m * W;
    for (int c = 0; c <= L; ++c) g[c] = bad ? __builtin_nan("") : a.slot[(long)c * a.M + m];
    for (int l = 0; l < L; ++l) {
        double v;
        if (a.twice)
            v = 0.5 * (a.slot[(long)(L + 1 + 2 * l) * a.M + m] + a.slot[(long)(L + 2 + 2 * l) * a.M + m]);
        else
            v = a.slot[(long)(L + 1 + l) * a.M + m];
        g[L + 1 + l] = bad ? __builtin_nan("") : v;
    }
    for (int c = 0; c < 2 * L; ++c) g[2 * L + 1 + c] = bad ? __builtin_nan("") : a.slot[(long)(L + 1 + ntau + c) * a.M + m];
}

template <> hipError_t gpcc_markov_noise_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovNoiseArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_noise_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovNoiseArgs &);

hipError_t gpcc_markov_noise_launch(const GpccMkLaunch &g, const GpccMarkovNoiseArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsNoise>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_noise_launch_p<P()>(g, 0, a); });
}

hipError_t gpcc_markov_noise_grad_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseArgs &a)
{
    if (slots < 1) return hipErrorInvalidValue;
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsNoise>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_noise_launch_p<P()>(g, slots, a); });
    if (e != hipSuccess) return e;
    gpcc_markov_noise_grad_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, g.s>>>(a);
    return hipGetLastError();
}
#endif
