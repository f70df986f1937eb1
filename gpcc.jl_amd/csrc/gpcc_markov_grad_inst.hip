// gpcc_markov_grad_inst.hip -- the instantiations of gpcc_markov_grad<P, NOFF> that ship (GpccMkShipsAll of gpcc_markov.hip.h; each
// holds the alpha, rho and tau bodies), the finish kernel and their launch, as an object of their own (gpcc.jl_amd/build.py compiles
// the objects side by side).
#include "gpcc_markov_grad.hip.h"

// the M x (2L + 1) rows from the slots: the tau pairs of OU averaged (first + last, in this order), NaN rows where info != 0
static __global__ void __launch_bounds__(64) gpcc_markov_grad_finish(const GpccMarkovGradArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int L = a.L, W = 2 * L + 1;
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
}

hipError_t gpcc_markov_grad_finish_launch(hipStream_t s, const GpccMarkovGradArgs &a)
{
    gpcc_markov_grad_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t gpcc_markov_grad_launch(const GpccMkLaunch &g, int slots, const GpccMarkovGradArgs &a)
{
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsAll>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_grad<P(), NOFF()>, g, slots, a);
    });
    return e != hipSuccess ? e : gpcc_markov_grad_finish_launch(g.s, a);
}
