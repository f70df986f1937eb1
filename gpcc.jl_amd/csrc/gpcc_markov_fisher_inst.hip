// gpcc_markov_fisher_inst.hip -- the instantiations of gpcc_markov_fisher<P, NOFF> that ship (GpccMkShipsFisher of gpcc_markov_fisher.hip.h;
// each holds the eight bodies of the kinds of pair) for one P = GPCC_INST_P, and their launch; with P = 1 also the finish kernel and
// the launch of the family, which picks the object: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_fisher.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_fisher<P, g.noff> on the grid (g.blocks, slots): each object defines its own P's
template <int P>
hipError_t gpcc_markov_fisher_launch_p(const GpccMkLaunch &g, int slots, const GpccMarkovFisherArgs &a);

template <>
hipError_t gpcc_markov_fisher_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int slots, const GpccMarkovFisherArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsFisher, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_fisher<P(), NOFF()>, g, slots, a);
    });
}

#if GPCC_INST_P == 1
// the M blocks: every pair from its slot to both halves; NaN blocks where info != 0 (a slot of a pair with a tau already holds NaN
// on an OU row with a tie)
static __global__ void __launch_bounds__(64) gpcc_markov_fisher_finish(const GpccMarkovFisherArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int W = 2 * a.L + 1;
    const bool bad = a.out_info[m] != 0;
    const double nan = __builtin_nan("");
    double *F = a.fisher + m * W * W;
    int slot = 0;
    for (int i = 0; i < W; ++i)
        for (int k = i; k < W; ++k, ++slot) F[i * W + k] = F[k * W + i] = bad ? nan : a.slot[(long)slot * a.M + m];
}

template <> hipError_t gpcc_markov_fisher_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovFisherArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_fisher_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovFisherArgs &);

hipError_t gpcc_markov_fisher_launch(const GpccMkLaunch &g, int slots, const GpccMarkovFisherArgs &a)
{
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsFisher>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_fisher_launch_p<P()>(g, slots, a); });
    if (e != hipSuccess) return e;
    gpcc_markov_fisher_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, g.s>>>(a);
    return hipGetLastError();
}
#endif
