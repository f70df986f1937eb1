// gpcc_markov_multi_inst.hip -- the instantiations of gpcc_markov_multi<P, NOFF, RB> that ship (GpccMkShipsMulti of
// gpcc_markov_multi.hip.h) for one P = GPCC_INST_P, and their launch; with P = 1 also the pack kernel's launch and the launch of the
// family, which picks the object: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_multi.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_multi<P, g.noff, rb> on the grid (g.blocks, blocks): each object defines its own P's
template <int P>
hipError_t gpcc_markov_multi_launch_p(const GpccMkLaunch &g, int blocks, const GpccMarkovMultiArgs &a);

template <>
hipError_t gpcc_markov_multi_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int blocks, const GpccMarkovMultiArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsMulti, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_multi<P(), NOFF(), GpccMkShipsMulti::rb(P(), NOFF())>, g, blocks, a);
    });
}

#if GPCC_INST_P == 1
// one thread per (sorted point i, block): gathers through perm, subtracts the band's mean, writes the RB residuals of the point
static __global__ void __launch_bounds__(256) gpcc_markov_multi_pack(const GpccMarkovMultiPackArgs a)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int blk = blockIdx.y;
    if (i >= a.N || blk >= a.blocks) return;
    int band = 0;
    for (int l = 1; l < a.L; ++l) band = (i >= a.off[l]) ? l : band;
    const long src = a.perm[i];
    double *dst = a.res + ((long)blk * a.N + i) * a.rb;
    for (int k = 0; k < a.rb; ++k) {
        const long r = min((long)blk * a.rb + k, (long)a.R - 1);   // (the tail: copies of the last realisation)
        const double v = a.Y[r * a.N + src] - a.mean[r * a.L + band];
        dst[k] = (v - v == 0.0) ? v : __builtin_nan("");           // not finite: NaN, so that the column is NaN and not -inf
    }
}

template <> hipError_t gpcc_markov_multi_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovMultiArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_multi_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovMultiArgs &);

hipError_t gpcc_markov_multi_launch(const GpccMkLaunch &g, int blocks, const GpccMarkovMultiArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsMulti>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_multi_launch_p<P()>(g, blocks, a); });
}

hipError_t gpcc_markov_multi_pack_launch(const GpccMarkovMultiPackArgs &a, hipStream_t s)
{
    return gpcc_mk_launch_kernel(gpcc_markov_multi_pack, dim3((a.N + 255) / 256, a.blocks), 256, 0, s, false, a);
}
#endif
