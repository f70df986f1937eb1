// gpcc_markov_resample_inst.hip -- the instantiations of gpcc_markov_resample<P, NOFF> that ship (GpccMkShipsResample of
// gpcc_markov_resample.hip.h) for one P = GPCC_INST_P, and their launch; with P = 1 also the pack kernel, its launch and the launch of
// the family, which picks the object: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_resample.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_resample<P, g.noff> on the grid (g.blocks): each object defines its own P's
template <int P>
hipError_t gpcc_markov_resample_launch_p(const GpccMkLaunch &g, const GpccMarkovResampleArgs &a);

template <>
hipError_t gpcc_markov_resample_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, const GpccMarkovResampleArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsResample, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_resample<P(), NOFF()>, g, 1, a);
    });
}

#if GPCC_INST_P == 1
// one thread per (realisation r, sorted point i): gathers through perm, subtracts the band's mean, divides the variance by the
// multiplicity; a point that is not drawn gets the marker, a negative variance
static __global__ void __launch_bounds__(256) gpcc_markov_resample_pack(const GpccMarkovResamplePackArgs a)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const long r = idx / a.N, i = idx - r * a.N;
    int band = 0;
    for (int l = 1; l < a.L; ++l) band = (i >= a.off[l]) ? l : band;
    const long src = r * a.N + a.perm[i];
    const int n = a.count ? a.count[src] : 1;
    double2 o = {0.0, -1.0};
    if (n > 0) {
        const double v = a.Y[src] - a.mean[r * a.L + band];
        o.x = (v - v == 0.0) ? v : __builtin_nan("");   // not finite: NaN, so that the rows of this realisation are NaN and not -inf
        o.y = a.sig2[i] / (double)n;
    }
    a.rv[idx] = o;
}

template <> hipError_t gpcc_markov_resample_launch_p<2>(const GpccMkLaunch &, const GpccMarkovResampleArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_resample_launch_p<3>(const GpccMkLaunch &, const GpccMarkovResampleArgs &);

hipError_t gpcc_markov_resample_launch(const GpccMkLaunch &g, const GpccMarkovResampleArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsResample>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_resample_launch_p<P()>(g, a); });
}

hipError_t gpcc_markov_resample_pack_launch(const GpccMarkovResamplePackArgs &a, hipStream_t s)
{
    return gpcc_mk_launch_kernel(gpcc_markov_resample_pack, dim3((unsigned)((a.total + 255) / 256)), 256, 0, s, false, a);
}
#endif
