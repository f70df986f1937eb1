// gpcc_markov_hess_tau_inst.hip -- the instantiations of gpcc_markov_hess_tau<P, NOFF> that ship (GpccMkShipsHess of gpcc_markov_hess.hip.h; each
// holds the four bodies of the kinds of pair) for one P = GPCC_INST_P, and their launch; with P = 1 also the finish kernel and the
// launch of the family, which picks the object: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_hess_tau.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_hess_tau<P, g.noff> on the grid (g.blocks, slots): each object defines its own P's
template <int P>
hipError_t gpcc_markov_hess_tau_launch_p(const GpccMkLaunch &g, int slots, const GpccMarkovHessTauArgs &a);

template <>
hipError_t gpcc_markov_hess_tau_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int slots, const GpccMarkovHessTauArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsHess, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_hess_tau<P(), NOFF()>, g, slots, a);
    });
}

#if GPCC_INST_P == 1
// the M blocks: the leading (L+1) x (L+1) block from gpcc_markov_hess_finish's of the same call, every pair with a tau from its slot
// to both halves; NaN blocks where info != 0
static __global__ void __launch_bounds__(64) gpcc_markov_hess_tau_finish(const GpccMarkovHessTauArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int L = a.L, n = L + 1, W = 2 * L + 1;
    const bool bad = a.out_info[m] != 0;
    const double nan = __builtin_nan("");
    double *H = a.hess + m * W * W;
    const double *B = a.hyper + m * n * n;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) H[i * W + k] = bad ? nan : B[i * n + k];
    int slot = 0;
    for (int i = 0; i < n; ++i)         // (alpha_i, tau_l), then (rho, tau_l)
        for (int l = 0; l < L; ++l, ++slot) H[i * W + n + l] = H[(n + l) * W + i] = bad ? nan : a.slot[(long)slot * a.M + m];
    for (int l = 0; l < L; ++l, ++slot) H[(n + l) * W + n + l] = bad ? nan : a.slot[(long)slot * a.M + m];
    for (int l = 0; l < L; ++l)
        for (int k = l + 1; k < L; ++k, ++slot) H[(n + l) * W + n + k] = H[(n + k) * W + n + l] = bad ? nan : a.slot[(long)slot * a.M + m];
}

template <> hipError_t gpcc_markov_hess_tau_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovHessTauArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_hess_tau_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovHessTauArgs &);

hipError_t gpcc_markov_hess_tau_launch(const GpccMkLaunch &g, int slots, const GpccMarkovHessTauArgs &a)
{
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsHess>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_hess_tau_launch_p<P()>(g, slots, a); });
    if (e != hipSuccess) return e;
    gpcc_markov_hess_tau_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, g.s>>>(a);
    return hipGetLastError();
}
#endif
