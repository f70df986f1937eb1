// gpcc_markov_noise_hess_tau_inst.hip -- the instantiations of gpcc_markov_noise_hess_tau<P, NOFF> that ship (GpccMkShipsNoiseHessTau of
// gpcc_markov_noise_hess_tau.hip.h; each holds the five bodies of the kinds of pair) for one P = GPCC_INST_P, and their launch; with
// P = 1 also the finish kernel and the launch of the family, which picks the object: three objects (gpcc.jl_amd/build.py compiles the
// objects side by side).
#include "gpcc_markov_noise_hess_tau.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

// gpcc_markov_noise_hess_tau<P, g.noff> on the grid (g.blocks, slots): each object defines its own P's
template <int P>
hipError_t gpcc_markov_noise_hess_tau_launch_p(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessTauArgs &a);

template <>
hipError_t gpcc_markov_noise_hess_tau_launch_p<GPCC_INST_P>(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessTauArgs &a)
{
    return gpcc_mk_dispatch<GpccMkShipsNoiseHessTau, GPCC_INST_P, GPCC_INST_P>(g.p, g.noff, [&](auto P, auto NOFF) {
        return gpcc_mk_launch_kernel(gpcc_markov_noise_hess_tau<P(), NOFF()>, g, slots, a);
    });
}

#if GPCC_INST_P == 1
// the M blocks over [alpha, rho, tau, kappa, nu]: the rows and columns of [alpha, rho, kappa, nu] from gpcc_markov_noise_hess_finish's
// blocks of the same call, every pair with a tau from its slot to both halves; NaN blocks where info != 0
static __global__ void __launch_bounds__(64) gpcc_markov_noise_hess_tau_finish(const GpccMarkovNoiseHessTauArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int L = a.L, n = L + 1, T = n, K = 2 * L + 1, W = 4 * L + 1, nb = 3 * L + 1;
    const bool bad = a.out_info[m] != 0;
    const double nan = __builtin_nan("");
    double *H = a.hess + m * W * W;
    const double *B = a.noise + m * nb * nb;
    for (int i = 0; i < nb; ++i)
        for (int k = 0; k < nb; ++k) H[(i < n ? i : i + L) * W + (k < n ? k : k + L)] = bad ? nan : B[i * nb + k];
    int slot = 0;
    for (int i = 0; i < n; ++i)         // (alpha_i, tau_l), then (rho, tau_l)
        for (int l = 0; l < L; ++l, ++slot) H[i * W + T + l] = H[(T + l) * W + i] = bad ? nan : a.slot[(long)slot * a.M + m];
    for (int l = 0; l < L; ++l, ++slot) H[(T + l) * W + T + l] = bad ? nan : a.slot[(long)slot * a.M + m];
    for (int l = 0; l < L; ++l)
        for (int k = l + 1; k < L; ++k, ++slot) H[(T + l) * W + T + k] = H[(T + k) * W + T + l] = bad ? nan : a.slot[(long)slot * a.M + m];
    for (int q = 0; q < 2; ++q)         // (tau_l, kappa_k), then (tau_l, nu_k)
        for (int l = 0; l < L; ++l)
            for (int k = 0; k < L; ++k, ++slot)
                H[(T + l) * W + K + q * L + k] = H[(K + q * L + k) * W + T + l] = bad ? nan : a.slot[(long)slot * a.M + m];
}

template <> hipError_t gpcc_markov_noise_hess_tau_launch_p<2>(const GpccMkLaunch &, int, const GpccMarkovNoiseHessTauArgs &);   // (the other two objects')
template <> hipError_t gpcc_markov_noise_hess_tau_launch_p<3>(const GpccMkLaunch &, int, const GpccMarkovNoiseHessTauArgs &);

hipError_t gpcc_markov_noise_hess_tau_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessTauArgs &a)
{
    if (slots != gpcc_markov_noise_hess_tau_slots(a.L)) return hipErrorInvalidValue;
    const hipError_t e = gpcc_mk_dispatch<GpccMkShipsNoiseHessTau>(g.p, g.noff, [&](auto P, auto) { return gpcc_markov_noise_hess_tau_launch_p<P()>(g, slots, a); });
    if (e != hipSuccess) return e;
    gpcc_markov_noise_hess_tau_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, g.s>>>(a);
    return hipGetLastError();
}
#endif
