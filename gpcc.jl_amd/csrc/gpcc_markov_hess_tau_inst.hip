// gpcc_markov_hess_tau_inst.hip -- the instantiations of gpcc_markov_hess_tau<P, NOFF> for one P = GPCC_INST_P (1, 2, 3 states of the
// process; NOFF = 0 .. 4 offset states, each holding the four bodies of the kinds of pair), their launch, and with P = 1 the finish
// kernel: three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_hess_tau.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

#if GPCC_INST_P == 1
#define GPCC_MKT_EACH(F) GPCC_MKT_EACH_P1(F)
#elif GPCC_INST_P == 2
#define GPCC_MKT_EACH(F) GPCC_MKT_EACH_P2(F)
#else
#define GPCC_MKT_EACH(F) GPCC_MKT_EACH_P3(F)
#endif

template <>
hipError_t gpcc_markov_hess_tau_launch_p<GPCC_INST_P>(int noff, const GpccMarkovHessTauArgs &a, int blocks, int slots, int threads,
                                                      size_t lds, hipStream_t s)
{
#define GPCC_MKT_CASE(PP, NN)                                                                      \
    if (noff == NN) {                                                                              \
        gpcc_markov_hess_tau<PP, NN><<<dim3(blocks, slots), dim3(threads), lds, s>>>(a);           \
        return hipGetLastError();                                                                  \
    }
    GPCC_MKT_EACH(GPCC_MKT_CASE)
#undef GPCC_MKT_CASE
    return hipErrorInvalidValue;
}

// more than the default 64 KiB of dynamic LDS for the staged light curves (per device, idempotent)
template <>
hipError_t gpcc_markov_hess_tau_configure_p<GPCC_INST_P>()
{
#define GPCC_MKT_ATTR(PP, NN)                                                                                                            \
    {                                                                                                                                    \
        const hipError_t e = hipFuncSetAttribute((const void *)gpcc_markov_hess_tau<PP, NN>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                                 GPCC_MARKOV_LDS_MAX);                                                                   \
        if (e != hipSuccess) return e;                                                                                                   \
    }
    GPCC_MKT_EACH(GPCC_MKT_ATTR)
#undef GPCC_MKT_ATTR
    return hipSuccess;
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

hipError_t gpcc_markov_hess_tau_finish_launch(const GpccMarkovHessTauArgs &a, hipStream_t s)
{
    gpcc_markov_hess_tau_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
    return hipGetLastError();
}
#endif
