// gpcc_markov_hess_inst.hip -- the instantiations of gpcc_markov_hess<P, NOFF> for one P = GPCC_INST_P (1, 2, 3 states of the process;
// NOFF = 0 .. 4 offset states, each holding the four bodies of the kinds of pair), their launch, and with P = 1 the finish kernel:
// three objects (gpcc.jl_amd/build.py compiles the objects side by side).
#include "gpcc_markov_hess.hip.h"

#ifndef GPCC_INST_P
#error "GPCC_INST_P (1, 2 or 3) selects the instantiations of this object"
#endif

#if GPCC_INST_P == 1
#define GPCC_MKH_EACH(F) GPCC_MKH_EACH_P1(F)
#elif GPCC_INST_P == 2
#define GPCC_MKH_EACH(F) GPCC_MKH_EACH_P2(F)
#else
#define GPCC_MKH_EACH(F) GPCC_MKH_EACH_P3(F)
#endif

template <>
hipError_t gpcc_markov_hess_launch_p<GPCC_INST_P>(int noff, const GpccMarkovHessArgs &a, int blocks, int slots, int threads, size_t lds,
                                                  hipStream_t s)
{
#define GPCC_MKH_CASE(PP, NN)                                                                  \
    if (noff == NN) {                                                                          \
        gpcc_markov_hess<PP, NN><<<dim3(blocks, slots), dim3(threads), lds, s>>>(a);           \
        return hipGetLastError();                                                              \
    }
    GPCC_MKH_EACH(GPCC_MKH_CASE)
#undef GPCC_MKH_CASE
    return hipErrorInvalidValue;
}

// more than the default 64 KiB of dynamic LDS for the staged light curves (per device, idempotent)
template <>
hipError_t gpcc_markov_hess_configure_p<GPCC_INST_P>()
{
#define GPCC_MKH_ATTR(PP, NN)                                                                                                        \
    {                                                                                                                                \
        const hipError_t e = hipFuncSetAttribute((const void *)gpcc_markov_hess<PP, NN>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                                 GPCC_MARKOV_LDS_MAX);                                                               \
        if (e != hipSuccess) return e;                                                                                               \
    }
    GPCC_MKH_EACH(GPCC_MKH_ATTR)
#undef GPCC_MKH_ATTR
    return hipSuccess;
}

#if GPCC_INST_P == 1
// the M blocks from the slots: every pair (a, b), a <= b, to both halves of its row's block; NaN blocks where info != 0
static __global__ void __launch_bounds__(64) gpcc_markov_hess_finish(const GpccMarkovHessArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int n = a.L + 1;
    const bool bad = a.out_info[m] != 0;
    double *H = a.hess + m * n * n;
    int slot = 0;
    for (int i = 0; i < n; ++i)
        for (int k = i; k < n; ++k, ++slot) H[i * n + k] = H[k * n + i] = bad ? __builtin_nan("") : a.slot[(long)slot * a.M + m];
}

hipError_t gpcc_markov_hess_finish_launch(const GpccMarkovHessArgs &a, hipStream_t s)
{
    gpcc_markov_hess_finish<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
    return hipGetLastError();
}
#endif
